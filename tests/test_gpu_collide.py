"""GPU (-m gpu): vt_collision_loss (vistracker_amd/csrc/collide.hip, collide_geom.h) against the float64 model (tests/collide_model.py) per triangle pair and per frame, on
the cases of tests/collide_cases.py, through the C ABI.  A frame is an independent case of the call, so with NFs = NFo = 1 a frame is one pair; the per-frame value is the
same call with B = 1 on that frame's slice.

Gates (u = 2^-24; S_V, S_g, n_f from the model; E32 = the float32 CPU oracle's own worst error in units of u S, recorded per family in collide_cases.E32):
* decided frames (no box-overlapping pair with |margin| < TAU = 64 u max|coordinate|):  pairs_per_frame == model, exactly.
* value of a frame (B = 1 call):  |V - V64| <= 8 E32_V u S_V + n_f 2^-41        (n_f object faces round into the 2^40 fixed-point accumulators)
* gradient, per component:        |dt - dt64| <= (8 E32_g u S_g + n_f 2^-41) gscale / B + u |dt64|     (+ u |start| with start values)
* batched term: against the model's mean, the sum of the frame gates divided by B.
Frames left out: only random frames of `pairs` with an undecided pair (tests/test_host_collide.py holds them to 1 %; here: 1 of 503).  order, blocks and the planted
frames are compared whole.

fit_like (the geometry of test_gpu_edges.py::test_collision_term_vs_oracle, B = 2; that test is unchanged) has 1 and 6 undecided pairs.  Adding what those pairs can change
to the gates (collide_model.slack: every resolution of them, displaced pairs under max_coll included) gives 2.5e-5 / 1.7e-3 of V and 4.7e-4 / 3.2e-2 of the largest
gradient component: for the gradient of frame 1 that is NOT tighter than the existing test's 5e-3, because one borderline pair carries up to 1.5 % of a frame's
gradient.  So the test asserts more than that: the kernel's frame must equal ONE resolution of the undecided pairs -- count exactly, value and gradient inside the
arithmetic gates above, which are about 1e-5 of V and 4e-4 of the largest component and so tighter than the 2e-3 and 5e-3 of the existing test (asserted below).
The slack form follows from it and is asserted too.

Every gate is printed as a fraction of itself before it is asserted.  tools/collide_perpair_report.py prints the same figures (tests/golden/collide_perpair.md)."""
import numpy as np
import pytest

import collide_cases as C
import collide_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = M.U


_bits = C._bits


def check_case(name, mc=None, gscale=1.0, start=None, alone=True):
    """the batched call and (alone) every decided frame on its own against the model (collide_cases.measure_case): printed, then asserted"""
    w = C.measure_case(name, mc, gscale, start, alone)
    print(w["line"])
    assert C.case(name)["family"] == "pairs" or w["left_out"] == 0
    assert w["moved"] == 0, (name, "a frame without pairs changed d_obj_t or the term")
    assert w["differ"] == 0, (name, "a frame alone differs from the frame in its batch")
    assert w["pairs"] == 0 and w["value"] <= 1 and w["grad"] <= 1 and w["term"] <= 1, (name, mc, w)
    return w


def test_pairs_one_triangle_pair_per_frame():
    w = check_case("pairs")
    assert w["left_out"] <= 0.01 * (512 - len(C.PLANTED))
    ref = C.reference("pairs"); out = C.run("pairs")
    for name, b in C.PLANTED.items():                                      # the planted frames are all decided: compared above; here what they must show
        assert out["pairs"][b] == ref[b]["pairs"] == (1 if name in ("axis", "phi_under", "phi_over", "apex", "linear") else 0), name


@pytest.mark.parametrize("mc", C.ORDER_MAX_COLL)
@pytest.mark.parametrize("name", C.ORDER_CASES)
def test_order_the_first_max_coll_in_face_order(name, mc):
    """the value names the kept subset (tests/test_host_collide.py: any two subsets of one size are more than 100 gates apart)"""
    check_case(name, mc)


@pytest.mark.parametrize("name", C.BLOCK_CASES)
def test_blocks_object_faces_and_vertices_at_the_block_edges(name):
    check_case(name)


def test_fit_like_equals_one_resolution_of_the_undecided_pairs():
    frames, term = C.measure_fit_like()
    for b, f in enumerate(frames):
        print("fit_like frame %d: %d undecided pairs, %d pairs (model %d, possible %d..%d); nearest resolution: value %.3f of its gate, gradient %.3f; the gates are %.1e of V and %.1e of "
              "the largest component (existing test: 2e-3, 5e-3); with the undecided pairs' slack instead: %.1e and %.1e"
              % (b, f["undecided"], f["pairs"], f["model"], f["lo"], f["hi"], f["value"], f["grad"], f["relV"], f["relg"], f["relV"] + f["slackV"], f["relg"] + f["slackg"]))
        assert not f["differ"], (b, "a frame alone differs from the frame in its batch")
        assert f["matched"] and f["value"] <= 1 and f["grad"] <= 1, (b, f)
        assert f["relV"] < 2e-3 and f["relg"] < 5e-3                      # the ARITHMETIC gates are tighter than tests/test_gpu_edges.py::test_collision_term_vs_oracle; the slack form is not
        assert f["in_slack"], (b, f)
    print("fit_like batched term: %.3f of its gate" % term)
    assert term <= 1


@pytest.mark.parametrize("name,mc", [("pairs", None), ("order_700", 8), ("order_513", 2), ("blocks_513_770", None), ("fit_like", None)])
def test_a_second_run_repeats_the_first_bit_for_bit(name, mc):
    a = C.run(name, mc, 3.0); b = C.run(name, mc, 3.0)
    assert a["term"] == b["term"] and np.array_equal(_bits(a["dt"]), _bits(b["dt"])) and np.array_equal(a["pairs"], b["pairs"])


@pytest.mark.parametrize("name,mc", [("pairs", None), ("order_513", 8), ("blocks_257_257", None)])
def test_term_and_gradient_accumulate_onto_start_values(name, mc):
    B = len(C.case(name)["sv"]); rng = np.random.default_rng(9)
    check_case(name, mc, start=(float(rng.normal(0, 0.3)), rng.normal(0, 0.5, (B, 3)).astype(np.float32)), alone=False)


@pytest.mark.parametrize("name,mc", [("order_700", 8), ("blocks_256_257", None)])
def test_a_null_pointer_changes_nothing_else(name, mc):
    full = C.run(name, mc, 2.0)
    for skip in ("term", "dt", "pairs"):
        o = C.run(name, mc, 2.0, **{"want_" + skip: False})
        assert skip == "term" or o["term"] == full["term"], skip
        assert skip == "dt" or np.array_equal(_bits(o["dt"]), _bits(full["dt"])), skip
        assert skip == "pairs" or np.array_equal(o["pairs"], full["pairs"]), skip
        if skip == "term": assert o["term"] == 0.0
        if skip == "dt": assert not o["dt"].any()
        if skip == "pairs": assert (o["pairs"] == -1).all()
    o = C.run(name, mc, 2.0, want_term=False, want_dt=False, want_pairs=False)
    assert o["term"] == 0.0 and not o["dt"].any() and (o["pairs"] == -1).all()


@pytest.mark.parametrize("gscale", [1.0, 9.0, 2.0 ** -10])
@pytest.mark.parametrize("name,mc", [("pairs", None), ("order_511", 8), ("blocks_255_257", None)])
def test_gscale_sweep(name, mc, gscale):
    check_case(name, mc, gscale, alone=False)
