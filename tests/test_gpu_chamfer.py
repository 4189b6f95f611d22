"""GPU (-m gpu): the contact Chamfer kernels (vt_chamfer_ragged, vt_chamfer_ragged_ws, vt_chamfer_ragged_idx) and vt_nn_distance against the float64 model
(tests/chamfer_model.py), per gradient row and per point, on the cases of tests/chamfer_cases.py.

Every gate is derived from the number format (u = 2^-24), none from a kernel's output and none from another row's magnitude:
* term:  |term - term64| <= 8 u term64.  Every float32 minimum is within 5 u of the float64 one (5 roundings in d0 d0 + d1 d1 + d2 d2), all summands are
  positive and the sum is carried in float64.
* gradient row, per component:  |g - g64| <= (n + 8) u S, n the number of terms added into the row and S the sum of their absolute values, both from the model.
  A term 2 (a - b) gs / na, gs = gscale / P, carries 4 roundings, the row's sum n - 1.  A row with S = 0 must be exactly 0.
  With a nonzero start value the gate is (n + 9) u (S + |start|).
* no near point of a non-lattice case has a second admissible winner (tests/test_host_chamfer.py::test_no_near_point_of_a_case_is_ambiguous): no row is excluded.
* lattice_ties: every operation is exact in float32, so the rows are bit-equal to the model's and the term equal to 1e-15; this pins the tie rule (smallest index
  among equal distances) through the far side: the lower-indexed copy of a duplicated winner receives every record, the higher one none.
* vt_nn_distance:  |d - d64| <= 4 u d64  (5 roundings under a square root: 2.5 u, and the root's own).
tests/test_host_chamfer.py shows that float32 arithmetic in the kernels' order of operations stays inside every one of these gates.
tools/chamfer_perpoint_report.py prints the measured fractions of the gates (profiles/r16_chamfer_perpoint.txt)."""
import numpy as np
import pytest

import chamfer_cases as C
import chamfer_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = M.U
NON_LATTICE = [n for n in C.CASES if n != "lattice_ties"]


def _check(out, r, init=None, what=""):
    """the term gate and the row gate; prints the worst fraction of each before it asserts"""
    te = abs(out["term"] - r["term"])
    rows = []
    for k, i in (("x", 0), ("y", 1)):
        g = out["d" + k]
        if g is None:
            continue
        start = None if init is None else init[i]
        want = r["d" + k] if start is None else r["d" + k] + start.astype(np.float64)
        err = np.abs(g.astype(np.float64) - want); gate = M.row_gate(r["n_" + k], r["S_" + k], start)
        frac = np.where(gate > 0, err / np.where(gate > 0, gate, 1), np.where(err > 0, np.inf, 0.0))
        rows.append((k, err, gate, frac))
    print("%s: term error %.2f u of the term (gate 8 u); worst row %s" % (what, te / (U * r["term"]), ", ".join("d%s %.3f of its gate (row %d)" % (k, f.max(), int(f.max(1).argmax()))
                                                                                                               for k, _, _, f in rows)))
    assert te <= M.term_gate(r), (what, out["term"], r["term"])
    for k, err, gate, frac in rows:
        assert np.isfinite(out["d" + k]).all() and (err <= gate).all(), (what, k, int(frac.max(1).argmax()), float(frac.max()))


@pytest.mark.parametrize("form", C.FORMS)
@pytest.mark.parametrize("name", NON_LATTICE)
def test_term_and_rows_against_the_model(name, form):
    _check(C.run_kernels(form, name), C.reference(name), what=f"{name} {form}")


@pytest.mark.parametrize("form", C.FORMS)
def test_lattice_ties_are_bit_equal_to_the_model(form):
    c = C.case("lattice_ties"); r = C.reference("lattice_ties")
    out = C.run_kernels(form, "lattice_ties")
    assert abs(out["term"] - r["term"]) <= 1e-15 * r["term"], (out["term"], r["term"])
    for k in ("x", "y"):
        g = out["d" + k]
        if g is None:
            continue
        want = r["d" + k].astype(np.float32); assert np.array_equal(want.astype(np.float64), r["d" + k])           # the model's rows are float32 numbers
        bad = np.flatnonzero((g.view(np.int32) != want.view(np.int32)).any(1))
        assert len(bad) == 0, (form, k, len(bad), bad[:8], g[bad[:4]], want[bad[:4]])
    # the tie rule through the far side, spelled out on pair 0: the lower-indexed copy of a planted winner gets the records, the higher one only its own near-side term
    o = r["offy"][0]; own = lambda j: 2 * (c["ys"][0][j].astype(np.float64) - c["xs"][0][r["nn_y"][0][j]]) * c["gscale"] / (2048 * 8)
    for i0, i1 in C.LATTICE_DUPLICATES + [C.LATTICE_MIDWAY]:
        assert np.array_equal(out["dy"][o + i1], own(i1)) and not np.array_equal(out["dy"][o + i0], own(i0)), (form, i0, i1)


@pytest.mark.parametrize("form", C.FORMS)
@pytest.mark.parametrize("name", ["edges", "many_pairs_1030"])
def test_gradients_are_accumulated(name, form):
    """dx / dy start from seeded nonzero values; the indexed form's rows outside the index list keep their bits (checked by the runner)"""
    x, y, _, _ = C.packed(name); rng = np.random.default_rng(5)
    init = tuple(rng.normal(0, 1e-3, a.shape).astype(np.float32) for a in (x, y))
    _check(C.run_kernels(form, name, init=init), C.reference(name), init, what=f"{name} {form} accumulated")


@pytest.mark.parametrize("name", ["edges", "many_pairs_2051"])
def test_guard_rows_poisoned_workspace_and_plan_reuse(name):
    """the runner puts 64 sentinel rows before and after x, y, dx, dy and the indexed form's big arrays and fills the workspace with 0xFF bytes before every planning
    call; it raises if a sentinel changed.  A second indexed call with run_plan = 0 on the same workspace repeats the first bit for bit."""
    for form in C.FORMS:
        C.run_kernels(form, name)
    a = C.run_kernels("idx", name)
    b = C.run_kernels("idx", name, ws=a["ws"], run_plan=0)
    assert a["term"] == b["term"] and np.array_equal(a["dy"].view(np.int32), b["dy"].view(np.int32))
    _check(b, C.reference(name), what=f"{name} idx, plan reused")


@pytest.mark.parametrize("name", ["edges", "many_pairs_1030", "many_pairs_2051"])
def test_a_missing_gradient_pointer_changes_nothing_else(name):
    full = C.run_kernels("ws", name)
    no_dx = C.run_kernels("ws", name, want_dx=False); no_dy = C.run_kernels("ws", name, want_dy=False)
    bits = lambda a: a.view(np.int32)
    assert no_dx["term"] == full["term"] and no_dy["term"] == full["term"], (full["term"], no_dx["term"], no_dy["term"])
    assert not no_dx["dx"].any() and np.array_equal(bits(no_dx["dy"]), bits(full["dy"]))
    assert not no_dy["dy"].any() and np.array_equal(bits(no_dy["dx"]), bits(full["dx"]))
    none = C.run_kernels("ws", name, want_dx=False, want_dy=False)
    assert none["term"] == full["term"] and not none["dx"].any() and not none["dy"].any()


@pytest.mark.parametrize("form", C.FORMS)
@pytest.mark.parametrize("gscale", [1.0, 900.0, 2.0 ** -10])
def test_gscale_sweep(gscale, form):
    _check(C.run_kernels(form, "edges", gscale=gscale), C.reference("edges", gscale), what=f"edges {form} gscale {gscale:g}")


@pytest.mark.parametrize("form", C.FORMS)
@pytest.mark.parametrize("name", C.CASES)
def test_repeatable(name, form):
    a = C.run_kernels(form, name); b = C.run_kernels(form, name)
    for k in ("dx", "dy"):
        assert a[k] is None or np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), (name, form, k)
    assert a["term"] == b["term"], (name, form, a["term"], b["term"], a["term"] - b["term"])


def test_nn_distance_per_point():
    worst = 0.0
    for nq, ns in C.NN_CASES:
        q, s = C.nn_case(nq, ns); want = M.nn_distance(q, s); d = C.run_nn(nq, ns).astype(np.float64)
        err = np.abs(d - want); worst = max(worst, float((err[want > 0] / (U * want[want > 0])).max()))
        assert (d[want == 0] == 0).all(), (nq, ns)                                  # exact zeros stay exactly zero
        assert (err <= 4 * U * want).all(), (nq, ns, float((err[want > 0] / (U * want[want > 0])).max()))
    print("vt_nn_distance: worst error %.2f u of the distance (gate 4 u)" % worst)
