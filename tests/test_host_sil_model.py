"""The numpy model of the silhouette term (tests/sil_model.py) and the gates of tests/test_gpu_sil_perpixel.py, checked on the CPU: the model's forward against the
float32 oracle pixel for pixel (contested pixels capped), the model's backward against the float32 oracle per vertex component in units of u S (this is where
sil_cases.E32 comes from) and, in float64, against the float64 oracle on exactly reproduced corners, every precondition the case families claim, and faulty variants of the model held to the per-vertex gates.  Measured figures: tests/golden/sil_perpixel.md."""
import numpy as np
import pytest

import sil_cases as SC
import sil_model as M


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in SC.all_cases()}


def test_every_family_at_every_size_class(cases):
    fam = {}
    for c in cases.values():
        fam.setdefault(c.family, set()).add(c.size)
    assert set(SC.E32) == set(cases) and set(fam) == set(SC.family_e32())
    for f, sizes in fam.items():
        assert {64, 192, 320} <= sizes, (f, sizes)
    assert fam["inside"] == set(SC.SIZES)
    assert sorted(c.NF for c in cases.values() if c.name.startswith("counts-64")) == [1, 15, 16, 17]
    assert all(c.NF <= 200 and c.B in (1, 3) and c.eps == 1e-4 for c in cases.values())


def test_model_forward_equals_the_float32_oracle(cases):
    """coverage and owner, pixel for pixel.  Exact cases (lattice at 64, 192, 256, layers with gaps >= 1e-4, slivers; float32 edge tests): no pixel differs.
    Elsewhere the pixels that differ -- and only those are left out of the GPU comparison -- are each one the float64 model calls contested, at most 0.5 %
    of the case's covered pixels."""
    for c in cases.values():
        if not c.asserted:
            continue
        r = SC.reference(c); skip = r["skip"]; n = int(skip.sum())
        if c.exact:
            assert n == 0, (c.name, n, np.argwhere(skip)[:5])
        else:
            assert not (skip & ~r["contested"]).any(), (c.name, np.argwhere(skip & ~r["contested"])[:5])
            assert n <= SC.MAX_CONTESTED * int((r["fi"] >= 0).sum()), (c.name, n)


def _measure(c):
    from oracle import oracle as O
    r = SC.reference(c)
    dvo = O.sil_backward(c.verts, c.faces, c.K, r["dimg"], c.size, c.eps)
    return M.units(dvo, r["grad"], r["S"], r["Q"])


def test_model_backward_equals_the_float32_oracle_and_e32_is_current(cases):
    """|oracle - model| per vertex component in units of u S; the worst of a case is its E32 (recorded constant within a factor of 2 of this measurement, never
    below 1); S = 0 -> exactly 0"""
    for c in cases.values():
        u = _measure(c)
        assert np.isfinite(u).all(), c.name                                        # (inf: a non-zero value where no term entered)
        e = SC.E32[c.name]; w = max(float(u.max()), 1.0)
        assert e / 2 <= w <= 2 * e, (c.name, e, w)


def test_model_is_at_float64_level(cases):
    """The float64 oracle projects in float64, so on a case's own vertices its corners differ from the float32 ones by ~u.  Here it is given vertices from which it
    reproduces a case's float32 corners EXACTLY (K = [1 0 .5; 0 1 .5], x = u_n / 2, y = -v_n / 2, z + 1e-9 == 1: every operation of its projection is exact,
    checked below), flat in depth; the model takes the float64 oracle's own owner map and decides in float64 like it.  What is left is float64 rounding, amplified by
    the same cancellation d1 - d1_cross that E32 measures in float32: the bound is GATE x E32 x 2^-29 (2^-53 / 2^-24) of one float32 unit."""
    from oracle import oracle64 as O64
    z1 = 1.0 - 1e-9
    assert z1 + 1e-9 == 1.0
    K1 = np.array([1, 0, .5, 0, 1, .5, 0, 0, 1], np.float64)
    n = 0
    for name in ("inside-64", "cut-192", "near-64", "slivers-320", "lattice-64", "lattice-192", "counts-320-nf17"):
        c = cases[name]; r = SC.reference(c); pv = r["pv"].astype(np.float64)
        v = np.stack([pv[..., 0] / 2, -pv[..., 1] / 2, np.full(pv.shape[:2], z1)], -1)
        x_ = v[..., 0] / (v[..., 2] + 1e-9); y_ = v[..., 1] / (v[..., 2] + 1e-9)
        assert np.array_equal(2.0 * ((1.0 * x_ + 0.0 * y_ + 0.5) - 0.5), pv[..., 0]) and np.array_equal(2.0 * ((1.0 - (0.0 * x_ + 1.0 * y_ + 0.5)) - 0.5), pv[..., 1]), name
        Kb = np.tile(K1, (c.B, 1))
        fi64 = O64.sil_face_index(v, c.faces, Kb, c.size); dv = O64.sil_backward(v, c.faces, Kb, r["dimg"], c.size, c.eps)
        assert (fi64 >= 0).any()
        for b in range(c.B):
            g, S, _, _ = M.backward(r["pv"][b], c.faces, K1, v[b], fi64[b], r["dimg"][b], c.size, c.eps, decide=np.float64)
            u = M.units(dv[b], g, S); n += int((S > 0).sum())
            assert u.max() <= SC.gate(c) * 2.0 ** -29, (name, b, u.max(), SC.gate(c) * 2.0 ** -29)
    assert n > 1000


def test_cut_cases_touch_the_border(cases):
    for s in (64, 192, 320):
        c = cases[f"cut-{s}"]; r = SC.reference(c); img = r["img"] > 0
        assert img[0, :, 0].any() and (img[0, 0, :].any() or img[0, -1, :].any()), "frame 0 crosses two borders"
        assert img[0, 0, 0] or img[0, -1, 0], "... and the corner between them"
        pv = r["pv"][1]; ctr = pv[:, :2].mean(0)
        assert np.abs(ctr).max() > 1 and img[1].any(), "frame 1: centre outside, still visible"
        assert img[2, :, -1].any() and (img[2, 0, -1] or img[2, -1, -1])
        st = r["stats"]
        assert sum(x["breaks"] for x in st) > 50 and sum(x["d0_clamped"] for x in st) > 20 and sum(x["d1_clamped"] for x in st) > 0, st


def test_depth_plane_cases_straddle_the_planes(cases):
    for fam, plane in (("near", M.NEAR), ("far", M.FAR)):
        for s in (64, 192, 320):
            c = cases[f"{fam}-{s}"]; r = SC.reference(c)
            assert c.verts[..., 2].min() > 0.02
            for b in range(c.B):
                z = c.verts[b][:, 2][c.faces]
                assert int(((z.min(1) < plane) & (z.max(1) > plane)).sum()) >= 10, (c.name, b)
            both = sum(int(((fw["clipped"] > 0) & (fw["accepted"] > 0)).sum()) for fw in r["fw"])
            assert both > 0, c.name                                                # a face with a clipped and an unclipped pixel


def test_layer_cases_have_the_stated_gaps(cases):
    for s in (64, 192, 320):
        for name, gaps in ((f"layers-{s}", SC.LAYER_GAPS), (f"layers-narrow-{s}", SC.NARROW_GAPS)):
            c = cases[name]; r = SC.reference(c)
            for b, g in enumerate(gaps):
                zB = M.forward(r["pv"][b], c.faces[:8], c.size)["z1"]; zA = M.forward(r["pv"][b][9:], c.faces[:8], c.size)["z1"]      # each sheet alone
                both = np.isfinite(zA) & np.isfinite(zB)
                rel = (zB[both] - zA[both]) / zA[both]
                assert both.sum() > 0.3 * s * s and 0.5 * g < rel.min() < 3 * g + 2e-4 * 64 / s, (name, b, rel.min())
                if g >= 1e-4:
                    assert (r["fi"][b][both] >= c.NF // 2).all()                   # the near sheet (the LARGER ids) owns the overlap
            box = np.ptp(r["pv"][0][c.faces][:, :, :2], axis=1) * s / 2                      # (NF, 2) pixel extents of the faces' boxes
            assert c.NF == 16 and (box[:, 0] * box[:, 1]).min() > 2 * 128                     # every box well above SIL_BIG: the whole-wave path


def test_lattice_vertices_sit_on_pixel_centres(cases):
    for s in (64, 256):
        c = cases[f"lattice-{s}"]; r = SC.reference(c); pv = r["pv"][0].astype(np.float64)
        px = (pv[:, :2] * s + s - 1) / 2
        assert np.array_equal(px, np.round(px)) and px.min() == 0 and px.max() == s - 1 and ((px > 0) & (px < s - 1)).all(1).any()
        st = r["stats"][0]
        assert st["int_cross"] > 1000 and st["on_corner"] > 100 and st["out_terms"] > 0 and st["in_terms"] > 0, st
        fw = M.forward(r["pv"][0], c.faces, s, edge="f32")
        assert (np.isfinite(fw["z2"]) & (fw["z2"] == fw["z1"])).sum() > 100          # exact depth ties on the shared edges


def test_sliver_cases(cases):
    for s in (64, 192, 320):
        c = cases[f"slivers-{s}"]; r = SC.reference(c); fi = r["fi"][0]; pv = r["pv"][0]
        own = lambda f: int(((fi == f) | (fi == f + c.NF)).sum())
        box = np.ptp(pv[c.faces[0]][:, :2], axis=0) * s / 2
        assert box[0] * box[1] > 128 and 0 < own(0) < 0.05 * box[0] * box[1]
        assert own(1) == own(2) == own(3) == 0 and own(4) == 0
        q = pv[c.faces[4]]; assert q[0, 0] * (q[1, 1] - q[2, 1]) + q[1, 0] * (q[2, 1] - q[0, 1]) + q[2, 0] * (q[0, 1] - q[1, 1]) == 0
        assert own(5) > 0 and own(6) == 0 and np.array_equal(c.faces[5], c.faces[6])


def test_sweeps_cross_words_and_reach_the_last_one(cases):
    for s in (320, 512):
        c = cases[f"inside-{s}"]; r = SC.reference(c)
        assert max(x["max_words"] for x in r["stats"]) >= 3
        row, col = M.sweep_masks(r["fi"][2], r["dimg"][2])
        w = M.pack_words(row)
        assert (w[:, -1] != 0).any() and ((w[:, 1:] & np.uint64(1)) & (w[:, :-1] >> np.uint64(63))).any()      # the last word; bits 63 | 64 of a row
        assert (M.pack_words(col)[:, -1] != 0).any()
    assert max(x["max_words"] for x in SC.reference(cases["cut-320"])["stats"]) >= 3
    assert (cases["inside-64"].keep == 0).any()


FAULTS = {"drop_word": ("inside-192", "inside-320"), "swap_round": ("inside-64", "lattice-64"), "border_empty": ("cut-64", "cut-192", "cut-320")}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_faulty_sweeps_miss_the_gate(cases, fault):
    """a variant of the MODEL held to the gate of the GPU test as if it were the kernel: one sweep word dropped / floor and ceil swapped on the walks along x /
    the second border break dropped (a d1_out beyond the image taken for an empty pixel, so that the inward sweep runs).  Every listed case must catch its fault.
    (Clamping d1_in and d1_out onto the border instead is not a fault: it computes the same numbers.)"""
    for name in FAULTS[fault]:
        c = cases[name]; r = SC.reference(c); caught = False
        for b in range(c.B):
            g, _, _, _ = M.backward(r["pv"][b], c.faces, c.K[b], c.verts[b], r["fi"][b], r["dimg"][b], c.size, c.eps, fault=fault)
            caught |= bool((M.units(g, r["grad"][b], r["S"][b], r["Q"][b]) > SC.gate(c)).any())
        assert caught, (fault, name)


def test_larger_id_on_a_tie_is_caught(cases):
    caught = []
    for name in ("lattice-64", "slivers-64", "lattice-256"):
        c = cases[name]; r = SC.reference(c)
        fw = M.forward(r["pv"][0], c.faces, c.size, edge="f32", tie_larger=True)
        if (fw["owner"] != r["fi"][0]).any():
            caught.append(name)
    assert set(caught) == {"lattice-64", "slivers-64", "lattice-256"}, caught
