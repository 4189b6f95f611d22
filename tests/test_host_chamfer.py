"""CPU: the float64 model of the contact Chamfer term (tests/chamfer_model.py) against the CPU oracle and a hand-computed example, the properties of the cases
(tests/chamfer_cases.py) that the GPU tests rely on, and a float32 restatement of the kernels' formulas against the gates of tests/test_gpu_chamfer.py: the gates
are derived from the number format, and this file shows that float32 arithmetic in the kernels' order of operations meets them on every case."""
import numpy as np
import pytest

import chamfer_cases as C
import chamfer_model as M

U = M.U
NON_LATTICE = [n for n in C.CASES if not C.case(n)["lattice"]]


def test_model_matches_a_hand_computed_example():
    """x = (0,0,0), (4,0,0); y = (1,0,0), (0,2,0), (5,1,0); P = 1, gscale = 3.
    x0: d = 1, 4, 26 -> y0;  x1: d = 9, 20, 2 -> y2.   y0: d = 1, 9 -> x0;  y1: d = 4, 20 -> x0;  y2: d = 26, 2 -> x1.
    term = (1 + 2) / 2 + (1 + 4 + 2) / 3 = 23 / 6.
    near-side terms 2 (a - b) gscale / na:  x0: 3 (-1, 0, 0); x1: 3 (-1, -1, 0); y0: 2 (1, 0, 0); y1: 2 (0, 2, 0); y2: 2 (1, 1, 0).
    dx0 = (-3,0,0) - (2,0,0) - (0,4,0) = (-5,-4,0);  dx1 = (-3,-3,0) - (2,2,0) = (-5,-5,0);  dy0 = (2,0,0) + (3,0,0) = (5,0,0);  dy1 = (0,4,0);  dy2 = (2,2,0) + (3,3,0) = (5,5,0)."""
    x = np.array([[0, 0, 0], [4, 0, 0]], np.float32); y = np.array([[1, 0, 0], [0, 2, 0], [5, 1, 0]], np.float32)
    r = M.chamfer([x], [y], 3.0)
    assert abs(r["term"] - 23 / 6) < 1e-15
    assert np.array_equal(r["dx"], [[-5, -4, 0], [-5, -5, 0]]) and np.array_equal(r["dy"], [[5, 0, 0], [0, 4, 0], [5, 5, 0]])
    assert list(r["nn_x"][0]) == [0, 2] and list(r["nn_y"][0]) == [0, 0, 1]
    assert list(r["n_x"]) == [3, 2] and list(r["n_y"]) == [2, 1, 2]
    assert np.array_equal(r["S_x"], [[5, 4, 0], [5, 5, 0]]) and np.array_equal(r["S_y"], [[5, 0, 0], [0, 4, 0], [5, 5, 0]])
    assert M.ambiguous(r) == 0
    # an empty pair counts in P and adds nothing; an exact tie goes to the smaller index and shows in the tie set
    r2 = M.chamfer([x, x[:0]], [y, y], 3.0)
    assert abs(r2["term"] - 23 / 12) < 1e-15 and np.array_equal(r2["dx"] * 2, r["dx"]) and not r2["dy"][3:].any() and not r2["n_y"][3:].any()
    r3 = M.chamfer([np.zeros((1, 3), np.float32)], [np.array([[0, 1, 0], [1, 0, 0], [0, -1, 0]], np.float32)], 1.0)
    assert list(r3["nn_x"][0]) == [0] and list(r3["ties_x"][0][0]) == [0, 1, 2] and M.ambiguous(r3) == 1
    assert np.array_equal(r3["dy"], [[0, 2 / 3 + 2, 0], [2 / 3, 0, 0], [0, -2 / 3, 0]]) and list(r3["n_y"]) == [2, 1, 1]
    assert np.array_equal(M.nn_distance(x[None], y[None]), [[1.0, np.sqrt(2.0)]])


@pytest.mark.parametrize("name", NON_LATTICE)
def test_model_matches_the_oracle(name):
    """the oracle computes in float64 and rounds every gradient term to float32 before it adds it (float32 rows): (n + 1) u S per row.  It averages over the live
    pairs, the model (like the kernels) over all P."""
    from oracle import oracle as O
    c = C.case(name); r = C.reference(name)
    live = [k for k in range(len(c["xs"])) if len(c["xs"][k]) and len(c["ys"][k])]
    val, dxo, dyo, _, _ = O.chamfer_ragged([c["xs"][k] for k in live], [c["ys"][k] for k in live], c["gscale"], True)
    scale = len(live) / len(c["xs"])
    assert abs(val * scale - r["term"]) <= 1e-13 * r["term"]
    keep_x = np.concatenate([np.full(len(a), len(a) > 0 and len(b) > 0) for a, b in zip(c["xs"], c["ys"])]); keep_y = np.concatenate([np.full(len(b), len(a) > 0 and len(b) > 0) for a, b in zip(c["xs"], c["ys"])])
    for g, go, n, S, keep in ((r["dx"], dxo, r["n_x"], r["S_x"], keep_x), (r["dy"], dyo, r["n_y"], r["S_y"], keep_y)):
        assert not g[~keep].any() and not n[~keep].any()
        assert (np.abs(go.astype(np.float64) * scale - g[keep]) <= (n[keep][:, None] + 1) * U * S[keep]).all()


@pytest.mark.parametrize("name", NON_LATTICE)
def test_no_near_point_of_a_case_is_ambiguous(name):
    """the ambiguity condition: every near point has ONE admissible float32 winner, so the GPU tests exclude no row"""
    r = C.reference(name)
    points = sum(len(t) for k in ("ties_x", "ties_y") for t in r[k])
    print(f"{name}: {M.ambiguous(r)} ambiguous near points of {points}")
    assert points > 0 and M.ambiguous(r) == 0


def test_case_shapes():
    e = C.case("edges"); sizes = [(len(a), len(b)) for a, b in zip(e["xs"], e["ys"])]
    assert [s for s in sizes if s[0] and s[1]] == C.EDGE_SIZES
    for at in (slice(0, 3), slice(9, 12), slice(-3, None)):           # empty pairs at the front, in the middle and at the end: (0, n), (n, 0), (0, 0)
        a, b, z = sizes[at]; assert a[0] == 0 < a[1] and b[0] > 0 == b[1] and z == (0, 0)
    for name, swap in (("winner_position", False), ("winner_position_swapped", True)):
        r = C.reference(name); c = C.case(name); assert len(c["xs"]) == 8
        assert [int((r["nn_y"] if swap else r["nn_x"])[p][0]) for p in range(8)] == C.WINNERS
        assert all(len(a) == (1030 if swap else 1) and len(b) == (1 if swap else 1030) for a, b in zip(c["xs"], c["ys"]))
    for P, per in ((1030, 2), (2051, 3)):
        c = C.case("many_pairs_%d" % P); sizes = [(len(a), len(b)) for a, b in zip(c["xs"], c["ys"])]
        assert len(sizes) == P and (P + 1023) // 1024 == per and sizes[P // 2] == (300, 260) and sizes[-1] == (300, 260)
        empty = sum(a == 0 or b == 0 for a, b in sizes); assert 0.07 * P < empty < 0.13 * P
        assert all(0 <= a <= 5 and 0 <= b <= 5 for k, (a, b) in enumerate(sizes) if k not in (P // 2, P - 1))
    assert len(C.NN_CASES) == 20
    q, s = C.nn_case(257, 4097); d = M.nn_distance(q, s)
    assert q.shape == (3, 257, 3) and s.shape == (3, 4097, 3) and (d[2][::2] == 0).all() and (d[2] > 0).any()
    assert (np.sqrt(((q[1][:, None].astype(np.float64) - s[1][None, :4096]) ** 2).sum(-1)).min(1) > d[1] + 0.5).all()       # every winner of pair 1 is in the last chunk


def test_lattice_case_is_exact_and_places_the_ties():
    c = C.case("lattice_ties"); r = C.reference("lattice_ties"); r32 = M.chamfer(c["xs"], c["ys"], c["gscale"], np.float32)
    pow2 = lambda v: v > 0 and v & (v - 1) == 0
    assert pow2(len(c["xs"])) and pow2(int(c["gscale"])) and all(pow2(len(a)) and pow2(len(b)) for a, b in zip(c["xs"], c["ys"]))
    for a in c["xs"] + c["ys"]:
        assert np.array_equal(a * 64, np.round(a * 64)) and np.abs(a * 64).max() <= 256
    assert max(len(a) for a in c["xs"][2:3]) > 1024 and len(c["ys"][2]) > 1024
    # float32 and float64 evaluations of the model: the same bits
    assert r32["term"] == r["term"]
    for k in ("dx", "dy", "S_x", "S_y"):
        assert r32[k].dtype == (np.float32 if k[0] == "d" else np.float64) and np.array_equal(r32[k].astype(np.float64), r[k]), k
    assert all(np.array_equal(a, b) for k in ("nn_x", "nn_y") for a, b in zip(r32[k], r[k]))
    # pair 0: near point q has its planted winner twice, the scan keeps the lower index; the lower copy receives every record, the higher one none
    dy0 = r["dy"][r["offy"][0]:r["offy"][1]]; n0 = r["n_y"][r["offy"][0]:r["offy"][1]]
    for q, (i0, i1) in enumerate(C.LATTICE_DUPLICATES):
        assert list(r["ties_x"][0][q]) == [i0, i1] and r["nn_x"][0][q] == i0
        assert n0[i0] == (4 if q == 0 else 2) and n0[i1] == 1          # near points 6 and 7 are copies of near point 0: three records name i0
        far_part = lambda j: dy0[j] - 2 * (c["ys"][0][j].astype(np.float64) - c["xs"][0][r["nn_y"][0][j]]) * c["gscale"] / (2048 * 8)
        assert far_part(i0).any() and not far_part(i1).any()
    assert list(r["ties_x"][0][5]) == list(C.LATTICE_MIDWAY) and r["nn_x"][0][5] == C.LATTICE_MIDWAY[0]
    assert all(r["nn_x"][0][q] == r["nn_x"][0][0] for q in (6, 7))
    # pair 1 = pair 0 with the roles swapped; pair 2: ties on both sides of a pair with more than one LDS chunk; pair 4: coincident points, no gradient
    assert all(np.array_equal(r["nn_y"][1][q], r["nn_x"][0][q]) for q in range(8))
    assert sum(len(t) > 1 for t in r["ties_x"][2]) > 1024 and sum(len(t) > 1 for t in r["ties_y"][2]) > 1024
    assert not r["S_x"][r["offx"][4]].any() and not r["dx"][r["offx"][4]].any()
    assert list(r["ties_x"][5][0]) == [0, 1]


# ---- a float32 restatement of the kernels' formulas: float32 distances, 2 (a - b) gs / na with gs = gscale / P, far-side sums in record order -----------------------
def _restatement32(xs, ys, gscale, dx0=None, dy0=None):
    f = np.float32; P = len(xs); gs = f(gscale) / f(P)
    offx = np.concatenate([[0], np.cumsum([len(a) for a in xs])]); offy = np.concatenate([[0], np.cumsum([len(b) for b in ys])])
    dx = np.zeros((offx[-1], 3), f) if dx0 is None else dx0.copy(); dy = np.zeros((offy[-1], 3), f) if dy0 is None else dy0.copy()
    term = 0.0
    for p in range(P):
        if len(xs[p]) == 0 or len(ys[p]) == 0:
            continue
        ga, gb = dx[offx[p]:offx[p + 1]], dy[offy[p]:offy[p + 1]]
        for a, b, ga, gb in ((xs[p], ys[p], ga, gb), (ys[p], xs[p], gb, ga)):
            e = a[:, None, :] - b[None, :, :]; d = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]; assert d.dtype == f
            nn = d.argmin(1); na = f(len(a))
            g = f(2) * (a - b[nn]) * gs / na; assert g.dtype == f
            ga += g
            s = np.zeros_like(gb); np.add.at(s, nn, g); hit = np.zeros(len(b), bool); hit[nn] = True
            gb[hit] -= s[hit]
            term += float(d[np.arange(len(a)), nn].astype(np.float64).sum()) / len(a)
    return term / P, dx, dy


def _inside(term, dx, dy, r, ix=None, iy=None):
    assert abs(term - r["term"]) <= M.term_gate(r)
    for g, k, init in ((dx, "x", ix), (dy, "y", iy)):
        want = r["d" + k] if init is None else r["d" + k] + init.astype(np.float64)
        assert (np.abs(g.astype(np.float64) - want) <= M.row_gate(r["n_" + k], r["S_" + k], init)).all(), k


@pytest.mark.parametrize("name", NON_LATTICE)
def test_float32_arithmetic_meets_the_gates(name):
    c = C.case(name)
    for gscale in ((1.0, 900.0, 2.0 ** -10) if name == "edges" else (c["gscale"],)):
        r = C.reference(name, gscale)
        _inside(*_restatement32(c["xs"], c["ys"], gscale), r)
    x, y, _, _ = C.packed(name); rng = np.random.default_rng(5)
    ix, iy = (rng.normal(0, 1e-3, a.shape).astype(np.float32) for a in (x, y))
    _inside(*_restatement32(c["xs"], c["ys"], c["gscale"], ix, iy), C.reference(name), ix, iy)


def test_float32_arithmetic_is_exact_on_the_lattice():
    c = C.case("lattice_ties"); r = C.reference("lattice_ties")
    term, dx, dy = _restatement32(c["xs"], c["ys"], c["gscale"])
    assert term == r["term"] and np.array_equal(dx.astype(np.float64), r["dx"]) and np.array_equal(dy.astype(np.float64), r["dy"])


def test_float32_nn_distance_meets_its_gate():
    for nq, ns in C.NN_CASES:
        q, s = C.nn_case(nq, ns); want = M.nn_distance(q, s)
        e = q[:, :, None, :] - s[:, None, :, :]; d = np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2]).min(2)); assert d.dtype == np.float32
        assert (np.abs(d.astype(np.float64) - want) <= 4 * U * want).all(), (nq, ns)
