"""Named, seeded inputs of the contact Chamfer tests (tests/test_host_chamfer.py, tests/test_gpu_chamfer.py, tools/chamfer_perpoint_report.py).  Everything here
is built on the CPU.  A case is a dict: xs, ys (lists of (n, 3) float32 arrays, one per pair; n may be 0), gscale, lattice (bool).

Fit-like geometry unless a case says otherwise: a pair's clouds have about 5 cm extent, sit at depth 2.3 m and are 1 to 2 cm apart -- the contact sets of the
object stage (human surface points against object surface points within the contact distance).

The sizes are the edges of the kernels (vistracker_amd/csrc/chamfer.hip): far-cloud padding to multiples of 4 and 16, the 1024-point LDS chunk, the 128-point
work item of the split form, the 512-point sweep of the one-workgroup form, and the 1024 threads of the planning kernel (more than 1024 pairs: several pairs a thread).
"""
import functools

import numpy as np

import chamfer_model as M

EDGE_SIZES = [(1, 1), (1, 1025), (1025, 1), (3, 5), (16, 17), (127, 129), (128, 128), (129, 127), (511, 513), (512, 1024), (513, 1023), (1024, 1025)]
WINNERS = [0, 3, 4, 15, 16, 1023, 1024, 1029]
NN_NQ = [1, 255, 256, 257]
NN_NS = [1, 2047, 2048, 2049, 4097]
SEEDS = dict(edges=101, winner_position=102, many_pairs_1030=103, many_pairs_2051=104, nn=105, lattice_ties=106)


def _pair(rng, nx, ny):
    """two clouds of 5 cm extent at depth 2.3 m, their centres 1 to 2 cm apart"""
    c = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 2.3])
    d = rng.normal(size=3); d *= rng.uniform(0.01, 0.02) / np.linalg.norm(d)
    x = c + rng.uniform(-0.025, 0.025, (nx, 3)); y = c + d + rng.uniform(-0.025, 0.025, (ny, 3))
    return x.astype(np.float32), y.astype(np.float32)


def _edges():
    rng = np.random.default_rng(SEEDS["edges"])
    live = list(EDGE_SIZES)
    sizes = [(0, 7), (5, 0), (0, 0)] + live[:6] + [(0, 3), (2, 0), (0, 0)] + live[6:] + [(0, 9), (4, 0), (0, 0)]
    prs = [_pair(rng, a, b) for a, b in sizes]
    return dict(xs=[p[0] for p in prs], ys=[p[1] for p in prs], gscale=1.0, lattice=False)


def _winner_position(swap):
    """one near point against 1030 far points on a shell of 1 to 3 cm around it; the far point at index w is moved to 3 mm: the unique winner"""
    rng = np.random.default_rng(SEEDS["winner_position"]); xs, ys = [], []
    for w in WINNERS:
        a = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), 2.3])
        d = rng.normal(size=(1030, 3)); d *= (rng.uniform(0.01, 0.03, 1030) / np.linalg.norm(d, axis=1))[:, None]
        d[w] *= 0.003 / np.linalg.norm(d[w])
        xs.append(a[None].astype(np.float32)); ys.append((a + d).astype(np.float32))
    return dict(xs=ys, ys=xs, gscale=1.0, lattice=False) if swap else dict(xs=xs, ys=ys, gscale=1.0, lattice=False)


def _many_pairs(P, seed):
    rng = np.random.default_rng(seed); xs, ys = [], []
    for p in range(P):
        nx, ny = (300, 260) if p in (P // 2, P - 1) else (int(rng.integers(1, 6)), int(rng.integers(1, 6)))
        if p not in (P // 2, P - 1) and rng.random() < 0.1:
            nx, ny = [(0, ny), (nx, 0), (0, 0)][int(rng.integers(0, 3))]
        x, y = _pair(rng, nx, ny); xs.append(x); ys.append(y)
    return dict(xs=xs, ys=ys, gscale=1.0, lattice=False)


# ---- lattice_ties: coordinates k / 64, |k| <= 256; P, every cloud size and gscale powers of two: every distance, gradient term, sum and mean is exact in float32 ---
def _lat(k):
    k = np.asarray(k, np.int64).reshape(-1, 3); assert np.abs(k).max() <= 256
    return (k / 64.0).astype(np.float32)


# (index of the first copy, index of the second copy) of the planted winners of pair 0 (far cloud of 2048 points): index distances 1, 4, 16, 128 and the chunk edge
LATTICE_DUPLICATES = [(10, 11), (20, 24), (40, 56), (100, 228), (1023, 1024)]
LATTICE_MIDWAY = (5, 1500)              # near point 5 of pair 0 lies exactly midway between these two far points


def _lattice():
    """Pair 0 (8 near, 2048 far): the far cloud's filler points have k_x <= -64, the planted far points and all near points k_x >= 64, so a near point's candidates
    are the planted points only: near point q sits one lattice step from planted winner q, which is stored twice (LATTICE_DUPLICATES); near point 5 sits midway
    between two planted points (LATTICE_MIDWAY); near points 6 and 7 are copies of near point 0 (duplicated near points, one far winner).
    Pair 1 is pair 0 with the roles swapped.  Pair 2 (2048, 2048): k in [-6, 6]^3, 2197 positions for 2048 points on each side: duplicates and ties everywhere,
    more than one LDS chunk on both sides.  Pairs 3..7: small clouds, a coincident pair (zero gradient), a near point midway between the two far points."""
    rng = np.random.default_rng(SEEDS["lattice_ties"])
    far = np.stack([rng.integers(-256, -63, 2048), rng.integers(-256, 257, 2048), rng.integers(-256, 257, 2048)], 1)
    near = np.zeros((8, 3), np.int64)
    for q, (i0, i1) in enumerate(LATTICE_DUPLICATES):
        w = np.array([128, 96 * q - 192, 32 * q]); far[i0] = far[i1] = w; near[q] = w + [1, 2, -1]
    m = np.array([200, 240, -200]); far[LATTICE_MIDWAY[0]] = m + [0, 6, 0]; far[LATTICE_MIDWAY[1]] = m - [0, 6, 0]; near[5] = m
    near[6] = near[7] = near[0]
    small = lambda n: rng.integers(-6, 7, (n, 3))
    xs = [near, far, small(2048), small(16), [[3, 3, 3]], [[0, 0, 0]], small(1024), small(4)]
    ys = [far, near, small(2048), small(16), [[3, 3, 3]], [[0, -5, 0], [0, 5, 0]], small(2), small(512)]
    return dict(xs=[_lat(a) for a in xs], ys=[_lat(b) for b in ys], gscale=1024.0, lattice=True)


CASES = ["edges", "winner_position", "winner_position_swapped", "lattice_ties", "many_pairs_1030", "many_pairs_2051"]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "edges": return _edges()
    if name == "winner_position": return _winner_position(False)
    if name == "winner_position_swapped": return _winner_position(True)
    if name == "lattice_ties": return _lattice()
    if name == "many_pairs_1030": return _many_pairs(1030, SEEDS[name])
    if name == "many_pairs_2051": return _many_pairs(2051, SEEDS[name])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, gscale=None):
    """the float64 model of a case (computed once per process and shared: do not modify)"""
    c = case(name)
    return M.chamfer(c["xs"], c["ys"], c["gscale"] if gscale is None else gscale)


def packed(name):
    """-> x (total_x, 3), y (total_y, 3) float32, offx, offy (P + 1) int32"""
    c = case(name)
    offx = np.concatenate([[0], np.cumsum([len(a) for a in c["xs"]])]).astype(np.int32); offy = np.concatenate([[0], np.cumsum([len(b) for b in c["ys"]])]).astype(np.int32)
    return np.concatenate(c["xs"]).reshape(-1, 3), np.concatenate(c["ys"]).reshape(-1, 3), offx, offy


def index_list(name):
    """the index list of the indexed form: the y rows are rows idx[r] of an array with three times as many rows, in permuted order.  -> idx (total_y) int32, rows"""
    total_y = int(sum(len(b) for b in case(name)["ys"])); rows = 3 * max(total_y, 1)
    return np.random.default_rng(7).permutation(rows)[:total_y].astype(np.int32), rows


# ---- vt_nn_distance: P = 3 equal-sized pairs per (nq, ns) -----------------------------------------------------------------------------------------------------
NN_CASES = [(nq, ns) for nq in NN_NQ for ns in NN_NS]


@functools.lru_cache(maxsize=None)
def nn_case(nq, ns):
    """pair 0: fit-like clouds; pair 1: the winner of every query is in the last 2048-point chunk of the searched cloud (the points before it are a metre away);
    pair 2: lattice points, every other query coincides with a searched point (distance exactly 0).  -> query (3, nq, 3), search (3, ns, 3) float32"""
    rng = np.random.default_rng(SEEDS["nn"] + 10000 * nq + ns)
    q0, s0 = _pair(rng, nq, ns)
    q1, s1 = _pair(rng, nq, ns); last = ((ns - 1) // 2048) * 2048; s1[:last] += np.float32(1.0)
    s2 = rng.integers(-256, 257, (ns, 3)); q2 = rng.integers(-256, 257, (nq, 3)); q2[::2] = s2[(7 * np.arange(0, nq, 2)) % ns]
    return np.stack([q0, q1, _lat(q2)]), np.stack([s0, s1, _lat(s2)])


# ---- running the kernels (GPU): every device array is a VIEW into a larger tensor with GUARD sentinel rows before and after it, the workspace is filled with
#      0xFF bytes before every planning call; the sentinels must keep their bits (checked here, on every run) ---------------------------------------------------------
FORMS = ["ragged", "ws", "idx"]
GUARD = 64


class _Guarded:
    def __init__(self, torch, rows_np, seed):
        g = torch.Generator().manual_seed(seed)
        self.full = (torch.rand((len(rows_np) + 2 * GUARD, 3), generator=g) + 0.5).cuda()          # sentinels in [0.5, 1.5): no zero, no value of a case
        self.view = self.full[GUARD:GUARD + len(rows_np)]; self.view.copy_(torch.from_numpy(np.ascontiguousarray(rows_np)))
        self.before = self.full.clone()

    def guards_intact(self, torch):
        a, b = self.full.view(torch.int32), self.before.view(torch.int32)
        return bool(torch.equal(a[:GUARD], b[:GUARD]) and torch.equal(a[-GUARD:], b[-GUARD:]))

    def unchanged(self, torch):
        return bool(torch.equal(self.full.view(torch.int32), self.before.view(torch.int32)))


def run_kernels(form, name, gscale=None, init=None, want_dx=True, want_dy=True, ws=None, run_plan=1):
    """One call of vt_chamfer_ragged ("ragged"), vt_chamfer_ragged_ws ("ws") or vt_chamfer_ragged_idx ("idx") on a case.
    init: None (gradients start from zero) or (ix, iy) float32 start values of the compact rows (the indexed form scatters iy into its big gradient array, whose
    other rows get seeded nonzero values).  -> dict: term (float), dx, dy (numpy float32, compact rows; dx is None for the indexed form, which has no x gradient),
    ws (the workspace, for a second call with run_plan = 0).  Raises AssertionError if a sentinel row, an input, or a row outside the index list changed."""
    import torch
    from vistracker_amd import _lib as L
    lib = L.lib(); c = case(name); gscale = c["gscale"] if gscale is None else gscale
    x, y, offx, offy = packed(name); P = len(offx) - 1
    ox, oy = torch.from_numpy(offx).cuda(), torch.from_numpy(offy).cuda()
    ix, iy = (np.zeros_like(x), np.zeros_like(y)) if init is None else init
    X = _Guarded(torch, x, 1); DX = _Guarded(torch, ix, 2)
    term = torch.zeros(1, dtype=torch.float64, device="cuda")
    nbytes = int(lib.vt_chamfer_ws_bytes(len(x), len(y), P))
    if form != "ragged" and run_plan:
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    if form == "idx":
        idx, rows = index_list(name); idx_t = torch.from_numpy(idx).cuda()
        ybig = np.full((rows, 3), 7.0, np.float32); ybig[idx] = y
        gbig = np.zeros((rows, 3), np.float32) if init is None else np.random.default_rng(11).normal(0, 1e-3, (rows, 3)).astype(np.float32)
        gbig[idx] = iy
        Y = _Guarded(torch, ybig, 3); DY = _Guarded(torch, gbig, 4)
        L.check(lib.vt_chamfer_ragged_idx(X.view.data_ptr(), ox.data_ptr(), len(x), Y.view.data_ptr(), idx_t.data_ptr(), oy.data_ptr(), len(y), P, gscale, term.data_ptr(),
                                          DY.view.data_ptr(), ws.data_ptr(), int(run_plan), L.stream_ptr()))
    else:
        Y = _Guarded(torch, y, 3); DY = _Guarded(torch, iy, 4)
        a = (DX.view.data_ptr() if want_dx else None, DY.view.data_ptr() if want_dy else None)
        if form == "ws":
            L.check(lib.vt_chamfer_ragged_ws(X.view.data_ptr(), ox.data_ptr(), len(x), Y.view.data_ptr(), oy.data_ptr(), len(y), P, gscale, term.data_ptr(), a[0], a[1],
                                             ws.data_ptr(), L.stream_ptr()))
        else:
            L.check(lib.vt_chamfer_ragged(X.view.data_ptr(), ox.data_ptr(), Y.view.data_ptr(), oy.data_ptr(), P, gscale, term.data_ptr(), a[0], a[1], L.stream_ptr()))
    torch.cuda.synchronize()
    assert X.unchanged(torch) and Y.unchanged(torch), "an input array changed"
    assert DX.guards_intact(torch) and DY.guards_intact(torch), "a sentinel row around a gradient array changed"
    dy = DY.view.cpu().numpy()
    if form == "idx":
        assert DX.unchanged(torch), "the indexed form has no x gradient"
        other = np.ones(rows, bool); other[idx] = False
        assert np.array_equal(dy[other].view(np.int32), gbig[other].view(np.int32)), "a row of the big gradient array that the index list does not name changed"
        return dict(term=float(term.item()), dx=None, dy=dy[idx], ws=ws)
    return dict(term=float(term.item()), dx=DX.view.cpu().numpy(), dy=dy, ws=ws)


def run_nn(nq, ns):
    """vt_nn_distance on nn_case(nq, ns) -> (3, nq) float32; the output sits between sentinel values that must keep their bits"""
    import torch
    from vistracker_amd import _lib as L
    q, s = nn_case(nq, ns); qt, st = torch.from_numpy(q).cuda(), torch.from_numpy(s).cuda()
    full = torch.full((3 * nq + 2 * GUARD,), -3.0, device="cuda"); out = full[GUARD:GUARD + 3 * nq]
    L.check(L.lib().vt_nn_distance(qt.data_ptr(), nq, st.data_ptr(), ns, 3, out.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((full[:GUARD] == -3.0).all() and (full[-GUARD:] == -3.0).all()), "a sentinel around the output changed"
    return out.cpu().numpy().reshape(3, nq)
