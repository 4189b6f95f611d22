"""Named, seeded inputs of the per-pair tests of the interpenetration term (tests/test_host_collide.py, tests/test_gpu_collide.py, tools/collide_perpair_report.py).
Everything here is built on the CPU.  A case is a dict: sv (B, NVs, 3), ov (B, NVo, 3) float32, sf (NFs, 3), of (NFo, 3) int32, sigma, max_coll, and family extras.
A frame is an independent case of vt_collision_loss: with NFs = NFo = 1 frame b IS one triangle pair.

Fit-like placement (depth about 2.3 m, x and y within +-0.3 m) unless a family says otherwise.

pairs    NFs = NFo = 1, B = 512: random triangles with corners in a +-12 mm cube, centres offset by N(0, 4 mm), and the planted frames of PLANTED.
order    NFo = 1 (one 20 cm object triangle), NFs in ORDER_NFS, B = 6, max_coll in ORDER_MAX_COLL: small SMPL triangles inside the object face's box but clear of
         the face (candidates: more than 256 of them from NFs = 511 on), some outside the box, and planted faces that pierce it at indices that include 0, 255, 256,
         257, 511, 512 and NFs - 1.  Planted face of rank j sits where (1 - Phi)^4 is about 2^-j, so the value names the subset that was kept.
         Frame 1 has no candidates (the object is 5 m away), frame 3 has candidates and no hit; both sit between frames with hits.
blocks   two jittered grids of quads pushed through each other, NFs = 312, B = 3, max_coll = 8, (NFo, NVo) in BLOCKS.  The last object vertex (index NVo - 1: the
         second or fourth pass of the stride-256 loop of the bounding box) is the tip of a flap that pierces the SMPL grid beyond the object grid: without it the
         object's box ends before those SMPL faces.  Object faces that cross the SMPL grid sit at the edges of the blocks of 256 (block_edge_faces: 0, 254, 255,
         256, 511, 512, NFo - 1 -- at NFo = 257 and 513 the last one is the lone thread of the tail block): each has a kept pair in some frame.  The seeds were searched until no box-overlapping pair is undecided and every edge face has a pair (search_block_seed) and are recorded here.
fit_like the geometry of tests/test_gpu_edges.py::_collision_case at B = 2: the object template pushed half-way into the SMPL body."""
import functools

import numpy as np

import collide_model as M

SIGMA = 0.5
GUARD = 64
ORDER_NFS = [255, 256, 257, 511, 513, 700]
ORDER_MAX_COLL = [1, 2, 8, 64]
BLOCKS = [(1, 3), (255, 257), (256, 257), (257, 257), (513, 770)]
BLOCK_SEEDS = {(1, 3): 300, (255, 257): 302, (256, 257): 302, (257, 257): 302, (513, 770): 307}          # search_block_seed(NFo, NVo)
SEEDS = dict(pairs=201, order=202, fit_like=4)

# E32[family] = (value, gradient): the float32 oracle's worst |error| / (u S) against the float64 model on that family (tests/test_host_collide.py measures it afresh
# and holds these figures to the measurement within a factor of 2)
E32 = dict(pairs=(0.48, 0.52), order=(0.029, 0.046), blocks=(0.022, 0.042), fit_like=(0.028, 0.034))

TRI = np.array([[0, 1, 2]], np.int32)


# ---- pairs ------------------------------------------------------------------------------------------------------------------------------------------------------
def _iso(c, s):
    """isosceles triangle in the plane z = c_z with circumcentre c and circumradius 2.5 s; with dyadic c and s every step of the float32 circumcentre formula is exact"""
    return np.array([c + [-2 * s, -1.5 * s, 0], c + [2 * s, -1.5 * s, 0], c + [0, 2.5 * s, 0]])


def _planted():
    """-> list of (name, S, O): the branch is taken by object vertex 0 in the SMPL triangle's cone (side 0, vertex 0) where the name is a branch"""
    c = np.array([0.125, -0.25, 2.25]); s = 2.0 ** -8; big = 0.25; h = 2.0 ** -7; out = []
    out.append(("axis", _iso(c, s), np.array([c + [0, 0, -s / 2], c + [s / 2, 0, s / 2], c + [0, s / 2, s / 2]])))
    for name, eps in (("phi_under", -2.0 ** -12), ("phi_over", 2.0 ** -12)):
        rho = 2.5 * s * (1 + s / SIGMA) * (1 + eps)
        out.append((name, _iso(c, s), np.array([c + [rho, 0, -s], c + [-s, 0, s / 4], c + [0, s, s / 4]])))
    out.append(("apex", _iso(c, big), np.array([c + [0, 0, 0.75], c + [0.1, 0, -0.25], c + [0, 0.1, -0.25]])))
    out.append(("linear", _iso(c, big), np.array([c + [0.05, 0, -0.75], c + [0.1, 0, 0.25], c + [0, 0.1, 0.25]])))
    out.append(("coplanar", _iso(c, s), _iso(c + [s, s / 2, 0], s)))
    seg = np.array([c + [-2 * s, 0, 0], c + [-2 * s, 0, 0], c + [2 * s, 0, 0]]); through = np.array([c + [0, -s, -s], c + [0, s, -s], c + [0, 0, s]])
    out.append(("zero_area_smpl", seg, through)); out.append(("zero_area_object", through, seg))
    p = c + [1.6 * h, 1.6 * h, 0]
    out.append(("separated", np.array([c, c + [2 * h, 0, 0], c + [0, 2 * h, 0]]), np.array([p + [0, 0, -1e-3], p + [1e-3, 0, 1e-3], p + [0, 1e-3, 1e-3]])))
    return out


PLANTED = {name: 7 + 50 * i for i, (name, _, _) in enumerate(_planted())}                    # name -> frame


def _pairs():
    rng = np.random.default_rng(SEEDS["pairs"]); B = 512
    c = np.stack([rng.uniform(-0.3, 0.3, B), rng.uniform(-0.3, 0.3, B), np.full(B, 2.3)], 1)[:, None]
    sv = c + rng.uniform(-0.012, 0.012, (B, 3, 3)); ov = c + rng.normal(0, 0.004, (B, 1, 3)) + rng.uniform(-0.012, 0.012, (B, 3, 3))
    for name, S, O in _planted():
        sv[PLANTED[name]] = S; ov[PLANTED[name]] = O
    return dict(sv=sv.astype(np.float32), sf=TRI, ov=ov.astype(np.float32), of=TRI, sigma=SIGMA, max_coll=8, family="pairs")


# ---- order ------------------------------------------------------------------------------------------------------------------------------------------------------
def _order(NFs):
    rng = np.random.default_rng(SEEDS["order"] + NFs); B = 6
    c = np.array([0.1, -0.15, 2.3]); n = np.array([0.3, 0.2, 1.0]); n /= np.linalg.norm(n)
    u1 = np.cross(n, [0, 1, 0]); u1 /= np.linalg.norm(u1); u2 = np.cross(n, u1); r = 0.115
    obj = np.array([c + r * (np.cos(a) * u1 + np.sin(a) * u2) for a in (0.0, 2 * np.pi / 3, 4 * np.pi / 3)])
    lo, hi = obj.min(0) + 0.006, obj.max(0) - 0.006
    pool = sorted({i for i in (0, 255, 256, 257, 511, 512, NFs - 1) if i < NFs} | {int(i) for i in rng.choice(NFs, 2, replace=False)})
    perm = rng.permutation(3 * NFs); sf = perm.reshape(NFs, 3).astype(np.int32)
    sv = np.zeros((B, 3 * NFs, 3)); ov = np.tile(obj, (B, 1, 1)); planted = []
    for b in range(B):
        p = rng.uniform(lo, hi, (40 * NFs, 3)); p = p[np.abs((p - c) @ n) > 0.015][:NFs]; assert len(p) == NFs
        far = rng.random(NFs) < 0.15
        p[far] += np.where(rng.random((int(far.sum()), 1)) < 0.5, -1.0, 1.0) * np.array([rng.uniform(0.5, 1.0), 0, 0])
        tris = p[:, None] + rng.uniform(-0.002, 0.002, (NFs, 3, 3))
        if b == 1:
            ov[b] += [5.0, 0, 0]
        chosen = [] if b in (1, 3) else pool if b == 0 else sorted(int(i) for i in rng.choice(pool, len(pool) - 2, replace=False))
        ranks = rng.permutation(len(chosen))
        for f, j in zip(chosen, ranks):
            q = c + (1 - 0.95 * 2.0 ** (-j / 4.0)) * r * u1
            tris[f] = [q - 0.003 * n + 0.0005 * u2, q + 0.003 * n + 0.002 * u1, q + 0.003 * n - 0.002 * u1 + 0.001 * u2]
        planted.append(list(chosen))
        sv[b][sf.reshape(-1)] = tris.reshape(-1, 3)
    return dict(sv=sv.astype(np.float32), sf=sf, ov=ov.astype(np.float32), of=TRI, sigma=SIGMA, max_coll=8, family="order", planted=planted)


# ---- blocks -----------------------------------------------------------------------------------------------------------------------------------------------------
def _grid(nx, ny, dx, dy):
    """(nx + 1)(ny + 1) vertices of a grid of nx x ny quads centred on the origin in the plane z = 0, and its 2 nx ny triangles"""
    x, y = np.meshgrid((np.arange(nx + 1) - nx / 2) * dx, (np.arange(ny + 1) - ny / 2) * dy, indexing="ij")
    v = np.stack([x, y, np.zeros_like(x)], -1).reshape(-1, 3); idx = lambda i, j: i * (ny + 1) + j
    f = [t for i in range(nx) for j in range(ny) for t in ((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))]
    return v, np.array(f, np.int32)


def _blocks(NFo, NVo, seed):
    rng = np.random.default_rng(seed); B = 3; c = np.array([-0.2, 0.1, 2.3])
    gs, sf = _grid(12, 13, 0.01, 0.01)
    sv = c + gs[None] + np.stack([np.zeros((B, len(gs))), np.zeros((B, len(gs))), rng.normal(0, 0.0015, (B, len(gs)))], -1)
    tilt = np.deg2rad(30.0); Rx = np.array([[1, 0, 0], [0, np.cos(tilt), -np.sin(tilt)], [0, np.sin(tilt), np.cos(tilt)]])
    if NFo == 1:
        base = np.array([[-0.03, -0.025, 0], [0.03, -0.02, 0], [0.002, 0.035, 0]]); of = TRI
        ov = c + (base @ Rx.T)[None] + rng.normal(0, 0.001, (B, 3, 3))
    else:
        nx, ny = (12, 11) if NVo == 257 else (16, 17)
        go, fo = _grid(nx, ny, 0.08 / nx, 0.08 / ny); assert len(go) < NVo - 1 and len(fo) >= NFo - 1
        ov = np.zeros((B, NVo, 3)); ov[:, :len(go)] = c + (go @ Rx.T)[None] + rng.normal(0, 0.0007, (B, len(go), 3))
        ov[:, len(go):NVo - 1] = ov[:, rng.integers(0, len(go), NVo - 1 - len(go))]                      # vertices that no face names: copies, inside the box
        i0, i1 = nx * (ny + 1) + ny, nx * (ny + 1) + ny - 1                                                # the last two vertices of the column at the largest x
        ov[:, NVo - 1] = c + [0.058, 0.02, -0.015] + rng.normal(0, 0.0007, (B, 3))
        # the object grid is tilted about its row y = 0, so the faces of the quad row that straddles y = 0 cross the SMPL grid: one of them goes to every edge slot
        # (first and last thread of a block of 256, the lone thread of the tail block), the flap to a seeded slot that is no edge
        edge = block_edge_faces(NFo); y = go[fo][:, :, 1]; line = np.flatnonzero((y.min(1) < 0) & (y.max(1) > 0)); assert len(line) >= len(edge)
        on_edge = rng.choice(line, len(edge), replace=False); rest = np.setdiff1d(np.arange(len(fo)), on_edge); rest = rest[rng.permutation(len(rest))]
        of = np.zeros((NFo, 3), np.int32); free = np.setdiff1d(np.arange(NFo), edge); flap = int(rng.choice(free)); free = free[free != flap]
        of[edge] = fo[on_edge]; of[flap] = [i0, i1, NVo - 1]; of[free] = fo[rest[:len(free)]]
    return dict(sv=sv.astype(np.float32), sf=sf, ov=ov.astype(np.float32), of=of, sigma=SIGMA, max_coll=8, family="blocks", seed=seed)


def block_edge_faces(NFo):
    """the object faces at the edges of the one-thread-per-face blocks of 256: every one of them carries a kept pair in some frame of its case"""
    return [i for i in (0, 254, 255, 256, 511, 512) if i < NFo - 1] + [NFo - 1]


def search_block_seed(NFo, NVo, start=300, tries=200):
    """the first seed from `start` on at which no box-overlapping pair of the case is undecided and every face of block_edge_faces has a kept pair in some frame"""
    for seed in range(start, start + tries):
        c = _blocks(NFo, NVo, seed); fr = [M.frame(c["sv"][b], c["sf"], c["ov"][b], c["of"], SIGMA, 8) for b in range(len(c["sv"]))]
        if all(not r["undecided"].any() for r in fr) and set(block_edge_faces(NFo)) <= set(np.concatenate([r["kept"][:, 0] for r in fr]).tolist()):
            return seed
    raise RuntimeError("no seed found")


# ---- fit_like ---------------------------------------------------------------------------------------------------------------------------------------------------
def _fit_like():
    from oracle import oracle as O
    from vistracker_amd import synthetic as syn
    B = 2; rng = np.random.default_rng(SEEDS["fit_like"])
    model = syn.smplh_model(0); seq = syn.sequence_params(B, seed=5)
    sverts, jtr, _ = O.SmplModel(model).forward(seq["pose"], seq["betas"], seq["trans"])
    ov, of = syn.object_template(); R = syn.random_rotations(B, rng)
    t = (jtr[:, 3] + rng.normal(0, 0.03, (B, 3)) + [0.25, 0.0, 0.0]).astype(np.float32)
    Vo = (np.einsum("nc,bcd->bnd", 0.5 * ov, R) + t[:, None]).astype(np.float32)
    return dict(sv=sverts.astype(np.float32), sf=np.asarray(model["f"]).astype(np.int32), ov=Vo, of=of.astype(np.int32), sigma=SIGMA, max_coll=8, family="fit_like")


ORDER_CASES = ["order_%d" % n for n in ORDER_NFS]
BLOCK_CASES = ["blocks_%d_%d" % b for b in BLOCKS]
CASES = ["pairs"] + ORDER_CASES + BLOCK_CASES + ["fit_like"]
FAMILY = dict(pairs=[("pairs", 8)], order=[(n, mc) for n in ORDER_CASES for mc in ORDER_MAX_COLL], blocks=[(n, 8) for n in BLOCK_CASES], fit_like=[("fit_like", 8)])


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "pairs": return _pairs()
    if name == "fit_like": return _fit_like()
    k = name.split("_")
    if k[0] == "order": return _order(int(k[1]))
    if k[0] == "blocks": return _blocks(int(k[1]), int(k[2]), BLOCK_SEEDS[(int(k[1]), int(k[2]))])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name, max_coll=None, dtype=np.float64):
    """the model of every frame of a case (computed once per process and shared: do not modify) -> list of M.frame dicts"""
    c = case(name); mc = c["max_coll"] if max_coll is None else max_coll
    return [M.frame(c["sv"][b], c["sf"], c["ov"][b], c["of"], c["sigma"], mc, dtype) for b in range(len(c["sv"]))]


def decided(name, max_coll=None):
    """frames without an undecided box-overlapping pair"""
    return [b for b, r in enumerate(reference(name, max_coll)) if not r["undecided"].any()]


def measure_e32(name, max_coll=None):
    """the float32 oracle's worst |error| / (u S) of a frame's value and gradient on the model's pair list, and the number of decided pairs on which its own
    decision differs from the model's"""
    r64 = reference(name, max_coll); r32 = reference(name, max_coll, np.float32); eV = eg = 0.0; differ = 0
    for a, o in zip(r64, r32):
        differ += int(((a["collide"] != o["collide"]) & ~a["undecided"]).sum())
        if a["pairs"]:
            t = M.pair_terms(a["S_kept"], a["O_kept"], case(name)["sigma"], np.float32)
            eV = max(eV, abs(float(t["v"].sum(dtype=np.float64)) - a["V"]) / (M.U * a["S_V"]))
            eg = max(eg, float(np.abs(t["g"].sum(0, dtype=np.float64) - a["g"]).max() / (M.U * a["S_g"])))
    return eV, eg, differ


# ---- running the kernels (GPU): d_obj_t, pairs_per_frame and the workspace are views into larger tensors with GUARD sentinel words before and after them; the
#      workspace is exactly vt_collision_workspace_bytes long and filled with 0xFF bytes.  The sentinels must keep their bits (checked here, on every run) ----------
def run(name, max_coll=None, gscale=1.0, frames=None, start=None, want_term=True, want_dt=True, want_pairs=True):
    """One call of vt_collision_loss on a case (frames: None = the whole batch, or a list of frame numbers).  start: None or (term0, dt0 (B, 3) float32).
    -> dict: term (float), dt (B, 3) float32, pairs (B) int32 (the start values / -1 where the pointer was NULL)"""
    import torch
    from vistracker_amd import _lib as L
    lib = L.lib(); c = case(name); mc = c["max_coll"] if max_coll is None else max_coll
    sel = slice(None) if frames is None else list(frames)
    sv = torch.from_numpy(np.ascontiguousarray(c["sv"][sel])).cuda(); ov = torch.from_numpy(np.ascontiguousarray(c["ov"][sel])).cuda()
    sf = torch.from_numpy(c["sf"]).cuda(); of = torch.from_numpy(c["of"]).cuda(); B = sv.shape[0]
    term0, dt0 = (0.0, np.zeros((B, 3), np.float32)) if start is None else start
    term = torch.full((1,), float(term0), dtype=torch.float64, device="cuda")
    g = torch.Generator().manual_seed(1)
    dfull = (torch.rand(3 * B + 2 * GUARD, generator=g) + 0.5).cuda(); dt = dfull[GUARD:GUARD + 3 * B]; dt.copy_(torch.from_numpy(np.ascontiguousarray(dt0)).reshape(-1))
    pfull = torch.full((B + 2 * GUARD,), -1, dtype=torch.int32, device="cuda"); pairs = pfull[GUARD:GUARD + B]
    nbytes = int(lib.vt_collision_workspace_bytes(B, sf.shape[0])); assert nbytes % 4 == 0
    wfull = torch.full((nbytes + 8 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda"); ws = wfull[4 * GUARD:4 * GUARD + nbytes]; assert ws.data_ptr() % 8 == 0
    dbefore = dfull.clone()
    L.check(lib.vt_collision_loss(sv.data_ptr(), sv.shape[1], sf.data_ptr(), sf.shape[0], ov.data_ptr(), ov.shape[1], of.data_ptr(), of.shape[0], B, float(c["sigma"]), int(mc),
                                  float(gscale), term.data_ptr() if want_term else None, dt.data_ptr() if want_dt else None, pairs.data_ptr() if want_pairs else None,
                                  ws.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    ok = lambda full, before, n: bool(torch.equal(full[:n], before[:n]) and torch.equal(full[-n:], before[-n:]))
    assert ok(dfull.view(torch.int32), dbefore.view(torch.int32), GUARD), "a sentinel word around d_obj_t changed"
    assert bool((pfull[:GUARD] == -1).all() and (pfull[-GUARD:] == -1).all()), "a sentinel word around pairs_per_frame changed"
    assert bool((wfull[:4 * GUARD] == 0xFF).all() and (wfull[-4 * GUARD:] == 0xFF).all()), "a sentinel word around the workspace changed"
    return dict(term=float(term.item()), dt=dt.cpu().numpy().reshape(B, 3).copy(), pairs=pairs.cpu().numpy().copy())


# ---- measuring (GPU): the figures that tests/test_gpu_collide.py asserts and tools/collide_perpair_report.py prints; nothing is asserted here ---------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def measure_case(name, mc=None, gscale=1.0, start=None, alone=True):
    """the batched call and (alone) every decided frame on its own against the model.  -> dict: the worst fractions of the gates (value, grad, term), wrong pair
    counts (pairs), frames left out as undecided (left_out), frames without pairs whose d_obj_t or term moved (moved), frames that alone differ from the frame
    in its batch (differ), and `line`, the figures in words"""
    c = case(name); fam = c["family"]; EV, Eg = E32[fam]; ref = reference(name, mc); B = len(ref); ok = decided(name, mc)
    term0, dt0 = (0.0, np.zeros((B, 3), np.float32)) if start is None else start
    out = run(name, mc, gscale, start=start)
    w = dict(pairs=0, grad=0.0, value=0.0, term=0.0, left_out=B - len(ok), moved=0, differ=0)
    tgate = M.U * abs(term0); want = term0
    for b, r in enumerate(ref):
        want += r["V"] / B; tgate += (M.value_gate(r, EV) + (M.slack(r, c["max_coll"] if mc is None else mc)[0] if b not in ok else 0)) / B
    for b in ok:
        r = ref[b]; w["pairs"] += int(out["pairs"][b] != r["pairs"])
        err = np.abs(out["dt"][b].astype(np.float64) - (dt0[b].astype(np.float64) + r["g"] * gscale / B))
        if r["pairs"] == 0:
            w["moved"] += int(not np.array_equal(_bits(out["dt"][b]), _bits(dt0[b])))
        else:
            w["grad"] = max(w["grad"], float((err / M.grad_gate(r, Eg, gscale, B, dt0[b] if start is not None else None)).max()))
    w["term"] = abs(out["term"] - want) / tgate if tgate > 0 else float(out["term"] != want)
    if alone:
        same = run(name, mc, float(B))                                     # gscale / B = 1: the same float conversion as a frame alone with gscale = 1
        for b in ok:
            r = ref[b]; o = run(name, mc, 1.0, frames=[b])
            w["differ"] += int(o["pairs"][0] != out["pairs"][b] or not np.array_equal(_bits(o["dt"][0]), _bits(same["dt"][b])))
            if r["pairs"] == 0:
                w["moved"] += int(o["term"] != 0.0)
            else:
                w["value"] = max(w["value"], abs(o["term"] - r["V"]) / M.value_gate(r, EV))
                w["grad"] = max(w["grad"], float((np.abs(o["dt"][0].astype(np.float64) - r["g"]) / M.grad_gate(r, Eg, 1.0, 1)).max()))
    w["line"] = ("%s max_coll %s gscale %g%s: %d frames (%d left out), wrong pair counts %d, worst value %.3f of its gate, worst gradient %.3f, batched term %.3f"
                 % (name, mc, gscale, " +start" if start is not None else "", B, w["left_out"], w["pairs"], w["value"], w["grad"], w["term"]))
    return w


def measure_fit_like():
    """fit_like against the resolutions of its undecided pairs.  -> (frames, term): per frame a dict -- pairs, the model's count and the range lo..hi the undecided
    pairs allow, matched (a resolution with the kernel's count exists), value / grad = error as a fraction of the arithmetic gate of the nearest such resolution,
    relV / relg = those gates relative to V and to the largest gradient component, slackV / slackg = what the undecided pairs can change, in the same units,
    in_slack (the slack form of the gate holds), differ (the frame alone differs from the frame in its batch); term = the batched term's error / gate"""
    name = "fit_like"; EV, Eg = E32[name]; ref = reference(name); B = len(ref); batch = run(name, None, float(B)); term = 0.0; tgate = 0.0; frames = []
    for b, r in enumerate(ref):
        o = run(name, None, 1.0, frames=[b]); V = o["term"]; g = o["dt"][0].astype(np.float64); sV, sg, lo, hi = M.slack(r, 8)
        fr = [(q, abs(V - q["V"]) / M.value_gate(q, EV), float((np.abs(g - q["g"]) / M.grad_gate(q, Eg, 1.0, 1)).max())) for q in M.resolutions(r, 8) if q["pairs"] == o["pairs"][0]]
        q, fV, fg = min(fr, key=lambda t: max(t[1], t[2])) if fr else (r, np.inf, np.inf)
        frames.append(dict(pairs=int(o["pairs"][0]), model=r["pairs"], lo=lo, hi=hi, undecided=int(r["undecided"].sum()), matched=bool(fr), value=fV, grad=fg,
                           relV=M.value_gate(q, EV) / q["V"], relg=float(M.grad_gate(q, Eg, 1.0, 1).max() / np.abs(q["g"]).max()),
                           slackV=sV / r["V"], slackg=float(sg.max() / np.abs(r["g"]).max()),
                           in_slack=bool(lo <= o["pairs"][0] <= hi and abs(V - r["V"]) <= M.value_gate(r, EV) + sV and (np.abs(g - r["g"]) <= M.grad_gate(r, Eg, 1.0, 1) + sg).all()),
                           differ=bool(o["pairs"][0] != batch["pairs"][b] or not np.array_equal(_bits(o["dt"][0]), _bits(batch["dt"][b])))))
        term += q["V"] / B; tgate += M.value_gate(q, EV) / B
    return frames, abs(run(name)["term"] - term) / tgate
