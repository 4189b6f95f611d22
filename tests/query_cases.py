"""The cases of the per-point pin of the SIF-Net point query (tests/test_host_query_model.py on the CPU oracle, tests/test_gpu_query_perpoint.py on the kernels),
each aimed at one mechanism of query_kernel<G, MODE, USEP> / query_f32.hip, and the evaluation both tests share: a BACKEND (the float32 oracle, or the C ABI on
the GPU) answers a case's operations, evaluate() expresses every output of every point as |got - model| / (u S) against tests/query_model.py.

Feature maps are synthetic.feature_maps at res_scale 1/8 (16 / 32 texels), decoders synthetic.sifnet_decoders; B <= 3."""
import numpy as np

import query_model as Q

FAMILIES = ("tiles", "goexp", "borders", "fused", "gain")
EXACT_CAM = (1024.0, 1024.0, 0.0, 0.0, 1024.0)     # with crop_center (512, 512) and z = 2: nx = x - 1, ny = y - 1, every intermediate exact in float32 in any order
W_DFH, W_PART, W_OBJ, W_ACCEL = 100.0, 0.0025, 900.0, 37.5
GAIN = 8.0                                          # sifnet_decoders(gain=GAIN): activations of the last hidden layer beyond 1023 (level 0) and below 16 368 (level 1)

# Worst error of the float32 ORACLE (oracle.oracle.SifNet on the CPU) against the model, in units of u S, per family and kind of output -- measured by
# tests/test_host_query_model.py::test_oracle32_meets_every_gate, which fails if the oracle exceeds a figure here; tests/golden/query_perpoint.md has the measurements.
# The GPU gate is GATE x these, on both routes; the split-f16 route adds GATE x E_SPLIT, the measured error of the split-operand emulation (same file).
E32 = {
    "tiles":   dict(value=0.0038, dpts=0.07),
    "goexp":   dict(value=0.004, dpts=0.045),
    "borders": dict(value=0.0024, dpts=0.026),
    "fused":   dict(value=0.0036, dpts=0.034, point=0.016),
    "gain":    dict(value=0.0026, dpts=0.23, point=0.0125),
}
# Per range level (vt_maps::act_level): the rescaling of the operands by 16^-level is exact, the split of the rescaled number into two float16 halves is not -- at level 2
# the lo half of an operand of ordinary size is a float16 subnormal (absolute spacing 2^-24) and the operand keeps fewer than 22 bits.  The level-aware emulation
# (query_model.emu_decoder with operand_scales) measures it; on an MI355X the values at level 2 sit where it predicts (tests/golden/query_perpoint.md).
E_SPLIT = {0: dict(value=0.00115, dpts=0.033, point=0.03415), 1: dict(value=0.0017, dpts=0.033, point=0.0347), 2: dict(value=0.037, dpts=0.033, point=0.07)}
MAX_EXCLUDED = 0.02                                 # of a case's points may sit within float32 reach of a kink; none of the placed ones


def gate(family, kind, route, level=0):
    g = Q.GATE * E32[family][kind]
    return g + Q.GATE * E_SPLIT[level][kind] if route == "split-f16" else g


class Case:
    def __init__(self, name, family, pts, cc, bc, map_seed, cam=Q.DEFAULT_CAM, gain=1.0, placed=None, **extra):
        self.name, self.family = name, family
        self.pts = np.ascontiguousarray(pts, np.float32); self.cc = np.ascontiguousarray(cc, np.float32); self.bc = np.ascontiguousarray(bc, np.float32)
        self.B, self.N = self.pts.shape[:2]
        self.map_seed, self.cam, self.gain = map_seed, cam, gain
        self.placed = np.zeros((self.B, self.N), bool) if placed is None else placed
        self.__dict__.update(extra)

    _maps, _dec = {}, {}

    def maps(self):
        from vistracker_amd import synthetic as syn
        k = (self.B, self.map_seed)
        if k not in Case._maps:
            Case._maps[k] = syn.feature_maps(self.B, self.map_seed, res_scale=1 / 8)
        return Case._maps[k]

    def decoders(self):
        from vistracker_amd import synthetic as syn
        if self.gain not in Case._dec:
            Case._dec[self.gain] = syn.sifnet_decoders(3, gain=self.gain)
        return Case._dec[self.gain]

    def model(self, mutant=None):
        return Q.QueryModel(self.decoders(), self.maps(), self.cam, mutant=mutant)


def _random_inputs(B, N, seed):
    rng = np.random.default_rng(seed)
    pts = rng.normal(0, 0.3, (B, N, 3)) + [0, 0, 2.2]
    cc = np.array([[1018.952, 779.486]]) + rng.normal(0, 30, (B, 2))          # a different crop and body centre per frame
    bc = np.array([[0, 0, 2.2]]) + rng.normal(0, 0.1, (B, 3))
    return rng, pts, cc, bc


def tile_edges(N):
    """first and last point of every 64-point tile and of the frame"""
    return sorted({n for t in range(0, N, 64) for n in (t, min(t + 63, N - 1))})


def _edges_mask(B, N):
    m = np.zeros((B, N), bool); m[:, tile_edges(N)] = True
    return m


# ---- tile edges, every head alone and the pairs the launcher forms --------------------------------------------------------------------------------------------
PAIRS = ((0, 2), (1, 4))          # vt_query_backward with (d_df, d_parts) and (d_pca, d_vis): the G = 2 instantiation


def tiles_case(N, seed=None):
    if seed is None:
        seed = {1: 201, 63: 202, 64: 203, 65: 208, 150: 204}[N]       # the first seeds that keep the kink exclusions under the cap (host test)
    rng, pts, cc, bc = _random_inputs(2, N, seed)
    g = {h: rng.normal(0, 1, (2, k, N)).astype(np.float32) for h, k in enumerate(Q.HEAD_DIMS)}
    return Case("tiles-N%d" % N, "tiles", pts, cc, bc, 21, placed=_edges_mask(2, N), g=g)


# ---- upstream gradients spanning 2^-20 .. 2^10 within one tile: the per-point normalisation ---------------------------------------------------------------------
def goexp_case(seed=301):
    B, N = 1, 70
    rng, pts, cc, bc = _random_inputs(B, N, seed)
    g = {}
    for h, k in enumerate(Q.HEAD_DIMS):
        per_point = np.ldexp(1.0, rng.integers(-20, 11, (B, 1, N)))             # per point ...
        per_out = np.ldexp(1.0, rng.integers(-6, 1, (B, k, N)))                 # ... and per output of the head
        g[h] = (rng.normal(0, 1, (B, k, N)) * per_point * per_out).astype(np.float32)
        g[h][0, :, 10] = np.ldexp(rng.choice([-1.0, 1.0], k), 10)               # 2^10 ...
        g[h][0, :, 11] = 0.0                                                    # ... next to exactly zero: its dpts must be exactly zero
        g[h][0, :, 12] = np.ldexp(rng.normal(0, 1, k), -20)
    placed = np.zeros((B, N), bool); placed[0, 10:13] = True
    return Case("goexp", "goexp", pts, cc, bc, 22, placed=placed, g=g, zero_point=(0, 11))


# ---- image and grid borders, placed exactly ----------------------------------------------------------------------------------------------------------------------
def borders_case(seed=121):
    """EXACT_CAM, crop_center (512, 512), body_center 0, z = 2: nx = x - 1, ny = y - 1; triplane coordinates right (z, y), back (-x, y), top (x, -z) are the point's
    own coordinates.  The placed coordinates are dyadic, so float32 and float64 evaluate the same texel coordinate and the same floor.  (A texel strictly inside a
    map cannot be hit exactly: (g + 1) (W - 1) / 2 is an integer m only for g = 2 m / 15 - 1 or 2 m / 31 - 1, not a float32 number for 0 < m < W - 1.  The first and
    the last texel, g = -1 and g = +1, can.)"""
    st = 2.0 ** -23
    P = [  # (x, y, z), what it places
        (0.0, 1.0, 2.0),            # nx = -1 exactly (in the image); back u = 0
        (2.0, 1.0, 2.0),            # nx = +1 exactly (in the image); back u = -2: beyond the map, all four taps padded
        (1.0, 0.0, 2.0),            # ny = -1 exactly
        (1.0, 2.0, 2.0),            # ny = +1 exactly
        (-st, 1.0, 2.0),            # nx = -1 - 2^-23: one float32 step outside
        (2.0 + 2 * st, 1.0, 2.0),   # nx = +1 + 2^-22: the smallest step outside +1 that every float32 evaluation order of the projection carries exactly
        (1.0, -st, 2.0),            # ny one step outside
        (1.0, 1.0, 1.0),            # right (z, y) = (1, 1): the last texel of both axes, three taps padded (weight 0 on them: value of the texel, one-sided gradient)
        (-1.0, 1.0, 1.0),           # back (-x, y) = (1, 1), top (x, -z) = (-1, -1): the first texel; nx = -3: outside
        (1.0, -1.0, 1.0),           # right (1, -1), back (-1, -1): first / last texel mixed
        (1.0 + 2.0 ** -4, 0.25, 1.0),        # top u = 1 + 2^-4: half a texel beyond the last one: two taps padded
        (1.0 + 2.0 ** -4, 0.25, -1.0 - 2.0 ** -4),   # top (1 + 2^-4, 1 + 2^-4): one tap left
        (1.25, 0.25, 1.0),          # top u = 1.25: more than a texel beyond: all four padded
        (0.5, 0.5, -1.0),           # right u = -1 exactly: first texel column
    ]
    n_placed = len(P); B, N = 1, 24
    rng = np.random.default_rng(seed)
    zr = rng.uniform(0.5, 0.95, N - n_placed)                                   # the rest: in the image (0 < x, y < z) and inside the three maps (|x|, |y|, |z| < 1)
    rest = np.stack([zr * rng.uniform(0.05, 0.95, N - n_placed), zr * rng.uniform(0.05, 0.95, N - n_placed), zr], -1)
    pts = np.concatenate([np.array(P), rest])[None]
    placed = np.zeros((B, N), bool); placed[0, :n_placed] = True
    g = {h: rng.normal(0, 1, (B, k, N)).astype(np.float32) for h, k in enumerate(Q.HEAD_DIMS)}
    outside = np.zeros((B, N), bool); outside[0, [4, 5, 6, 8, 9, 10, 11, 12, 13]] = True
    inside_exact = np.zeros((B, N), bool); inside_exact[0, [0, 1, 2, 3, 7]] = True
    return Case("borders", "borders", pts, [[512.0, 512.0]], [[0.0, 0.0, 0.0]], 23, cam=EXACT_CAM, placed=placed, g=g, outside=outside, inside_exact=inside_exact)


# ---- the fused objectives: clamp edges, `order`, the hoisted projection, the projection step, the human step --------------------------------------------------------
def fused_case(gain=1.0, seed=None, N=150):
    """B = 3 (the acceleration term needs three frames), N = 150.  Tile 1 (points 64..127) of frame 0 is ARRANGED from a pool of candidates by the model's own df:
    63 points past the clamp of the human term (df[:, 0] > 0.1) and one point, at position 100, below it; the points past / below / far beyond (outside the image)
    the clamps of the other tiles are whatever the random positions give; tests/test_host_query_model.py asserts a minimum count of every class (clamp_classes)."""
    B = 3; seed = (401 if gain == 1.0 else 418) if seed is None else seed
    rng, pts, cc, bc = _random_inputs(B, N, seed)
    c = Case("tmp", "fused", pts, cc, bc, 24, gain=gain)
    pool = rng.normal(0, 0.3, (B, 1500, 3)) + [0, 0, 2.2]
    fw = Case("tmp", "fused", pool, cc, bc, 24, gain=gain).model().forward(np.float32(pool), c.cc, c.bc, heads=(0,))
    d0 = fw["df"][0, 0]; ok = fw["in_img"][0]
    above = np.flatnonzero(ok & (d0 > 0.15))[:64]; below = np.flatnonzero(ok & (d0 < 0.05))[:1]
    assert len(above) == 64 and len(below) == 1
    pts[0, 64:128] = pool[0, above]; pts[0, 100] = pool[0, below[0]]
    pts[1, :3, 0] += 3.0                                                        # three points outside the image: df = 5.0, far beyond both clamps
    placed = np.zeros((B, N), bool); placed[0, 100] = True; placed[1, :3] = True
    labels = rng.integers(0, 14, N).astype(np.int32); occ = rng.uniform(0.3, 1, B).astype(np.float32)
    orders = dict(identity=None, random=rng.permutation(N).astype(np.int32), reversed=np.arange(N - 1, -1, -1).astype(np.int32))
    base = rng.normal(0, 1e-3, (B, N, 3)).astype(np.float32)                    # what vt_query_human_step accumulates onto
    return Case("fused" if gain == 1.0 else "gain", "fused" if gain == 1.0 else "gain", pts, cc, bc, 24, gain=gain, placed=placed, labels=labels, occ=occ, orders=orders,
                base=base, lonely=(0, 100))


def all_cases():
    return [tiles_case(N) for N in (1, 63, 64, 65, 150)] + [goexp_case(), borders_case(), fused_case(), fused_case(gain=GAIN)]


# ---- evaluation ----------------------------------------------------------------------------------------------------------------------------------------------------
class Record:
    """one output array of one operation: units = |got - model| / (u S) per element, gated = the elements the gate applies to"""
    def __init__(self, case, op, kind, got, ref, S, gated=None, old_rel=None, allow=None):
        self.case, self.op, self.kind = case, op, kind
        if allow is None:
            self.units = Q.units(got, ref, S)
        else:           # allow: an absolute error that roundings OUTSIDE the network add whatever the network's own error is -- derived from the format, taken off first
            self.units = Q.units(ref + np.maximum(np.abs(np.asarray(got, np.float64) - ref) - allow, 0.0), ref, S)
        self.gated = np.ones(self.units.shape, bool) if gated is None else np.broadcast_to(gated, self.units.shape)
        self.level = 0                  # vt_maps::act_level of the call (evaluate sets it)
        self.old_rel = old_rel          # what the whole-array metric of test_gpu_parity.py sees, and its bar there
        self.got, self.ref = np.asarray(got), ref

    def worst(self):
        return float(self.units[self.gated].max()) if self.gated.any() else 0.0


def exact_coords(case, margins):
    """the placed points of the border case have dyadic coordinates: every float32 evaluation order of the projections computes them exactly, so float32 takes
    the float64 branch however close the coordinate is to it (the host test holds the float32 oracle's gradient at these points to the gate: the same cell)"""
    return dict(margins, coord=np.where(case.placed, np.inf, margins["coord"])) if case.family == "borders" else margins


def _pt(mask):
    return mask[..., None]          # (B, N) -> (B, N, 1) for dpts


def evaluate(case, be, route="fp32", mutant=None, fused_opts=None, level=0):
    """-> records, terms [(op, err, gate)], exact [(what, bool)].  `be`: forward(case, heads, level) -> {head: (B, k, N)}, backward(case, {head: g}, level) -> dpts, and
    for the fused families human_loss / object_loss / project_step (see OracleBackend).  `level`: vt_maps::act_level of the plain forward / backward (an exact power-of-two
    rescaling of the operands: the same model, the same gate; the CPU backends have no such thing).  `mutant` replaces the BACKEND by the model with that defect."""
    M = case.model(); recs, terms, exact = [], [], []
    if mutant is not None:
        be = ModelBackend(mutant)
    B, N = case.B, case.N
    if case.family in ("tiles", "goexp", "borders"):
        fw = M.forward(case.pts, case.cc, case.bc)
        excl = lambda mg: Q.excluded(exact_coords(case, mg)); lv = " level=%d" % level if level else ""
        for heads in ((0, 1, 2, 3, 4), (0, 2)):                                   # all five outputs, and outputs 1, 3, 4 NULL
            got = be.forward(case, heads, level)
            for h in heads:
                n = Q.HEADS[h]
                recs.append(Record(case, "fwd%s:%s%s" % (len(heads), n, lv), "value", got[h], fw[n], fw["S_" + n], old_rel=(np.abs(got[h] - fw[n]).max() / max(1.0, np.abs(fw[n]).max()), 5e-6)))
            exact.append(("df == 5.0 bit for bit outside the image", all(bool((np.asarray(got[0])[b][:, ~fw["in_img"][b]] == 5.0).all()) for b in range(B))))
        single = {}
        for h in range(5):
            fh = M.forward(case.pts, case.cc, case.bc, heads=(h,)); ok = ~excl(fh["margins"])
            ref, S = M.backward(fh, {h: case.g[h]}); got = be.backward(case, {h: case.g[h]}, level); single[h] = (ref, S, ok, got)
            recs.append(Record(case, "bwd:" + Q.HEADS[h] + lv, "dpts", got, ref, S, _pt(ok), old_rel=(Q.rel(got, ref), 5e-6)))
        for (ha, hb) in PAIRS:
            # head B's gradients 2^10 times head A's.  The kernel adds both heads into one dpts, so: the pair call against the sum, on the sum of the two own scales;
            # the small head on its own scale in a second call of the SAME two-head kernel with a zero gradient for the large head.
            gb = (case.g[hb] * np.float32(1024.0)).astype(np.float32)
            fp = M.forward(case.pts, case.cc, case.bc, heads=(ha, hb)); ok = ~excl(fp["margins"])
            ref, S = M.backward(fp, {ha: case.g[ha], hb: gb}); got = be.backward(case, {ha: case.g[ha], hb: gb}, level)
            recs.append(Record(case, "bwd:%s+1024 %s%s" % (Q.HEADS[ha], Q.HEADS[hb], lv), "dpts", got, ref, S, _pt(ok), old_rel=(Q.rel(got, ref), 5e-6)))
            refa, Sa = M.backward(fp, {ha: case.g[ha], hb: np.zeros_like(gb)}); gota = be.backward(case, {ha: case.g[ha], hb: np.zeros_like(gb)}, level)
            recs.append(Record(case, "bwd:%s+0 %s%s" % (Q.HEADS[ha], Q.HEADS[hb], lv), "dpts", gota, refa, Sa, _pt(ok), old_rel=(Q.rel(gota, refa), 5e-6)))
            # linearity: pair - small head alone = the large head alone.  Both calls carry their own errors into the difference, so its scale is the sum of the
            # two calls' own scales (about the large head's own where it is 2^10 times the small one's)
            refb, Sb, okb, _ = single[hb]
            recs.append(Record(case, "bwd:pair-small=1024 %s%s" % (Q.HEADS[hb], lv), "dpts", np.float64(got) - np.float64(gota), 1024.0 * refb, S + Sa,
                               _pt(ok & okb)))
        if case.family == "goexp":
            b, n = case.zero_point
            for h in range(5):
                exact.append(("zero upstream gradient gives exactly zero dpts (%s)" % Q.HEADS[h], bool((np.asarray(single[h][3])[b, n] == 0).all())))
        if case.family == "borders":
            fd = M.forward(case.pts, case.cc, case.bc, heads=(0,))
            assert (fd["in_img"][case.inside_exact]).all() and np.array_equal(~fd["in_img"][case.placed], case.outside[case.placed])
            exact.append(("zero df gradient outside the image", bool((np.asarray(single[0][3])[case.outside] == 0).all())))
            exact.append(("parts keeps a gradient outside the image", bool((np.abs(np.asarray(single[2][3])[case.outside]).max(-1) > 0).all())))
        for r in recs:
            r.level = level
        return recs, terms, exact

    # fused families
    opts = fused_opts or [dict(order="identity", proj=False)]
    for o in opts:
        vg = gate(case.family, "value", route, o.get("level", 0)); n0 = len(recs)
        tag = "[order=%s proj=%d level=%d]" % (o["order"], o.get("proj", False), o.get("level", 0))
        od = case.orders[o["order"]]
        hm = M.human_loss(case.pts, case.cc, case.bc, case.labels, W_DFH, W_PART); ok = ~Q.excluded(hm["margins"], vg)
        got, t = be.human_loss(case, od, o)
        recs.append(Record(case, "human" + tag, "dpts", got, hm["dpts"], hm["S"], _pt(ok), old_rel=(Q.rel(got, hm["dpts"]), 3e-4)))
        for k in range(2):
            terms.append(("human" + tag + " term %d" % k, abs(t[k] - hm["terms"][k]), Q.term_gate(B * N, hm["summands"][k], hm["s_summands"][k], vg)))
        if "step" in o:
            # vt_query_human_step = the human gradient + the acceleration stencil's (+ what dpts held).  The network part keeps the dpts gate on ITS scale; what the float32
            # arithmetic around it adds whatever the network's error is comes off first, derived from the format: the stencil's gradient carries at most 6 roundings
            # relative to its own terms (three in a = (v1 - v0) - (v2 - v1), one in the product with the weight, two where three a's meet in one element), and the result
            # is the float32 sum of up to three numbers -- two additions, each within u of a partial sum no larger than |base| + |human| + |stencil|
            ta, ga, Sa, ta_abs = Q.accel(case.pts.reshape(B, -1), W_ACCEL); ga, Sa = ga.reshape(B, N, 3), Sa.reshape(B, N, 3)
            for acc in (0, 1):
                base = case.base.astype(np.float64) if acc else np.zeros((B, N, 3))
                ref = hm["dpts"] + ga + base
                allow = Q.U * (6 * Sa + 2 * (np.abs(base) + np.abs(hm["dpts"]) + np.abs(ga)))
                got, t, tacc = be.human_step(case, od, o, acc)
                recs.append(Record(case, "human_step acc=%d" % acc + tag, "dpts", got, ref, hm["S"], _pt(ok), allow=allow))
                terms.append(("human_step acc=%d" % acc + tag + " accel term", abs(tacc - ta), (3 * N * (B - 2) + 8) * Q.U * ta_abs))
                for k in range(2):
                    terms.append(("human_step acc=%d" % acc + tag + " term %d" % k, abs(t[k] - hm["terms"][k]), Q.term_gate(B * N, hm["summands"][k], hm["s_summands"][k], vg)))
        ob = M.object_loss(case.pts, case.cc, case.bc, case.occ, W_OBJ); oko = ~Q.excluded(ob["margins"], vg)
        got, t = be.object_loss(case, o)
        recs.append(Record(case, "object" + tag, "dpts", got, ob["dpts"], ob["S"], _pt(oko), old_rel=(Q.rel(got, ob["dpts"]), 3e-4)))
        exact.append(("object: the gradient of a clamped point is exactly zero" + tag, bool((np.asarray(got)[~ob["live"]] == 0).all())))
        terms.append(("object" + tag + " term", abs(t[0] - ob["terms"][0]), Q.term_gate(B * N, ob["summands"][0], ob["s_summands"][0], vg)))
        for idx, thr in ((0, 0.5), (1, 1.0)):
            pj = M.project_step(case.pts, case.cc, case.bc, idx, thr); okp = ~Q.excluded(pj["margins"], vg)
            out, tgt = be.project_step(case, idx, thr, o)
            recs.append(Record(case, "project idx=%d" % idx + tag + " target", "value", tgt, pj["target"], pj["S_target"]))
            recs.append(Record(case, "project idx=%d" % idx + tag + " point", "point", out, pj["out"], pj["S"], _pt(okp & pj["live"])))
            exact.append(("project: a clamped point does not move" + tag, bool((np.asarray(out)[~pj["live"]] == case.pts[~pj["live"]]).all())))
        for r in recs[n0:]:
            r.level = o.get("level", 0)
    # the human term with w_part = 0: the gradient of a point past the clamp is exactly zero, and the one point below it among 63 clamped neighbours is held to ITS scale
    hm0 = M.human_loss(case.pts, case.cc, case.bc, case.labels, W_DFH, 0.0); vg = gate(case.family, "value", route, opts[0].get("level", 0))
    got, _ = be.human_loss(case, None, dict(opts[0], w_part=0.0))
    exact.append(("human: the gradient of a clamped point is exactly zero", bool((np.asarray(got)[~hm0["live"]] == 0).all())))
    b, n = case.lonely
    assert hm0["live"][b, n] and not hm0["live"][b, 64:128].sum() > 1
    recs.append(Record(case, "human w_part=0", "dpts", got, hm0["dpts"], hm0["S"], _pt(~Q.excluded(hm0["margins"], vg)))); recs[-1].level = opts[0].get("level", 0)
    return recs, terms, exact


def clamp_classes(case):
    """how many points of a fused case sit in each class of the two clamps: in the image below / past the threshold, and outside the image (df = 5.0, far beyond)"""
    fw = case.model().forward(case.pts, case.cc, case.bc, heads=(0,)); ins = fw["in_img"]
    return dict(human_below=int((ins & (fw["df"][:, 0] <= Q.THR_HUMAN)).sum()), human_past=int((ins & (fw["df"][:, 0] > Q.THR_HUMAN)).sum()),
                object_below=int((ins & (fw["df"][:, 1] <= Q.THR_OBJECT)).sum()), object_past=int((ins & (fw["df"][:, 1] > Q.THR_OBJECT)).sum()), outside=int((~ins).sum()))


def excluded_fraction(case, route="split-f16"):
    """per operation kind: the fraction of the case's points within float32 reach of a kink, and whether a placed point is among them"""
    M = case.model(); vg = gate(case.family, "value", route, 2) if case.family in ("fused", "gain") else 0.0          # the widest clamp margin: level 2
    if case.family in ("fused", "gain"):
        ex = [Q.excluded(M.human_loss(case.pts, case.cc, case.bc, case.labels, W_DFH, W_PART)["margins"], vg),
              Q.excluded(M.object_loss(case.pts, case.cc, case.bc, case.occ, W_OBJ)["margins"], vg)] + \
             [Q.excluded(M.project_step(case.pts, case.cc, case.bc, i, t)["margins"], vg) for i, t in ((0, 0.5), (1, 1.0))]
    else:
        ex = [Q.excluded(exact_coords(case, M.forward(case.pts, case.cc, case.bc, heads=hs)["margins"])) for hs in [(h,) for h in range(5)] + list(PAIRS)]
    return max(float(e.mean()) for e in ex), bool(any((e & case.placed).any() for e in ex))


# ---- backends on the CPU -------------------------------------------------------------------------------------------------------------------------------------------
def loss_head_human(df, parts, labels, w_dfh, w_part):
    """the fused human objective on given network outputs, float64 arithmetic on the values as given -> terms, d_df, d_parts (recon_fit_base.py:640-647)"""
    B, _, N = df.shape; d = np.asarray(df[:, 0], np.float64)
    g_df = np.zeros(df.shape); g_df[:, 0] = (np.asarray(df[:, 0]) <= np.float32(0.1)) * (w_dfh / (B * N))
    lg = np.asarray(parts, np.float64); mx = lg.max(1, keepdims=True); lse = np.log(np.exp(lg - mx).sum(1)) + mx[:, 0]
    lab = np.broadcast_to(np.asarray(labels)[None], (B, N))
    ce = lse - np.take_along_axis(lg, lab[:, None], 1)[:, 0]
    sm = np.exp(lg - lse[:, None]); np.put_along_axis(sm, lab[:, None], np.take_along_axis(sm, lab[:, None], 1) - 1, 1)
    return np.array([np.minimum(d, np.float32(0.1)).mean(), ce.sum(1).mean()]), g_df, sm * (w_part / B)


class OracleBackend:
    """the CPU oracle (oracle.oracle = float32, oracle.oracle64 = float64) behind the interface of evaluate(); the fused objectives are its forward, the loss head
    above and its backward, as in tests/test_gpu_parity.py::test_query_fused_objectives_vs_oracle"""
    def __init__(self, O):
        self.O = O; self._nets = {}

    def net(self, case):
        k = (case.B, case.map_seed, case.gain, tuple(case.cam))
        if k not in self._nets:
            self._nets[k] = self.O.SifNet(case.decoders(), case.maps(), cam=np.asarray(case.cam, np.float32))
        return self._nets[k]

    def forward(self, case, heads, level=0):
        outs = self.net(case).query(case.pts, case.cc, case.bc, head_mask=sum(1 << h for h in heads))
        return {h: outs[h] for h in heads}

    def backward(self, case, g, level=0):
        return self.net(case).query_bwd(case.pts, case.cc, case.bc, **{"d_" + Q.HEADS[h]: v for h, v in g.items()})

    def human_loss(self, case, order, o):
        df, _, parts, _, _ = self.net(case).query(case.pts, case.cc, case.bc, head_mask=5)
        t, g_df, g_parts = loss_head_human(df, parts, case.labels, W_DFH, o.get("w_part", W_PART))
        return self.backward(case, {0: g_df.astype(np.float32), 2: g_parts.astype(np.float32)}), t

    def object_loss(self, case, o):
        df = self.net(case).query(case.pts, case.cc, case.bc, head_mask=1)[0]; B, _, N = df.shape
        g = np.zeros(df.shape, np.float32); g[:, 1] = (df[:, 1] <= np.float32(0.8)) * (case.occ[:, None].astype(np.float64) * W_OBJ / (B * N))
        return self.backward(case, {0: g}), np.array([(np.minimum(df[:, 1], np.float32(0.8)).astype(np.float64).mean(-1) * case.occ).mean()])

    def human_step(self, case, order, o, acc):
        d, t = self.human_loss(case, order, o); dv = (case.base.copy() if acc else np.zeros_like(case.base)).astype(self.O.REAL) + d
        ta = self.O.accel_loss(case.pts.reshape(case.B, -1), None, W_ACCEL, dv.reshape(case.B, -1))
        return dv, t, ta

    def project_step(self, case, idx, thr, o):
        x, tgt = self.O.approx_surface(self.net(case), case.pts, 1, case.cc, case.bc, idx, threshold=thr)
        return x, tgt


class ModelBackend:
    """the model with one deliberate defect, behind the same interface: what a kernel with that defect would return"""
    def __init__(self, mutant):
        self.mutant = mutant

    def forward(self, case, heads, level=0):
        fw = case.model(self.mutant).forward(case.pts, case.cc, case.bc, heads=heads)
        return {h: fw[Q.HEADS[h]] for h in heads}

    def backward(self, case, g, level=0):
        M = case.model(self.mutant)
        return M.backward(M.forward(case.pts, case.cc, case.bc, heads=tuple(g)), g)[0]

    def human_loss(self, case, order, o):
        M = case.model(self.mutant); r = M.human_loss(case.pts, case.cc, case.bc, case.labels, W_DFH, o.get("w_part", W_PART))
        return M.apply_order_mutant(r["dpts"], order), r["terms"]

    def object_loss(self, case, o):
        r = case.model(self.mutant).object_loss(case.pts, case.cc, case.bc, case.occ, W_OBJ)
        return r["dpts"], r["terms"]

    def project_step(self, case, idx, thr, o):
        r = case.model(self.mutant).project_step(case.pts, case.cc, case.bc, idx, thr)
        return r["out"], r["target"]
