"""Float64 model of the human/object interpenetration term (vistracker_amd/csrc/collide.hip, survey row A21), restated from the published definition (Tzionas et al.,
IJCV 2016; the formulas in the header comment of collide.hip), not from collide_geom.h.

Pair decision: the separating-axis test over the 11 axes of two triangles (2 normals, 9 edge cross products), in float64 on the float32 corners.  margin() is signed and
in metres: the smallest overlap over the axes if none separates (the penetration depth along the best of these axes), minus the largest gap otherwise.  The product's
conventions: a pair whose boxes do not overlap is never tested, a coplanar pair and a pair with a zero-area triangle do not collide.  A pair is UNDECIDED when
|margin| < TAU = 64 u max|coordinate| (u = 2^-24): float32 arithmetic on coordinates of that size cannot be asked to take the float64 decision there.

Pair list: per object face the first max_coll colliding SMPL faces in face order.

Value of a frame:  V = sum over kept pairs (f_s, f_o) of  sum_{v in f_o} Psi_{f_s}(v)^2 + sum_{v in f_s} Psi_{f_o}(v)^2,   Psi_f(v) = ((1 - Phi) Upsilon(x))^2 inside the cone.
dV/dt for one translation t of all object vertices with the pair list fixed, twice: analytically (object intruders move with t; an object cone moves with t, which is minus
the derivative at the SMPL vertex) and by torch float64 autograd through the whole expression, circumcentre, normal and radius of the moved object triangles included.

Error scales, from model quantities only (cmax = largest |coordinate| of the pair; the sums run over the live (pair, side, vertex) triples):
  S_V = V + sum |dPsi^2/dv|_1 cmax
  S_g = sum |dPsi^2/dv|_1 (1 / (Dn (1 - Phi)) + 1 / rho + 1 / r) cmax          (a vertex with rho = 0 has no 1 / rho: only its n part enters the gradient)
dtype = numpy.float32 evaluates the same formulas in float32: the float32 CPU oracle that E32 is measured from (it is not the product's header)."""
import itertools

import numpy as np

U = 2.0 ** -24
QFIX = 2.0 ** -41                     # half a unit of the 2^40 fixed-point accumulators, per object face that adds into them
APEX, OUTSIDE, LINEAR, QUAD = 0, 1, 2, 3          # branch of one (receiver triangle, intruder vertex): Dn <= 0 | Phi >= 1 | live, x <= -sigma | live, -sigma < x < sigma


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def tau(A, B):
    return 64 * U * np.maximum(np.abs(A).max((1, 2)), np.abs(B).max((1, 2))).astype(np.float64)


def margin(A, B, dtype=np.float64):
    """A, B (N, 3, 3) triangles.  -> margin (N) in metres, coplanar (N) bool, degenerate (N) bool"""
    A = A.astype(dtype); B = B.astype(dtype)
    eA = [A[:, 1] - A[:, 0], A[:, 2] - A[:, 1], A[:, 0] - A[:, 2]]; eB = [B[:, 1] - B[:, 0], B[:, 2] - B[:, 1], B[:, 0] - B[:, 2]]
    nA, nB = _cross(eA[0], eA[1]), _cross(eB[0], eB[1])
    axes = np.stack([nA, nB] + [_cross(a, b) for a in eA for b in eB], 1)                                        # (N, 11, 3)
    ref = np.stack([_dot(eA[0], eA[0]) + _dot(eA[1], eA[1]), _dot(eB[0], eB[0]) + _dot(eB[1], eB[1])] + [np.sqrt(_dot(a, a) * _dot(b, b)) for a in eA for b in eB], 1)
    ln = np.sqrt(_dot(axes, axes))
    valid = ln > 1e-6 * ref                            # an edge pair closer to parallel than 1e-6 rad gives no axis of its own (the normals cover it)
    unit = axes / np.where(valid, ln, 1)[..., None]
    pA = np.einsum("nak,nvk->nav", unit, A); pB = np.einsum("nak,nvk->nav", unit, B)
    over = np.minimum(pA.max(2) - pB.min(2), pB.max(2) - pA.min(2))            # the shift along the axis that separates the two intervals; negative: the gap
    m = np.where(valid, over, np.inf).min(1)
    degenerate = (_dot(nA, nA) == 0) | (_dot(nB, nB) == 0)
    dA = np.abs(pA[:, 1] - pB[:, 1, :1]).max(1); dB = np.abs(pB[:, 0] - pA[:, 0, :1]).max(1)                      # distances to the other triangle's plane
    coplanar = ~degenerate & (np.maximum(dA, dB) < tau(A, B))
    return m, coplanar, degenerate


def decide(A, B, dtype=np.float64):
    """-> collide (N) bool, undecided (N) bool, margin (N), coplanar, degenerate.  A coplanar pair is decided (no collision) only when it is coplanar exactly."""
    m, cop, deg = margin(A, B, dtype)
    m = np.where(deg, -np.inf, m)
    collide = (m >= 0) & ~cop & ~deg
    exact = cop & (_plane_dist(A, B) == 0)
    undecided = ~deg & ((np.abs(m) < tau(A, B)) & ~cop | cop & ~exact)
    return collide, undecided, m, cop, deg


def _plane_dist(A, B):
    A = A.astype(np.float64); B = B.astype(np.float64)
    nA = _cross(A[:, 1] - A[:, 0], A[:, 2] - A[:, 0]); nB = _cross(B[:, 1] - B[:, 0], B[:, 2] - B[:, 0])
    dA = np.abs(np.einsum("nk,nvk->nv", nB, A - B[:, :1])).max(1); dB = np.abs(np.einsum("nk,nvk->nv", nA, B - A[:, :1])).max(1)
    return np.maximum(dA, dB)


def _side(recv, intr, sigma, dtype):
    """Psi_recv(v)^2 for the three vertices v of intr.  recv, intr (N, 3, 3).  -> dict of (N, 3) arrays (value, x, Phi, rho, Dn, code) and grad (N, 3, 3) = dPsi^2/dv, r (N)"""
    recv = recv.astype(dtype); intr = intr.astype(dtype); sigma = dtype(sigma)
    a = recv[:, 0]; e1 = recv[:, 1] - a; e2 = recv[:, 2] - a
    n = _cross(e1, e2); nn = _dot(n, n); ok = nn > 0; nn1 = np.where(ok, nn, 1)
    rel = (_dot(e2, e2)[:, None] * _cross(n, e1) + _dot(e1, e1)[:, None] * _cross(e2, n)) / (2 * nn1)[:, None]
    o = a + rel; r = np.sqrt(_dot(rel, rel)); nh = n / np.sqrt(nn1)[:, None]
    d = intr - o[:, None]; x = np.einsum("nk,nvk->nv", nh, d)
    er = d - x[..., None] * nh[:, None]; rho = np.sqrt(_dot(er, er))
    Dn = r[:, None] - (r / sigma)[:, None] * x
    pos = ok[:, None] & (Dn > 0)
    Phi = rho / np.where(pos, Dn, 1)
    lin = x <= -sigma; a2 = -(1 - 2 * sigma) / (4 * sigma * sigma)
    Ups = np.where(lin, -x + 1 - sigma, a2 * x * x - x / (2 * sigma) + (3 - 2 * sigma) / 4); dUps = np.where(lin, dtype(-1), 2 * a2 * x - 1 / (2 * sigma))
    live = pos & (Phi < 1) & (x < sigma)
    code = np.where(~pos, APEX, np.where(~live, OUTSIDE, np.where(lin, LINEAR, QUAD)))
    w = np.where(live, (1 - Phi) * Ups, 0)
    erh = er / np.where(rho > 0, rho, 1)[..., None]                                # 0 on the axis: the |e_r| term has no derivative there and none is taken
    Dn1 = np.where(pos, Dn, 1)
    dPhi = erh / Dn1[..., None] + (rho * (r / sigma)[:, None] / (Dn1 * Dn1))[..., None] * nh[:, None]
    grad = (4 * w ** 3)[..., None] * (-Ups[..., None] * dPhi + ((1 - Phi) * dUps)[..., None] * nh[:, None])
    grad = np.where(live[..., None], grad, 0)
    return dict(value=w ** 4, grad=grad, x=x, Phi=np.where(pos, Phi, np.inf), rho=rho, Dn=Dn, code=code, live=live, r=r)


def pair_terms(S, O, sigma, dtype=np.float64):
    """S, O (N, 3, 3): SMPL and object triangles of N pairs.  -> per pair: v (N), g (N, 3) = d v / dt, sV (N), sG (N), and the two sides' details (side 0: object
    vertices in the SMPL triangle's cone, side 1: SMPL vertices in the object triangle's cone)"""
    s0 = _side(S, O, sigma, dtype); s1 = _side(O, S, sigma, dtype)
    v = s0["value"].sum(1, dtype=dtype) + s1["value"].sum(1, dtype=dtype)
    g = s0["grad"].sum(1, dtype=dtype) - s1["grad"].sum(1, dtype=dtype)
    cmax = np.maximum(np.abs(S).max((1, 2)), np.abs(O).max((1, 2))).astype(np.float64)
    sV = np.zeros(len(S)); sG = np.zeros(len(S))
    for s in (s0, s1):
        l1 = np.abs(s["grad"].astype(np.float64)).sum(2); live = s["live"]
        Dn = np.where(live, s["Dn"], 1).astype(np.float64); Phi = np.where(live, s["Phi"], 0).astype(np.float64); rho = s["rho"].astype(np.float64)
        amp = 1 / (Dn * (1 - Phi)) + np.where(rho > 0, 1 / np.where(rho > 0, rho, 1), 0) + (1 / np.where(s["r"] > 0, s["r"], 1).astype(np.float64))[:, None]
        sV += np.where(live, l1, 0).sum(1); sG += np.where(live, l1 * amp, 0).sum(1)
    return dict(v=v, g=g, sV=sV * cmax, sG=sG * cmax, sides=(s0, s1))


def value_autograd(S, O, sigma):
    """the value of the pairs (S[i], O[i] + t) at t = 0 and its derivative by t, by torch float64 autograd on the CPU through the whole expression"""
    import torch
    S = torch.from_numpy(np.ascontiguousarray(S, np.float64)); t = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    O = torch.from_numpy(np.ascontiguousarray(O, np.float64)) + t

    def side(recv, intr):
        a = recv[:, 0]; e1 = recv[:, 1] - a; e2 = recv[:, 2] - a
        n = torch.linalg.cross(e1, e2); nn = (n * n).sum(-1)
        rel = ((e2 * e2).sum(-1)[:, None] * torch.linalg.cross(n, e1) + (e1 * e1).sum(-1)[:, None] * torch.linalg.cross(e2, n)) / (2 * nn)[:, None]
        o = a + rel; r = rel.norm(dim=-1); nh = n / nn.sqrt()[:, None]
        d = intr - o[:, None]; x = (d * nh[:, None]).sum(-1)
        er = d - x[..., None] * nh[:, None]; q = (er * er).sum(-1)
        rho = torch.where(q > 0, torch.where(q > 0, q, torch.ones_like(q)).sqrt(), torch.zeros_like(q))
        Dn = r[:, None] * (1 - x / sigma); pos = Dn > 0
        Phi = rho / torch.where(pos, Dn, torch.ones_like(Dn))
        lin = x <= -sigma
        Ups = torch.where(lin, -x + 1 - sigma, -(1 - 2 * sigma) / (4 * sigma * sigma) * x * x - x / (2 * sigma) + (3 - 2 * sigma) / 4)
        live = pos & (Phi < 1) & (x < sigma)
        return torch.where(live, ((1 - Phi) * Ups) ** 4, torch.zeros_like(x)).sum()

    V = side(S, O) + side(O, S)
    if len(S) == 0:
        return 0.0, np.zeros(3)
    V.backward()
    return float(V.detach()), t.grad.numpy().copy()


def frame(sv, sf, ov, of, sigma=0.5, max_coll=8, dtype=np.float64):
    """One frame: sv (NVs, 3), ov (NVo, 3) float32, sf (NFs, 3), of (NFo, 3) int.  The box tests compare the float32 corners and are exact in every format.
    -> dict: V, g (3) = dV/dt, pairs (count), S_V, S_g, n_f, kept (K, 2) [object face, SMPL face], box_pairs (P, 2), the per-box-pair arrays collide, undecided, margin,
    coplanar, degenerate, keep, v, g_pair, sV, sG (v.. are 0 where the pair neither collides nor is undecided), n_cand, and `terms` (pair_terms of the kept pairs)"""
    sv = np.asarray(sv, np.float32); ov = np.asarray(ov, np.float32)
    S = sv[sf]; O = ov[of]
    slo, shi, olo, ohi = S.min(1), S.max(1), O.min(1), O.max(1); blo, bhi = ov.min(0), ov.max(0)
    cand = np.flatnonzero((slo <= bhi).all(1) & (blo <= shi).all(1))
    io, ic = np.nonzero((slo[cand][None] <= ohi[:, None]).all(2) & (olo[:, None] <= shi[cand][None]).all(2))        # sorted by object face, then by SMPL face
    is_ = cand[ic]
    collide, undecided, m, cop, deg = decide(S[is_], O[io], dtype) if len(io) else (np.zeros(0, bool),) * 2 + (np.zeros(0),) + (np.zeros(0, bool),) * 2
    keep = first_per_face(io, collide, max_coll)
    want = collide | undecided
    v = np.zeros(len(io)); gp = np.zeros((len(io), 3)); sV = np.zeros(len(io)); sG = np.zeros(len(io))
    if want.any():
        t = pair_terms(S[is_[want]], O[io[want]], sigma, dtype)
        v[want] = t["v"]; gp[want] = t["g"]; sV[want] = t["sV"]; sG[want] = t["sG"]
    terms = pair_terms(S[is_[keep]], O[io[keep]], sigma, dtype)
    V = float(v[keep].sum()); g = gp[keep].sum(0)
    return dict(V=V, g=g, pairs=int(keep.sum()), S_V=V + float(sV[keep].sum()), S_g=float(sG[keep].sum()), n_f=len(np.unique(io[keep])), kept=np.stack([io[keep], is_[keep]], 1),
                box_pairs=np.stack([io, is_], 1), collide=collide, undecided=undecided, margin=m, coplanar=cop, degenerate=deg, keep=keep, v=v, g_pair=gp, sV=sV, sG=sG,
                n_cand=len(cand), terms=terms, S_kept=S[is_[keep]], O_kept=O[io[keep]])


def first_per_face(io, collide, max_coll):
    """io sorted.  the first max_coll True entries of `collide` within every run of equal io"""
    if len(io) == 0:
        return np.zeros(0, bool)
    cs = np.cumsum(collide); start = np.r_[True, io[1:] != io[:-1]]
    before = np.maximum.accumulate(np.where(start, cs - collide, 0))                 # cs - collide is nondecreasing, so the running maximum is the run's own start value
    return collide & (cs - before <= max_coll)


def slack(r, max_coll):
    """What the undecided pairs of a frame can change: every object face with undecided pairs is re-listed under every resolution of them (an undecided pair that
    turns on can displace a kept pair under max_coll, one that turns off lets the next one in).  -> (largest |change of V|, largest |change of g| per component (3),
    lowest and highest pair count), each summed over the faces"""
    io = r["box_pairs"][:, 0]; dV = 0.0; dg = np.zeros(3); lo = hi = r["pairs"]
    for f in np.unique(io[r["undecided"]]):
        at = np.flatnonzero(io == f); und = np.flatnonzero(r["undecided"][at]); assert len(und) <= 12, "too many undecided pairs on one object face"
        base = r["keep"][at]; v = r["v"][at]; g = r["g_pair"][at]
        wV = 0.0; wg = np.zeros(3); cl, ch = 0, 0
        for bits in itertools.product((False, True), repeat=len(und)):
            c = r["collide"][at].copy(); c[und] = bits
            k = first_per_face(np.zeros(len(at), int), c, max_coll)
            wV = max(wV, abs(v[k].sum() - v[base].sum())); wg = np.maximum(wg, np.abs(g[k].sum(0) - g[base].sum(0)))
            cl = min(cl, int(k.sum()) - int(base.sum())); ch = max(ch, int(k.sum()) - int(base.sum()))
        dV += wV; dg += wg; lo += cl; hi += ch
    return dV, dg, lo, hi


def resolutions(r, max_coll):
    """every way to resolve the undecided pairs of a frame (2^k of them) -> frame dicts with V, g, pairs, S_V, S_g, n_f; the first one is the model's own"""
    io = r["box_pairs"][:, 0]; und = np.flatnonzero(r["undecided"]); assert len(und) <= 12, "too many undecided pairs in one frame"
    out = [r]
    for bits in itertools.product((False, True), repeat=len(und)):
        c = r["collide"].copy(); c[und] = bits
        if np.array_equal(c, r["collide"]):
            continue
        k = first_per_face(io, c, max_coll); V = float(r["v"][k].sum())
        out.append(dict(V=V, g=r["g_pair"][k].sum(0), pairs=int(k.sum()), S_V=V + float(r["sV"][k].sum()), S_g=float(r["sG"][k].sum()), n_f=len(np.unique(io[k]))))
    return out


def value_gate(r, E32_V, start=0.0):
    return 8 * E32_V * U * r["S_V"] + r["n_f"] * QFIX + U * abs(start)


def grad_gate(r, E32_g, gscale, B, start=None):
    """per component of d_obj_t[b] = start + gscale / B dV/dt"""
    want = r["g"] * gscale / B
    return (8 * E32_g * U * r["S_g"] + r["n_f"] * QFIX) * gscale / B + U * np.abs(want) + (0 if start is None else U * np.abs(np.asarray(start, np.float64)))
