"""Test helper (not a test file): the operations of the Adam-step kernels (csrc/step.hip, csrc/misc.hip; stated once in csrc/step_ops.h) restated in float64 numpy.

Written from the contract comments of step_ops.h / step.hip and DESIGN.md 4.5, not from the kernels' loops: every sum is ``np.sum``, the SVD is
``np.linalg.svd``, the stencils are array slices.  Nothing here touches libvistracker_hip.so.

Every function takes ``fp32=True`` to evaluate the SAME expression in float32 numpy.  That switch exists to size tolerances only: the distance
between the float32 and the float64 evaluation of an operation on a test's inputs (``e32``) is what rounding alone does to it, and a kernel is
allowed ``4 * e32`` (it sums in another order than numpy's pairwise sum), never less than the bar the suite already holds the operation to.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

ADAM_MIN_SQRT_V = 1e-3          # Adam normalises by sqrt(v): inputs keep it far above eps so that the comparison is well conditioned


def _dt(fp32):
    return np.float32 if fp32 else np.float64


def _c(x, fp32):
    return None if x is None else np.asarray(x, _dt(fp32))


# ---------------------------------------------------------------------------------------------------------------------------------
# SO(3) projection
# ---------------------------------------------------------------------------------------------------------------------------------
def so3_input(M0, noise=None, fp32=False):
    """the matrix that is projected: M0 + 1e-4 noise, (B, 3, 3)"""
    dt = _dt(fp32)
    M = _c(M0, fp32).reshape(-1, 3, 3)
    return M if noise is None else M + dt(1e-4) * _c(noise, fp32).reshape(-1, 3, 3)


def project_so3(M0, noise=None, fp32=False):
    """R = U diag(1, 1, det(U V^T)) V^T of M0 + 1e-4 noise.  Returns a dict: R, U, s, V (columns = right singular vectors), d, h = (s1, s2, d s3)."""
    dt = _dt(fp32)
    M = so3_input(M0, noise, fp32)
    U, s, Vt = np.linalg.svd(M)
    V = np.swapaxes(Vt, 1, 2)
    d = np.sign(np.linalg.det(U @ Vt)).astype(dt)
    D = np.stack([np.ones_like(d), np.ones_like(d), d], -1)
    R = (U * D[:, None, :]) @ Vt
    h = s * D
    return {"R": R.astype(dt), "U": U, "s": s, "V": V, "d": d, "h": h}


def so3_margin(M0, noise=None):
    """min_{i<j} (h_i + h_j) / s1 per matrix: what the VJP divides by, relative to the matrix' scale"""
    h = project_so3(M0, noise)["h"]
    pairs = np.stack([h[:, 0] + h[:, 1], h[:, 0] + h[:, 2], h[:, 1] + h[:, 2]], -1)
    return pairs.min(-1) / h[:, 0]


def so3_vjp_polar(M0, noise, G, fp32=False):
    """VJP of project_so3 in polar form (header of the SO(3) section of step_ops.h): dM = U D Z V^T, Q = D U^T G V, Z_ij = (Q_ij - Q_ji) / (h_i + h_j)"""
    p = project_so3(M0, noise, fp32)
    U, V, h = p["U"], p["V"], p["h"]
    G = _c(G, fp32).reshape(-1, 3, 3)
    D = np.stack([np.ones_like(p["d"]), np.ones_like(p["d"]), p["d"]], -1)
    Q = D[:, :, None] * (np.swapaxes(U, 1, 2) @ G @ V)
    den = h[:, :, None] + h[:, None, :]
    den = den + np.eye(3, dtype=den.dtype)              # the diagonal of Z is zero by definition; keep the division finite
    Z = (Q - np.swapaxes(Q, 1, 2)) / den
    Z = Z * (1 - np.eye(3, dtype=Z.dtype))
    return ((U * D[:, None, :]) @ Z @ np.swapaxes(V, 1, 2)).astype(_dt(fp32))


def so3_vjp_autograd(M0, noise, G):
    """the same VJP taken by torch float64 autograd through torch.linalg.svd / det (needs distinct singular values)"""
    import torch
    M = torch.tensor(so3_input(M0, noise), dtype=torch.float64, requires_grad=True)
    U, s, Vt = torch.linalg.svd(M)
    d = torch.linalg.det(U @ Vt)
    D = torch.stack([torch.ones_like(d), torch.ones_like(d), d], -1)
    R = (U * D[:, None, :]) @ Vt
    (R * torch.tensor(np.asarray(G, np.float64).reshape(-1, 3, 3))).sum().backward()
    return M.grad.numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# rigid transform  X[b, n] = (X0[n] R[b] + t[b]) s[b]
# ---------------------------------------------------------------------------------------------------------------------------------
def rigid(X0, R, t, s, fp32=False):
    X0, R, t, s = _c(X0, fp32), _c(R, fp32).reshape(-1, 3, 3), _c(t, fp32), _c(s, fp32)
    return ((X0[None] @ R) + t[:, None, :]) * s[:, None, None]


def rigid_vjp(X0, s, dX, fp32=False):
    """(dR (B, 3, 3), dt (B, 3)) of sum(X * dX)"""
    X0, s, dX = _c(X0, fp32), _c(s, fp32), _c(dX, fp32)
    g = dX * s[:, None, None]
    dR = np.sum(X0[None, :, :, None] * g[:, :, None, :], axis=1)
    return dR, np.sum(g, axis=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# temporal terms on v (B, D)
# ---------------------------------------------------------------------------------------------------------------------------------
def accel_term(v, gscale=1.0, elem_w=None, fp32=False):
    """mean over interior frames and columns of w a^2, a = v[f+1] - 2 v[f] + v[f-1]; returns (term, gscale * d term / d v)"""
    dt = _dt(fp32)
    v = _c(v, fp32)
    B, D = v.shape
    w = np.ones(D, dt) if elem_w is None else _c(elem_w, fp32)
    a = v[2:] - dt(2) * v[1:-1] + v[:-2]
    cnt = dt((B - 2) * D)
    term = np.sum(w * a * a) / cnt
    ga = dt(2) * dt(gscale) * w * a / cnt
    dv = np.zeros_like(v)
    dv[2:] += ga
    dv[1:-1] -= dt(2) * ga
    dv[:-2] += ga
    return term, dv


def velocity_term(v, gscale=1.0, fp32=False):
    """mean over the B - 1 differences d = v[f] - v[f-1] of d^2; returns (term, gscale * gradient)"""
    dt = _dt(fp32)
    v = _c(v, fp32)
    B, D = v.shape
    d = v[1:] - v[:-1]
    cnt = dt((B - 1) * D)
    term = np.sum(d * d) / cnt
    gd = dt(2) * dt(gscale) * d / cnt
    dv = np.zeros_like(v)
    dv[1:] += gd
    dv[:-1] -= gd
    return term, dv


# ---------------------------------------------------------------------------------------------------------------------------------
# regularisers of the two fits
# ---------------------------------------------------------------------------------------------------------------------------------
def trans_reg(t, t_init, w=1.0, fp32=False):
    """mean((t - t_init)^2) over (B, 3); returns (term, w * gradient)"""
    dt = _dt(fp32)
    d = _c(t, fp32) - _c(t_init, fp32)
    return np.sum(d * d) / dt(d.size), dt(2) * dt(w) * d / dt(d.size)


def body_prior(pose, mean, prec, gscale=1.0, fp32=False):
    """mean_B |(pose[:, 3:66] - mean) P|^2 with the (63, 63) precision factor P; returns (term, gradient (B, 156) scaled by gscale PER FRAME:
    d/dpose of gscale * sum_B |.|^2 -- the caller folds weight / B into gscale)"""
    dt = _dt(fp32)
    pose, mean, P = _c(pose, fp32), _c(mean, fp32), _c(prec, fp32).reshape(63, 63)
    d = pose[:, 3:66] - mean[None]
    y = d @ P
    g = np.zeros_like(pose)
    g[:, 3:66] = dt(2) * dt(gscale) * (y @ P.T)
    return np.sum(y * y) / dt(pose.shape[0]), g


def pinit_term(pose, pose_init, w=1.0, fp32=False):
    """mean_B sum_{columns 3..71} (pose - pose_init)^2; returns (term, w * gradient (B, 156))"""
    dt = _dt(fp32)
    pose, pose_init = _c(pose, fp32), _c(pose_init, fp32)
    B = pose.shape[0]
    d = pose[:, 3:72] - pose_init[:, 3:72]
    g = np.zeros_like(pose)
    g[:, 3:72] = dt(2) * dt(w) * d / dt(B)
    return np.sum(d * d) / dt(B), g


def csr_dense(indptr, indices, data, K, V):
    A = np.zeros((K, V), np.float64)
    for k in range(K):
        np.add.at(A[k], np.asarray(indices[indptr[k]:indptr[k + 1]]), np.asarray(data[indptr[k]:indptr[k + 1]], np.float64))
    return A


def kpts_chain(A, verts, kpts, crop_center, mode, cam, net_size, gscale=1.0, fp32=False):
    """J = A verts; pixel = pinhole projection (mode 1: moved into the crop of side cam[4] around crop_center and scaled to net_size);
    term = sum conf |pixel - kpts|^2 / count (mode 0: B K 2, mode 1: B K).  Returns (J, term, gscale * d term / d verts)."""
    dt = _dt(fp32)
    A, verts, kpts = _c(A, fp32), _c(verts, fp32), _c(kpts, fp32)
    fx, fy, cx, cy, crop = (dt(c) for c in np.asarray(cam, np.float64)[:5])
    B, K = verts.shape[0], A.shape[0]
    J = np.stack([np.stack([np.sum(A * verts[b, :, c][None, :], axis=1) for c in range(3)], -1) for b in range(B)])
    x, y, z = J[..., 0], J[..., 1], J[..., 2]
    px, py, sc = fx * x / z + cx, fy * y / z + cy, dt(1)
    if mode == 1:
        cc = _c(crop_center, fp32)
        sc = dt(net_size) / crop
        px = (crop / dt(2) + px - cc[:, :1]) * sc
        py = (crop / dt(2) + py - cc[:, 1:]) * sc
    ex, ey, conf = px - kpts[..., 0], py - kpts[..., 1], kpts[..., 2]
    cnt = dt(B * K * 2 if mode == 0 else B * K)
    term = np.sum((ex * ex + ey * ey) * conf) / cnt
    gpx, gpy = dt(2) * dt(gscale) * ex * conf * sc / cnt, dt(2) * dt(gscale) * ey * conf * sc / cnt
    dJ = np.stack([gpx * fx / z, gpy * fy / z, -(gpx * fx * x + gpy * fy * y) / (z * z)], -1)
    dverts = np.stack([np.stack([np.sum(A * dJ[b, :, c][:, None], axis=0) for c in range(3)], -1) for b in range(B)])
    return J, term, dverts


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam, closing a step
# ---------------------------------------------------------------------------------------------------------------------------------
def adam(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, fp32=False):
    """one torch.optim.Adam step (no weight decay, no amsgrad); returns (p, m, v)"""
    dt = _dt(fp32)
    p, g, m, v = _c(p, fp32), _c(g, fp32), _c(m, fp32), _c(v, fp32)
    m = dt(beta1) * m + dt(1 - dt(beta1)) * g
    v = dt(beta2) * v + dt(1 - dt(beta2)) * g * g
    assert np.sqrt(v.astype(np.float64)).min() >= ADAM_MIN_SQRT_V, "test inputs must keep sqrt(v) far above eps"
    bc1, bc2 = 1.0 - float(beta1) ** step, 1.0 - float(beta2) ** step
    denom = np.sqrt(v) / dt(np.sqrt(bc2)) + dt(eps)
    return p - dt(lr / bc1) * (m / denom), m, v


def weighted_loss(terms, w):
    """float32(sum_k float64(w_k) terms_k), the fp64 operations in index order.  Returns the two float32 values a correct device evaluation can
    give: with every multiply-add rounded once (fused) and rounded twice.  They differ only when the fp64 sum sits within one ulp of a float32 tie."""
    fused, plain = 0.0, 0.0
    for wk, tk in zip(np.asarray(w, np.float32), np.asarray(terms, np.float64)):
        fused = float(Fraction(float(wk)) * Fraction(float(tk)) + Fraction(fused))
        plain = plain + float(wk) * float(tk)
    return np.float32(fused), np.float32(plain)


def close_step(terms, w, prev, tol, armed):
    """(loss float32, stop, ratio): the reference's rule abs(prev - loss) / prev < prev * tol; ratio = (abs(prev - loss) / prev) / (prev * tol)"""
    loss = weighted_loss(terms, w)[1]
    prev = float(np.float32(prev))
    if not np.isfinite(prev):
        return loss, False, float("nan")
    lhs, rhs = abs(prev - float(loss)) / prev, prev * float(np.float32(tol))
    return loss, bool(armed and lhs < rhs), lhs / rhs


# ---------------------------------------------------------------------------------------------------------------------------------
# the fused launches, composed of the operations above.  `c` is a dict of inputs (numpy); every function returns a dict of outputs.
# ---------------------------------------------------------------------------------------------------------------------------------
def objstep_head(c, fp32=False):
    p = project_so3(c["M0"], c.get("noise"), fp32)
    out = {"R": p["R"], "X_points": rigid(c["X0_points"], p["R"], c["t"], c["s"], fp32), "svd": p}
    if c.get("X0_verts") is not None:
        out["X_verts"] = rigid(c["X0_verts"], p["R"], c["t"], c["s"], fp32)
    return out


def objstep_tail(c, fp32=False):
    """tail of an object-stage step.  c: X0_points, dX_points, s, M0, noise, t; optional X0_verts + dX_verts, t_init + w_trans, temporal = dict(X, w_accel,
    w_velocity, init_zero); rot (bool), trans (bool), Adam state mR, vR, mT, vT, lrR, lrT, adam_step.  Returns gradients, stepped parameters, term additions."""
    dt = _dt(fp32)
    B = np.asarray(c["M0"]).reshape(-1, 9).shape[0]
    out = {}
    g = _c(c["dX_points"], fp32)
    tmp = c.get("temporal")
    if tmp is not None:
        if tmp["init_zero"]:
            g = np.zeros(np.asarray(c["dX_points"]).shape, dt)
        v = _c(tmp["X"], fp32).reshape(B, -1)
        out["term_accel"], da = accel_term(v, tmp["w_accel"], None, fp32)
        out["term_velocity"], dv = velocity_term(v, tmp["w_velocity"], fp32)
        g = g + (da + dv).reshape(g.shape)
    dR, dtr = rigid_vjp(c["X0_points"], c["s"], g, fp32)
    if c.get("dX_verts") is not None:
        dRv, dtv = rigid_vjp(c["X0_verts"], c["s"], c["dX_verts"], fp32)
        dR, dtr = dR + dRv, dtr + dtv
    if c.get("t_init") is not None:
        out["term_trans"], gt = trans_reg(c["t"], c["t_init"], c["w_trans"], fp32)
        dtr = dtr + gt
    out["dt"] = dtr
    if c["rot"]:
        out["dR"] = dR.reshape(B, 9)
        out["dM"] = so3_vjp_polar(c["M0"], c.get("noise"), dR, fp32).reshape(B, 9)
        out["pR"], out["mR"], out["vR"] = adam(np.asarray(c["M0"]).reshape(B, 9), out["dM"], c["mR"], c["vR"], c["adam_step"], c["lrR"], fp32=fp32)
    if c["trans"]:
        out["pT"], out["mT"], out["vT"] = adam(c["t"], out["dt"], c["mT"], c["vT"], c["adam_step"], c["lrT"], fp32=fp32)
    return out


def smplstep_tail(c, fp32=False):
    """tail of a SMPL-stage step.  c: pose, pose_init, dpose (starting gradient, accumulated into), mean, prec, gscale_prior, w_pinit, groups = list of dicts
    (name, p, g, m, v, ncols, lr; the group named 'pose' takes its gradient from the accumulated dpose), adam_step."""
    tp, gp = body_prior(c["pose"], c["mean"], c["prec"], c["gscale_prior"], fp32)
    ti, gi = pinit_term(c["pose"], c["pose_init"], c["w_pinit"], fp32)
    dpose = _c(c["dpose"], fp32) + gp + gi
    out = {"term_prior": tp, "term_pinit": ti, "dpose": dpose, "groups": []}
    for grp in c["groups"]:
        n = grp["ncols"]
        g = dpose[:, :n] if grp["name"] == "pose" else np.asarray(grp["g"])[:, :n]
        out["groups"].append(adam(np.asarray(grp["p"])[:, :n], g, grp["m"], grp["v"], c["adam_step"], grp["lr"], fp32=fp32))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded input generators shared by the host test (which asserts their conditions) and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
SO3_KINDS = ("rotation", "fit", "reflection", "small", "large", "random")
SO3_MIN_MARGIN = 0.1            # random matrices are drawn by rejection on so3_margin >= this
SO3_MAX_REJECT = 0.25
SO3_SEEDS = (11, 12, 13, 14, 15, 16, 17, 19)          # every seed the GPU tests hand to so3_inputs ...
SO3_BATCHES = (1, 2, 3, 4, 5, 6, 96, 97)              # ... and every batch size (the draws depend on it: the noise block comes first)


def random_rotations(rng, n):
    q, r = np.linalg.qr(rng.normal(0, 1, (n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 2] *= np.sign(np.linalg.det(q))[:, None]
    return q


def so3_inputs(seed, B, with_noise=True):
    """(M0 (B, 3, 3) float32, noise (B, 3, 3) float32 or None, kinds, rejected fraction): frame b is of kind SO3_KINDS[b % 6].
    rotation: exact rotations (repeated singular values, what a fit starts from); fit: rotation + U(0, 1e-4); reflection: U diag(3, 2, 0.5) V^T with
    det < 0; small / large: normal matrices times 1e-3 / 1e3; random: normal matrices.  The last three are drawn by rejection on the margin of
    M0 + 1e-4 noise as float32."""
    rng = np.random.default_rng(seed)
    noise = rng.normal(0, 1, (B, 3, 3)).astype(np.float32) if with_noise else None
    M0 = np.zeros((B, 3, 3), np.float32)
    kinds, drawn, rejected = [], 0, 0
    for b in range(B):
        kind = SO3_KINDS[b % len(SO3_KINDS)]
        kinds.append(kind)
        nb = None if noise is None else noise[b:b + 1]
        if kind in ("rotation", "fit"):
            M0[b] = random_rotations(rng, 1)[0] + (rng.uniform(0, 1e-4, (3, 3)) if kind == "fit" else 0)
        elif kind == "reflection":
            U, V = random_rotations(rng, 2)
            U[:, 2] *= -1
            M0[b] = U @ np.diag([3.0, 2.0, 0.5]) @ V.T
        else:
            scale = {"small": 1e-3, "large": 1e3, "random": 1.0}[kind]
            while True:
                cand = (rng.normal(0, 1, (1, 3, 3)) * scale).astype(np.float32)
                drawn += 1
                if so3_margin(cand, nb)[0] >= SO3_MIN_MARGIN:
                    break
                rejected += 1
            M0[b] = cand[0]
    return M0, noise, kinds, rejected / max(drawn, 1)


def adam_moments(rng, g_ref):
    """starting moments of the size of the gradient they will meet, row by row: m ~ N(0, scale), sqrt(v) in [0.5, 2] x scale,
    scale = max(|g|, 1e-2 max_row |g|, 1e-2)"""
    g = np.abs(np.asarray(g_ref, np.float64))
    scale = np.maximum(g, 1e-2 * np.maximum(g.max(axis=-1, keepdims=True), 1.0))
    m = (rng.normal(0, 1, g.shape) * scale).astype(np.float32)
    v = ((rng.uniform(0.5, 2.0, g.shape) * scale) ** 2).astype(np.float32)
    return m, v
