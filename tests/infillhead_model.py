"""numpy model of the ends of HVOP-Net's training step (csrc/infillhead.hip), written from the definitions with the derivatives by hand, parametrised by dtype:

proj_forward / proj_backward           y = x W^T + b (mfiller_cond.py:82-96) and dW = d_y^T x, db = sum over rows of d_y
head_forward / head_backward           h = f W1^T + b1, pred = leaky_relu(h, 0.01) W2^T + b2 (mfiller_cond.py:97-104) and d_f, dW1, db1, dW2, db2 from a d_pred
objective                              the two terms of motion_losses (trainer_infiller.py:33-47) and d_pred of their sum in the gather form of the kernel:
                                       d_pred[t] = up (c_pos s[t] + c_acc (sa[t-2] - 2 sa[t-1] + sa[t])), rows outside the clip dropped
proj_run / head_run / e32_of           {tensor: float64 array} of a `dt` run; e32 = the float32 run against the float64 run, per tensor
MUTANTS                                deliberate defects by name (`mut=`)
proj_cases / head_cases / objective_cases     the inputs of tests/test_gpu_infillhead.py and tests/test_host_infillhead.py, built once
ratios / failures                      the 4 e32 gate both test files use
"""
import numpy as np

HEAD_KEYS = ("predictor.0.weight", "predictor.0.bias", "predictor.2.weight", "predictor.2.bias")
MUTANTS = ("sign0_is_one", "accel_mean_over_T", "stencil_crosses_clips", "leaky_ge", "bias_grad_dropped", "accel_in_fp32_order")
GATE = 4.0
F32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)      # noqa: E731  float32-representable float64: the GPU and both model runs see the same numbers


# ---- projection ------------------------------------------------------------------------------------------------------------------------------------------------
def proj_forward(x, W, b, dt=np.float64):
    return (np.asarray(x).astype(dt) @ np.asarray(W).astype(dt).T + np.asarray(b).astype(dt)).astype(dt)


def proj_backward(dy, x, dt=np.float64, mut=None):
    dy, x = np.asarray(dy).astype(dt), np.asarray(x).astype(dt)
    dy2, x2 = dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1])
    db = dy2.sum(0)
    return (dy2.T @ x2).astype(dt), (np.zeros_like(db) if mut == "bias_grad_dropped" else db).astype(dt)


def proj_run(x, W, b, dy, dt=np.float64, mut=None):
    dW, db = proj_backward(dy, x, dt, mut)
    return {k: np.asarray(v, dtype=np.float64) for k, v in dict(y=proj_forward(x, W, b, dt), dW=dW, db=db).items()}


# ---- predictor -------------------------------------------------------------------------------------------------------------------------------------------------
def head_forward(P, f, dt=np.float64, mut=None):
    """-> (pred, h)"""
    W1, b1, W2, b2 = (np.asarray(P[k]).astype(dt) for k in HEAD_KEYS)
    h = np.asarray(f).astype(dt) @ W1.T + b1
    a = np.where(h >= 0 if mut == "leaky_ge" else h > 0, h, h * dt(0.01))
    return (a @ W2.T + b2).astype(dt), h.astype(dt)


def head_backward(P, f, h, d_pred, dt=np.float64, mut=None):
    W1, _, W2, _ = (np.asarray(P[k]).astype(dt) for k in HEAD_KEYS)
    f, h, d = np.asarray(f).astype(dt), np.asarray(h).astype(dt), np.asarray(d_pred).astype(dt)
    pos = h >= 0 if mut == "leaky_ge" else h > 0
    a = np.where(pos, h, h * dt(0.01))
    dh = (d @ W2) * np.where(pos, dt(1), dt(0.01))
    g = {"d_f": dh @ W1, HEAD_KEYS[0]: np.einsum("bth,btd->hd", dh, f), HEAD_KEYS[1]: dh.sum((0, 1)), HEAD_KEYS[2]: np.einsum("btc,bth->ch", d, a), HEAD_KEYS[3]: d.sum((0, 1))}
    if mut == "bias_grad_dropped":
        g[HEAD_KEYS[1]] = np.zeros_like(g[HEAD_KEYS[1]]); g[HEAD_KEYS[3]] = np.zeros_like(g[HEAD_KEYS[3]])
    return {k: v.astype(dt) for k, v in g.items()}


def head_run(P, f, d_pred, dt=np.float64, mut=None):
    pred, h = head_forward(P, f, dt, mut)
    g = head_backward(P, f, h, d_pred, dt, mut)
    g.update(pred=pred, h=h)
    return {k: np.asarray(v, dtype=np.float64) for k, v in g.items()}


def e32_of(run, *args):
    """-> (float64 results, e32 per tensor) of run(*args, dt)"""
    r64, r32 = run(*args, np.float64), run(*args, np.float32)
    return r64, {k: float(np.abs(r32[k] - r64[k]).max()) for k in r64}


# ---- objective -------------------------------------------------------------------------------------------------------------------------------------------------
def _acc(a):
    return a[:, :-2] - 2 * a[:, 1:-1] + a[:, 2:]


def objective(pred, gt, lw_pose=1.0, lw_accel=0.1, dt=np.float64, mut=None, upstream=1.0):
    """-> (loss_pos, loss_accel, d_pred of upstream (loss_pos + loss_accel)); pred, gt (B, T, C), T >= 3"""
    p, g = np.asarray(pred).astype(dt), np.asarray(gt).astype(dt)
    B, T, C = p.shape
    assert T >= 3
    if mut == "stencil_crosses_clips":
        p, g = p.reshape(1, B * T, C), g.reshape(1, B * T, C)
    e = p - g
    if mut == "accel_in_fp32_order":
        ea = (_acc(p.astype(np.float32)) - _acc(g.astype(np.float32))).astype(dt)
    else:
        ea = _acc(p) - _acc(g)
    n_pos, n_acc = e.size, (e.size if mut == "accel_mean_over_T" else ea.size)
    sg = (lambda v: np.where(v >= 0, 1.0, -1.0)) if mut == "sign0_is_one" else np.sign
    s, sa = sg(e).astype(dt), sg(ea).astype(dt)
    k = np.zeros_like(e)
    k[:, :-2] += sa; k[:, 1:-1] -= 2 * sa; k[:, 2:] += sa               # small integers: exact in any order
    c_pos, c_acc = dt(upstream) * (dt(lw_pose) / dt(n_pos)), dt(upstream) * (dt(lw_accel) / dt(n_acc))
    d = c_pos * s + c_acc * k
    loss_pos = dt(lw_pose) * (np.abs(e).sum(dtype=dt) / dt(n_pos))
    loss_accel = dt(lw_accel) * (np.abs(ea).sum(dtype=dt) / dt(n_acc))
    return loss_pos, loss_accel, d.reshape(B, T, C).astype(dt)


# ---- the gate ----------------------------------------------------------------------------------------------------------------------------------------------------
def ratios(got, truth, e32):
    """per tensor: largest |got - truth| / e32 (0 / 0 = 0, x / 0 = inf)"""
    out = {}
    for k, t in truth.items():
        err = float(np.abs(np.asarray(got[k], dtype=np.float64) - t).max())
        out[k] = err / e32[k] if e32[k] > 0 else (0.0 if err == 0 else np.inf)
    return out


def failures(got, truth, e32, gate=GATE):
    return {k: r for k, r in ratios(got, truth, e32).items() if not r <= gate}


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------------------------
BT = ((1, 3), (3, 17), (2, 33), (1, 180), (3, 180))        # T = 3: the smallest clip with an acceleration row; M = 3, 51, 66 straddle 16-row tiles; 540 crosses a chunk
PROJ = ((147, 128), (6, 32), (9, 32))                      # (Kin, N): feat_proj_smpl, feat_proj_obj of '6d' and of '9d'
ZERO = (0, 1, 2)                                           # (clip, frame, hidden unit) of the planted exact zero of h in every head case
_built = {}


def proj_cases():
    """every (B, T) once with a table of two projections, the object side alternating between Kin 6 and 9"""
    return [dict(id=f"B{B}-T{T}-K147+{PROJ[1 + i % 2][0]}", B=B, T=T, probs=(PROJ[0], PROJ[1 + i % 2]), seed=400 + i) for i, (B, T) in enumerate(BT)]


def build_proj(c):
    if ("proj", c["id"]) not in _built:
        r = np.random.RandomState(c["seed"])
        probs = []
        for K, N in c["probs"]:
            x, W, b, dy = F32(r.randn(c["B"], c["T"], K)), F32(r.randn(N, K) / np.sqrt(K)), F32(0.1 * r.randn(N)), F32(r.randn(c["B"], c["T"], N))
            r64, e32 = e32_of(lambda dt, x=x, W=W, b=b, dy=dy: proj_run(x, W, b, dy, dt))
            probs.append(dict(x=x, W=W, b=b, dy=dy, r64=r64, e32=e32))
        _built[("proj", c["id"])] = dict(c, p=probs)
    return _built[("proj", c["id"])]


# seeds chosen so that no hidden pre-activation of the float64 model lies within 64 e32(h) of 0 (tests/test_host_infillhead.py asserts it; the GPU test again)
def head_cases():
    out = [dict(id=f"B{B}-T{T}-D160-H32-C{6 + 3 * (i % 2)}", B=B, T=T, D=160, Hd=32, C=6 + 3 * (i % 2), seed=s) for i, ((B, T), s) in enumerate(zip(BT, HEAD_SEEDS))]
    out.append(dict(id="B3-T17-D32-H16-C9", B=3, T=17, D=32, Hd=16, C=9, seed=HEAD_SEEDS[5]))
    return out


HEAD_SEEDS = (500, 501, 502, 503, 564, 505)                # 504 .. 554 put a pre-activation of the B3-T180 case within 64 e32(h) of 0


def head_inputs(c, seed=None):
    """-> (P, f, d_pred): float32-representable; the planted zero: frame ZERO[:2] of f is all zero and b1[ZERO[2]] = 0, so h is exactly 0 there in any precision"""
    r = np.random.RandomState(c["seed"] if seed is None else seed)
    B, T, D, Hd, C = c["B"], c["T"], c["D"], c["Hd"], c["C"]
    P = {HEAD_KEYS[0]: F32(r.randn(Hd, D) / np.sqrt(D)), HEAD_KEYS[1]: F32(0.1 * r.randn(Hd)), HEAD_KEYS[2]: F32(r.randn(C, Hd) / np.sqrt(Hd)),
         HEAD_KEYS[3]: F32(0.1 * r.randn(C))}
    f, d_pred = F32(r.randn(B, T, D)), F32(r.randn(B, T, C))
    f[ZERO[0], ZERO[1]] = 0; P[HEAD_KEYS[1]][ZERO[2]] = 0
    return P, f, d_pred


def kink_margin(c, seed=None):
    """the smallest |h| of the float64 model apart from the planted zero, in units of e32(h): the case condition is margin > 64"""
    P, f, d = head_inputs(c, seed)
    r64, e32 = e32_of(lambda dt: head_run(P, f, d, dt))
    h = np.abs(r64["h"]).copy()
    assert h[ZERO] == 0
    h[ZERO] = np.inf
    return float(h.min() / e32["h"])


def build_head(c):
    if ("head", c["id"]) not in _built:
        P, f, d = head_inputs(c)
        r64, e32 = e32_of(lambda dt: head_run(P, f, d, dt))
        _built[("head", c["id"])] = dict(c, P=P, f=f, d_pred=d, r64=r64, e32=e32)
    return _built[("head", c["id"])]


def _smooth(r, B, T, C):
    t = np.linspace(0, 1, T)[None, :, None]
    return np.sin(2 * np.pi * (t * r.uniform(0.5, 2, (B, 1, C)) + r.uniform(0, 1, (B, 1, C)))) * 0.5


def objective_cases():
    """every (B, T) with random smooth motion (C alternating 6 / 9), one case with planted exact zeros, one where float32-ordered stencils flip signs"""
    out = [dict(id=f"B{B}-T{T}-C{6 + 3 * (i % 2)}", B=B, T=T, C=6 + 3 * (i % 2), seed=600 + i, kind="smooth") for i, (B, T) in enumerate(BT)]
    out.append(dict(id="B3-T17-C6-zeros", B=3, T=17, C=6, seed=610, kind="zeros"))
    out.append(dict(id="B2-T33-C9-flip", B=2, T=33, C=9, seed=611, kind="flip"))
    return out


def build_objective(c):
    """pred, gt as float32 arrays; the float64 model's terms and d_pred"""
    if ("obj", c["id"]) not in _built:
        r = np.random.RandomState(c["seed"])
        B, T, C = c["B"], c["T"], c["C"]
        gt = (_smooth(r, B, T, C) + 0.02 * r.randn(B, T, C)).astype(np.float32)
        if c["kind"] == "flip":
            # pred a few float32 steps from gt: the exact second-difference error is a few units of 2^-25 and the float32-ordered one rounds each stencil first
            pred = gt.copy()
            for _ in range(2):
                step = r.randint(0, 3, gt.shape)
                pred = np.where(step == 1, np.nextafter(pred, np.float32(2)), np.where(step == 2, np.nextafter(pred, np.float32(-2)), pred)).astype(np.float32)
        else:
            pred = (gt.astype(np.float64) + 0.05 * _smooth(r, B, T, C) + 0.01 * r.randn(B, T, C)).astype(np.float32)
        if c["kind"] == "zeros":
            pred[1, 4:7, 2] = gt[1, 4:7, 2]                  # three equal elements in a column: e = 0 there and the acceleration error of row 4 is exactly 0
            pred[0, 0, 0] = gt[0, 0, 0]; pred[2, T - 1, C - 1] = gt[2, T - 1, C - 1]
        lp, la, d = objective(pred, gt)
        _built[("obj", c["id"])] = dict(c, pred=pred, gt=gt, loss_pos=float(lp), loss_accel=float(la), d_pred=d)
    return _built[("obj", c["id"])]
