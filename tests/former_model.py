"""numpy model of HVOP-Net's pre-norm encoder layer (former_deci.py:77-93) and of a stack of them, written from the definitions with the derivative by hand.

PARAM_KEYS                               the twelve parameters of a layer, in the order of the C ABI
make_params(D, F, seed) / make_inputs(B, T, D, seed, mask)       name-free seeded parameters, x, pos, d_y, key-padding mask
dropout_hash(seed, site, index)          csrc/dropout_hash.h restated with numpy uint32 / uint64 operations; keep_scale(...) = the mask times the fp32 1 / (1 - p)
layer_forward(P, x, pos, mask, H, act, p, seed, dt, mut, tape)   y and everything the backward reads; dt = float64 or float32 (the model's own float32 run);
                                         mut names a deliberate defect (MUTANTS); tape = a GPU forward's saved tensors to evaluate the backward AT
                                         (statistics, q|k|v, O, y1, h; the saved log-sum-exp is a function of q|k and is not taken: the model normalises its own softmax)
layer_backward(P, S, dy)                 d_x and the twelve parameter gradients
reference_and_e32(...)                   the float64 result + per tensor the largest |float32 run - float64 run| on the same inputs (tests/hourglass_model.py)
stack_forward / stack_backward           L layers and the optional final LayerNorm
infiller_forward / infiller_backward / motion_losses / infiller_run / adam_trajectory     the whole ConditionalMInfiller, its objective, and torch.optim.Adam on it
"""
import math

import numpy as np

PARAM_KEYS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "linear1.weight", "linear1.bias",
              "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
ACTS = ("relu", "gelu", "leaky_relu")
MUTANTS = ("ln_unbiased", "mask_after_softmax", "pos_on_value", "scale_1_over_hd", "tanh_gelu", "drop2_unscaled")
SITE_ATTN, SITE_1, SITE_FF, SITE_2 = 0, 1, 2, 3

try:
    from scipy.special import erf as _erf
except Exception:      # noqa: BLE001
    _erf = np.vectorize(math.erf, otypes=[np.float64])


def mix32(x):
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d); x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846ca68b); x = x ^ (x >> np.uint32(16))
    return x


def dropout_hash(seed, site, index):
    """(seed: python int < 2^64, site: int, index: uint64 array) -> uint32 array"""
    index = np.asarray(index, dtype=np.uint64)
    lo, hi = np.uint32(seed & 0xffffffff), np.uint32((seed >> 32) & 0xffffffff)
    c = np.uint32((0x9e3779b9 * (site + 1)) & 0xffffffff)
    h = mix32(np.full(index.shape, lo ^ c, dtype=np.uint32))
    h = mix32(h ^ hi)
    h = mix32(h ^ (index & np.uint64(0xffffffff)).astype(np.uint32))
    h = mix32(h ^ (index >> np.uint64(32)).astype(np.uint32))
    return h


def keep_scale(seed, site, shape, p, scaled=True):
    """the dropout multiplier of every element of a C-ordered array of `shape`: 0 or the fp32 1 / (1 - p) (1 where p = 0)"""
    if p == 0:
        return np.ones(shape)
    thr = int(math.floor(float(np.float32(p)) * 2.0 ** 32))
    if thr == 0:
        return np.ones(shape)
    inv = float(np.float32(1) / (np.float32(1) - np.float32(p))) if scaled else 1.0
    h = dropout_hash(seed, site, np.arange(int(np.prod(shape)), dtype=np.uint64).reshape(shape))
    return np.where(h >= np.uint32(thr), inv, 0.0)


def make_params(D, F, seed, dt=np.float64):
    r = np.random.RandomState(seed)
    P = {"self_attn.in_proj_weight": r.randn(3 * D, D) / math.sqrt(D), "self_attn.in_proj_bias": 0.1 * r.randn(3 * D),
         "self_attn.out_proj.weight": r.randn(D, D) / math.sqrt(D), "self_attn.out_proj.bias": 0.1 * r.randn(D),
         "linear1.weight": r.randn(F, D) / math.sqrt(D), "linear1.bias": 0.1 * r.randn(F),
         "linear2.weight": r.randn(D, F) / math.sqrt(F), "linear2.bias": 0.1 * r.randn(D),
         "norm1.weight": 1 + 0.2 * r.randn(D), "norm1.bias": 0.1 * r.randn(D), "norm2.weight": 1 + 0.2 * r.randn(D), "norm2.bias": 0.1 * r.randn(D)}
    return {k: v.astype(np.float32).astype(dt) for k, v in P.items()}       # float32-representable: the GPU and both model runs see the same numbers


MASKS = ("none", "block", "key0", "all_but_one")


def make_mask(B, T, kind):
    if kind == "none":
        return None
    m = np.zeros((B, T), dtype=bool)
    b = B - 1
    if kind == "block":
        m[b, T // 3:max(T // 3 + 1, 2 * T // 3)] = True
        if m[b].all():
            return None
    elif kind == "key0":
        if T == 1:
            return None
        m[b, 0] = True
    elif kind == "all_but_one":
        m[b] = True; m[b, T // 2] = False
    return m


def make_inputs(B, T, D, seed, mask="none"):
    r = np.random.RandomState(seed)
    f = lambda a: a.astype(np.float32).astype(np.float64)
    return f(r.randn(B, T, D)), f(0.5 * r.randn(T, D)), f(r.randn(B, T, D)), make_mask(B, T, mask)


def act_f(act, h, tanh_gelu=False):
    if act == "relu":
        return np.maximum(h, 0)
    if act == "leaky_relu":
        return np.where(h > 0, h, 0.01 * h)
    if tanh_gelu:
        return (0.5 * h * (1 + np.tanh(math.sqrt(2 / math.pi) * (h + 0.044715 * h ** 3)))).astype(h.dtype)
    return (0.5 * h * (1 + _erf(h.astype(np.float64) / math.sqrt(2)).astype(h.dtype))).astype(h.dtype)


def act_d(act, h):
    if act == "relu":
        return (h > 0).astype(h.dtype)
    if act == "leaky_relu":
        return np.where(h > 0, 1.0, 0.01).astype(h.dtype)
    h64 = h.astype(np.float64)
    return (0.5 * (1 + _erf(h64 / math.sqrt(2))) + h64 * np.exp(-0.5 * h64 * h64) / math.sqrt(2 * math.pi)).astype(h.dtype)


def _ln(x, g, b, unbiased=False, stats=None):
    D = x.shape[-1]
    if stats is None:
        mean = x.mean(-1, keepdims=True)
        var = ((x - mean) ** 2).sum(-1, keepdims=True) / (D - 1 if unbiased else D)
        rstd = 1 / np.sqrt(var + x.dtype.type(1e-5))
    else:
        mean, rstd = stats
    xh = (x - mean) * rstd
    return xh * g + b, xh, mean, rstd


def _ln_bwd(dz, xh, rstd, g):
    gz = dz * g
    return rstd * (gz - gz.mean(-1, keepdims=True) - xh * (gz * xh).mean(-1, keepdims=True)), (dz * xh).sum((0, 1)), dz.sum((0, 1))


def _heads(a, H):
    B, T, D = a.shape
    return a.reshape(B, T, H, D // H).transpose(0, 2, 1, 3)


def _unheads(a):
    B, H, T, hd = a.shape
    return a.transpose(0, 2, 1, 3).reshape(B, T, H * hd)


def layer_forward(P, x, pos, mask, H, act, p=0.0, seed=0, dt=np.float64, mut=None, tape=None):
    P = {k: np.asarray(v).astype(dt) for k, v in P.items()}
    x, pos = np.asarray(x).astype(dt), np.asarray(pos).astype(dt)
    B, T, D = x.shape
    F, hd = P["linear1.weight"].shape[0], D // H
    tp = (lambda k: np.asarray(tape[k]).astype(dt)) if tape is not None else None
    S = dict(x=x, H=H, act=act)
    xn, S["xh1"], S["mean1"], S["rstd1"] = _ln(x, P["norm1.weight"], P["norm1.bias"], mut == "ln_unbiased", (tp("mean1"), tp("rstd1")) if tape else None)
    S["qk_in"], S["v_in"] = xn + pos, (xn + pos if mut == "pos_on_value" else xn)
    Wi, bi = P["self_attn.in_proj_weight"], P["self_attn.in_proj_bias"]
    q, k, v = S["qk_in"] @ Wi[:D].T + bi[:D], S["qk_in"] @ Wi[D:2 * D].T + bi[D:2 * D], S["v_in"] @ Wi[2 * D:].T + bi[2 * D:]
    if tape:
        q, k, v = tp("qkv")[..., :D], tp("qkv")[..., D:2 * D], tp("qkv")[..., 2 * D:]
    S["qkv"] = np.concatenate([q, k, v], -1)
    qh, kh, vh = _heads(q, H), _heads(k, H), _heads(v, H)
    S["scale"] = scale = dt(1 / hd if mut == "scale_1_over_hd" else 1 / math.sqrt(hd))
    s = np.einsum("bhid,bhjd->bhij", qh, kh) * scale
    neg = np.zeros((B, 1, 1, T), dtype=bool) if mask is None else mask[:, None, None, :]
    if mut != "mask_after_softmax":
        s = np.where(neg, -np.inf, s)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m); sm = e.sum(-1, keepdims=True)
    S["lse"] = (m + np.log(sm))[..., 0]
    Pm = e / sm
    if mut == "mask_after_softmax":
        Pm = np.where(neg, 0, Pm)
    S["ka"] = keep_scale(seed, SITE_ATTN, (B, H, T, T), p).astype(dt)
    S["Pm"], S["Pd"] = Pm, Pm * S["ka"]
    S["O"] = tp("O") if tape else _unheads(np.einsum("bhij,bhjd->bhid", S["Pd"], vh))
    S["k1"] = keep_scale(seed, SITE_1, (B, T, D), p).astype(dt)
    S["y1"] = tp("y1") if tape else x + S["k1"] * (S["O"] @ P["self_attn.out_proj.weight"].T + P["self_attn.out_proj.bias"])
    S["z"], S["xh2"], S["mean2"], S["rstd2"] = _ln(S["y1"], P["norm2.weight"], P["norm2.bias"], mut == "ln_unbiased", (tp("mean2"), tp("rstd2")) if tape else None)
    S["h"] = tp("h") if tape else S["z"] @ P["linear1.weight"].T + P["linear1.bias"]
    S["kf"] = keep_scale(seed, SITE_FF, (B, T, F), p).astype(dt)
    S["af"] = act_f(act, S["h"], mut == "tanh_gelu").astype(dt) * S["kf"]
    S["k2"] = keep_scale(seed, SITE_2, (B, T, D), p, scaled=mut != "drop2_unscaled").astype(dt)
    y = S["y1"] + S["k2"] * (S["af"] @ P["linear2.weight"].T + P["linear2.bias"])
    return y.astype(dt), S


def layer_backward(P, S, dy):
    dt = S["x"].dtype
    P = {k: np.asarray(v).astype(dt) for k, v in P.items()}
    dy = np.asarray(dy).astype(dt)
    H, act = S["H"], S["act"]
    B, T, D = dy.shape
    g = {}
    du = dy * S["k2"]
    g["linear2.weight"], g["linear2.bias"] = np.einsum("btd,btf->df", du, S["af"]), du.sum((0, 1))
    dh = (du @ P["linear2.weight"]) * S["kf"] * act_d(act, S["h"])
    g["linear1.weight"], g["linear1.bias"] = np.einsum("btf,btd->fd", dh, S["z"]), dh.sum((0, 1))
    dln, g["norm2.weight"], g["norm2.bias"] = _ln_bwd(dh @ P["linear1.weight"], S["xh2"], S["rstd2"], P["norm2.weight"])
    dy1 = dy + dln
    dop = dy1 * S["k1"]
    g["self_attn.out_proj.weight"], g["self_attn.out_proj.bias"] = np.einsum("bte,btd->ed", dop, S["O"]), dop.sum((0, 1))
    doh = _heads(dop @ P["self_attn.out_proj.weight"], H)
    q, k, v = S["qkv"][..., :D], S["qkv"][..., D:2 * D], S["qkv"][..., 2 * D:]
    qh, kh, vh = _heads(q, H), _heads(k, H), _heads(v, H)
    dP = np.einsum("bhid,bhjd->bhij", doh, vh) * S["ka"]
    dv = _unheads(np.einsum("bhij,bhid->bhjd", S["Pd"], doh))
    dS = S["Pm"] * (dP - (dP * S["Pm"]).sum(-1, keepdims=True)) * S["scale"]
    dq, dk = _unheads(np.einsum("bhij,bhjd->bhid", dS, kh)), _unheads(np.einsum("bhij,bhid->bhjd", dS, qh))
    Wi = P["self_attn.in_proj_weight"]
    g["self_attn.in_proj_weight"] = np.concatenate([np.einsum("bte,btd->ed", dq, S["qk_in"]), np.einsum("bte,btd->ed", dk, S["qk_in"]),
                                                    np.einsum("bte,btd->ed", dv, S["v_in"])], 0)
    g["self_attn.in_proj_bias"] = np.concatenate([dq.sum((0, 1)), dk.sum((0, 1)), dv.sum((0, 1))])
    dxn = dq @ Wi[:D] + dk @ Wi[D:2 * D] + dv @ Wi[2 * D:]
    dln, g["norm1.weight"], g["norm1.bias"] = _ln_bwd(dxn, S["xh1"], S["rstd1"], P["norm1.weight"])
    g["d_x"] = dy1 + dln
    return {k: a.astype(dt) for k, a in g.items()}


def run(P, x, pos, mask, dy, H, act, p=0.0, seed=0, dt=np.float64, mut=None, tape=None):
    """{"y", "d_x", the twelve gradients} in float64 arrays (of a `dt` run)"""
    y, S = layer_forward(P, x, pos, mask, H, act, p, seed, dt, mut, tape)
    g = layer_backward(P, S, dy)
    g["y"] = y
    return {k: v.astype(np.float64) for k, v in g.items()}, S


TAPE_KEYS = ("mean1", "rstd1", "mean2", "rstd2", "qkv", "O", "y1", "h", "lse")


def reference_and_e32(P, x, pos, mask, dy, H, act, p=0.0, seed=0):
    """-> (float64 results, e32 per tensor, the float64 run's saved tensors); e32 also holds "tape/<k>" for the tensors a forward saves (TAPE_KEYS)"""
    g64, S = run(P, x, pos, mask, dy, H, act, p, seed, np.float64)
    g32, S32 = run(P, x, pos, mask, dy, H, act, p, seed, np.float32)
    e32 = {n: float(np.abs(g32[n] - g64[n]).max()) for n in g64}
    e32.update({"tape/" + k: float(np.abs(np.asarray(S32[k], dtype=np.float64) - S[k]).max()) for k in TAPE_KEYS})
    return g64, e32, S


def near_kink(P, S, act):
    """relu / leaky_relu: the (B, T, F) elements whose feed-forward pre-activation a float32 run cannot place on one side of 0: |h| <= 2^-23 sqrt(D + 1) times
    (|z| |W1|^T + |b1|), the random-walk rounding of a float32 sum of D + 1 terms of those magnitudes, doubled.  Empty for gelu."""
    h = np.asarray(S["h"], dtype=np.float64)
    if act == "gelu":
        return np.zeros(h.shape, dtype=bool)
    W1, b1 = np.abs(np.asarray(P["linear1.weight"], dtype=np.float64)), np.abs(np.asarray(P["linear1.bias"], dtype=np.float64))
    reach = 2.0 ** -23 * math.sqrt(W1.shape[1] + 1) * (np.abs(np.asarray(S["z"], dtype=np.float64)) @ W1.T + b1)
    return np.abs(h) <= reach


# ---- a stack (TransformerV2: L layers, an optional final LayerNorm) ---------------------------------------------------------------------------------------------
def stack_forward(Ps, norm, x, pos, mask, H, act, dt=np.float64):
    saved = []
    for P in Ps:
        x, S = layer_forward(P, x, pos, mask, H, act, dt=dt)
        saved.append(S)
    fin = None
    if norm is not None:
        xin = x
        x, xh, _, rstd = _ln(xin, np.asarray(norm[0]).astype(dt), np.asarray(norm[1]).astype(dt))
        fin = (xh, rstd)
    return x, (saved, fin)


def stack_backward(Ps, norm, saved, dy):
    saved, fin = saved
    g = {}
    dy = np.asarray(dy).astype(saved[0]["x"].dtype)
    if norm is not None:
        dy, g["encoder.norm.weight"], g["encoder.norm.bias"] = _ln_bwd(dy, fin[0], fin[1], np.asarray(norm[0]).astype(dy.dtype))
    for i in reversed(range(len(Ps))):
        gl = layer_backward(Ps[i], saved[i], dy)
        dy = gl.pop("d_x")
        g.update({f"encoder.layers.{i}.{k}": v for k, v in gl.items()})
    g["d_x"] = dy
    return g


# ---- the whole infiller (mfiller_cond.py:84-107), the motion losses (trainer_infiller.py:33-47) and Adam -----------------------------------------------------
ENCODERS = (("encoder_smpl.", "smpl"), ("encoder_obj.", "obj"), ("encoder_joint.", "joint"))


def position_table(T, D, temperature=10000.0):
    """PositionEmbeddingSine_1D (posi_embed.py:37-66) for an even D in float64: positions over [0, 2 pi], sin in even and cos in odd channels.  The reference
    builds this table in float32 whatever the model's dtype, so comparisons with it take infill.position_embedding_sine_1d (7e-7 from this one)."""
    pos = np.arange(T, dtype=np.float64)
    pos = pos / (pos[-1:] + 1e-6) * 2 * math.pi
    ang = pos[:, None] / temperature ** (2 * np.arange(D // 2, dtype=np.float64) / (D // 2))
    pe = np.zeros((T, D)); pe[:, 0::2] = np.sin(ang); pe[:, 1::2] = np.cos(ang)
    return pe


def _enc_cfg(opt, tag):
    D = opt.d_model_smpl + opt.d_model_obj if tag == "joint" else getattr(opt, f"d_model_{tag}")
    return D, getattr(opt, f"num_layers_{tag}"), getattr(opt, f"num_heads_{tag}"), getattr(opt, f"activation_{tag}"), getattr(opt, f"pre_norm_{tag}")


def _enc_params(sd, prefix, n, has_norm):
    Ps = [{k: sd[f"{prefix}encoder.layers.{i}.{k}"] for k in PARAM_KEYS} for i in range(n)]
    return Ps, ((sd[prefix + "encoder.norm.weight"], sd[prefix + "encoder.norm.bias"]) if has_norm else None)


def infiller_forward(sd, opt, batch, pos, dt=np.float64):
    """-> (prediction (B, T, out_dim), cache).  pos: {D: (T, D) table}; batch: data_smpl, mask_smpl, data_obj, mask_obj"""
    g = lambda k: np.asarray(sd[k]).astype(dt)                                # noqa: E731
    C = {"in": {}, "enc": {}}
    feats = {}
    for prefix, tag in ENCODERS[:2]:
        x = np.asarray(batch[f"data_{tag}"]).astype(dt)
        C["in"][tag] = x
        D, n, H, act, has_norm = _enc_cfg(opt, tag)
        Ps, norm = _enc_params(sd, prefix, n, has_norm)
        feats[tag], C["enc"][tag] = stack_forward(Ps, norm, x @ g(f"feat_proj_{tag}.weight").T + g(f"feat_proj_{tag}.bias"), pos[D],
                                                  np.asarray(batch[f"mask_{tag}"]).astype(bool), H, act, dt)
    D, n, H, act, has_norm = _enc_cfg(opt, "joint")
    Ps, norm = _enc_params(sd, "encoder_joint.", n, has_norm)
    x, C["enc"]["joint"] = stack_forward(Ps, norm, np.concatenate([feats["smpl"], feats["obj"]], -1), pos[D], None, H, act, dt)
    C["head"] = []
    nh = len(opt.hidden_dims) + 1
    for i in range(nh):
        h = x @ g(f"predictor.{2 * i}.weight").T + g(f"predictor.{2 * i}.bias")
        C["head"].append((x, h))
        x = np.where(h > 0, h, h * dt(0.01)) if i + 1 < nh else h
    return x.astype(dt), C


def infiller_backward(sd, opt, C, d_pred):
    """every parameter gradient under the state_dict's names, from the gradient to the prediction"""
    dt = d_pred.dtype
    g, d = {}, d_pred
    nh = len(C["head"])
    for i in reversed(range(nh)):
        x, h = C["head"][i]
        if i + 1 < nh:
            d = d * np.where(h > 0, 1.0, 0.01).astype(dt)
        g[f"predictor.{2 * i}.weight"], g[f"predictor.{2 * i}.bias"] = np.einsum("bto,bti->oi", d, x), d.sum((0, 1))
        d = d @ np.asarray(sd[f"predictor.{2 * i}.weight"]).astype(dt)
    D, n, H, act, has_norm = _enc_cfg(opt, "joint")
    Ps, norm = _enc_params(sd, "encoder_joint.", n, has_norm)
    gj = stack_backward(Ps, norm, C["enc"]["joint"], d)
    d = gj.pop("d_x")
    g.update({"encoder_joint." + k: v for k, v in gj.items()})
    Ds = opt.d_model_smpl
    for (prefix, tag), dd in zip(ENCODERS[:2], (d[..., :Ds], d[..., Ds:])):
        D, n, H, act, has_norm = _enc_cfg(opt, tag)
        Ps, norm = _enc_params(sd, prefix, n, has_norm)
        ge = stack_backward(Ps, norm, C["enc"][tag], dd)
        dx = ge.pop("d_x")
        g.update({prefix + k: v for k, v in ge.items()})
        g[f"feat_proj_{tag}.weight"], g[f"feat_proj_{tag}.bias"] = np.einsum("bto,bti->oi", dx, C["in"][tag]), dx.sum((0, 1))
    return {k: v.astype(dt) for k, v in g.items()}


def motion_losses(gt, pred, lw_pose=1.0, lw_accel=0.1):
    """-> (loss_accel, loss_pos, d_pred of their sum)"""
    dt = pred.dtype.type
    gt = np.asarray(gt).astype(dt)
    e = pred - gt
    acc = lambda a: a[:, :-2] - 2 * a[:, 1:-1] + a[:, 2:]                      # noqa: E731
    ea = acc(pred) - acc(gt)
    d = np.sign(e) * dt(lw_pose / e.size)
    da = np.sign(ea) * dt(lw_accel / ea.size)
    d[:, :-2] += da; d[:, 1:-1] -= 2 * da; d[:, 2:] += da
    return np.abs(ea).mean(dtype=dt) * dt(lw_accel), np.abs(e).mean(dtype=dt) * dt(lw_pose), d.astype(dt)


def infiller_run(sd, opt, batch, pos, dt=np.float64, lw=(1.0, 0.1)):
    """{"pred", "loss_accel", "loss_pos", every parameter gradient of loss_pos + loss_accel} as float64 arrays of a `dt` run"""
    pred, C = infiller_forward(sd, opt, batch, pos, dt)
    la, lp, d = motion_losses(batch["gt_obj"], pred, *lw)
    g = infiller_backward(sd, opt, C, d)
    g.update(pred=pred, loss_accel=np.asarray(la), loss_pos=np.asarray(lp))
    return {k: np.asarray(v, dtype=np.float64) for k, v in g.items()}


def adam_trajectory(sd, opt, batch, pos, steps, lr, dt=np.float64, betas=(0.9, 0.999), eps=1e-8):
    """the objective BEFORE each of `steps` torch.optim.Adam steps (defaults) on one fixed batch, all arithmetic in `dt`"""
    P = {k: np.asarray(v).astype(dt) for k, v in sd.items()}
    m = {k: np.zeros_like(v) for k, v in P.items()}; v2 = {k: np.zeros_like(v) for k, v in P.items()}
    out = []
    for t in range(1, steps + 1):
        r = infiller_run(P, opt, batch, pos, dt)
        out.append(float(r["loss_pos"] + r["loss_accel"]))
        bc1, bc2 = 1 - betas[0] ** t, 1 - betas[1] ** t
        for k in P:
            gk = r[k].astype(dt)
            m[k] = dt(betas[0]) * m[k] + dt(1 - betas[0]) * gk
            v2[k] = dt(betas[1]) * v2[k] + dt(1 - betas[1]) * gk * gk
            P[k] = (P[k] - dt(lr / bc1) * m[k] / (np.sqrt(v2[k]) / dt(math.sqrt(bc2)) + dt(eps))).astype(dt)
    return out
