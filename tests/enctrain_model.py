"""A float64 model of the rows that make the reference's ``HGFilter`` (model/HGFilters.py:56-203) whole: the stem conv1 -> bn1 -> ReLU (lines 120, 125, 167), the
1 x 1 tail of a stack (lines 191-201) and the filter itself, written from those lines with F.conv2d / F.group_norm and autograd.  It extends
tests/convblock_model.py (M) and tests/hourglass_model.py (HM) and shares no code with the product (vistracker_amd/csrc/enctrain.hip, ops.stem_train,
ops.stack_tail_train, encoder.TrainableHGFilter).  Tensors are NCHW numpy / torch arrays.

stem_* / tail_*     make_params, make_inputs, autograd_grads (float64 or float32), reference_and_e32, manual_grads: the explicit formulas in float64 AT saved
                    activations (a GPU forward's or the model's own).  ``mutant`` exists for tests/test_host_enctrain.py only.
filter_*            make_params under the reference's state_dict keys, autograd_grads / reference_and_e32 over every leaf, and manual_grads: the chain of the
                    blocks' manual formulas over a tape of saved activations.
"""
import numpy as np
import torch
import torch.nn.functional as F

import convblock_model as M
import hourglass_model as HM
import resample_model as R

GOLDEN_WEIGHT_STEP = 32         # tests/golden/enctrain_*.npz keep every 32nd element of a convolution's weight gradient (flattened)
# the whole-filter cases of tests/test_gpu_enctrain.py and tools/gen_golden_enctrain.py: Cin, tmpx, hourglass_dim, seed; 2 stacks of depth 1, B = 1, 64 x 128 input --
# the smallest size at which the innermost level of an hourglass is still 8 x 16, with a joined stack and a last stack
FILTER_CASES = {"image": (5, 64, 256, 51), "triplane": (1, 32, 64, 53)}
FILTER_NUM_STACK, FILTER_DEPTH, FILTER_B, FILTER_H, FILTER_W = 2, 1, 1, 64, 128


def _t(a, dtype=torch.float64):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def _e32(g64, g32):
    return {n: float(np.abs(g32[n] - g64[n]).max()) for n in g64}


# ---- the stem -------------------------------------------------------------------------------------------------------------------------------------------------
def stem_make_params(cin, cout, seed):
    r = np.random.RandomState(seed)
    return {"conv1.weight": (r.randn(cout, cin, 7, 7) / np.sqrt(49 * cin)).astype(np.float32), "conv1.bias": (0.3 * r.randn(cout)).astype(np.float32),
            "bn1.weight": (1 + 0.3 * r.randn(cout)).astype(np.float32), "bn1.bias": (0.3 * r.randn(cout)).astype(np.float32)}


def stem_make_inputs(B, H, W, cin, cout, seed):
    r = np.random.RandomState(seed)
    return r.rand(B, cin, H, W).astype(np.float32), r.randn(B, cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1).astype(np.float32)


def stem_forward(p, x):
    """-> (tmpx, conv1's output) on torch tensors"""
    y1 = F.conv2d(x, p["conv1.weight"], p["conv1.bias"], 2, 3)
    return F.relu(F.group_norm(y1, M.GROUPS, p["bn1.weight"], p["bn1.bias"], M.EPS)), y1


def stem_autograd_grads(P, x, dy, dtype=torch.float64):
    p = {k: _t(v, dtype).requires_grad_(True) for k, v in P.items()}
    y, _ = stem_forward(p, _t(x, dtype))
    (y * _t(dy, dtype)).sum().backward()
    g = {k: v.grad.double().numpy() for k, v in p.items()}
    g["out"] = y.detach().double().numpy()
    return g


def stem_reference_and_e32(P, x, dy):
    g64 = stem_autograd_grads(P, x, dy)
    return g64, _e32(g64, stem_autograd_grads(P, x, dy, torch.float32))


def stem_saved_from_model(P, x):
    with torch.no_grad():
        y, y1 = stem_forward({k: _t(v) for k, v in P.items()}, _t(x))
    return {"y1": y1.numpy(), "y": y.numpy(), "stats": tuple(s.numpy() for s in M.group_stats(y1))}


def gn_relu_backward_masked(g, x, mean, rstd, gamma, m):
    """GroupNorm + ReLU backward with the mask GIVEN: dbeta = sum g m, dgamma = sum g m xhat, s1 = sum g m gamma, s2 = sum g m gamma xhat per (frame, group),
    d_x = rstd (g m gamma - (s1 + xhat s2) / n), n = elements of a group in one frame"""
    B, C, H, W = x.shape
    cg = C // M.GROUPS
    e_ = lambda s: s.repeat_interleave(cg, 1)[:, :, None, None]      # noqa: E731
    xhat = (x - e_(mean)) * e_(rstd)
    gm = g * m
    dbeta, dgamma = gm.sum((0, 2, 3)), (gm * xhat).sum((0, 2, 3))
    e = gm * gamma[None, :, None, None]
    s1 = e_(e.reshape(B, M.GROUPS, -1).sum(2))
    s2 = e_((e * xhat).reshape(B, M.GROUPS, -1).sum(2))
    return e_(rstd) * (e - (s1 + xhat * s2) / (cg * H * W)), dgamma, dbeta


def staging_mask(y1, mean, rstd, gamma, beta):
    """[fma(x, rstd gamma, beta - mean rstd gamma) > 0] in float32 (the expression vt_gn_relu_backward recomputes); float32 arrays, mean / rstd (B, 32)"""
    cg = y1.shape[1] // M.GROUPS
    a_ = np.repeat(rstd, cg, 1)[:, :, None, None] * gamma[None, :, None, None]
    s_ = beta[None, :, None, None] - np.repeat(mean, cg, 1)[:, :, None, None] * a_
    return (y1.astype(np.float64) * a_.astype(np.float64) + s_.astype(np.float64)).astype(np.float32) > 0        # exact product, one rounding: the fma


def forward_expression(y1, mean, rstd, gamma, beta):
    """max((x - mean) rstd gamma + beta, 0) in float32, operation by operation (vt_groupnorm_nhwc)"""
    cg = y1.shape[1] // M.GROUPS
    return np.maximum((y1 - np.repeat(mean, cg, 1)[:, :, None, None]) * np.repeat(rstd, cg, 1)[:, :, None, None] * gamma[None, :, None, None] + beta[None, :, None, None],
                      np.float32(0))


def planted_gn_case(C, B, H, W, seed):
    """a GroupNorm + ReLU backward case with elements planted where the forward's expression and the staging expression disagree in sign: values next to the zero
    crossing of their channel, searched float by float.  -> dict(g, y1, y = the forward's float32 output, stats = (mean, rstd) float32 (B, 32), gamma, beta,
    disagree = number of elements whose two masks differ)"""
    r = np.random.RandomState(seed)
    y1 = (r.randn(B, C, H, W) * (0.5 + r.rand(1, C, 1, 1)) + 0.5 * r.randn(1, C, 1, 1)).astype(np.float32)
    gamma, beta = (1 + 0.3 * r.randn(C)).astype(np.float32), (0.3 * r.randn(C)).astype(np.float32)
    mean, rstd = (s.numpy().astype(np.float32) for s in M.group_stats(_t(y1)))
    if H * W == 1 and C == M.GROUPS:            # one element per group: xhat = 0, the sign is beta's alone; nothing to plant
        rstd = np.full_like(rstd, 1.0 / np.sqrt(M.EPS))
    else:
        cg = C // M.GROUPS
        a_ = np.repeat(rstd, cg, 1) * gamma[None]
        zero = (np.repeat(mean, cg, 1) - beta[None] / a_).astype(np.float32)         # (B, C): the crossing, up to rounding
        v = np.zeros((B, C, 1, 1), np.float32) + zero[:, :, None, None]
        for _ in range(40):
            v = np.nextafter(v, np.float32(np.inf))
        for _ in range(80):
            v = np.nextafter(v, np.float32(-np.inf))
            dis = staging_mask(v, mean, rstd, gamma, beta) != (forward_expression(v, mean, rstd, gamma, beta) > 0)
            for b, c in zip(*np.nonzero(dis[:, :, 0, 0])):
                y1[b, c, (c // W) % H, c % W] = v[b, c, 0, 0]
    y = forward_expression(y1, mean, rstd, gamma, beta)
    return dict(g=r.randn(B, C, H, W).astype(np.float32), y1=y1, y=y, stats=(mean, rstd), gamma=gamma, beta=beta,
                disagree=int((staging_mask(y1, mean, rstd, gamma, beta) != (y > 0)).sum()))


def gn_y_grads(c, dtype=torch.float64, mask=None):
    """{"d_x", "dgamma", "dbeta"} of a planted_gn_case by the masked formula at its saved tensors, in dtype; mask None: read from y"""
    m = _t((c["y"] > 0) if mask is None else mask, dtype)
    d_x, dgamma, dbeta = gn_relu_backward_masked(_t(c["g"], dtype), _t(c["y1"], dtype), _t(c["stats"][0], dtype), _t(c["stats"][1], dtype), _t(c["gamma"], dtype), m)
    return {"d_x": d_x.double().numpy(), "dgamma": dgamma.double().numpy(), "dbeta": dbeta.double().numpy()}


def stem_wgrad(d_y1, x, pad=3):
    """dW[co,ci,ky,kx] = sum (b,oy,ox) d_y1[b,co,oy,ox] x[b,ci,2oy+ky-pad,2ox+kx-pad], zero outside the image"""
    B, co, H2, W2 = d_y1.shape
    xp = F.pad(x, (4, 4, 4, 4))
    dW = torch.zeros(co, x.shape[1], 7, 7, dtype=x.dtype)
    for ky in range(7):
        for kx in range(7):
            y0, x0 = ky - pad + 4, kx - pad + 4
            dW[:, :, ky, kx] = torch.einsum("bohw,bihw->oi", d_y1, xp[:, :, y0:y0 + 2 * H2 - 1:2, x0:x0 + 2 * W2 - 1:2])
    return dW


def stem_manual_grads(P, x, dy, saved=None, mutant=None):
    """float64, explicit, at SAVED activations: y1 = conv1's output, y = tmpx (the mask is y > 0), stats = (mean, rstd) of bn1"""
    saved = saved or stem_saved_from_model(P, x)
    p = {k: _t(v) for k, v in P.items()}
    y1, y, (mean, rstd) = _t(saved["y1"]), _t(saved["y"]), tuple(_t(s) for s in saved["stats"])
    m = (y > 0).double()
    if mutant == "staging_mask":        # the mask recomputed with the float32 staging expression instead of read from y
        f32 = lambda t: t.float().numpy()       # noqa: E731
        m = _t(staging_mask(f32(y1), f32(mean), f32(rstd), f32(p["bn1.weight"]), f32(p["bn1.bias"])).astype(np.float64))
    d_y1, dgamma, dbeta = gn_relu_backward_masked(_t(dy), y1, mean, rstd, p["bn1.weight"], m)
    frames = d_y1[1:] if mutant == "bias_missing_frame" else d_y1
    return {"conv1.weight": stem_wgrad(d_y1, _t(x), pad=2 if mutant == "pad2" else 3).numpy(), "conv1.bias": frames.sum((0, 2, 3)).numpy(),
            "bn1.weight": dgamma.numpy(), "bn1.bias": dbeta.numpy()}


# ---- the tail of a stack ----------------------------------------------------------------------------------------------------------------------------------------
TAIL_NAMES = ("conv_last", "bn_end", "l", "bl", "al")


def tail_make_params(C, Co, last, seed):
    r = np.random.RandomState(seed)
    P = {}
    for n, (co, ci) in (("conv_last", (C, C)), ("l", (Co, C))) + (() if last else (("bl", (C, C)), ("al", (C, Co)))):
        P[n + ".weight"] = (r.randn(co, ci, 1, 1) / np.sqrt(ci)).astype(np.float32)
        P[n + ".bias"] = (0.3 * r.randn(co)).astype(np.float32)
    P["bn_end.weight"] = (1 + 0.3 * r.randn(C)).astype(np.float32)
    P["bn_end.bias"] = (0.3 * r.randn(C)).astype(np.float32)
    return P


def tail_make_inputs(B, H, W, C, Co, seed):
    """ll, previous, d_out, d_prev"""
    r = np.random.RandomState(seed)
    ll = (r.randn(B, C, H, W) * (0.5 + r.rand(1, C, 1, 1)) + 0.5 * r.randn(1, C, 1, 1)).astype(np.float32)
    return ll, r.randn(B, C, H, W).astype(np.float32), r.randn(B, Co, H, W).astype(np.float32), r.randn(B, C, H, W).astype(np.float32)


def tail_forward(p, ll, previous):
    """HGFilters.py:191-201 on torch tensors -> (out, previous' or None, raw)"""
    raw = F.conv2d(ll, p["conv_last.weight"], p["conv_last.bias"])
    a = F.relu(F.group_norm(raw, M.GROUPS, p["bn_end.weight"], p["bn_end.bias"], M.EPS))
    out = F.conv2d(a, p["l.weight"], p["l.bias"])
    if "bl.weight" not in p:
        return out, None, raw
    return out, previous + F.conv2d(a, p["bl.weight"], p["bl.bias"]) + F.conv2d(out, p["al.weight"], p["al.bias"]), raw


def tail_autograd_grads(P, ll, previous, d_out, d_prev, dtype=torch.float64):
    """{"d_ll", parameter names, "out", "prev"}; d_out / d_prev None = zero"""
    p = {k: _t(v, dtype).requires_grad_(True) for k, v in P.items()}
    llt = _t(ll, dtype).requires_grad_(True)
    out, prev, _ = tail_forward(p, llt, _t(previous, dtype))
    loss = 0
    if d_out is not None:
        loss = loss + (out * _t(d_out, dtype)).sum()
    if d_prev is not None and prev is not None:
        loss = loss + (prev * _t(d_prev, dtype)).sum()
    loss.backward()
    g = {k: v.grad.double().numpy() for k, v in p.items() if v.grad is not None}
    g["d_ll"] = llt.grad.double().numpy()
    g["out"] = out.detach().double().numpy()
    if prev is not None:
        g["prev"] = prev.detach().double().numpy()
    return g


def tail_reference_and_e32(P, ll, previous, d_out, d_prev):
    g64 = tail_autograd_grads(P, ll, previous, d_out, d_prev)
    return g64, _e32(g64, tail_autograd_grads(P, ll, previous, d_out, d_prev, torch.float32))


def tail_saved_from_model(P, ll, previous):
    with torch.no_grad():
        out, _, raw = tail_forward({k: _t(v) for k, v in P.items()}, _t(ll), _t(previous))
    return {"raw": raw.numpy(), "out": out.numpy(), "stats": tuple(s.numpy() for s in M.group_stats(raw))}


def tail_manual_grads(P, ll, d_out, d_prev, saved, mutant=None):
    """the formulas of the issue in float64 at SAVED activations (raw, out, the (mean, rstd) of bn_end); d_out / d_prev None = zero"""
    p = {k: _t(v) for k, v in P.items()}
    raw, out, (mean, rstd) = _t(saved["raw"]), _t(saved["out"]), tuple(_t(s) for s in saved["stats"])
    llt = _t(ll)
    w = lambda n: p[n + ".weight"][:, :, 0, 0]      # noqa: E731
    bwd = lambda wt, d: torch.einsum("oi,bohw->bihw", wt, d)        # noqa: E731  W^T d
    outer = lambda d, a: torch.einsum("bohw,bihw->oi", d, a)[:, :, None, None]      # noqa: E731
    a = M.gn_relu(raw, mean, rstd, p["bn_end.weight"], p["bn_end.bias"])[0]
    g = {}
    dp = None if d_prev is None or "bl.weight" not in p else _t(d_prev)
    g_out = torch.zeros_like(out) if d_out is None else _t(d_out)
    if dp is not None:
        if mutant != "no_al_in_gout":
            g_out = g_out + bwd(w("al"), dp)
        g["al.weight"], g["bl.weight"] = outer(dp, out), outer(dp, a)
        g["al.bias"] = g["bl.bias"] = (dp[1:] if mutant == "bias_missing_frame" else dp).sum((0, 2, 3))
    d_a = bwd(w("l"), g_out)
    if dp is not None and mutant != "no_bl_in_da":
        d_a = d_a + bwd(w("bl"), dp)
    g["l.weight"], g["l.bias"] = outer(g_out, a), (g_out[1:] if mutant == "bias_missing_frame" else g_out).sum((0, 2, 3))
    d_raw, g["bn_end.weight"], g["bn_end.bias"] = M.gn_relu_backward(d_a, raw, mean, rstd, p["bn_end.weight"], p["bn_end.bias"])
    g["conv_last.weight"], g["conv_last.bias"] = outer(d_raw, llt), (d_raw[1:] if mutant == "bias_missing_frame" else d_raw).sum((0, 2, 3))
    g["d_ll"] = bwd(w("conv_last"), d_raw)
    return {k: v.numpy() for k, v in g.items()}


# ---- the whole filter -------------------------------------------------------------------------------------------------------------------------------------------
def filter_block_names(num_stack):
    return ["conv2", "conv3", "conv4"] + [f"top_m_{i}" for i in range(num_stack)]


def filter_make_params(cin, tmpx, hg_dim, num_stack, depth, seed):
    """synthetic parameters under HGFilter.state_dict()'s keys (identity blocks carry no bn4 here: the reference never uses it, net_util.py:371-372)"""
    P = dict(stem_make_params(cin, tmpx, seed))
    for j, (n, (ci, co)) in enumerate((("conv2", (tmpx, 128)), ("conv3", (128, 128)), ("conv4", (128, 256)))):
        P.update({f"{n}.{k}": v for k, v in M.make_params(ci, co, seed + 10 + j).items() if ci != co or not k.startswith("bn4")})
    for i in range(num_stack):
        P.update({f"m{i}.{k}": v for k, v in HM.make_params(depth, 256, seed + 100 * (i + 1)).items() if ".bn4" not in k})
        P.update({f"top_m_{i}.{k}": v for k, v in M.make_params(256, 256, seed + 100 * (i + 1) + 50).items() if not k.startswith("bn4")})
        for k, v in tail_make_params(256, hg_dim, i == num_stack - 1, seed + 100 * (i + 1) + 60).items():
            n, s = k.split(".")
            P[f"{n}{i}.{s}"] = v
    return P


def filter_case(tag):
    """(P, x, d_outs, d_normx) of a FILTER_CASES entry, regenerated from its seed"""
    cin, tmpx, hg, seed = FILTER_CASES[tag]
    P = filter_make_params(cin, tmpx, hg, FILTER_NUM_STACK, FILTER_DEPTH, seed)
    r = np.random.RandomState(seed + 1)
    x = r.rand(FILTER_B, cin, FILTER_H, FILTER_W).astype(np.float32)
    d_outs = [r.randn(FILTER_B, hg, FILTER_H // 4, FILTER_W // 4).astype(np.float32) for _ in range(FILTER_NUM_STACK)]
    return P, x, d_outs, r.randn(FILTER_B, 128, FILTER_H // 4, FILTER_W // 4).astype(np.float32)


def _sub(P, prefix):
    return {k[len(prefix):]: v for k, v in P.items() if k.startswith(prefix)}


def filter_tail_params(P, i):
    return {f"{n}.{s}": P[f"{n}{i}.{s}"] for n in TAIL_NAMES for s in ("weight", "bias") if f"{n}{i}.{s}" in P}


def _num_stack(P):
    return 1 + max(int(k[len("conv_last"):].split(".")[0]) for k in P if k.startswith("conv_last"))


def _block(p, x):
    o1 = F.conv2d(F.relu(F.group_norm(x, M.GROUPS, p["bn1.weight"], p["bn1.bias"], M.EPS)), p["conv1.weight"], None, 1, 1)
    o2 = F.conv2d(F.relu(F.group_norm(o1, M.GROUPS, p["bn2.weight"], p["bn2.bias"], M.EPS)), p["conv2.weight"], None, 1, 1)
    o3 = F.conv2d(F.relu(F.group_norm(o2, M.GROUPS, p["bn3.weight"], p["bn3.bias"], M.EPS)), p["conv3.weight"], None, 1, 1)
    res = x
    if "downsample.2.weight" in p:
        res = F.conv2d(F.relu(F.group_norm(x, M.GROUPS, p["bn4.weight"], p["bn4.bias"], M.EPS)), p["downsample.2.weight"])
    return torch.cat((o1, o2, o3), 1) + res, o1, o2


def filter_run(P, x, dtype=torch.float64, leaves=False):
    """HGFilter.forward (HGFilters.py:162-203) -> (outputs, tmpx, normx, p the leaves, tape): tape[name] = (input, o1, o2) per ConvBlock ("conv2", "m0.b1_2", ...),
    tape["stem"] = (y1, y), tape["tail<i>"] = (ll, raw, out)"""
    p = {k: _t(v, dtype) for k, v in P.items() if ".downsample.0" not in k}
    if leaves:
        for v in p.values():
            v.requires_grad_(True)
    tape = {}

    def blk(name, t):
        o, o1, o2 = _block(_sub(p, name + "."), t)
        tape[name] = (t, o1, o2)
        return o

    y, y1 = stem_forward(p, _t(x, dtype))
    tape["stem"] = (y1, y)
    pool = torch.as_tensor
    c2 = blk("conv2", y)
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    normx = torch.einsum("oy,bcyx,px->bcop", pool(R.pool_matrix(c2.shape[2], np_dt)), c2, pool(R.pool_matrix(c2.shape[3], np_dt)))
    previous = blk("conv4", blk("conv3", normx))
    outputs = []
    depth = HM._depth(_sub(P, "m0."))
    for i in range(_num_stack(P)):
        sub = {}
        hg = HM._level(_sub(p, f"m{i}."), depth, previous, sub)
        tape.update({f"m{i}.{k}": v for k, v in sub.items()})
        ll = blk(f"top_m_{i}", hg)
        out, prev2, raw = tail_forward(filter_tail_params(p, i), ll, previous)
        tape[f"tail{i}"] = (ll, raw, out)
        outputs.append(out)
        if prev2 is not None:
            previous = prev2
    return outputs, y, normx, p, tape


def filter_autograd_grads(P, x, d_outs, d_normx=None, dtype=torch.float64):
    """gradients of sum_i <outputs[i], d_outs[i]> (+ <normx, d_normx>) to every leaf; d_outs[i] None = zero.  + "out<i>", "tmpx", "normx" """
    outputs, tmpx, normx, p, _ = filter_run(P, x, dtype, leaves=True)
    loss = 0
    for o, d in zip(outputs, d_outs):
        if d is not None:
            loss = loss + (o * _t(d, dtype)).sum()
    if d_normx is not None:
        loss = loss + (normx * _t(d_normx, dtype)).sum()
    loss.backward()
    g = {k: v.grad.double().numpy() for k, v in p.items() if v.grad is not None}
    g.update({f"out{i}": o.detach().double().numpy() for i, o in enumerate(outputs)})
    g["tmpx"], g["normx"] = tmpx.detach().double().numpy(), normx.detach().double().numpy()
    return g


def filter_reference_and_e32(P, x, d_outs, d_normx=None):
    g64 = filter_autograd_grads(P, x, d_outs, d_normx)
    return g64, _e32(g64, filter_autograd_grads(P, x, d_outs, d_normx, torch.float32))


def filter_saved_from_model(P, x):
    """the tape of the float64 forward in the form filter_manual_grads reads"""
    with torch.no_grad():
        tape = filter_run(P, x)[4]
    sv = {}
    for name, t in tape.items():
        if name == "stem":
            sv[name] = {"y1": t[0].numpy(), "y": t[1].numpy(), "stats": tuple(s.numpy() for s in M.group_stats(t[0]))}
        elif name.startswith("tail"):
            sv[name] = {"ll": t[0].numpy(), "raw": t[1].numpy(), "out": t[2].numpy(), "stats": tuple(s.numpy() for s in M.group_stats(t[1]))}
        else:
            sv[name] = {"x": t[0].numpy(), "raw": torch.cat((t[1], t[2]), 1).numpy(), "stats": [tuple(s.numpy() for s in M.group_stats(v)) for v in t]}
    return sv


def filter_manual_grads(P, x, d_outs, d_normx, saved):
    """the backward of HGFilter.forward in float64 AT saved activations: the manual formulas of every block (M.manual_grads, HM.manual_grads, tail_manual_grads,
    stem_manual_grads) chained by hand.  saved: filter_saved_from_model's layout (a GPU forward's tensors, or the model's)."""
    g = {}
    ns = _num_stack(P)
    depth = HM._depth(_sub(P, "m0."))

    def block_back(name, d):
        gb = M.manual_grads(_sub(P, name + "."), saved[name]["x"], d, saved[name])
        g.update({f"{name}.{k}": v for k, v in gb.items() if k != "d_x"})
        return gb["d_x"]

    d_prev = None
    for i in range(ns - 1, -1, -1):
        sv = saved[f"tail{i}"]
        if d_outs[i] is None and d_prev is None:
            continue
        gt = tail_manual_grads(filter_tail_params(P, i), sv["ll"], d_outs[i], d_prev, sv)
        for k, v in gt.items():
            if k != "d_ll":
                n, s = k.split(".")
                g[f"{n}{i}.{s}"] = v
        d_hg = block_back(f"top_m_{i}", gt["d_ll"])
        gh = HM.manual_grads(_sub(P, f"m{i}."), None, d_hg, {k[len(f"m{i}."):]: v for k, v in saved.items() if k.startswith(f"m{i}.")})
        g.update({f"m{i}.{k}": v for k, v in gh.items() if k != "d_x"})
        d_prev = gh["d_x"] if d_prev is None else gh["d_x"] + d_prev         # previous feeds the hourglass and the sum (HGFilters.py:186, 201)
    d_n = None if d_normx is None else np.asarray(d_normx, np.float64)
    if d_prev is not None:
        d3 = block_back("conv3", block_back("conv4", d_prev))
        d_n = d3 if d_n is None else d_n + d3
    d_t = block_back("conv2", R.avgpool_backward(d_n))
    g.update(stem_manual_grads(_sub(P, ""), x, d_t, saved["stem"]))
    return g
