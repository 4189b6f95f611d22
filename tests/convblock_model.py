"""A float64 torch model of the encoders' ConvBlock (model/net_util.py:346-396) and of its backward, written from those lines with F.group_norm / F.conv2d and
autograd.  It shares no code with the product (vistracker_amd/csrc/convtrain.hip, ops.conv_block_train).  Tensors are NCHW numpy / torch arrays here.

reference_and_e32(P, x, dy)           the float64 gradients per output tensor and e32 = the largest |float32 run - float64 run| of each (the bound convention of
                                      tests/test_gpu_dectrain.py / test_gpu_mapgrad.py: the kernel gets 4 e32)
manual_grads(P, x, dy, saved=None)    the same gradients from the explicit formulas (GroupNorm + ReLU backward below), in float64, at SAVED activations:
                                      saved = {"raw": o1 | o2, "stats": [(mean, rstd) of bn1, bn2, bn3]} from outside (a GPU forward) or the model's own.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
GROUPS = 32
GRAD_NAMES = ("d_x", "conv1.weight", "conv2.weight", "conv3.weight", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias", "bn3.weight", "bn3.bias",
              "bn4.weight", "bn4.bias", "downsample.2.weight")
GOLDEN_WEIGHT_STEP = 4          # tests/golden/convblock.npz keeps every 4th element of a convolution's weight gradient (flattened)


def make_params(cin, cout, seed):
    """synthetic parameters under the reference's state_dict keys (float32 values): convolution weights ~ N(0, 1 / fan_in), gamma ~ 1 +- 0.3, beta ~ +- 0.3"""
    r = np.random.RandomState(seed)
    c1, c2, c3 = cout // 2, cout // 4, cout // 4
    P = {}
    for i, (co, ci) in enumerate(((c1, cin), (c2, c1), (c3, c2)), 1):
        P[f"conv{i}.weight"] = (r.randn(co, ci, 3, 3) / np.sqrt(9 * ci)).astype(np.float32)
        P[f"bn{i}.weight"] = (1 + 0.3 * r.randn(ci)).astype(np.float32)
        P[f"bn{i}.bias"] = (0.3 * r.randn(ci)).astype(np.float32)
    P["bn4.weight"] = (1 + 0.3 * r.randn(cin)).astype(np.float32)
    P["bn4.bias"] = (0.3 * r.randn(cin)).astype(np.float32)
    if cin != cout:
        P["downsample.2.weight"] = (r.randn(cout, cin, 1, 1) / np.sqrt(cin)).astype(np.float32)
        P["downsample.0.weight"], P["downsample.0.bias"] = P["bn4.weight"], P["bn4.bias"]
    return P


def make_inputs(B, H, W, cin, cout, seed):
    """block input x (B,cin,H,W): per-channel offsets and scales so that GroupNorm has work to do; upstream gradient dy (B,cout,H,W)"""
    r = np.random.RandomState(seed)
    x = (r.randn(B, cin, H, W) * (0.5 + r.rand(1, cin, 1, 1)) + 0.5 * r.randn(1, cin, 1, 1)).astype(np.float32)
    dy = r.randn(B, cout, H, W).astype(np.float32)
    return x, dy


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def forward(P, x, dtype=torch.float64, leaves=False):
    """net_util.py:374-396 -> (out, {name: tensor} of the leaves when ``leaves``, o1, o2)"""
    p = {k: _t(v, dtype) for k, v in P.items() if not k.startswith("downsample.0")}
    xt = _t(x, dtype)
    if leaves:
        xt.requires_grad_(True)
        for v in p.values():
            v.requires_grad_(True)
    o1 = F.conv2d(F.relu(F.group_norm(xt, GROUPS, p["bn1.weight"], p["bn1.bias"], EPS)), p["conv1.weight"], None, 1, 1)
    o2 = F.conv2d(F.relu(F.group_norm(o1, GROUPS, p["bn2.weight"], p["bn2.bias"], EPS)), p["conv2.weight"], None, 1, 1)
    o3 = F.conv2d(F.relu(F.group_norm(o2, GROUPS, p["bn3.weight"], p["bn3.bias"], EPS)), p["conv3.weight"], None, 1, 1)
    res = xt
    if "downsample.2.weight" in p:
        res = F.conv2d(F.relu(F.group_norm(xt, GROUPS, p["bn4.weight"], p["bn4.bias"], EPS)), p["downsample.2.weight"])
    out = torch.cat((o1, o2, o3), 1) + res
    return out, dict(p, d_x=xt), o1, o2


def autograd_grads(P, x, dy, dtype=torch.float64):
    """{name: float64 numpy} over GRAD_NAMES (those the block has; an identity block's bn4 is unused and absent), + "out" """
    out, lv, _, _ = forward(P, x, dtype, leaves=True)
    (out * _t(dy, dtype)).sum().backward()
    g = {"out": out.detach().double().numpy()}
    for n in GRAD_NAMES:
        if n in lv and lv[n].grad is not None:
            g[n] = lv[n].grad.double().numpy()
    return g


def reference_and_e32(P, x, dy):
    g64, g32 = autograd_grads(P, x, dy, torch.float64), autograd_grads(P, x, dy, torch.float32)
    return g64, {n: float(np.abs(g32[n] - g64[n]).max()) for n in g64}


def group_stats(x):
    """(mean, rstd), each (B, 32), of a float64 NCHW tensor"""
    B, C = x.shape[:2]
    v = x.reshape(B, GROUPS, -1)
    mean = v.mean(2)
    return mean, 1.0 / torch.sqrt(((v - mean[..., None]) ** 2).mean(2) + EPS)


def saved_from_model(P, x):
    _, _, o1, o2 = forward(P, x, torch.float64)
    xt = _t(x, torch.float64)
    return {"raw": torch.cat((o1, o2), 1).numpy(), "stats": [tuple(s.numpy() for s in group_stats(t)) for t in (xt, o1, o2)]}


def gn_relu(x, mean, rstd, gamma, beta):
    """a = max(xhat gamma + beta, 0), xhat, mask; x (B,C,H,W) float64, mean / rstd (B,32)"""
    B, C = x.shape[:2]
    e = lambda s: s.repeat_interleave(C // GROUPS, 1)[:, :, None, None]     # noqa: E731
    xhat = (x - e(mean)) * e(rstd)
    pre = xhat * gamma[None, :, None, None] + beta[None, :, None, None]
    return pre.clamp_min(0), xhat, (pre > 0).to(x.dtype)


def gn_relu_backward(g, x, mean, rstd, gamma, beta):
    """the formula of the issue / vt_gn_relu_backward: m = [xhat gamma + beta > 0], n = elements of a group in one frame;
    dbeta = sum g m, dgamma = sum g m xhat, s1 = sum g m gamma, s2 = sum g m gamma xhat per (frame, group), d_x = rstd (g m gamma - (s1 + xhat s2) / n)"""
    B, C, H, W = x.shape
    cg = C // GROUPS
    _, xhat, m = gn_relu(x, mean, rstd, gamma, beta)
    gm = g * m
    dbeta, dgamma = gm.sum((0, 2, 3)), (gm * xhat).sum((0, 2, 3))
    e = gm * gamma[None, :, None, None]
    s1 = e.reshape(B, GROUPS, -1).sum(2).repeat_interleave(cg, 1)[:, :, None, None]
    s2 = (e * xhat).reshape(B, GROUPS, -1).sum(2).repeat_interleave(cg, 1)[:, :, None, None]
    n = cg * H * W
    d_x = rstd.repeat_interleave(cg, 1)[:, :, None, None] * (e - (s1 + xhat * s2) / n)
    return d_x, dgamma, dbeta


def conv_grads(a, w, d_o, pad):
    """(d_a, dW) of o = conv2d(a, w, padding=pad) for the upstream d_o, by autograd on the convolution alone"""
    a = a.detach().requires_grad_(True); w = w.detach().requires_grad_(True)
    da, dw = torch.autograd.grad(F.conv2d(a, w, None, 1, pad), (a, w), d_o)
    return da, dw


def manual_grads(P, x, dy, saved=None):
    """net_util.py:374-396 backwards, float64, explicit: every activation is recomputed from SAVED tensors (x, raw = o1 | o2, the {mean, rstd} of bn1..3) the way
    the kernels do, so that with a GPU forward's saved tensors this is the exact gradient AT those activations."""
    saved = saved or saved_from_model(P, x)
    p = {k: _t(v, torch.float64) for k, v in P.items()}
    xt, dyt, raw = _t(x, torch.float64), _t(dy, torch.float64), _t(saved["raw"], torch.float64)
    st = [tuple(_t(s, torch.float64) for s in pair) for pair in saved["stats"]]
    c1, c2 = p["conv1.weight"].shape[0], p["conv2.weight"].shape[0]
    o1, o2 = raw[:, :c1], raw[:, c1:c1 + c2]
    g = {}
    a3 = gn_relu(o2, *st[2], p["bn3.weight"], p["bn3.bias"])[0]
    da3, g["conv3.weight"] = conv_grads(a3, p["conv3.weight"], dyt[:, c1 + c2:], 1)
    t, g["bn3.weight"], g["bn3.bias"] = gn_relu_backward(da3, o2, *st[2], p["bn3.weight"], p["bn3.bias"])
    d_o2 = dyt[:, c1:c1 + c2] + t
    a2 = gn_relu(o1, *st[1], p["bn2.weight"], p["bn2.bias"])[0]
    da2, g["conv2.weight"] = conv_grads(a2, p["conv2.weight"], d_o2, 1)
    t, g["bn2.weight"], g["bn2.bias"] = gn_relu_backward(da2, o1, *st[1], p["bn2.weight"], p["bn2.bias"])
    d_o1 = dyt[:, :c1] + t
    a1 = gn_relu(xt, *st[0], p["bn1.weight"], p["bn1.bias"])[0]
    da1, g["conv1.weight"] = conv_grads(a1, p["conv1.weight"], d_o1, 1)
    d_x, g["bn1.weight"], g["bn1.bias"] = gn_relu_backward(da1, xt, *st[0], p["bn1.weight"], p["bn1.bias"])
    if "downsample.2.weight" in p:
        a4 = gn_relu(xt, *st[0], p["bn4.weight"], p["bn4.bias"])[0]
        da4, g["downsample.2.weight"] = conv_grads(a4, p["downsample.2.weight"], dyt, 0)
        t, g["bn4.weight"], g["bn4.bias"] = gn_relu_backward(da4, xt, *st[0], p["bn4.weight"], p["bn4.bias"])
        d_x = d_x + t
    else:
        d_x = d_x + dyt
    g["d_x"] = d_x
    return {k: v.numpy() for k, v in g.items()}
