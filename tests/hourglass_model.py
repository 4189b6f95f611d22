"""A float64 model of the reference's ``HourGlass(1, depth, features, norm='group')`` (model/HGFilters.py:4-53) and of its backward: the ConvBlock of
tests/convblock_model.py joined by the matrices of tests/resample_model.py.  It shares no code with the product.  Tensors are NCHW numpy / torch arrays.

make_params(depth, features, seed)     {"b1_2.conv1.weight": ...} under the reference's state_dict keys: convblock_model.make_params per block, seed + its index
make_inputs(B, H, W, features, seed)   convblock_model.make_inputs
forward(P, x, dtype)                   the output (numpy float64)
reference_and_e32(P, x, dy)            float64 autograd gradients {"d_x", "<block>.<parameter>", "out"} and e32 = the largest |float32 run - float64 run| of each
manual_grads(P, x, dy, saved)          the same gradients in float64 AT saved activations: saved[block] = {"x": the block's input, "raw", "stats"} (a GPU forward's,
                                       or saved_from_model's); convblock_model.manual_grads per block, chained through the transposed matrices
"""
import numpy as np
import torch
import torch.nn.functional as F

import convblock_model as M
import resample_model as R

GOLDEN_WEIGHT_STEP = M.GOLDEN_WEIGHT_STEP
GOLDEN_OUT_STEP = 64            # tests/golden/hourglass.npz keeps every 64th element of the flattened output (d_x is stored whole)


def block_names(depth):
    """registration order of HourGlass._generate_network (HGFilters.py:14-24)"""
    names = []
    for n in range(depth, 0, -1):
        names += [f"b1_{n}", f"b2_{n}"]
    names.append("b2_plus_1")
    return names + [f"b3_{n}" for n in range(1, depth + 1)]


def make_params(depth, features, seed):
    P = {}
    for i, name in enumerate(block_names(depth)):
        P.update({f"{name}.{k}": v for k, v in M.make_params(features, features, seed + i).items()})
    return P


def make_inputs(B, H, W, features, seed):
    return M.make_inputs(B, H, W, features, features, seed)


def block_params(P, name):
    return {k[len(name) + 1:]: v for k, v in P.items() if k.startswith(name + ".")}


def _block(p, x):
    """net_util.py:374-396 for an identity-residual block on torch tensors -> (out, o1, o2)"""
    o1 = F.conv2d(F.relu(F.group_norm(x, M.GROUPS, p["bn1.weight"], p["bn1.bias"], M.EPS)), p["conv1.weight"], None, 1, 1)
    o2 = F.conv2d(F.relu(F.group_norm(o1, M.GROUPS, p["bn2.weight"], p["bn2.bias"], M.EPS)), p["conv2.weight"], None, 1, 1)
    o3 = F.conv2d(F.relu(F.group_norm(o2, M.GROUPS, p["bn3.weight"], p["bn3.bias"], M.EPS)), p["conv3.weight"], None, 1, 1)
    return torch.cat((o1, o2, o3), 1) + x, o1, o2


def _mat(m, dtype):
    return torch.as_tensor(m).to(dtype)


def _pool(x):
    np_dt = np.float64 if x.dtype == torch.float64 else np.float32
    return torch.einsum("oy,bcyx,px->bcop", _mat(R.pool_matrix(x.shape[2], np_dt), x.dtype), x, _mat(R.pool_matrix(x.shape[3], np_dt), x.dtype))


def _up(x):
    np_dt = np.float64 if x.dtype == torch.float64 else np.float32
    return torch.einsum("oy,bcyx,px->bcop", _mat(R.upsample_matrix(x.shape[2], np_dt), x.dtype), x, _mat(R.upsample_matrix(x.shape[3], np_dt), x.dtype))


def _level(p, n, x, tape):
    """HourGlass._forward (HGFilters.py:26-50); tape[block] = (input, o1, o2)"""
    def run(name, t):
        out, o1, o2 = _block({k[len(name) + 1:]: v for k, v in p.items() if k.startswith(name + ".")}, t)
        tape[name] = (t, o1, o2)
        return out
    up1 = run(f"b1_{n}", x)
    low = run(f"b2_{n}", _pool(x))
    low = _level(p, n - 1, low, tape) if n > 1 else run("b2_plus_1", low)
    low = run(f"b3_{n}", low)
    return up1 + _up(low)


def _depth(P):
    return max(int(k.split(".")[0][3:]) for k in P if k.startswith("b1_"))


def _run(P, x, dtype, leaves):
    p = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in P.items() if ".downsample.0" not in k}
    xt = torch.as_tensor(np.asarray(x)).to(dtype)
    if leaves:
        xt.requires_grad_(True)
        for v in p.values():
            v.requires_grad_(True)
    tape = {}
    return _level(p, _depth(P), xt, tape), p, xt, tape


def forward(P, x, dtype=torch.float64):
    with torch.no_grad():
        return _run(P, x, dtype, False)[0].double().numpy()


def autograd_grads(P, x, dy, dtype=torch.float64):
    out, p, xt, _ = _run(P, x, dtype, True)
    (out * torch.as_tensor(np.asarray(dy)).to(dtype)).sum().backward()
    g = {"out": out.detach().double().numpy(), "d_x": xt.grad.double().numpy()}
    g.update({k: v.grad.double().numpy() for k, v in p.items() if v.grad is not None})          # an identity block's bn4 is unused: absent
    return g


def reference_and_e32(P, x, dy):
    g64, g32 = autograd_grads(P, x, dy, torch.float64), autograd_grads(P, x, dy, torch.float32)
    return g64, {n: float(np.abs(g32[n] - g64[n]).max()) for n in g64}


def saved_from_model(P, x):
    with torch.no_grad():
        tape = _run(P, x, torch.float64, False)[3]
    return {name: {"x": t.numpy(), "raw": torch.cat((o1, o2), 1).numpy(), "stats": [tuple(s.numpy() for s in M.group_stats(v)) for v in (t, o1, o2)]}
            for name, (t, o1, o2) in tape.items()}


def manual_grads(P, x, dy, saved=None):
    saved = saved or saved_from_model(P, x)
    g = {}

    def block_back(name, d):
        gb = M.manual_grads(block_params(P, name), saved[name]["x"], d, saved[name])
        g.update({f"{name}.{k}": v for k, v in gb.items() if k != "d_x"})
        return gb["d_x"]

    def level_back(n, d_out):
        d_low = R.upsample_backward(d_out)                  # up1 + U low: d_up1 = d_out, d_low = U^T d_out
        d_low = block_back(f"b3_{n}", d_low)
        d_low = level_back(n - 1, d_low) if n > 1 else block_back("b2_plus_1", d_low)
        d_pool = block_back(f"b2_{n}", d_low)
        return block_back(f"b1_{n}", d_out) + R.avgpool_backward(d_pool)

    g["d_x"] = level_back(_depth(P), np.asarray(dy, np.float64))
    return g
