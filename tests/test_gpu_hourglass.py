"""GPU: encoder.TrainableHourglass (seven ConvBlocks joined by ops.avgpool2x2_train / upsample2x_bicubic_add_train) against the float64 model of
tests/hourglass_model.py.  Bounds follow tests/test_gpu_convblock.py: e32 = the float32 run of the model against its float64 run on the test's inputs, per
tensor; the kernels get 4 e32 against the float64 gradient AT THE SAME saved activations (the split-f16 forward flips ReLU masks that a float64 forward does
not: that difference is e_fwd, measured and added only where the pure float64 gradient is the reference).  Measured ratios: tests/golden/hourglass.md."""
import numpy as np
import pytest
import torch

import hourglass_model as HM
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the smallest sizes the ConvBlock kernels serve at the innermost level (H % 8 == 0, W % 16 == 0); the first is the recorded reference's (tools/gen_golden_hourglass.py)
CASES = {"d2_f128": (2, 128, 1, 32, 64, 61), "d1_f256": (1, 256, 2, 16, 32, 71)}
KEYS = {"dW1": "conv1.weight", "dW2": "conv2.weight", "dW3": "conv3.weight"}
for _i in "123":
    KEYS["dgamma" + _i], KEYS["dbeta" + _i] = f"bn{_i}.weight", f"bn{_i}.bias"
_cases = {}


def L():
    from vistracker_amd import _lib
    return _lib


def cl(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).to(DEV).contiguous(memory_format=torch.channels_last)


def nchw(t):
    return t.detach().double().cpu().numpy()


def dv(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV).contiguous()


def case(tag):
    if tag not in _cases:
        depth, feat, b, h, w, seed = CASES[tag]
        P = HM.make_params(depth, feat, seed)
        x, dy = HM.make_inputs(b, h, w, feat, seed + 100)
        g64, e32 = HM.reference_and_e32(P, x, dy)
        _cases[tag] = dict(depth=depth, feat=feat, b=b, P=P, x=x, dy=dy, g64=g64, e32=e32)
    return _cases[tag]


def make_hourglass(c):
    from vistracker_amd.encoder import TrainableHourglass
    return TrainableHourglass.from_state_dict({"image_filter.m0." + k: v for k, v in c["P"].items()}, "image_filter.m0.", depth=c["depth"], device=DEV)


def gpu_walk(params, saved, depth, dy):
    """the backward of HourGlass._forward (HGFilters.py:26-50) written out by hand over per-block saved tensors: saved[name] = (x, raw, [stats1..3]) on the
    device, params[name] = the block's tensors in ops.CONV_BLOCK_PARAMS order.  -> {"d_x", "<block>.<parameter>"}"""
    from vistracker_amd import ops
    g = {}

    def block_back(name, d):
        x, raw, stats = saved[name]
        res = ops.conv_block_backward_raw(d, x, raw, list(stats), dict(zip(ops.CONV_BLOCK_PARAMS, params[name])))
        g.update({f"{name}.{KEYS[k]}": v for k, v in res.items() if k != "d_x"})
        return res["d_x"]

    def level(n, d_out):
        d = ops.upsample2x_bicubic_backward(d_out)
        d = block_back(f"b3_{n}", d)
        d = level(n - 1, d) if n > 1 else block_back("b2_plus_1", d)
        d = block_back(f"b2_{n}", d)
        return torch.add(block_back(f"b1_{n}", d_out), ops.avgpool2x2_backward(d))         # the fork at the level's input: two addends

    g["d_x"] = level(depth, dy)
    return g


def graph_nodes(up, n, out):
    """the autograd nodes of level n by the reference's module names, found from the level's up-sampling node; -> the node that produced the level's input"""
    assert "UpsampleAddTrainFn" in type(up).__name__
    b3, b1 = up.next_functions[0][0], up.next_functions[1][0]
    out[f"b3_{n}"], out[f"b1_{n}"] = b3, b1
    inner = b3.next_functions[0][0]          # a block node's edges: its input, then its leaves (the non-tensor argument has none)
    if n > 1:
        b2 = graph_nodes(inner, n - 1, out)
    else:
        out["b2_plus_1"], b2 = inner, inner.next_functions[0][0]
    out[f"b2_{n}"] = b2
    pool = b2.next_functions[0][0]
    assert "AvgPoolTrainFn" in type(pool).__name__ and pool.next_functions[0][0] is b1.next_functions[0][0]
    return pool.next_functions[0][0]


def run_autograd(c):
    """one forward + backward through the class; -> (hg, y, got {"d_x", "<block>.<parameter>"}, nodes' saved tensors per block)"""
    hg = make_hourglass(c)
    x = cl(c["x"]).requires_grad_(True)
    y = hg(x)
    nodes = {}
    graph_nodes(y.grad_fn, c["depth"], nodes)
    assert sorted(nodes) == sorted(hg.blocks) and all("ConvBlockTrainFn" in type(v).__name__ for v in nodes.values())
    saved = {k: (v.saved_tensors[0], v.saved_tensors[1], v.saved_tensors[2:5]) for k, v in nodes.items()}
    y.backward(cl(c["dy"]))
    got = {"d_x": x.grad}
    for name, blk in hg.blocks.items():
        got.update({f"{name}.{k}": t.grad for k, t in blk.leaves.items() if t.grad is not None})
    return hg, y, got, saved


def model_saved(saved, b):
    """the nodes' saved tensors as hourglass_model.manual_grads reads them"""
    out = {}
    for name, (x, raw, stats) in saved.items():
        st = [s[:b * 32].view(torch.float32).reshape(b, 32, 2) for s in stats]
        out[name] = {"x": nchw(x), "raw": nchw(raw), "stats": [(nchw(s[..., 0]), nchw(s[..., 1])) for s in st]}
    return out


def check(what, got, truth, e32, e_extra=None):
    assert set(got) == set(truth), (sorted(set(got) ^ set(truth)))
    bad = []
    for n, t in got.items():
        e = e32[n] + (e_extra[n] if e_extra else 0.0)
        err = float(np.abs(nchw(t) - truth[n]).max())
        print(f"\n[{what}] {n:>24}: bound unit {e:.3e} | kernel error {err:.3e} ({err / e if e > 0 else 0.0:.2f}) | largest element {float(np.abs(truth[n]).max()):.3e}", end="")
        if not (np.isfinite(err) and err <= 4 * e):
            bad.append((n, err, e))
    assert not bad, bad


@pytest.mark.parametrize("tag", list(CASES))
def test_a_forward_graph_and_model(tag):
    from vistracker_amd.encoder import HGFilterEncoder
    c = case(tag)
    hg, y, got, saved = run_autograd(c)
    # forward == the inference recursion on the same weights, bit for bit
    sd = {"enc.conv1.weight": np.zeros((64, 8, 7, 7), np.float32)}
    sd.update({"enc.m0." + k: v for k, v in c["P"].items()})
    enc = HGFilterEncoder(sd, "enc.", num_hourglass=c["depth"], device=DEV)
    with torch.no_grad():
        want = enc._hourglass(c["depth"], cl(c["x"]), "m0.")
    assert torch.equal(y.detach(), want)
    # graph, no tolerance: autograd == the hand-written walk over the nodes' saved tensors
    direct = gpu_walk({n: b.tensors() for n, b in hg.blocks.items()}, saved, c["depth"], cl(c["dy"]))
    assert sorted(direct) == sorted(got)
    assert all(torch.equal(direct[k], got[k]) for k in got), [k for k in got if not torch.equal(direct[k], got[k])]
    # against the float64 model at the GPU forward's saved activations: 4 e32
    at_saved = HM.manual_grads(c["P"], c["x"], c["dy"], model_saved(saved, c["b"]))
    check(f"a {tag} at saved activations", got, at_saved, c["e32"])
    # against pure float64 autograd: 4 (e32 + e_fwd)
    truth = {n: c["g64"][n] for n in at_saved}
    e_fwd = {n: float(np.abs(at_saved[n] - truth[n]).max()) for n in at_saved}
    print(f"\n[a {tag}] e_fwd: " + ", ".join(f"{n} {v:.2e}" for n, v in e_fwd.items()), end="")
    check(f"a {tag} against float64 autograd", got, truth, c["e32"], e_extra=e_fwd)


def test_b_recorded_reference():
    """the kernels, fed with the float64 model's saved activations rounded to fp32 (as test_g_recorded_reference of tests/test_gpu_convblock.py feeds the block), are
    within 4 x the reference's own float32 error against the float64 model, per tensor (tests/golden/hourglass.npz, hourglass_wgrad.npz)"""
    gold = dict(golden("hourglass"), **golden("hourglass_wgrad"))
    c = case("d2_f128")
    sv = HM.saved_from_model(c["P"], c["x"])
    sv32 = {n: {"x": s["x"].astype(np.float32), "raw": s["raw"].astype(np.float32), "stats": [tuple(a.astype(np.float32) for a in p) for p in s["stats"]]} for n, s in sv.items()}
    truth = HM.manual_grads(c["P"], c["x"], c["dy"], sv32)
    dev = {n: (cl(s["x"]), cl(s["raw"]), [dv(np.stack(p, -1)) for p in s["stats"]]) for n, s in sv32.items()}
    params = {}
    for n in HM.block_names(c["depth"]):
        p = HM.block_params(c["P"], n)
        params[n] = [dv(p[k]) for k in ("conv1.weight", "conv2.weight", "conv3.weight", "bn1.weight", "bn2.weight", "bn3.weight", "bn1.bias", "bn2.bias", "bn3.bias")] + [None] * 3
    got = gpu_walk(params, dev, c["depth"], cl(c["dy"]))
    assert set(got) == set(gold) - {"out"}
    bad = []
    for n, t in got.items():
        sub = (lambda a: a.reshape(-1)[::HM.GOLDEN_WEIGHT_STEP]) if n.endswith(("conv1.weight", "conv2.weight", "conv3.weight")) else (lambda a: a)
        e_ref = float(np.abs(gold[n] - sub(c["g64"][n])).max())
        err = float(np.abs(sub(nchw(t)) - sub(truth[n])).max())
        print(f"\n[b {n}] reference's float32 error {e_ref:.3e} | kernel error {err:.3e} ({err / e_ref if e_ref > 0 else 0.0:.2f})", end="")
        if not err <= 4 * e_ref:
            bad.append((n, err, e_ref))
    assert not bad, bad


def test_c_leaves_and_state():
    from vistracker_amd.encoder import TrainableHourglass
    c = case("d1_f256")
    hg, y, got, _ = run_autograd(c)
    assert sorted(hg.blocks) == sorted(HM.block_names(c["depth"]))
    for name, blk in hg.blocks.items():
        for k, t in blk.leaves.items():
            assert (t.grad is None) == k.startswith("bn4."), (name, k)           # an identity block never uses bn4 (net_util.py:371-372)
    assert len(hg.parameters()) == 9 * len(hg.blocks) and all(p.grad is not None for p in hg.parameters())
    sd = hg.state_dict()
    assert "b2_plus_1.conv1.weight" in sd and "b1_1.bn3.bias" in sd
    again = TrainableHourglass.from_state_dict({"module.image_filter.m1." + k: v.cpu().numpy() for k, v in sd.items()}, "image_filter.m1.", depth=c["depth"], device=DEV)
    sd2 = again.state_dict()
    assert sorted(sd) == sorted(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    with torch.no_grad():
        assert torch.equal(again(cl(c["x"])), y.detach())
    # a shape that a block does not serve raises the block's own error: 8 x 16 is 4 x 8 one level down
    with pytest.raises(L().VtError, match="conv_block_train"):
        hg(cl(c["x"][:, :, :8, :16]))
    with pytest.raises(L().VtError):
        hg(torch.zeros(1, 256, 16, 32))
