"""GPU: the backward of the encoders' ConvBlock (csrc/convtrain.hip, ops.conv_block_train, encoder.TrainableConvBlock) against the float64 model of
tests/convblock_model.py.  Every bound is MEASURED (the convention of tests/test_gpu_dectrain.py): e32 = the float32 run of the model against its float64 run on
the inputs of the test, per output tensor, and the kernel gets 4 e32.  The primitives and the block entry are fed with float64-model activations rounded to
fp32, so no forward error enters; the end-to-end test adds e_fwd, what the forward's split-f16 operand format alone causes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convblock_model as M
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W = 2, 16, 32             # 2 x 2 pixel tiles of 8 x 16: halos cross tile seams and image borders, split K has several tiles and frames
LAYERS = ((32, 64), (64, 32), (128, 64), (256, 128))
T64 = torch.float64


def L():
    from vistracker_amd import _lib
    return _lib


def cl(a):
    """NCHW numpy / tensor -> channels-last float32 device tensor"""
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).to(DEV).contiguous(memory_format=torch.channels_last)


def nchw(t):
    return t.detach().double().cpu().numpy()


def dv(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV).contiguous()


def stats_dev(mean, rstd):
    """(B,32) mean, rstd -> the B x 32 {mean, rstd} float pairs vt_groupnorm_finalize leaves"""
    return dv(np.stack([np.asarray(mean, np.float32), np.asarray(rstd, np.float32)], -1))


def ws_bytes(n):
    assert n >= 0
    return torch.empty(int(n) // 4 + 4, device=DEV)


def report(what, name, err, e32, scale):
    print(f"\n[{what}] {name:>20}: e32 {e32:.3e} | kernel error {err:.3e} ({err / e32 if e32 > 0 else 0.0:.2f} e32) | largest element {scale:.3e}", end="")


def layer_case(cin, cout, taps, seed):
    """one GN -> ReLU -> conv layer: inputs, the float64 results and e32 of d_a, dW, and of the GroupNorm + ReLU backward (d_x, dgamma, dbeta)"""
    r = np.random.RandomState(seed)
    k = 3 if taps == 9 else 1
    x = (r.randn(B, cin, H, W) * (0.5 + r.rand(1, cin, 1, 1)) + 0.5 * r.randn(1, cin, 1, 1)).astype(np.float32)
    w = (r.randn(cout, cin, k, k) / np.sqrt(taps * cin)).astype(np.float32)
    gamma, beta = (1 + 0.3 * r.randn(cin)).astype(np.float32), (0.3 * r.randn(cin)).astype(np.float32)
    d_o, g = r.randn(B, cout, H, W).astype(np.float32), r.randn(B, cin, H, W).astype(np.float32)
    mean, rstd = (s.numpy().astype(np.float32) for s in M.group_stats(torch.tensor(x, dtype=T64)))
    c = dict(cin=cin, cout=cout, taps=taps, x=x, w=w, gamma=gamma, beta=beta, d_o=d_o, g=g, mean=mean, rstd=rstd)
    for dt, tag in ((T64, "64"), (torch.float32, "32")):
        t = lambda a: torch.tensor(a).to(dt)      # noqa: E731
        a = M.gn_relu(t(x), t(mean), t(rstd), t(gamma), t(beta))[0]
        c["d_a" + tag], c["dW" + tag] = (v.double().numpy() for v in M.conv_grads(a, t(w), t(d_o), k // 2))
        c["d_x" + tag], c["dgamma" + tag], c["dbeta" + tag] = (v.double().numpy() for v in M.gn_relu_backward(t(g), t(x), t(mean), t(rstd), t(gamma), t(beta)))
    c["e32"] = {n: float(np.abs(c[n + "32"] - c[n + "64"]).max()) for n in ("d_a", "dW", "d_x", "dgamma", "dbeta")}
    return c


_cases = {}


def case(cin, cout, taps=9):
    key = (cin, cout, taps)
    if key not in _cases:
        _cases[key] = layer_case(cin, cout, taps, 100 + cin + cout + taps)
    return _cases[key]


def run_dgrad(c, d_o, scale=1.0):
    lib = L().lib()
    d = cl(d_o) * scale
    out = torch.full((B, c["cin"], H, W), float("nan"), device=DEV).contiguous(memory_format=torch.channels_last)
    ws = ws_bytes(lib.vt_conv_dgrad_workspace_bytes(c["cout"], c["cin"], c["taps"])).fill_(float("nan"))
    fn = lib.vt_conv3x3_dgrad if c["taps"] == 9 else lib.vt_conv1x1_dgrad
    w = dv(c["w"])
    L().check(fn(w.data_ptr(), c["cout"], c["cin"], d.data_ptr(), c["cout"], 0, B, H, W, out.data_ptr(), c["cin"], 0, ws.data_ptr(), L().stream_ptr()))
    return out


def run_wgrad(c, d_o, scale=1.0, acc=None):
    lib = L().lib()
    d = cl(d_o) * scale
    out = torch.full(c["w"].shape, float("nan"), device=DEV) if acc is None else acc.clone()
    ws = ws_bytes(lib.vt_conv_wgrad_workspace_bytes(B, H, W, c["cout"], c["cin"], c["taps"])).fill_(float("nan"))
    fn = lib.vt_conv3x3_wgrad if c["taps"] == 9 else lib.vt_conv1x1_wgrad
    x, st, ga, be = cl(c["x"]), stats_dev(c["mean"], c["rstd"]), dv(c["gamma"]), dv(c["beta"])        # named: alive until the call is enqueued
    L().check(fn(d.data_ptr(), c["cout"], 0, x.data_ptr(), c["cin"], 0, st.data_ptr(), ga.data_ptr(),
                 be.data_ptr(), 32, B, H, W, c["cin"], c["cout"], out.data_ptr(), 0 if acc is None else 1, ws.data_ptr(), L().stream_ptr()))
    return out


def run_gnb(c, scale=1.0, base=None):
    lib = L().lib()
    C_ = c["cin"]
    g = cl(c["g"]) * scale
    dx = torch.full((B, C_, H, W), float("nan"), device=DEV).contiguous(memory_format=torch.channels_last) if base is None else base.clone(memory_format=torch.channels_last)
    dg, db = torch.full((C_,), float("nan"), device=DEV), torch.full((C_,), float("nan"), device=DEV)
    ws = ws_bytes(lib.vt_gn_relu_backward_workspace_bytes(B, H * W, C_, 32)).fill_(float("nan"))
    x, st, ga, be = cl(c["x"]), stats_dev(c["mean"], c["rstd"]), dv(c["gamma"]), dv(c["beta"])
    L().check(lib.vt_gn_relu_backward(g.data_ptr(), C_, 0, x.data_ptr(), C_, 0, st.data_ptr(), ga.data_ptr(),
                                      be.data_ptr(), 32, B, H * W, C_, None if base is None else dx.data_ptr(), C_, 0, dx.data_ptr(), C_, 0,
                                      dg.data_ptr(), db.data_ptr(), 0, ws.data_ptr(), L().stream_ptr()))
    return dx, dg, db


def held(what, name, got, want, e32):
    err = float(np.abs(nchw(got) - want).max())
    report(what, name, err, e32, float(np.abs(want).max()))
    assert np.isfinite(err) and err <= 4 * e32, (what, name, err, e32)


@pytest.mark.parametrize("cin,cout", LAYERS)
def test_a_primitives_3x3(cin, cout):
    c = case(cin, cout)
    what = f"a {cin}->{cout}"
    held(what, "dgrad d_a", run_dgrad(c, c["d_o"]), c["d_a64"], c["e32"]["d_a"])
    held(what, "wgrad dW", run_wgrad(c, c["d_o"]), c["dW64"], c["e32"]["dW"])
    dx, dg, db = run_gnb(c)
    held(what, "gn d_x", dx, c["d_x64"], c["e32"]["d_x"])
    held(what, "gn dgamma", dg, c["dgamma64"], c["e32"]["dgamma"])
    held(what, "gn dbeta", db, c["dbeta64"], c["e32"]["dbeta"])
    # adds onto a destination that holds the other contributions; accumulate adds onto dW
    base = cl(np.random.RandomState(5).randn(B, cin, H, W))
    dx2 = run_gnb(c, base=base)[0]
    assert float((dx2 - (base + dx)).abs().max()) <= 2e-7 * float(dx2.abs().max())
    w0 = dv(np.random.RandomState(6).randn(*c["w"].shape))
    assert torch.equal(run_wgrad(c, c["d_o"], acc=w0), w0 + run_wgrad(c, c["d_o"]))


@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 256)])
def test_b_primitives_1x1(cin, cout):
    c = case(cin, cout, 1)
    what = f"b 1x1 {cin}->{cout}"
    held(what, "dgrad d_a", run_dgrad(c, c["d_o"]), c["d_a64"], c["e32"]["d_a"])
    held(what, "wgrad dW", run_wgrad(c, c["d_o"]), c["dW64"], c["e32"]["dW"])


@pytest.mark.parametrize("cin,cout", [(32, 64), (256, 128)])
def test_c_range_property(cin, cout):
    """a gradient of 2^-20 or 2^10 times the size gives the same result times that factor, bit for bit: no range assumption (what rules out the split-f16 route)"""
    c = case(cin, cout)
    d0, w0, g0 = run_dgrad(c, c["d_o"]), run_wgrad(c, c["d_o"]), run_gnb(c)
    for s in (2.0 ** -20, 2.0 ** 10):
        assert torch.equal(run_dgrad(c, c["d_o"], s), d0 * s)
        assert torch.equal(run_wgrad(c, c["d_o"], s), w0 * s)
        for a, b_ in zip(run_gnb(c, s), g0):
            assert torch.equal(a, b_ * s)
    assert torch.equal(run_dgrad(c, c["d_o"]), d0) and torch.equal(run_wgrad(c, c["d_o"]), w0)       # two calls, equal bits


@pytest.mark.parametrize("y,x", [(0, 0), (H - 1, W - 1), (7, 15), (8, 16)])
def test_d_one_hot_pixel(y, x):
    """a one-hot upstream pixel in a corner and on a tile seam: borders, flip and transpose of the taps"""
    c = case(64, 32)
    d_o = np.zeros_like(c["d_o"]); d_o[1, 5, y, x] = 1.0
    t = lambda a: torch.tensor(a, dtype=T64)      # noqa: E731
    a = M.gn_relu(t(c["x"]), t(c["mean"]), t(c["rstd"]), t(c["gamma"]), t(c["beta"]))[0]
    da, dw = (v.numpy() for v in M.conv_grads(a, t(c["w"]), t(d_o), 1))
    a32 = M.gn_relu(*(torch.tensor(c[k]) for k in ("x", "mean", "rstd", "gamma", "beta")))[0]
    da32, dw32 = (v.double().numpy() for v in M.conv_grads(a32, torch.tensor(c["w"]), torch.tensor(d_o), 1))
    # the data gradient is a copy of weights (exact in both); the weight gradient a copy of activations, whose float32 evaluation sets e32
    held(f"d one-hot ({y},{x})", "dgrad d_a", run_dgrad(c, d_o), da, float(np.abs(da32 - da).max()))
    held(f"d one-hot ({y},{x})", "wgrad dW", run_wgrad(c, d_o), dw, float(np.abs(dw32 - dw).max()))


# ---- the block entry ----------------------------------------------------------------------------------------------------------------------------------------
KEYS = {"d_x": "d_x", "dW1": "conv1.weight", "dW2": "conv2.weight", "dW3": "conv3.weight", "dWproj": "downsample.2.weight"}
for _i in "1234":
    KEYS["dgamma" + _i], KEYS["dbeta" + _i] = f"bn{_i}.weight", f"bn{_i}.bias"
_blocks = {}


def block_case(cin, cout, b, h, w, seed):
    key = (cin, cout, b, h, w, seed)
    if key not in _blocks:
        P = M.make_params(cin, cout, seed)
        x, dy = M.make_inputs(b, h, w, cin, cout, seed + 1)
        sv = M.saved_from_model(P, x)
        sv = {"raw": sv["raw"].astype(np.float32), "stats": [tuple(s.astype(np.float32) for s in p) for p in sv["stats"]]}      # what the kernel is fed
        g64, e32 = M.reference_and_e32(P, x, dy)
        _blocks[key] = dict(P=P, x=x, dy=dy, saved=sv, truth=M.manual_grads(P, x, dy, sv), g64=g64, e32=e32)
    return _blocks[key]


def dev_params(P):
    from vistracker_amd import ops
    names = dict(zip(ops.CONV_BLOCK_PARAMS, ("conv1.weight", "conv2.weight", "conv3.weight", "bn1.weight", "bn2.weight", "bn3.weight", "bn1.bias", "bn2.bias", "bn3.bias",
                                             "downsample.2.weight", "bn4.weight", "bn4.bias")))
    proj = "downsample.2.weight" in P
    return {k: (dv(P[n]) if (proj or k not in ("wproj", "gamma4", "beta4")) else None) for k, n in names.items()}


def run_block(bc, **kw):
    from vistracker_amd import ops
    sv = bc["saved"]
    return ops.conv_block_backward_raw(cl(bc["dy"]), cl(bc["x"]), cl(sv["raw"]), [stats_dev(*p) for p in sv["stats"]], dev_params(bc["P"]), **kw)


def check_block(what, got, bc, e_extra=None, truth=None):
    truth = truth or bc["truth"]
    assert set(KEYS[k] for k in got) == set(truth), (sorted(got), sorted(truth))
    bad = []
    for k, t in got.items():
        n = KEYS[k]
        e = bc["e32"][n] + (e_extra[n] if e_extra else 0.0)
        err = float(np.abs(nchw(t) - truth[n]).max())
        report(what, n, err, e, float(np.abs(truth[n]).max()))
        if not (np.isfinite(err) and err <= 4 * e):
            bad.append((n, err, e))
    assert not bad, bad


@pytest.mark.parametrize("cin,cout,b,h,w", [(64, 128, B, H, W), (128, 128, B, H, W), (256, 256, 1, 8, 16)])
def test_e_block_entry(cin, cout, b, h, w):
    bc = block_case(cin, cout, b, h, w, 31)
    check_block(f"e block {cin}->{cout}", run_block(bc), bc)


def test_f_block_calling_conventions():
    from vistracker_amd import ops
    bc = block_case(64, 128, B, H, W, 31)
    full = run_block(bc)
    again = run_block(bc)
    assert all(torch.equal(full[k], again[k]) for k in full), "two calls, equal bits"
    # NULL outputs skip their tensor and leave the others' bits
    for want in (["dW2", "dgamma4"], ["d_x"], ["dW1", "dW3", "dWproj", "dbeta1"]):
        part = run_block(bc, want=want)
        assert sorted(part) == sorted(want) and all(torch.equal(part[k], full[k]) for k in want), want
    # a NaN-filled workspace and NaN-filled outputs change no bit
    lib = L().lib()
    ws = ws_bytes(lib.vt_conv_block_backward_workspace(B, H, W, 64, 64, 32, 32)).fill_(float("nan"))
    outs = {k: torch.full_like(v, float("nan")) for k, v in full.items()}
    nan = run_block(bc, out=outs, ws=ws)
    assert all(torch.equal(nan[k], full[k]) for k in full)
    # accumulate adds onto the parameter gradients (d_x is written)
    r = np.random.RandomState(9)
    start = {k: dv(r.randn(*v.shape)) if k != "d_x" else torch.full_like(v, float("nan")) for k, v in full.items()}
    acc = run_block(bc, out={k: v.clone() for k, v in start.items()}, accumulate=1)
    assert torch.equal(acc["d_x"], full["d_x"])
    for k in full:
        if k != "d_x":
            assert torch.equal(acc[k], start[k] + full[k]), k
    # bad shapes are refused, not launched
    assert lib.vt_conv_block_backward_workspace(B, H + 1, W, 64, 64, 32, 32) == -1 and lib.vt_conv_block_backward_workspace(B, H, W, 48, 64, 32, 32) == -1


@pytest.mark.parametrize("cin,cout,seed", [(64, 128, 21), (128, 128, 23)])
def test_g_recorded_reference(cin, cout, seed):
    """the kernel is within 4 x the reference's own float32 error against the float64 model, per tensor (tests/golden/convblock.npz)"""
    gold = golden("convblock")
    bc = block_case(cin, cout, 1, 8, 16, seed)
    got = run_block(bc)
    tag, bad = f"b{cin}_{cout}.", []
    for k, t in got.items():
        n = KEYS[k]
        sub = (lambda a: a.reshape(-1)[::M.GOLDEN_WEIGHT_STEP]) if (n.startswith("conv") or n.startswith("downsample")) else (lambda a: a)
        want = sub(bc["truth"][n])
        e_ref = float(np.abs(gold[tag + n] - sub(bc["g64"][n])).max())
        err = float(np.abs(sub(nchw(t)) - want).max())
        print(f"\n[g {tag}{n}] reference's float32 error {e_ref:.3e} | kernel error {err:.3e}", end="")
        if not err <= 4 * e_ref:
            bad.append((n, err, e_ref))
    assert not bad, bad


# ---- end to end through autograd ------------------------------------------------------------------------------------------------------------------------------
def make_block(P, prefix=""):
    from vistracker_amd.encoder import TrainableConvBlock
    return TrainableConvBlock.from_state_dict({prefix + k: v for k, v in P.items()}, prefix, device=DEV)


def gpu_saved(y, b):
    """what the autograd node kept: x, raw and the three {mean, rstd} areas, and the same as the model's ``saved``"""
    sv = y.grad_fn.saved_tensors
    st = [s[:b * 32].view(torch.float32).reshape(b, 32, 2) for s in sv[2:5]]
    return sv, {"raw": nchw(sv[1]), "stats": [(nchw(s[..., 0]), nchw(s[..., 1])) for s in st]}


@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 128)])
def test_h_autograd_end_to_end(cin, cout):
    from vistracker_amd import ops
    from vistracker_amd.encoder import HGFilterEncoder
    bc = block_case(cin, cout, B, H, W, 31)
    P = bc["P"]
    blk = make_block(P)
    x = cl(bc["x"]).requires_grad_(True)
    y = blk(x)
    # forward == the inference path, bit for bit
    sd = {"enc.conv1.weight": np.zeros((64, 8, 7, 7), np.float32)}
    sd.update({"enc.blk." + k: v for k, v in P.items()})
    enc = HGFilterEncoder(sd, "enc.", device=DEV)
    with torch.no_grad():
        want = enc._conv_block_fused(cl(bc["x"]), "blk.", [cout // 2, cout // 4, cout // 4])
    assert torch.equal(y.detach(), want)
    sv, saved = gpu_saved(y, B)
    y.backward(cl(bc["dy"]))
    got = {"d_x": x.grad}
    inv = {v: k for k, v in KEYS.items()}
    for n, t in blk.leaves.items():
        if t.grad is not None:
            got[inv[n]] = t.grad
    # == a direct call on the saved tensors, bit for bit
    direct = ops.conv_block_backward_raw(cl(bc["dy"]), sv[0], sv[1], list(sv[2:5]), dict(zip(ops.CONV_BLOCK_PARAMS, blk.tensors())))
    assert sorted(direct) == sorted(got) and all(torch.equal(direct[k], got[k]) for k in got)
    # against the pure float64 model: 4 (e32 + e_fwd), e_fwd = the float64 gradient at the GPU forward's saved activations minus the pure float64 gradient
    at_saved = M.manual_grads(P, bc["x"], bc["dy"], saved)
    e_fwd = {n: float(np.abs(at_saved[n] - bc["g64"][n]).max()) for n in at_saved}
    print(f"\n[h {cin}->{cout}] e_fwd: " + ", ".join(f"{n} {v:.2e}" for n, v in e_fwd.items()), end="")
    check_block(f"h autograd {cin}->{cout}", got, bc, e_extra=e_fwd, truth={n: bc["g64"][n] for n in at_saved})


def test_i_chain_reuse_and_update():
    bc1 = block_case(64, 128, B, H, W, 31)
    P1, P2 = bc1["P"], M.make_params(128, 128, 41)
    b1, b2 = make_block(P1), make_block(P2)
    x = cl(bc1["x"]).requires_grad_(True)
    loss = (b2(b1(x)) ** 2).mean()
    loss.backward()
    # two chained blocks with a scalar loss against autograd on the float64 model of both (loose: this test is about the graph, the bounds are above)
    xt = torch.tensor(bc1["x"], dtype=T64, requires_grad=True)
    o1, lv1, _, _ = M.forward(P1, xt.detach().numpy(), T64, leaves=True)
    p2 = {k: torch.tensor(v, dtype=T64) for k, v in P2.items()}
    h = o1
    u1 = F.conv2d(F.relu(F.group_norm(h, 32, p2["bn1.weight"], p2["bn1.bias"], M.EPS)), p2["conv1.weight"], None, 1, 1)
    u2 = F.conv2d(F.relu(F.group_norm(u1, 32, p2["bn2.weight"], p2["bn2.bias"], M.EPS)), p2["conv2.weight"], None, 1, 1)
    u3 = F.conv2d(F.relu(F.group_norm(u2, 32, p2["bn3.weight"], p2["bn3.bias"], M.EPS)), p2["conv3.weight"], None, 1, 1)
    ((torch.cat((u1, u2, u3), 1) + h) ** 2).mean().backward()
    for name, got, want in (("x", x.grad, lv1["d_x"].grad), ("block 1 conv1.weight", b1.leaves["conv1.weight"].grad, lv1["conv1.weight"].grad),
                            ("block 1 bn4.weight", b1.leaves["bn4.weight"].grad, lv1["bn4.weight"].grad)):
        assert got is not None, name
        err, sc = float(np.abs(nchw(got) - want.numpy()).max()), float(want.abs().max())
        print(f"\n[i chain] {name}: |kernel - model64| {err:.3e} of {sc:.3e}", end="")
        assert err <= 1e-3 * sc, name
    assert b2.leaves["bn4.weight"].grad is None         # an identity block never uses bn4 (net_util.py:371-372)
    # a block used twice accumulates: grad(two uses) == grad(use a) + grad(use b), to float32 rounding of the sum
    blk = make_block(P2)
    xa, xb = cl(np.random.RandomState(1).randn(B, 128, H, W)), cl(np.random.RandomState(2).randn(B, 128, H, W))
    dy = cl(np.random.RandomState(3).randn(B, 128, H, W))
    (blk(xa) * dy).sum().backward(); ga = blk.leaves["conv2.weight"].grad.clone(); blk.leaves["conv2.weight"].grad = None
    (blk(xb) * dy).sum().backward(); gb = blk.leaves["conv2.weight"].grad.clone(); blk.leaves["conv2.weight"].grad = None
    ((blk(xa) * dy).sum() + (blk(xb) * dy).sum()).backward()
    assert torch.equal(blk.leaves["conv2.weight"].grad, ga + gb) or torch.equal(blk.leaves["conv2.weight"].grad, gb + ga)
    # a parameter update followed by a second forward uses the new weights (the handle-refresh path)
    with torch.no_grad():
        y0 = blk(xa).clone()
        blk.leaves["conv1.weight"].mul_(0.5)
        y1 = blk(xa)
    fresh = make_block({k: v.detach().cpu().numpy() for k, v in blk.state_dict().items()})
    with torch.no_grad():
        assert torch.equal(y1, fresh(xa)) and not torch.equal(y1, y0)
