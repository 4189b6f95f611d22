"""GPU: the stem, the stack tail and the whole trainable HGFilter (csrc/enctrain.hip, ops.stem_train / stack_tail_train, encoder.TrainableHGFilter) against the
float64 model of tests/enctrain_model.py.  The gate is the project's: 4 units per tensor, a unit = e32, the model's float32 run against its float64 run on the
test's inputs.  Chains through the split-f16 forward are compared AT the GPU forward's saved activations (4 e32) and against pure float64 autograd at
4 (e32 + e_fwd), e_fwd = the float64 gradient at the saved activations against the pure one (the method of tests/test_gpu_hourglass.py).  Measured ratios:
tests/golden/enctrain.md."""
import numpy as np
import pytest
import torch

import enctrain_model as EM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def L():
    from vistracker_amd import _lib
    return _lib


def cl(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).to(DEV).contiguous(memory_format=torch.channels_last)


def dv(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV).contiguous()


def host(t):
    return t.detach().double().cpu().numpy()


def stats_of(ws, b):
    """(mean, rstd), each (b, 32) float64 numpy, from a {mean, rstd} area"""
    s = ws[:b * 32].view(torch.float32).reshape(b, 32, 2)
    return host(s[..., 0]), host(s[..., 1])


def check(what, got, truth, e32, e_extra=None):
    bad = []
    for n, t in got.items():
        e = e32[n] + (e_extra[n] if e_extra else 0.0)
        err = float(np.abs(host(t) - truth[n]).max())
        print(f"\n[{what}] {n:>28}: bound unit {e:.3e} | kernel error {err:.3e} ({err / e if e > 0 else 0.0:.2f}) | largest element {float(np.abs(truth[n]).max()):.3e}", end="")
        if not (np.isfinite(err) and err <= 4 * e):
            bad.append((n, err, e))
    assert not bad, bad


# ---- vt_bias_grad ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", [1, 128, 255, 256, 257, 511, 513])      # the reduction's blocks are 256 pixels: one block, its edge - 1 / + 1, two blocks' edge - 1 / + 1
def test_bias_grad(B, HW):
    from vistracker_amd import ops
    r = np.random.RandomState(HW + B)
    Ct, C, off = 48, 32, 8
    d = r.randn(B, Ct, HW, 1).astype(np.float32)
    dt = cl(d)
    for c, o in ((Ct, 0), (C, off)):            # the whole tensor, and a slice with cstride > C and coff > 0
        want = d[:, o:o + c].astype(np.float64).sum((0, 2, 3))
        e32 = float(np.abs(d[:, o:o + c].sum((0, 2, 3), dtype=np.float32) - want).max())
        got = ops.bias_grad(dt, C=c, coff=o)
        err = float(np.abs(host(got) - want).max())
        print(f"\n[bias B={B} HW={HW} C={c}] e32 {e32:.3e} kernel error {err:.3e}", end="")
        assert err <= 4 * e32 and err <= 0.5 * float(np.spacing(np.abs(want).max().astype(np.float32)))        # and: one rounding of the fp64 sum
        assert torch.equal(got, ops.bias_grad(dt, C=c, coff=o))                 # the same bits on every call
        acc = ops.bias_grad(dt, C=c, coff=o, out=got.clone(), accumulate=1)
        assert torch.equal(acc, got + got)
        for s in (2.0 ** -20, 2.0 ** 10):
            assert torch.equal(ops.bias_grad(dt * s, C=c, coff=o), got * s)


def test_bias_grad_refusals():
    from vistracker_amd import ops
    with pytest.raises(L().VtError):
        ops.bias_grad(cl(np.zeros((1, 6, 4, 4))), C=6)          # C % 4
    with pytest.raises(L().VtError):
        ops.bias_grad(torch.zeros(1, 8, 4, 4))                  # no CPU path


# ---- vt_stem7x7_wgrad -----------------------------------------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (7, 5), (32, 32), (33, 31), (34, 66))         # odd sizes, one 16 x 16 output tile exactly, a tile edge + 1 in both directions


@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("cin", [1, 5, 8])
def test_stem_wgrad(cin, cout):
    from vistracker_amd import ops
    for (H, W) in SIZES:
        for B in (1, 2):
            x, dy = EM.stem_make_inputs(B, H, W, cin, cout, 1000 * cin + cout + H + B)
            want = EM.stem_wgrad(EM._t(dy), EM._t(x)).numpy()
            e32 = float(np.abs(EM.stem_wgrad(EM._t(dy, torch.float32), EM._t(x, torch.float32)).double().numpy() - want).max())
            xt, dt = cl(x), cl(dy)
            got = ops.stem7x7_wgrad(dt, xt)
            err = float(np.abs(host(got) - want).max())
            print(f"\n[stem wgrad {cin}->{cout} {H}x{W} B={B}] e32 {e32:.3e} kernel error {err:.3e} ({err / e32 if e32 else 0:.2f})", end="")
            assert err <= 4 * e32, (H, W, B, err, e32)
            if B == 2:
                assert torch.equal(got, ops.stem7x7_wgrad(dt, xt))
                assert torch.equal(ops.stem7x7_wgrad(dt, xt, out=got.clone(), accumulate=1), got + got)
                for s in (2.0 ** -20, 2.0 ** 10):
                    assert torch.equal(ops.stem7x7_wgrad(dt * s, xt), got * s)


@pytest.mark.parametrize("cin,cout", [(5, 64), (1, 32)])
def test_stem_wgrad_one_hot(cin, cout):
    """one-hot d_y at the four corners and the centre reads the operator entry by entry: against an all-ones image dW[co, :, ky, kx] is 1 exactly where the tap lies
    inside the image, against a one-hot image exactly one entry is 1; everything else is exactly zero"""
    from vistracker_amd import ops
    H, W = 33, 31
    H2, W2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    co, ci = cout - 3, cin - 1
    for (oy, ox) in ((0, 0), (0, W2 - 1), (H2 - 1, 0), (H2 - 1, W2 - 1), (H2 // 2, W2 // 2)):
        dy = np.zeros((1, cout, H2, W2), np.float32); dy[0, co, oy, ox] = 1
        want = np.zeros((cout, cin, 7, 7), np.float32)
        for ky in range(7):
            for kx in range(7):
                want[co, :, ky, kx] = 0 <= 2 * oy + ky - 3 < H and 0 <= 2 * ox + kx - 3 < W
        got = ops.stem7x7_wgrad(cl(dy), cl(np.ones((1, cin, H, W), np.float32)))
        assert torch.equal(got.cpu(), torch.as_tensor(want)), (oy, ox)
        for (ky, kx) in ((0, 0), (3, 3), (6, 2)):
            iy, ix = 2 * oy + ky - 3, 2 * ox + kx - 3
            want = np.zeros((cout, cin, 7, 7), np.float32)
            x = np.zeros((1, cin, H, W), np.float32)
            if 0 <= iy < H and 0 <= ix < W:
                x[0, ci, iy, ix] = 1; want[co, ci, ky, kx] = 1
            else:
                x[0, ci, min(max(iy, 0), H - 1), min(max(ix, 0), W - 1)] = 1           # the clamped pixel must NOT be read in the padding's place
                ky2, kx2 = min(max(iy, 0), H - 1) - 2 * oy + 3, min(max(ix, 0), W - 1) - 2 * ox + 3
                want[co, ci, ky2, kx2] = 1
            assert torch.equal(ops.stem7x7_wgrad(cl(dy), cl(x)).cpu(), torch.as_tensor(want)), (oy, ox, ky, kx)


# ---- vt_gn_relu_backward_y ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("H,W", [(1, 1), (8, 16)])
def test_gn_relu_backward_from_the_output(C, H, W):
    from vistracker_amd import ops
    B = 2
    c = EM.planted_gn_case(C, B, H, W, 7 + C + H)
    if H * W > 1:
        assert c["disagree"] >= 1
    g64, g32 = EM.gn_y_grads(c), EM.gn_y_grads(c, torch.float32)
    e32 = {n: float(np.abs(g32[n] - g64[n]).max()) for n in g64}
    ws = dv(np.stack(c["stats"], -1))
    d_x, dgamma, dbeta = ops.gn_relu_backward_y(cl(c["g"]), cl(c["y1"]), cl(c["y"]), ws, dv(c["gamma"]), 32)
    check(f"gn_y C={C} {H}x{W} ({c['disagree']} planted)", {"d_x": d_x, "dgamma": dgamma, "dbeta": dbeta}, g64, e32)
    again = ops.gn_relu_backward_y(cl(c["g"]), cl(c["y1"]), cl(c["y"]), ws, dv(c["gamma"]), 32)
    assert all(torch.equal(a, b) for a, b in zip((d_x, dgamma, dbeta), again))


# ---- the tail ---------------------------------------------------------------------------------------------------------------------------------------------------
TAILS = {"mid_8x16": (1, 8, 16, 256, 256, False, True, True), "mid_16x32_b2": (2, 16, 32, 256, 256, False, True, True), "last_8x16_b2": (2, 8, 16, 256, 256, True, True, False),
         "mid_co64_16x32": (1, 16, 32, 256, 64, False, True, True), "mid_no_d_out": (1, 8, 16, 256, 256, False, False, True), "mid_no_d_prev": (1, 8, 16, 256, 256, False, True, False)}


def make_tail(P, last):
    from vistracker_amd.encoder import TrainableStackTail, _leaf
    return TrainableStackTail({k: _leaf(v, DEV) for k, v in P.items()}, last, DEV)


@pytest.mark.parametrize("tag", list(TAILS))
def test_stack_tail(tag):
    B, H, W, C, Co, last, use_out, use_prev = TAILS[tag]
    P = EM.tail_make_params(C, Co, last, 41)
    ll, prev, d_out, d_prev = EM.tail_make_inputs(B, H, W, C, Co, 42)
    d_out, d_prev = (d_out if use_out else None), (d_prev if use_prev else None)
    g64, e32 = EM.tail_reference_and_e32(P, ll, prev, d_out, d_prev)
    tail = make_tail(P, last)
    llt, pt = cl(ll).requires_grad_(True), cl(prev).requires_grad_(True)
    res = tail(llt) if last else tail(llt, pt)
    out, prev2 = (res, None) if last else res
    node = out.grad_fn
    assert "StackTailTrainFn" in type(node).__name__
    s_ll, s_raw, s_out, s_ws = node.saved_tensors[:4]
    # forward against the float64 model: the split-f16 1 x 1 kernel, held to its own documented error by tests/test_gpu_encoder_kernels.py; here only sanity
    assert float(np.abs(host(out) - g64["out"]).max()) <= 2e-3 * max(1.0, float(np.abs(g64["out"]).max()))
    outs, grads = ([out], [cl(d_out)]) if use_out else ([], [])
    if use_prev and not last:
        outs.append(prev2); grads.append(cl(d_prev))
    torch.autograd.backward(outs, grads)
    got = {"d_ll": llt.grad}
    got.update({k: t.grad for k, t in tail.leaves.items() if t.grad is not None})
    live = set(g64) - {"out", "prev"}
    assert set(got) == live, sorted(set(got) ^ live)
    if not last:
        assert (pt.grad is None) == (not use_prev) and (not use_prev or torch.equal(pt.grad, cl(d_prev)))       # the gradient to previous is d_prev itself
    saved = {"raw": host(s_raw), "out": host(s_out), "stats": stats_of(s_ws, B)}
    at_saved = EM.tail_manual_grads(P, ll, d_out, d_prev, saved)
    check(f"tail {tag} at saved activations", got, at_saved, e32)
    e_fwd = {n: float(np.abs(at_saved[n] - g64[n]).max()) for n in got}
    check(f"tail {tag} against float64 autograd", got, g64, e32, e_extra=e_fwd)


# ---- the whole filter -------------------------------------------------------------------------------------------------------------------------------------------
FILTERS = EM.FILTER_CASES
NUM_STACK, DEPTH, FB = EM.FILTER_NUM_STACK, EM.FILTER_DEPTH, EM.FILTER_B
_filters = {}


def filter_case(tag):
    if tag not in _filters:
        P, x, d_outs, d_normx = EM.filter_case(tag)
        g64, e32 = EM.filter_reference_and_e32(P, x, d_outs, d_normx)
        _filters[tag] = dict(P=P, x=x, d_outs=d_outs, d_normx=d_normx, g64=g64, e32=e32)
    return _filters[tag]


def walk(enc, x):
    """TrainableHGFilter.__call__ written out block by block, keeping the autograd node of every block -> (outputs, tmpx, normx, nodes)"""
    from vistracker_amd import ops
    nodes = {}

    def run(name, blk, t):
        y = blk(t)
        nodes[name] = y.grad_fn
        return y

    def level(i, hg, n, t):
        up1 = run(f"m{i}.b1_{n}", hg.blocks[f"b1_{n}"], t)
        low = run(f"m{i}.b2_{n}", hg.blocks[f"b2_{n}"], ops.avgpool2x2_train(t))
        low = level(i, hg, n - 1, low) if n > 1 else run(f"m{i}.b2_plus_1", hg.blocks["b2_plus_1"], low)
        low = run(f"m{i}.b3_{n}", hg.blocks[f"b3_{n}"], low)
        return ops.upsample2x_bicubic_add_train(low, up1)

    t = run("stem", enc.stem, x)
    normx = ops.avgpool2x2_train(run("conv2", enc.blocks["conv2"], t))
    previous = run("conv4", enc.blocks["conv4"], run("conv3", enc.blocks["conv3"], normx))
    outputs = []
    for i, (hg, tail) in enumerate(zip(enc.hourglasses, enc.tails)):
        ll = run(f"top_m_{i}", enc.blocks[f"top_m_{i}"], level(i, hg, enc.depth, previous))
        res = tail(ll) if tail.last else tail(ll, previous)
        out = res if tail.last else res[0]
        nodes[f"tail{i}"] = out.grad_fn
        outputs.append(out)
        if not tail.last:
            previous = res[1]
    return outputs, t.detach(), normx, nodes


def model_saved(nodes, b):
    sv = {}
    for name, nd in nodes.items():
        s = nd.saved_tensors
        if name == "stem":
            sv[name] = {"y1": host(s[1]), "y": host(s[2]), "stats": stats_of(s[3], b)}
        elif name.startswith("tail"):
            sv[name] = {"ll": host(s[0]), "raw": host(s[1]), "out": host(s[2]), "stats": stats_of(s[3], b)}
        else:
            sv[name] = {"x": host(s[0]), "raw": host(s[1]), "stats": [stats_of(w, b) for w in s[2:5]]}
    return sv


def make_filter(c, tag):
    from vistracker_amd.encoder import TrainableHGFilter
    return TrainableHGFilter.from_state_dict({"module.enc." + k: v for k, v in c["P"].items()}, "enc.", num_stack=NUM_STACK, num_hourglass=DEPTH, device=DEV)


@pytest.mark.parametrize("tag", list(FILTERS))
def test_whole_filter(tag):
    from vistracker_amd.encoder import HGFilterEncoder
    c = filter_case(tag)
    enc = make_filter(c, tag)
    x = cl(c["x"])
    outputs, tmpx, normx = enc(x)
    # forward == the inference encoder on the same weights, bit for bit; tmpx is detached
    inf = HGFilterEncoder({"enc." + k: v for k, v in c["P"].items()}, "enc.", num_stack=NUM_STACK, num_hourglass=DEPTH, device=DEV)
    w_out, w_tmpx, w_normx = inf(x)
    assert all(torch.equal(a.detach(), b) for a, b in zip(outputs, w_out)) and torch.equal(tmpx, w_tmpx) and torch.equal(normx.detach(), w_normx)
    assert tmpx.grad_fn is None and not tmpx.requires_grad and normx.grad_fn is not None
    names = dict(enc.named_parameters())
    assert set(names) == {k for k in c["P"] if ".downsample.0" not in k}
    # a gradient on normx alone reaches conv2 and conv1, and no stack parameter
    normx.backward(cl(c["d_normx"]), retain_graph=True)
    reached = {k for k, v in names.items() if v.grad is not None}
    assert reached == {k for k in names if k.startswith(("conv1.", "bn1.", "conv2."))}, sorted(reached)
    for v in names.values():
        v.grad = None
    # the whole backward, through the block-by-block walk (the same launches: the outputs are the same bits) to have every node's saved tensors
    o2, t2, n2, nodes = walk(enc, x)
    assert all(torch.equal(a, b) for a, b in zip(o2, outputs)) and torch.equal(t2, tmpx) and torch.equal(n2, normx)
    saved = model_saved(nodes, FB)          # before the backward frees the nodes' tensors
    torch.autograd.backward(list(o2) + [n2], [cl(d) for d in c["d_outs"]] + [cl(c["d_normx"])])
    got = {k: v.grad for k, v in names.items()}
    assert all(v is not None for v in got.values()), [k for k, v in got.items() if v is None]
    at_saved = EM.filter_manual_grads(c["P"], c["x"], c["d_outs"], c["d_normx"], saved)
    assert set(at_saved) == set(got), sorted(set(at_saved) ^ set(got))
    check(f"filter {tag} at saved activations", got, at_saved, c["e32"])
    e_fwd = {n: float(np.abs(at_saved[n] - c["g64"][n]).max()) for n in got}
    check(f"filter {tag} against float64 autograd", got, c["g64"], c["e32"], e_extra=e_fwd)
    # and the class's own graph gives the same bits as the walk
    for v in names.values():
        v.grad = None
    torch.autograd.backward(list(outputs) + [normx], [cl(d) for d in c["d_outs"]] + [cl(c["d_normx"])])
    assert all(torch.equal(names[k].grad, got[k]) for k in got), [k for k in got if not torch.equal(names[k].grad, got[k])]


def test_state_dict_round_trip():
    from vistracker_amd.encoder import TrainableHGFilter
    c = filter_case("triplane")
    enc = make_filter(c, "triplane")
    sd = enc.state_dict()
    assert set(c["P"]) <= set(sd) and all(np.array_equal(sd[k].cpu().numpy(), c["P"][k]) for k in c["P"])        # the reference's keys
    again = TrainableHGFilter.from_state_dict({k: v.cpu().numpy() for k, v in sd.items()}, "", num_stack=NUM_STACK, num_hourglass=DEPTH, device=DEV)
    with torch.no_grad():
        a, b = enc(cl(c["x"])), again(cl(c["x"]))
    assert all(torch.equal(u, v) for u, v in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert len(enc.parameters()) == len(dict(enc.named_parameters()))
    with pytest.raises(KeyError):
        TrainableHGFilter.from_state_dict({k: v for k, v in sd.items() if k != "bl0.bias"}, "", num_stack=NUM_STACK, num_hourglass=DEPTH, device=DEV)


# ---- the recorded reference ---------------------------------------------------------------------------------------------------------------------------------------
_BLOCK_KEYS = ("conv1.weight", "conv2.weight", "conv3.weight", "bn1.weight", "bn2.weight", "bn3.weight", "bn1.bias", "bn2.bias", "bn3.bias", "downsample.2.weight", "bn4.weight", "bn4.bias")
_BLOCK_GRADS = ("dW1", "dW2", "dW3", "dgamma1", "dgamma2", "dgamma3", "dbeta1", "dbeta2", "dbeta3", "dWproj", "dgamma4", "dbeta4")


def r32(o):
    """a tape of saved activations rounded to float32, as the kernels read them"""
    if isinstance(o, dict):
        return {k: r32(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return type(o)(r32(v) for v in o)
    return np.asarray(o, np.float32).astype(np.float64)


def gpu_walk_filter(P, sv, x, d_outs, d_normx):
    """the backward of HGFilter.forward (HGFilters.py:162-203) written out by hand over the library's raw entry points, fed with a tape of saved activations in
    enctrain_model.filter_saved_from_model's layout.  -> {parameter name: gradient}"""
    from vistracker_amd import ops
    g = {}
    area = lambda pair: dv(np.stack(pair, -1))          # noqa: E731  a {mean, rstd} area
    depth = EM.HM._depth(EM._sub(P, "m0."))

    def block_back(name, d):
        p, s = EM._sub(P, name + "."), sv[name]
        params = dict(zip(ops.CONV_BLOCK_PARAMS, [dv(p[k]) if k in p else None for k in _BLOCK_KEYS]))
        res = ops.conv_block_backward_raw(d, cl(s["x"]), cl(s["raw"]), [area(q) for q in s["stats"]], params)
        g.update({f"{name}.{dict(zip(_BLOCK_GRADS, _BLOCK_KEYS))[k]}": v for k, v in res.items() if k != "d_x"})
        return res["d_x"]

    def level(i, n, d_out):
        d = ops.upsample2x_bicubic_backward(d_out)
        d = block_back(f"m{i}.b3_{n}", d)
        d = level(i, n - 1, d) if n > 1 else block_back(f"m{i}.b2_plus_1", d)
        d = block_back(f"m{i}.b2_{n}", d)
        return torch.add(block_back(f"m{i}.b1_{n}", d_out), ops.avgpool2x2_backward(d))

    param_of = {v: k for k, v in ops._TAIL_GRAD_OF.items()}
    d_prev = None
    for i in range(len(d_outs) - 1, -1, -1):
        s, tp = sv[f"tail{i}"], EM.filter_tail_params(P, i)
        res = ops.stack_tail_backward_raw(cl(d_outs[i]), d_prev, cl(s["ll"]), cl(s["raw"]), cl(s["out"]), area(s["stats"]),
                                          {k: dv(tp[k]) if k in tp else None for k in ops.STACK_TAIL_PARAMS})
        for k, v in res.items():
            if k != "d_ll":
                n_, s_ = param_of[k].split(".")
                g[f"{n_}{i}.{s_}"] = v
        d_in = level(i, depth, block_back(f"top_m_{i}", res["d_ll"]))
        d_prev = d_in if d_prev is None else torch.add(d_in, d_prev)
    d_n = torch.add(cl(d_normx), block_back("conv3", block_back("conv4", d_prev)))
    d_t = block_back("conv2", ops.avgpool2x2_backward(d_n))
    s = sv["stem"]
    d_y1, g["bn1.weight"], g["bn1.bias"] = ops.gn_relu_backward_y(d_t, cl(s["y1"]), cl(s["y"]), area(s["stats"]), dv(P["bn1.weight"]), 32)
    g["conv1.bias"], g["conv1.weight"] = ops.bias_grad(d_y1), ops.stem7x7_wgrad(d_y1, cl(x))
    return g


@pytest.mark.parametrize("tag", list(FILTERS))
def test_recorded_reference(tag):
    """the kernels, fed with the float64 model's saved activations rounded to fp32 (as test_b_recorded_reference of tests/test_gpu_hourglass.py feeds them), are within
    4 x the reference's own float32 error against the float64 model, per tensor (tests/golden/enctrain_<tag>.npz, tools/gen_golden_enctrain.py)"""
    from conftest import golden
    gold = golden("enctrain_" + tag)
    c = filter_case(tag)
    sv32 = r32(EM.filter_saved_from_model(c["P"], c["x"]))
    truth = EM.filter_manual_grads(c["P"], c["x"], c["d_outs"], c["d_normx"], sv32)
    got = gpu_walk_filter(c["P"], sv32, c["x"], c["d_outs"], c["d_normx"])
    assert set(got) == set(gold), sorted(set(got) ^ set(gold))
    bad = []
    for n, t in got.items():
        sub = (lambda a: a.reshape(-1)[::EM.GOLDEN_WEIGHT_STEP]) if c["g64"][n].ndim == 4 else (lambda a: a)
        e_ref = float(np.abs(gold[n] - sub(c["g64"][n])).max())
        err = float(np.abs(sub(host(t)) - sub(truth[n])).max())
        print(f"\n[recorded {tag} {n}] reference's float32 error {e_ref:.3e} | kernel error {err:.3e} ({err / e_ref if e_ref > 0 else 0.0:.2f})", end="")
        if not err <= 4 * e_ref:
            bad.append((n, err, e_ref))
    assert not bad, bad
