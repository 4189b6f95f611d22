"""GPU: the device-side weight packing (csrc/repack.hip), the forward reading its scale from device memory, the repack plan and encoder.EncoderAdam.
Everything here is an equality: the packed bytes and the scale word against the numpy model of tests/repack_model.py, forward outputs and optimiser states bit for
bit against the host-packed path."""
import ctypes as C

import numpy as np
import pytest
import torch

import convblock_model as M
import enctrain_model as EM
import repack_model as RM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K3, K1, K7 = 0, 1, 2            # VT_REPACK_CONV3X3 / CONV1X1 / STEM7X7


def L():
    from vistracker_amd import _lib
    return _lib


def dv(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(DEV).contiguous()


def cl(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).to(DEV).contiguous(memory_format=torch.channels_last)


def sp():
    return L().stream_ptr()


def packed_bytes(kind, cout, cin):
    lib = L().lib()
    if kind == K3:
        return int(lib.vt_conv3x3_packed_bytes(cout, cin))
    if kind == K1:
        return int(lib.vt_conv1x1_packed_bytes(cout, cin)) * int(lib.vt_conv1x1_parts(cout))
    return int(lib.vt_stem7x7_packed_bytes(cout, cin))


def model_pack(kind, w, b=None):
    """(uint16 halves or float32 words as bytes, scale word or None)"""
    if kind == K7:
        return RM.pack_stem(w, b).view(np.uint8), None
    halves, word = (RM.pack3x3 if kind == K3 else RM.pack1x1)(w)
    return halves.view(np.uint8), word


def raw_pack(kind, w, b=None):
    """the raw pack entry point into fresh buffers filled with 0xA5 -> (bytes, scale word or None, bias copy or None)"""
    lib = L().lib()
    cout, cin = w.shape[:2]
    out = torch.full((packed_bytes(kind, cout, cin),), 0xA5, dtype=torch.uint8, device=DEV)
    scale = torch.full((1,), -7.0, device=DEV)
    ws = torch.full((int(lib.vt_repack_workspace_bytes()) // 4,), float("nan"), device=DEV)
    wd, bd = dv(w), (dv(b) if b is not None else None)
    bo = torch.full((cout,), -7.0, device=DEV) if (b is not None and kind == K1) else None
    if kind == K3:
        L().check(lib.vt_conv3x3_pack(wd.data_ptr(), cout, cin, out.data_ptr(), scale.data_ptr(), ws.data_ptr(), sp()))
    elif kind == K1:
        L().check(lib.vt_conv1x1_pack(wd.data_ptr(), bd.data_ptr() if bd is not None else None, cout, cin, out.data_ptr(), bo.data_ptr() if bo is not None else None,
                                      scale.data_ptr(), ws.data_ptr(), sp()))
    else:
        L().check(lib.vt_stem7x7_pack(wd.data_ptr(), bd.data_ptr() if bd is not None else None, cout, cin, out.data_ptr(), sp()))
    return out.cpu().numpy(), (None if kind == K7 else scale.cpu().numpy()[0]), (bo.cpu().numpy() if bo is not None else None)


def same_packing(kind, got, want):
    """byte equality; where the model's half is a NaN (an inf or NaN weight) the device's must be one too, payload free"""
    assert got.shape == want.shape
    if kind == K7:
        g, w = got.view(np.float32), want.view(np.float32)
    else:
        g, w = got.view(np.float16), want.view(np.float16)
    nan = np.isnan(w)
    assert np.isnan(g[nan]).all()
    gb, wb = (g.view(np.uint32), w.view(np.uint32)) if kind == K7 else (g.view(np.uint16), w.view(np.uint16))
    bad = np.flatnonzero((gb != wb) & ~nan)
    assert bad.size == 0, f"{bad.size} of {gb.size} differ, first at {bad[:8]}: {gb[bad[:8]]} != {wb[bad[:8]]}"
    return int(nan.sum())


SHAPES = [(K3, 32, 32), (K3, 64, 32), (K3, 128, 32), (K3, 64, 64), (K3, 128, 96), (K1, 64, 32), (K1, 128, 64), (K1, 256, 32), (K1, 256, 256), (K7, 32, 1), (K7, 64, 5)]
KS = {K3: 3, K1: 1, K7: 7}


@pytest.mark.parametrize("kind,cout,cin", SHAPES)
def test_raw_pack_is_the_model_byte_for_byte(kind, cout, cin):
    k = KS[kind]
    for si, name in enumerate(RM.WEIGHT_SETS):
        w = RM.weights(name, (cout, cin, k, k), 1000 * kind + cout + cin + si)
        b = (0.3 * np.random.RandomState(si).randn(cout)).astype(np.float32) if (kind != K3 and si % 2 == 0) else None
        want, word = model_pack(kind, w, b)
        got, gword, gbias = raw_pack(kind, w, b)
        nn = same_packing(kind, got, want)
        if kind != K7:
            assert np.float32(gword).view(np.uint32) == np.float32(word).view(np.uint32), (name, gword, word)
            assert (nn > 0) == (name in ("inf", "nan"))
        if gbias is not None:
            assert np.array_equal(gbias, b)
        print(f"\n[{('3x3', '1x1', '7x7')[kind]} {cout}x{cin}] {name:>10}: {got.size} bytes equal, scale word {gword}, NaN halves {nn}", end="")


# ---- handles: host create, create_device, create_device + repack ------------------------------------------------------------------------------------------------
class Handles:
    def __init__(self):
        self.made = []

    def host(self, kind, w, b=None):
        lib, h = L().lib(), C.c_void_p()
        cout, cin = w.shape[:2]
        wh = np.ascontiguousarray(w.reshape(cout, cin, -1), np.float32)
        bh = np.ascontiguousarray(b, np.float32) if b is not None else None
        bp = bh.ctypes.data if bh is not None else None
        if kind == K3:
            L().check(lib.vt_conv3x3_create(C.byref(h), wh.ctypes.data, cout, cin, sp()))
        elif kind == K1:
            L().check(lib.vt_conv1x1_create(C.byref(h), wh.ctypes.data, bp, cout, cin, sp()))
        else:
            L().check(lib.vt_stem7x7_create(C.byref(h), wh.ctypes.data, bp, cout, cin, sp()))
        self.made.append((kind, h))
        return h

    def device(self, kind, w, b=None):
        lib, h = L().lib(), C.c_void_p()
        cout, cin = w.shape[:2]
        wd, bd = dv(w), (dv(b) if b is not None else None)
        bp = bd.data_ptr() if bd is not None else None
        if kind == K3:
            L().check(lib.vt_conv3x3_create_device(C.byref(h), wd.data_ptr(), cout, cin, sp()))
        elif kind == K1:
            L().check(lib.vt_conv1x1_create_device(C.byref(h), wd.data_ptr(), bp, cout, cin, sp()))
        else:
            L().check(lib.vt_stem7x7_create_device(C.byref(h), wd.data_ptr(), bp, cout, cin, sp()))
        self.made.append((kind, h))
        return h

    @staticmethod
    def repack(kind, h, wd, bd=None):
        lib = L().lib()
        bp = bd.data_ptr() if bd is not None else None
        if kind == K3:
            L().check(lib.vt_conv3x3_repack(h, wd.data_ptr(), sp()))
        elif kind == K1:
            L().check(lib.vt_conv1x1_repack(h, wd.data_ptr(), bp, sp()))
        else:
            L().check(lib.vt_stem7x7_repack(h, wd.data_ptr(), bp, sp()))

    def close(self):
        torch.cuda.synchronize()
        lib = L().lib()
        for kind, h in self.made:
            (lib.vt_conv3x3_destroy, lib.vt_conv1x1_destroy, lib.vt_stem7x7_destroy)[kind](h)
        self.made = []


@pytest.fixture
def handles():
    hs = Handles()
    yield hs
    hs.close()


def snapshot(kind, h, cout, cin):
    out = torch.full((packed_bytes(kind, cout, cin),), 0x5A, dtype=torch.uint8, device=DEV)
    scale = torch.full((1,), -3.0, device=DEV)
    L().check(L().lib().vt_repack_handle_snapshot(kind, h, out.data_ptr(), scale.data_ptr(), sp()))
    return out.cpu().numpy(), scale.cpu().numpy()[0]


def forward(kind, h, cout, cin, B, H, W, seed):
    """every output of the most general forward of the kind on fixed inputs: GroupNorm prologue, residual, output statistics"""
    lib = L().lib()
    r = np.random.RandomState(seed)
    if kind == K7:
        x = cl(r.rand(B, cin, 2 * H, 2 * W))
        y = torch.zeros(B, cout, H, W, device=DEV).contiguous(memory_format=torch.channels_last)
        L().check(lib.vt_stem7x7_forward(h, x.data_ptr(), cin, 0, B, 2 * H, 2 * W, y.data_ptr(), cout, 0, sp()))
        return [y]
    x = cl(r.randn(B, cin, H, W))
    gn = dv(np.stack([0.1 * r.randn(B, 32), 1 + 0.2 * r.rand(B, 32)], -1))           # {mean, rstd} per (frame, group)
    gamma, beta = dv(1 + 0.3 * r.randn(cin)), dv(0.3 * r.randn(cin))
    res = cl(r.randn(B, cout, H, W))
    tiles = int(lib.vt_conv3x3_tiles(H, W))
    ws = torch.zeros(B * 32 + tiles * B * cout * 2, dtype=torch.float64, device=DEV)
    fin = torch.zeros(B, cout, H, W, device=DEV).contiguous(memory_format=torch.channels_last)
    if kind == K1:
        plain = torch.zeros_like(fin, memory_format=torch.channels_last)
        ws2 = torch.zeros_like(ws)
        L().check(lib.vt_conv1x1_forward(h, x.data_ptr(), cin, 0, gn.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 32, B, H, W, fin.data_ptr(), cout, 0,
                                         res.data_ptr(), cout, 0, ws.data_ptr(), 32, sp()))
        L().check(lib.vt_conv1x1_forward(h, x.data_ptr(), cin, 0, None, None, None, 32, B, H, W, plain.data_ptr(), cout, 0, None, cout, 0, ws2.data_ptr(), 32, sp()))
        return [fin, ws, plain, ws2]
    raw = torch.zeros_like(fin, memory_format=torch.channels_last)
    wsf = torch.zeros_like(ws)
    L().check(lib.vt_conv3x3_forward_block_stats(h, x.data_ptr(), cin, 0, gn.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 32, B, H, W, raw.data_ptr(), cout, 0,
                                                 res.data_ptr(), cout, 0, fin.data_ptr(), cout, 0, ws.data_ptr(), 32, wsf.data_ptr(), 32, sp()))
    return [raw, fin, ws, wsf]


FWD = [(K3, 32, 32, False), (K3, 64, 64, False), (K3, 128, 64, False), (K1, 128, 32, True), (K1, 256, 64, True), (K1, 256, 256, False), (K7, 64, 5, True), (K7, 32, 1, False)]


@pytest.mark.parametrize("kind,cout,cin,bias", FWD)
def test_forward_is_the_same_from_all_three_handles(handles, kind, cout, cin, bias):
    k = KS[kind]
    r = np.random.RandomState(cout + cin)
    w = RM.weights("gauss", (cout, cin, k, k), 77 + cout)
    b = (0.3 * r.randn(cout)).astype(np.float32) if bias else None
    other = RM.weights("pow2", (cout, cin, k, k), 5)
    ob = (r.randn(cout)).astype(np.float32) if bias else None
    h_host, h_dev, h_re = handles.host(kind, w, b), handles.device(kind, w, b), handles.device(kind, other, ob)
    if kind != K7:
        assert snapshot(kind, h_re, cout, cin)[1] != snapshot(kind, h_host, cout, cin)[1]           # the other weights have another scale
    wd, bd = dv(w), (dv(b) if bias else None)
    handles.repack(kind, h_re, wd, bd)
    want, word = model_pack(kind, w, b)
    for h in (h_host, h_dev, h_re):         # the host packing is the model's too: one truth for all three
        got, gword = snapshot(kind, h, cout, cin)
        same_packing(kind, got, want)
        assert kind == K7 or gword == word
    for B in (1, 2):
        for H, W in ((8, 16), (16, 32)):
            outs = [forward(kind, h, cout, cin, B, H, W, 9) for h in (h_host, h_dev, h_re)]
            for o in outs[1:]:
                assert len(o) == len(outs[0]) and all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int64), c.view(torch.int32) if c.dtype == torch.float32 else c.view(torch.int64))
                                                      for a, c in zip(outs[0], o))
            assert all(bool(torch.isfinite(a).all()) and bool(a.abs().sum() > 0) for a in outs[0])
    # weights 2^10 times larger: the scale word must change, and the result is a fresh host handle's
    big = (w * np.float32(1024)).astype(np.float32)
    bigd = dv(big)
    handles.repack(kind, h_re, bigd, bd)
    h_big = handles.host(kind, big, b)
    if kind != K7:
        assert snapshot(kind, h_re, cout, cin)[1] == np.float32(word * 1024) == snapshot(kind, h_big, cout, cin)[1]
    a, c = forward(kind, h_big, cout, cin, 2, 16, 32, 9), forward(kind, h_re, cout, cin, 2, 16, 32, 9)
    assert all(torch.equal(u, v) for u, v in zip(a, c))
    assert not torch.equal(a[0], outs[0][0])


def test_repack_refusals(handles):
    lib = L().lib()
    w = RM.weights("gauss", (64, 32, 3, 3), 1)
    w1 = RM.weights("gauss", (64, 32, 1, 1), 2)
    wd, w1d, bd = dv(w), dv(w1), dv(np.zeros(64, np.float32))
    assert lib.vt_conv3x3_repack(handles.host(K3, w), wd.data_ptr(), sp()) == L().VT_ERR_ARG                # no device scale word
    assert lib.vt_conv1x1_repack(handles.host(K1, w1), w1d.data_ptr(), None, sp()) == L().VT_ERR_ARG
    assert lib.vt_conv1x1_repack(handles.device(K1, w1), w1d.data_ptr(), bd.data_ptr(), sp()) == L().VT_ERR_ARG          # created without a bias
    assert lib.vt_conv1x1_repack(handles.device(K1, w1, np.zeros(64, np.float32)), w1d.data_ptr(), None, sp()) == L().VT_ERR_ARG
    h = C.c_void_p()
    assert lib.vt_conv3x3_create_device(C.byref(h), wd.data_ptr(), 48, 32, sp()) == L().VT_ERR_ARG and not h.value


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------------------------
def test_plan_repacks_a_mixed_list_in_two_launches(handles):
    lib = L().lib()
    spec = [(K3, 64, 32, False), (K3, 128, 96, False), (K1, 64, 32, False), (K1, 256, 64, True), (K7, 64, 5, True)]
    r = np.random.RandomState(3)
    ws = [RM.weights(("gauss", "pow2", "below_pow2", "gauss", "gauss")[i], (co, ci, KS[k], KS[k]), 40 + i) for i, (k, co, ci, _) in enumerate(spec)]
    bs = [(0.3 * r.randn(co)).astype(np.float32) if hb else None for (_, co, _, hb) in spec]
    wd = [dv(w) for w in ws]
    bd = [dv(b) if b is not None else None for b in bs]
    # handles made from OTHER weights; the plan brings them to ws / bs
    hs = [handles.device(k, RM.weights("gauss", w.shape, 90 + i), None if b is None else np.ones_like(b)) for i, ((k, _, _, _), w, b) in enumerate(zip(spec, ws, bs))]
    single = [handles.device(k, w, b) for (k, _, _, _), w, b in zip(spec, ws, bs)]
    n = len(spec)
    plan = C.c_void_p()
    L().check(lib.vt_repack_plan_create(C.byref(plan), n, (C.c_int * n)(*[s[0] for s in spec]), (C.c_void_p * n)(*[h.value for h in hs]),
                                        (C.c_void_p * n)(*[t.data_ptr() for t in wd]), (C.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in bd])))
    try:
        assert lib.vt_repack_plan_launches(plan) == 2
        L().check(lib.vt_repack_plan_run(plan, sp()))
        first = [snapshot(k, h, co, ci) for (k, co, ci, _), h in zip(spec, hs)]
        for (k, co, ci, _), h1, got, w, b in zip(spec, single, first, ws, bs):
            want = snapshot(k, h1, co, ci)
            assert np.array_equal(got[0], want[0]) and (k == K7 or got[1] == want[1])
            same_packing(k, got[0], model_pack(k, w, b)[0])
        # the two-part 1 x 1 with its bias, through the forward
        a, c = forward(K1, hs[3], 256, 64, 1, 8, 16, 4), forward(K1, single[3], 256, 64, 1, 8, 16, 4)
        assert all(torch.equal(u, v) for u, v in zip(a, c))
        # one weight tensor changes (in place: the plan holds its address): only that handle's bytes do
        wd[1].mul_(-3.0)
        L().check(lib.vt_repack_plan_run(plan, sp()))
        second = [snapshot(k, h, co, ci) for (k, co, ci, _), h in zip(spec, hs)]
        for i, (f, s) in enumerate(zip(first, second)):
            assert np.array_equal(f[0], s[0]) == (i != 1)
        same_packing(K3, second[1][0], model_pack(K3, ws[1] * np.float32(-3.0))[0])
        assert second[1][1] == RM.scale(ws[1] * np.float32(-3.0))[1] != first[1][1]
        bad = (C.c_int * n)(*([s[0] for s in spec[:-1]] + [7]))
        p2 = C.c_void_p()
        assert lib.vt_repack_plan_create(C.byref(p2), n, bad, (C.c_void_p * n)(*[h.value for h in hs]), (C.c_void_p * n)(*[t.data_ptr() for t in wd]),
                                         (C.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in bd])) == L().VT_ERR_ARG
    finally:
        torch.cuda.synchronize()
        lib.vt_repack_plan_destroy(plan)


# ---- EncoderAdam ------------------------------------------------------------------------------------------------------------------------------------------------
STEPS, LR = 3, 1e-3


def make_module(which, host_repack, monkeypatch):
    from vistracker_amd import encoder as E
    monkeypatch.setattr(E._PackedHandles, "host_repack", host_repack)
    if which == "filter":
        cin, tmpx, hg, seed = EM.FILTER_CASES["image"]
        P = EM.filter_make_params(cin, tmpx, hg, EM.FILTER_NUM_STACK, EM.FILTER_DEPTH, seed)
        r = np.random.RandomState(seed + 1)
        x = cl(r.rand(EM.FILTER_B, cin, EM.FILTER_H, EM.FILTER_W))
        d = [cl(r.randn(EM.FILTER_B, hg, EM.FILTER_H // 4, EM.FILTER_W // 4)) for _ in range(EM.FILTER_NUM_STACK)]
        enc = E.TrainableHGFilter.from_state_dict(P, "", num_stack=EM.FILTER_NUM_STACK, num_hourglass=EM.FILTER_DEPTH, device=DEV)
        run = lambda: enc(x)[0]             # noqa: E731
    else:
        P = M.make_params(128, 256, 19)
        xn, dn = M.make_inputs(1, 8, 16, 128, 256, 20)
        x, d = cl(xn), [cl(dn)]
        enc = E.TrainableConvBlock.from_state_dict(P, "", device=DEV)
        assert enc.has_proj
        run = lambda: [enc(x)]              # noqa: E731
    return enc, run, d


def handle_addresses(enc):
    from vistracker_amd import encoder as E
    return [ent.handle.value for o in E._handle_owners(enc) for ent in o._handles.values()]


def reference_steps(which, monkeypatch):
    """the path this replaces: ops.FusedAdam per leaf, the handles rebuilt on the host after every step"""
    from vistracker_amd import encoder as E, ops
    enc, run, d = make_module(which, True, monkeypatch)
    opt = ops.FusedAdam(enc.parameters(), lr=LR)
    states = []
    for _ in range(STEPS):
        torch.autograd.backward(run(), d)
        opt.step()
        E.invalidate_handles(enc)           # FusedAdam writes through data_ptr(): the version counters do not see it
        opt.zero_grad()
        states.append(([p.detach().clone() for p in enc.parameters()], [m.clone() for m in opt.m], [v.clone() for v in opt.v]))
    with torch.no_grad():
        outs = [o.clone() for o in run()]
    sd = {k: v.clone() for k, v in enc.state_dict().items()}
    return states, outs, sd


_REF = {}


def reference(which, monkeypatch):
    if which not in _REF:
        _REF[which] = reference_steps(which, monkeypatch)
    return _REF[which]


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("which", ["filter", "block"])
def test_encoder_adam_is_fused_adam_bit_for_bit(which, monkeypatch):
    from vistracker_amd import encoder as E
    states, outs_ref, sd_ref = reference(which, monkeypatch)
    enc, run, d = make_module(which, False, monkeypatch)
    keys = list(enc.state_dict())
    ids = [id(p) for p in enc.parameters()]
    opt = E.EncoderAdam(enc, lr=LR)
    assert opt.launches_per_step == 3 and opt.n_handles == len(handle_addresses(enc))
    assert [id(p) for p in enc.parameters()] == ids and all(p.is_leaf and p.requires_grad for p in enc.parameters())
    addr = handle_addresses(enc)
    for s in range(STEPS):
        torch.autograd.backward(run(), d)
        assert all(p.grad.data_ptr() == g.data_ptr() for p, g in zip(opt.params, opt._gviews))         # autograd accumulated in place
        opt.step()
        opt.zero_grad()
        assert handle_addresses(enc) == addr
        ps, ms, vs = states[s]
        for i, (p, pr) in enumerate(zip(enc.parameters(), ps)):
            assert torch.equal(bits(p.detach()), bits(pr)), (s, i)
        for p, mr, vr in zip(opt.params, ms, vs):
            n = p.numel()
            off = p.data_ptr() - opt.flat.data_ptr()
            assert off % 4 == 0
            o = off // 4
            assert torch.equal(opt.m[o:o + n].view(p.shape), mr) and torch.equal(opt.v[o:o + n].view(p.shape), vr), s          # ==: the sign of a zero may differ
    assert not bool(opt.grad.any())
    with torch.no_grad():
        outs = run()
    assert len(outs) == len(outs_ref) and all(torch.equal(bits(a), bits(b)) for a, b in zip(outs, outs_ref))
    sd = enc.state_dict()
    assert list(sd) == keys == list(sd_ref) and all(torch.equal(bits(sd[k]), bits(sd_ref[k])) and sd[k].data_ptr() != opt.flat.data_ptr() for k in keys)
    assert handle_addresses(enc) == addr


def dropped_leaves(which, enc):
    """the leaves whose .grad the test drops: a convolution weight, a GroupNorm leaf and, in the filter, a tail bias and the stem's weight"""
    if which == "block":
        return [enc.leaves["conv2.weight"], enc.leaves["bn1.weight"]]
    return [enc.hourglasses[0].blocks["b2_plus_1"].leaves["conv2.weight"], enc.blocks["conv3"].leaves["bn1.weight"], enc.tails[0].leaves["bl.bias"],
            enc.stem.leaves["conv1.weight"]]


@pytest.mark.parametrize("which", ["filter", "block"])
def test_encoder_adam_step_needs_no_host(which, monkeypatch):
    """with every way to the host barred, a step followed by a forward and a backward completes; leaves whose .grad was dropped and refilled by autograd step as
    the reference does; a leaf without a gradient at step() is skipped, as ops.FusedAdam and torch skip it"""
    from vistracker_amd import encoder as E
    states, _, _ = reference(which, monkeypatch)
    enc, run, d = make_module(which, False, monkeypatch)
    opt = E.EncoderAdam(enc, lr=LR)
    index = {id(p): i for i, p in enumerate(opt.params)}
    torch.autograd.backward(run(), d)

    def barred(*a, **k):
        raise AssertionError("the optimiser step went to the host")

    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", barred)
        mp.setattr(torch.Tensor, "numpy", barred)
        mp.setattr(torch.cuda, "synchronize", barred)
        opt.step()
        opt.zero_grad()
        # second pass: the leaves lose their .grad, autograd binds fresh tensors, step() copies them into the flat buffer and binds the views again
        drop = dropped_leaves(which, enc)
        for p in drop:
            p.grad = None
        torch.autograd.backward(run(), d)
        for p in drop:
            assert p.grad is not None and p.grad.data_ptr() != opt._gviews[index[id(p)]].data_ptr()
        opt.step()
        for p in drop:
            assert p.grad.data_ptr() == opt._gviews[index[id(p)]].data_ptr()
        opt.zero_grad()
        # third pass, still barred: one leaf has no gradient at step()
        torch.autograd.backward(run(), d)
        lone = drop[1]
        i = index[id(lone)]
        sl = slice(opt._offs[i], opt._offs[i] + lone.numel())
        before = [t.clone() for t in (opt.flat[sl], opt.m[sl], opt.v[sl])]
        opt.grad[sl] = float("nan")             # whatever the buffer holds there must not matter
        lone.grad = None
        opt.step()
    assert lone.grad is None and bool(before[1].any()) and all(torch.equal(bits(a), bits(b)) for a, b in zip(before, (opt.flat[sl], opt.m[sl], opt.v[sl])))
    assert torch.equal(bits(lone.detach().reshape(-1)), bits(before[0]))
    for p, pr2, pr3 in zip(enc.parameters(), states[1][0], states[2][0]):
        if p is lone:
            assert torch.equal(bits(p.detach()), bits(pr2))         # where the second step left it
        else:
            assert torch.equal(bits(p.detach()), bits(pr3))         # every other leaf: the reference's third step (Adam is element-wise)


def test_replaced_leaf_is_followed_and_reported(monkeypatch):
    """another tensor put in a module's ``leaves``: the handle repacks from it once, not at every call, and an EncoderAdam built before says so"""
    from vistracker_amd import _lib, encoder as E
    enc, run, d = make_module("block", False, monkeypatch)
    opt = E.EncoderAdam(enc, lr=LR)
    ent = enc._handles["conv1.weight"]
    new = (enc.leaves["conv1.weight"].detach() * 2).requires_grad_(True)
    enc.leaves["conv1.weight"] = new
    calls = []
    real = _lib.lib().vt_conv3x3_repack

    def counted(*a):
        calls.append(a[0])
        return real(*a)

    monkeypatch.setattr(_lib.lib(), "vt_conv3x3_repack", counted)
    with torch.no_grad():
        run(); run()
    assert len(calls) == 1 and ent.weight is new and enc._handles["conv1.weight"] is ent
    with pytest.raises(_lib.VtError):
        opt.step()


# ---- the inference encoder on the same store --------------------------------------------------------------------------------------------------------------------
CREATE_DEVICE = ("vt_conv3x3_create_device", "vt_conv1x1_create_device", "vt_stem7x7_create_device")


def make_inference(tag, host_repack, monkeypatch):
    """a fresh HGFilterEncoder of a whole-filter case with strict routes, and its input"""
    from vistracker_amd import encoder as E
    monkeypatch.setattr(E._PackedHandles, "host_repack", host_repack)
    cin, tmpx, hg, seed = EM.FILTER_CASES[tag]
    P = EM.filter_make_params(cin, tmpx, hg, EM.FILTER_NUM_STACK, EM.FILTER_DEPTH, seed)
    enc = E.HGFilterEncoder(P, "", EM.FILTER_NUM_STACK, EM.FILTER_DEPTH, device=DEV)
    enc.strict_routes = True
    return enc, cl(np.random.RandomState(seed + 1).rand(EM.FILTER_B, cin, EM.FILTER_H, EM.FILTER_W)), P


def all_outputs(enc, x):
    outputs, tmpx, normx = enc(x)
    return [bits(t).clone() for t in outputs + [tmpx, normx]]


@pytest.mark.parametrize("tag", list(EM.FILTER_CASES))
def test_inference_device_packing_is_host_packing_bit_for_bit(tag, monkeypatch):
    """the stem's 7 x 7 and the 3 x 3 weights are stored channels-last: both packings must read them in NCHW order"""
    got = {}
    for host in (True, False):
        enc, x, _ = make_inference(tag, host, monkeypatch)
        assert not enc.sd["conv1.weight"].is_contiguous() or enc.sd["conv1.weight"].shape[1] == 1
        assert not enc.sd["conv3.conv1.weight"].is_contiguous()
        got[host] = all_outputs(enc, x)
        assert enc.routes and not any(k.startswith("miopen:") for k in enc.routes), dict(enc.routes)
        assert all(ent.on_host == host for ent in enc._handles.values()) and len(enc._handles) == sum(enc.routes.values())
    assert len(got[True]) == EM.FILTER_NUM_STACK + 2 == len(got[False])
    assert all(torch.equal(a, b) for a, b in zip(got[True], got[False])), [i for i, (a, b) in enumerate(zip(got[True], got[False])) if not torch.equal(a, b)]
    assert all(bool(a.view(torch.float32).abs().sum() > 0) and bool(torch.isfinite(a.view(torch.float32)).all()) for a in got[False])


def test_inference_needs_no_host(monkeypatch):
    """with every way to the host barred, the first forward of a fresh HGFilterEncoder completes: one vt_*_create_device per distinct convolution; the second
    forward packs nothing and gives the same bits"""
    from vistracker_amd import _lib
    enc, x, P = make_inference("image", False, monkeypatch)
    calls = []

    def counted(name):
        real = getattr(_lib.lib(), name)

        def f(*a):
            calls.append(name)
            return real(*a)
        return f

    def barred(*a, **k):
        raise AssertionError("the inference encoder went to the host")

    with monkeypatch.context() as mp:
        for name in CREATE_DEVICE:
            mp.setattr(_lib.lib(), name, counted(name))
        mp.setattr(torch.Tensor, "cpu", barred)
        mp.setattr(torch.Tensor, "numpy", barred)
        mp.setattr(torch.cuda, "synchronize", barred)
        first = all_outputs(enc, x)
        n_first = len(calls)
        second = all_outputs(enc, x)
    convs = [k for k, v in P.items() if np.ndim(v) == 4]            # every convolution weight of the filter is used once per forward
    assert n_first == len(convs) == len(enc._handles) and len(calls) == n_first, (n_first, len(convs), len(calls))
    assert calls.count("vt_stem7x7_create_device") == 1 and calls.count("vt_conv1x1_create_device") == sum(np.shape(P[k])[2] == 1 for k in convs)
    assert not any(k.startswith("miopen:") for k in enc.routes)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_version_change_repacks_in_place(monkeypatch):
    """without EncoderAdam: an in-place update that the version counter sees is followed by vt_*_repack on the same handle"""
    from vistracker_amd import encoder as E
    enc, run, _ = make_module("block", False, monkeypatch)
    with torch.no_grad():
        y0 = run()[0].clone()
        addr = handle_addresses(enc)
        for k in ("conv1.weight", "downsample.2.weight"):
            enc.leaves[k].mul_(1024.0)
        y1 = run()[0].clone()
    assert handle_addresses(enc) == addr and not torch.equal(y0, y1)
    monkeypatch.setattr(E._PackedHandles, "host_repack", True)
    fresh = E.TrainableConvBlock.from_state_dict(enc.state_dict(), "", device=DEV)
    with torch.no_grad():
        assert torch.equal(bits(fresh(cl(M.make_inputs(1, 8, 16, 128, 256, 20)[0]))), bits(y1))
