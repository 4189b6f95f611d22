"""Named, seeded inputs of the encoder forward tests (tests/test_host_encoder_model.py, tests/test_gpu_encoder_kernels.py, tools/encoder_perchannel_report.py) and
the calls of the kernels through ctypes.  Inputs and references are built on the CPU, once per case (lru_cache: do not modify what these functions return).

Every device tensor of a call is a view inside a larger allocation with GUARD pixel rows in front of and behind it.  Inputs hold NaN in the guard rows and in the
channels of `cstride` outside the slice that is read; outputs hold the bit pattern SENTINEL in the guard rows and outside [coff, coff + C), compared bit for bit
after every call (Out.get asserts it).  A read that is not zeroed, or a write past a border tile, shows as data, never as a fault."""
import ctypes
import functools

import numpy as np

import encoder_model as M

GUARD = 8
SENTINEL = 0x4B3C2D1E
EPS = 1e-5

# ---- 3 x 3: (Cin, Cout) classes -- Cout 32 runs with dead waves, 64 with NT = 1, 128 with NT = 2; chunk counts 1, 2, 3 and 8 ---------------------------------------------
CONV3_PAIRS = [(32, 32), (32, 64), (96, 64), (64, 128), (256, 128), (96, 32)]
CONV3_SIZES = [(8, 16), (8, 48), (24, 16), (24, 48)]                     # one tile; one row of three tiles; one column; 3 x 3 tiles with an interior one
CONV3_ALL_SIZES = [(96, 64), (256, 128)]
CONV3_CASES = [(ci, co, H, W) for ci, co in CONV3_PAIRS for H, W in CONV3_SIZES if (H, W) in ((8, 16), (24, 48)) or (ci, co) in CONV3_ALL_SIZES]
CONV1_CASES = [(ci, co, H, W) for ci in (32, 64, 128, 256) for co in (64, 128, 256) for H, W in ((8, 16), (16, 48))]
LATTICE_CASES = [(k, ci, H, W) for k in (3, 1) for ci in (96, 256) for H, W in ((8, 16), (24, 48)) if not (k == 1 and ci == 96)] + [(1, 64, 8, 16), (1, 64, 24, 48)]
STEM_CASES = [(co, ci, H, W) for co, ci in ((64, 1), (64, 8), (32, 3)) for H, W in ((1, 1), (2, 7), (33, 31), (32, 34), (7, 70))]
GN_C = [4, 32, 96, 256, 1024]
GN_HW = [1, 255, 257, 1000, 4096]
GN_CASES = [(C, g) for C in GN_C for g in sorted({1, 32, C}) if C % g == 0]
RATIOS = [0, 10, 64]          # per-group mean / std; 10 = 4 x the largest |mean| rstd (2.49) of the encoder's own GroupNorm inputs (test_host_encoder_model.py measures it)
SWEEP_OUT = [(2, 2), (4, 6), (10, 26), (32, 48)]
UP_SOURCES = [(1, 1), (1, 9), (2, 2), (3, 3), (5, 13), (2, 3), (16, 24)]
SWEEP_C = [4, 96, 256, 1024]


def conv_B(H, W):
    return 1 if (H, W) == (8, 16) else 3


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _weights(rng, cout, cin, k):
    """randn / sqrt(fan-in); every output channel has its own scale out of {1, .3, .1, .03, .01}: a per-tensor metric does not see the small ones"""
    w = rng.normal(size=(cout, cin, k, k)) / np.sqrt(k * k * cin)
    return (w * np.array([1, .3, .1, .03, .01])[rng.permutation(cout) % 5][:, None, None, None]).astype(np.float32)


def offset_data(rng, shape, groups, r, sigma=1.5):
    """NHWC / (B, HW, C) float32 data whose per-group mean is r standard deviations away from 0 (alternating sign over the groups)"""
    C = shape[-1]; sign = np.repeat(np.where(np.arange(groups) % 2 == 0, 1.0, -1.0), C // groups)
    return ((rng.normal(size=shape) + r * sign) * sigma).astype(np.float32)


def stats32(x, groups):
    """the {mean, rstd} pairs of the model, rounded to float32: what a test hands to a kernel's prologue (B, groups, 2)"""
    m = M.groupnorm_stats(x, groups, EPS)
    return np.stack([m["mean"], m["rstd"]], -1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def conv_case(k, cin, cout, H, W, form="plain"):
    """form: 'plain' (no prologue), 'gn' (GroupNorm(32) + ReLU prologue, a residual for `fin`), 'bias' (1 x 1: bias), 'gnres' (1 x 1: bias + prologue + residual)"""
    rng = _rng(k, cin, cout, H, W, len(form)); B = conv_B(H, W) if k == 3 else (1 if (H, W) == (8, 16) else 2)
    c = dict(k=k, cin=cin, cout=cout, H=H, W=W, B=B, x=(rng.normal(size=(B, H, W, cin)) * 1.5 + 0.3).astype(np.float32), w=_weights(rng, cout, cin, k),
             bias=None, gn=None, res=None)
    if form in ("bias", "gnres"):
        c["bias"] = (rng.normal(size=cout) * 0.3).astype(np.float32)
    if form in ("gn", "gnres"):
        c["gn"] = dict(stats=stats32(c["x"], 32), gamma=(rng.random(cin) + 0.5).astype(np.float32), beta=(rng.normal(size=cin) * 0.2).astype(np.float32), groups=32)
        c["res"] = (rng.normal(size=(B, H, W, cout)) + 8.0).astype(np.float32)          # a residual with a large mean: the statistics of fin see mean / std = 8
    return c


CONST_ACT = 16.0


def _group_sign(cout, groups=32):
    return np.repeat(np.where(np.arange(groups) % 2 == 0, 1.0, -1.0), cout // groups)


def _group_mean_std(a, groups=32):
    """per channel: the mean and the standard deviation of its group of `a` (B, H, W, C) float64, taken over all frames"""
    C = a.shape[-1]; g = a.reshape(-1, groups, C // groups); m = g.mean((0, 2))
    return np.repeat(m, C // groups), np.repeat(np.sqrt(((g - m[None, :, None]) ** 2).mean((0, 2))), C // groups)


@functools.lru_cache(maxsize=None)
def conv3_offset_case(cin, cout, H, W, r):
    """The 'gn' case with a convolution output AND a block result whose groups of 32 have mean / std = r (alternating sign over the groups).  A 3 x 3 handle has no
    bias, so the offset comes through the input: input channel 0 gets gamma = 0, beta = CONST_ACT -- the prologue's fma(x, 0, 16) is exactly 16 at every pixel --
    and the CENTRE tap of every output channel on that channel is (r sigma_g - mu_g) / 16 (the centre tap never reads padding: the offset is the same at the border),
    mu_g and sigma_g the group's mean and standard deviation of the output without the offset.  The residual's mean tops the block result up to r standard deviations of fin."""
    c = dict(conv_case(3, cin, cout, H, W, "gn")); rng = _rng(41, cin, cout, H, W, r); B = c["B"]
    g = dict(c["gn"]); g["gamma"] = g["gamma"].copy(); g["beta"] = g["beta"].copy(); g["gamma"][0] = 0.0; g["beta"][0] = CONST_ACT
    w = c["w"].copy(); w[:, 0, 1, 1] = 0.0
    mg, sg = _group_mean_std(M.conv3x3(c["x"], w, gn=g)["out"]); sign = _group_sign(cout)
    w[:, 0, 1, 1] = ((r * sign * sg - mg) / CONST_ACT).astype(np.float32)
    res = rng.normal(size=(B, H, W, cout)) + r * sign * (np.sqrt(sg * sg + 1.0) - sg)
    c.update(gn=g, w=w, res=res.astype(np.float32), r=r); return c


@functools.lru_cache(maxsize=None)
def conv3_offset_reference(cin, cout, H, W, r):
    c = conv3_offset_case(cin, cout, H, W, r); m = M.conv3x3(c["x"], c["w"], None, c["gn"], c["res"]); e = M.emu_conv(c["x"], c["w"], None, c["gn"], c["res"])
    return m, e, M.per_channel_error(e["out"], m["out"]), M.per_channel_error(e["fin"], m["fin"])


def conv1_offset_bias(ca, r0, r):
    """1 x 1, form (a): the bias that puts the output's groups of 32 at mean / std = r; r0 = the model of the convolution without a bias"""
    mg, sg = _group_mean_std(r0["out"] + ca["bias"].astype(np.float64))
    return (ca["bias"] + r * _group_sign(ca["cout"]) * sg - mg).astype(np.float32)


@functools.lru_cache(maxsize=None)
def conv_reference(k, cin, cout, H, W, form="plain"):
    """-> (model dict, emu dict, e_emu per channel of `out`, e_emu per channel of `fin` or None)"""
    c = conv_case(k, cin, cout, H, W, form); f = M.conv3x3 if k == 3 else M.conv1x1
    r = f(c["x"], c["w"], c["bias"], c["gn"], c["res"]); e = M.emu_conv(c["x"], c["w"], c["bias"], c["gn"], c["res"])
    return r, e, M.per_channel_error(e["out"], r["out"]), None if r["fin"] is None else M.per_channel_error(e["fin"], r["fin"])


@functools.lru_cache(maxsize=None)
def lattice_case(k, cin, H, W):
    """activations n / 16, weights n 2^-6, n integer in [-8, 8] (one weight is 8 2^-6, so the layer's scale is 2^16): every split has lo = 0, every product and every
    partial sum is an integer multiple of 2^10 below 2^34 in scaled units -- asserted here -- so every float32 operation of any summation order is exact"""
    rng = _rng(7, k, cin, H, W); cout = 128 if cin == 256 else 64; B = conv_B(H, W)
    xi = rng.integers(-8, 9, (B, H, W, cin)); wi = rng.integers(-8, 9, (cout, cin, k, k)); wi[0, 0, 0, 0] = 8
    x = (xi / 16.0).astype(np.float32); w = (wi / 64.0).astype(np.float32)
    r = (M.conv3x3 if k == 3 else M.conv1x1)(x, w)
    assert (r["S"] * 16 * 64).max() < 2 ** 24, "a partial sum could leave the exact range"
    assert M.weight_scale(w) == 2.0 ** 16 and all((lo == 0).all() for lo in (M.split_f16(x * 16)[1], M.split_f16(w * 2.0 ** 16)[1]))
    return dict(k=k, cin=cin, cout=cout, H=H, W=W, B=B, x=x, w=w, ref=r["out"])


@functools.lru_cache(maxsize=None)
def stem_case(cout, cin, H, W, B):
    rng = _rng(11, cout, cin, H, W, B)
    c = dict(x=rng.normal(size=(B, H, W, cin)).astype(np.float32), w=(rng.normal(size=(cout, cin, 7, 7)) / np.sqrt(49 * cin)).astype(np.float32),
             bias=rng.normal(size=cout).astype(np.float32))
    c["ref_bias"] = M.stem7x7(c["x"], c["w"], c["bias"]); c["ref_plain"] = M.stem7x7(c["x"], c["w"], None)
    return c


# ---- the longest float32 partial chain n_p of every statistics producer, read from the kernels ------------------------------------------------------------------------
def gn_blocks(HW):
    return min(max(HW // 256, 1), 128)


def np_pass(HW, C):
    """gn_stats_kernel: a thread adds every (256 / (C / 4))-th pixel of its block's ceil(HW / blocks) pixels in float32; everything after that is float64"""
    rows = -(-HW // gn_blocks(HW)); return -(-rows // (256 // (C // 4)))


def sweep_blocks(HW):
    return min(max(HW // 64, 1), 256)


def np_sweep(HW, C, op):
    """sweep_stats_kernel: as the pass with vt_sweep_blocks(HW) blocks; the up-sampling form (op 1) walks quads of four output pixels"""
    items = HW if op == 0 else HW // 4; rows = -(-items // sweep_blocks(HW)); per = -(-rows // (256 // (C // 4)))
    return per if op == 0 else 4 * per


NP_CONV_OUT = 8 + 4          # conv3x3_kernel, statistics of the output: 8 image rows in the lane, then the 4 steps of the 16-lane DPP sum; float64 from there
NP_CONV_FIN = 8 + 2          # statistics of fin: 8 pixels in the thread, two shuffle steps, float64 from there


# ---- device side --------------------------------------------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch
    from vistracker_amd import _lib as L
    return torch, L, L.lib()


class In:
    """an input slice [coff, coff + C) of an NHWC tensor with cstride channels; NaN everywhere else in the allocation"""
    def __init__(self, data, cstride=None, coff=0):
        torch = _torch()[0]; data = np.ascontiguousarray(data, np.float32); C = data.shape[-1]; cstride = cstride or C; rows = data.size // C
        full = np.full((rows + 2 * GUARD, cstride), np.nan, np.float32); full[GUARD:GUARD + rows, coff:coff + C] = data.reshape(rows, C)
        self.full = torch.from_numpy(full).cuda(); self.before = self.full.clone(); self.cstride, self.coff = cstride, coff
        self.ptr = self.full.data_ptr() + 4 * GUARD * cstride

    def unchanged(self):
        torch = _torch()[0]; return bool(torch.equal(self.full.view(torch.int32), self.before.view(torch.int32)))


class Out:
    """an output slice; SENTINEL everywhere, compared bit for bit outside the slice by get()"""
    def __init__(self, shape, cstride=None, coff=0):
        torch = _torch()[0]; self.shape = tuple(shape); C = shape[-1]; self.C, self.cstride, self.coff = C, cstride or C, coff
        self.rows = int(np.prod(shape[:-1]))
        self.full = torch.full((self.rows + 2 * GUARD, self.cstride), SENTINEL, dtype=torch.int32, device="cuda")
        self.ptr = self.full.data_ptr() + 4 * GUARD * self.cstride

    def reset(self):
        self.full.fill_(SENTINEL); return self

    def untouched(self):
        return bool((self.full == SENTINEL).all().item())

    def get(self):
        torch = _torch()[0]; torch.cuda.synchronize(); a = self.full.cpu().numpy()
        mid = a[GUARD:GUARD + self.rows]
        assert (a[:GUARD] == SENTINEL).all() and (a[GUARD + self.rows:] == SENTINEL).all(), "a guard row around an output changed"
        assert (mid[:, :self.coff] == SENTINEL).all() and (mid[:, self.coff + self.C:] == SENTINEL).all(), "a channel outside the output slice changed"
        return np.ascontiguousarray(mid[:, self.coff:self.coff + self.C]).view(np.float32).reshape(self.shape)


class Ws:
    """a statistics workspace of n doubles between sentinel doubles; pairs(B, groups) reads the {mean, rstd} float pairs at its start"""
    def __init__(self, n):
        torch = _torch()[0]; self.n = int(n); self.full = torch.full((self.n + 128,), -7.25, dtype=torch.float64, device="cuda"); self.full[64:64 + self.n] = float("nan")
        self.ptr = self.full.data_ptr() + 8 * 64

    def pairs(self, B, groups):
        torch = _torch()[0]; torch.cuda.synchronize()
        assert bool((self.full[:64] == -7.25).all() and (self.full[64 + self.n:] == -7.25).all()), "a write outside the statistics workspace"
        return self.full[64:64 + B * groups].view(torch.float32).reshape(B, groups, 2).cpu().numpy().astype(np.float64)


def dev(a):
    torch = _torch()[0]; return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return None if t is None else (t.ptr if hasattr(t, "ptr") else t.data_ptr())


class Conv3:
    def __init__(self, w):
        _, L, lib = _torch(); self.h = ctypes.c_void_p(); w = np.ascontiguousarray(w, np.float32); self.cout, self.cin = w.shape[:2]
        L.check(lib.vt_conv3x3_create(ctypes.byref(self.h), w.ctypes.data, self.cout, self.cin, L.stream_ptr()))

    def close(self):
        _torch()[2].vt_conv3x3_destroy(self.h)


class Conv1:
    def __init__(self, w, bias):
        _, L, lib = _torch(); self.h = ctypes.c_void_p(); w = np.ascontiguousarray(w, np.float32).reshape(w.shape[0], w.shape[1]); self.cout, self.cin = w.shape
        b = None if bias is None else np.ascontiguousarray(bias, np.float32)
        L.check(lib.vt_conv1x1_create(ctypes.byref(self.h), w.ctypes.data, None if b is None else b.ctypes.data, self.cout, self.cin, L.stream_ptr()))

    def close(self):
        _torch()[2].vt_conv1x1_destroy(self.h)


def finalize(ws, nblk, B, HW, C, groups):
    _, L, lib = _torch(); L.check(lib.vt_groupnorm_finalize(ws.ptr, nblk, B, HW, C, groups, EPS, L.stream_ptr())); return ws.pairs(B, groups)


def run_conv3x3_plain(c, coff=16, pad=32):
    """vt_conv3x3_forward into channels [coff, coff + Cout) of a wider tensor -> out (B, H, W, Cout) float32"""
    _, L, lib = _torch(); h = Conv3(c["w"]); x = In(c["x"]); o = Out((c["B"], c["H"], c["W"], c["cout"]), c["cout"] + pad, coff)
    L.check(lib.vt_conv3x3_forward(h.h, x.ptr, c["B"], c["H"], c["W"], o.ptr, o.cstride, o.coff, L.stream_ptr()))
    got = o.get(); assert x.unchanged(); h.close(); return got


def run_conv3x3_forms(c, stats_groups=32):
    """Every entry point of the 3 x 3 form on a 'gn' case (prologue, residual at a channel offset).  -> dict of outputs (float32) and finalized statistics"""
    _, L, lib = _torch(); B, H, W, cin, cout = c["B"], c["H"], c["W"], c["cin"], c["cout"]; g = c["gn"]; HW = H * W; sp = L.stream_ptr()
    h = Conv3(c["w"]); x = In(c["x"], cin + 8, 4); res = In(c["res"], cout + 8, 4)
    st, ga, be = dev(g["stats"]), dev(g["gamma"]), dev(g["beta"]); tiles = lib.vt_conv3x3_tiles(H, W); assert tiles == (H // 8) * (W // 16)
    gn = (st.data_ptr(), ga.data_ptr(), be.data_ptr(), g["groups"])
    mk = lambda: Out((B, H, W, cout), cout + 16, 8); R = {}
    o = mk(); L.check(lib.vt_conv3x3_forward_gn(h.h, x.ptr, x.cstride, x.coff, None, None, None, 0, B, H, W, o.ptr, o.cstride, o.coff, sp)); R["noprologue"] = o.get()
    o = mk(); L.check(lib.vt_conv3x3_forward_gn(h.h, x.ptr, x.cstride, x.coff, *gn, B, H, W, o.ptr, o.cstride, o.coff, sp)); R["gn"] = o.get()
    o = mk(); ws = Ws(B * stats_groups + tiles * B * cout * 2)
    L.check(lib.vt_conv3x3_forward_gn_stats(h.h, x.ptr, x.cstride, x.coff, *gn, B, H, W, o.ptr, o.cstride, o.coff, ws.ptr, stats_groups, sp))
    R["gn_stats"] = o.get(); R["gn_stats_pairs"] = finalize(ws, tiles, B, HW, cout, stats_groups)
    o, f = mk(), Out((B, H, W, cout), cout + 32, 12)
    L.check(lib.vt_conv3x3_forward_block(h.h, x.ptr, x.cstride, x.coff, *gn, B, H, W, o.ptr, o.cstride, o.coff, res.ptr, res.cstride, res.coff, f.ptr, f.cstride, f.coff, None, 0, sp))
    R["block_out"], R["block_fin"] = o.get(), f.get()
    f = Out((B, H, W, cout), cout + 32, 12)
    L.check(lib.vt_conv3x3_forward_block(h.h, x.ptr, x.cstride, x.coff, *gn, B, H, W, None, 0, 0, res.ptr, res.cstride, res.coff, f.ptr, f.cstride, f.coff, None, 0, sp))
    R["finonly_fin"] = f.get()
    # both statistics blocks; the result's statistics are those of a tensor of fin_cstride channels: this launch owns all of it (coff 0, cstride Cout)
    o, f = mk(), Out((B, H, W, cout)); ws = Ws(B * stats_groups + tiles * B * cout * 2); fws = Ws(B * stats_groups + tiles * B * cout * 2)
    L.check(lib.vt_conv3x3_forward_block_stats(h.h, x.ptr, x.cstride, x.coff, *gn, B, H, W, o.ptr, o.cstride, o.coff, res.ptr, res.cstride, res.coff, f.ptr, f.cstride, f.coff,
                                               ws.ptr, stats_groups, fws.ptr, stats_groups, sp))
    R["bs_out"], R["bs_fin"] = o.get(), f.get()
    R["bs_pairs"] = finalize(ws, tiles, B, HW, cout, stats_groups); R["bs_fin_pairs"] = finalize(fws, tiles, B, HW, cout, stats_groups)
    assert x.unchanged() and res.unchanged(); h.close(); return R


def run_conv1x1(ca, cb):
    """ca: the 'bias' case, cb: the 'gnres' case of one (cin, cout, H, W) (same weights are NOT shared: each case has its own).  Form (a): bias, channel-offset input
    and output, output statistics; form (b): prologue + residual; (c): a handle created with bias = NULL on ca's data."""
    _, L, lib = _torch(); B, H, W, cin, cout = ca["B"], ca["H"], ca["W"], ca["cin"], ca["cout"]; sp = L.stream_ptr(); HW = H * W; tiles = lib.vt_conv3x3_tiles(H, W); R = {}
    h = Conv1(ca["w"], ca["bias"]); x = In(ca["x"], cin + 8, 4); o = Out((B, H, W, cout), cout + 16, 8); ws = Ws(B * 32 + tiles * B * cout * 2)
    L.check(lib.vt_conv1x1_forward(h.h, x.ptr, x.cstride, x.coff, None, None, None, 0, B, H, W, o.ptr, o.cstride, o.coff, None, 0, 0, ws.ptr, 32, sp))
    R["a"] = o.get(); R["a_pairs"] = finalize(ws, tiles, B, HW, cout, 32)
    o = Out((B, H, W, cout), cout + 16, 8)
    L.check(lib.vt_conv1x1_forward(h.h, x.ptr, x.cstride, x.coff, None, None, None, 0, B, H, W, o.ptr, o.cstride, o.coff, None, 0, 0, None, 0, sp))
    R["a_nostats"] = o.get(); assert x.unchanged(); h.close()
    h = Conv1(ca["w"], None); o = Out((B, H, W, cout), cout + 16, 8)
    L.check(lib.vt_conv1x1_forward(h.h, x.ptr, x.cstride, x.coff, None, None, None, 0, B, H, W, o.ptr, o.cstride, o.coff, None, 0, 0, None, 0, sp))
    R["c"] = o.get(); h.close()
    g = cb["gn"]; h = Conv1(cb["w"], cb["bias"]); x = In(cb["x"], cin + 8, 4); res = In(cb["res"], cout + 4, 4); o = Out((B, H, W, cout))
    st, ga, be = dev(g["stats"]), dev(g["gamma"]), dev(g["beta"])
    L.check(lib.vt_conv1x1_forward(h.h, x.ptr, x.cstride, x.coff, st.data_ptr(), ga.data_ptr(), be.data_ptr(), g["groups"], B, H, W, o.ptr, o.cstride, o.coff,
                                   res.ptr, res.cstride, res.coff, None, 0, sp))
    R["b"] = o.get(); assert x.unchanged() and res.unchanged(); h.close(); return R


def run_conv1x1_stats(ca, bias):
    """form (a) of ca with another bias -> out, its finalized statistics"""
    _, L, lib = _torch(); B, H, W, cin, cout = ca["B"], ca["H"], ca["W"], ca["cin"], ca["cout"]; tiles = lib.vt_conv3x3_tiles(H, W)
    h = Conv1(ca["w"], bias); x = In(ca["x"], cin + 8, 4); o = Out((B, H, W, cout), cout + 16, 8); ws = Ws(B * 32 + tiles * B * cout * 2)
    L.check(lib.vt_conv1x1_forward(h.h, x.ptr, x.cstride, x.coff, None, None, None, 0, B, H, W, o.ptr, o.cstride, o.coff, None, 0, 0, ws.ptr, 32, L.stream_ptr()))
    got = o.get(); pairs = finalize(ws, tiles, B, H * W, cout, 32); assert x.unchanged(); h.close(); return got, pairs


def run_lattice(c):
    _, L, lib = _torch(); B, H, W = c["B"], c["H"], c["W"]
    if c["k"] == 3:
        return run_conv3x3_plain(c, coff=4, pad=8)
    h = Conv1(c["w"], None); x = In(c["x"], c["cin"] + 4, 4); o = Out((B, H, W, c["cout"]), c["cout"] + 8, 4)
    L.check(lib.vt_conv1x1_forward(h.h, x.ptr, x.cstride, x.coff, None, None, None, 0, B, H, W, o.ptr, o.cstride, o.coff, None, 0, 0, None, 0, L.stream_ptr()))
    got = o.get(); h.close(); return got


def run_stem(c, with_bias):
    _, L, lib = _torch(); w = np.ascontiguousarray(c["w"]); cout, cin = w.shape[:2]; B, H, W, _ = c["x"].shape; H2, W2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    h = ctypes.c_void_p(); b = np.ascontiguousarray(c["bias"])
    L.check(lib.vt_stem7x7_create(ctypes.byref(h), w.ctypes.data, b.ctypes.data if with_bias else None, cout, cin, L.stream_ptr()))
    x = In(c["x"], cin + 3, 2); o = Out((B, H2, W2, cout), cout + 8, 4)
    L.check(lib.vt_stem7x7_forward(h, x.ptr, x.cstride, x.coff, B, H, W, o.ptr, o.cstride, o.coff, L.stream_ptr()))
    got = o.get(); assert x.unchanged(); lib.vt_stem7x7_destroy(h); return got


def run_gn_stats(x, groups):
    """vt_groupnorm_stats on x (B, HW, C) as the channel slice [4, 4 + C) of a tensor of C + 8 channels -> pairs (B, groups, 2)"""
    _, L, lib = _torch(); B, HW, C = x.shape; xi = In(x, C + 8, 4); ws = Ws(lib.vt_groupnorm_workspace_doubles(B, HW, C, groups))
    assert ws.n == B * groups + gn_blocks(HW) * B * C * 2
    L.check(lib.vt_groupnorm_stats(xi.ptr, xi.cstride, xi.coff, B, HW, C, groups, EPS, ws.ptr, L.stream_ptr()))
    p = ws.pairs(B, groups); assert xi.unchanged(); return p


def run_gn_nhwc(x, gamma, beta, groups, relu):
    _, L, lib = _torch(); B, HW, C = x.shape; xi = In(x); ws = Ws(lib.vt_groupnorm_workspace_doubles(B, HW, C, groups)); y = Out((B, HW, C)); ga, be = dev(gamma), dev(beta)
    L.check(lib.vt_groupnorm_nhwc(xi.ptr, ga.data_ptr(), be.data_ptr(), B, HW, C, groups, EPS, int(relu), ws.ptr, y.ptr, L.stream_ptr()))
    return ws.pairs(B, groups), y.get()


def run_avgpool(x, groups, stats):
    """x (B, 2h, 2w, C) -> out (B, h, w, C), pairs or None"""
    _, L, lib = _torch(); B, H, W, C = x.shape; h, w = H // 2, W // 2; xi = In(x); o = Out((B, h, w, C)); nblk = lib.vt_sweep_blocks(h * w)
    ws = Ws(B * groups + nblk * B * C * 2) if stats else None
    L.check(lib.vt_avgpool2x2_stats(xi.ptr, B, H, W, C, o.ptr, _p(ws), groups if stats else 0, L.stream_ptr()))
    got = o.get(); assert xi.unchanged()
    return got, (finalize(ws, nblk, B, h * w, C, groups) if stats else None)


def run_upsample(low, skip, groups, form):
    """form: 'plain' (vt_upsample2x_bicubic_add), 'nostats' (the _stats entry with stats_ws = NULL), 'stats'"""
    _, L, lib = _torch(); B, h, w, C = low.shape; li = In(low); si = None if skip is None else In(skip); o = Out((B, 2 * h, 2 * w, C)); nblk = lib.vt_sweep_blocks(4 * h * w)
    ws = Ws(B * groups + nblk * B * C * 2) if form == "stats" else None
    if form == "plain":
        L.check(lib.vt_upsample2x_bicubic_add(li.ptr, _p(si), B, h, w, C, o.ptr, L.stream_ptr()))
    else:
        L.check(lib.vt_upsample2x_bicubic_add_stats(li.ptr, _p(si), B, h, w, C, o.ptr, _p(ws), groups if ws else 0, L.stream_ptr()))
    got = o.get(); assert li.unchanged() and (si is None or si.unchanged())
    return got, (finalize(ws, nblk, B, 4 * h * w, C, groups) if ws else None)
