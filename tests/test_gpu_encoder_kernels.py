"""GPU (-m gpu): the forward kernels of the HGFilter encoder (csrc/conv.hip, stem.hip, encoder_ops.hip) against the float64 model of tests/encoder_model.py, per
output channel and per element, on the cases of tests/encoder_cases.py.

No gate comes from a kernel's output; u = 2^-24.
* convolutions, per output channel c:  err_c = max_(b,y,x) |got - ref64| / max |ref64[..., c]| <= 8 e_emu_c, e_emu_c the same metric of encoder_model.emu_conv (the
  kernels' number format -- split-f16 operands, float32 products and sums -- in plain index order on the CPU).  The factor 8 is the allowance of the SMPL-H gate
  for another float32 summation order, taken from that precedent.  A channel whose reference is identically 0 must be exactly 0.
* convolutions, per element (backstop):  |got - ref64| <= (3 2^-22 + 3 K u) S, K = taps x Cin, S = sum |w| |act| (+ |bias|): the operands' 22 bits and the worst
  case of a sequential float32 sum of the 3 K partial products.  ASSUMPTION: how the MFMA rounds inside one instruction is not documented; it is taken as no worse
  than that sequential sum.  With the GroupNorm prologue + sum |w| dact, dact the four float32 roundings of a = rstd gamma, mean a, beta - mean a and fma(x, a, s)
  (encoder_model.prologue; the statistics are float32 INPUTS of kernel and model alike); for fin = conv + res + u |fin|.
* exact lattice: activations n / 16, weights n / 64, |n| <= 8: every operation is exact, the output is bit-equal to the model.
* stem, per element: (49 Cin + 2) u S (a chain of 49 Cin fmas, the bias).
* avgpool: bit-equal to the float32 statement ((v00 + v01) + v10 + v11) * 0.25f.
* up-sampling, per element: 9 u sum |w_y w_x v| + Sw + Sc + u |skip| (encoder_model.UPSAMPLE_N and upsample2x_bicubic_add: 8 roundings per term, one for the skip
  addition, the absolute errors of the float32 weights and source coordinate).
* statistics, per (frame, group), against the float64 statistics of the tensor the kernel STORED: mean within n_p u E|x| + u |mean|, rstd within what
  dvar <= (n_p + 2) u (E[x^2] + 2 |mean| E|x|) allows (encoder_model.stats_gates), n_p the producer's longest float32 chain (encoder_cases.np_pass, np_sweep,
  NP_CONV_OUT, NP_CONV_FIN).  At mean / std = 8 that bound on rstd is NOT below 1e-4 relative for chains longer than a few values (it crosses 1e-4 at
  (3 r^2 + 1) (n_p + 2) u / 2 = 1e-4: r = 2.9 for n_p = 128; the convolutions' epilogues, n_p <= 12, have 8e-5 at r = 8 and 1.3e-4 at r = 10), so the old tests' 1e-4
  is asserted next to the gate on centred data (r = 0) only.  Offset data (encoder_cases.RATIOS: mean / std 0, 10, 64) goes through the pass kernel, the
  convolutions' output statistics (3 x 3: a constant input channel under the centre tap; 1 x 1: the bias), the fin statistics (a residual with a mean) and both sweeps.
* GroupNorm apply pass, per element, given the pairs the kernel computed: 4 u (|(x - mean) rstd gamma| + |beta|) -- gn_apply_kernel evaluates
  ((x - mean) * rstd) * gamma + beta without contraction: the difference, two products and the sum round once each, each by at most u of its own result; the
  first three act on p = (x - mean) rstd gamma (3 u |p|), the last on p + beta (u (|p| + |beta|)).
tests/test_host_encoder_model.py shows that the references stay inside these gates and that the per-channel gate catches what the older whole-tensor metric misses.
Every test prints its worst fraction of its gate before it asserts."""
import numpy as np
import pytest

import encoder_cases as C
import encoder_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
U = M.U


def _frac(err, gate):
    return np.where(gate > 0, err / np.where(gate > 0, gate, 1), np.where(err > 0, np.inf, 0.0))


def check_conv(got, ref, e_emu, backstop, what):
    """the per-channel gate and the per-element backstop; -> (worst channel, its fraction of the channel gate, worst fraction of the backstop)"""
    assert np.isfinite(got).all(), what
    ec = M.per_channel_error(got, ref); fc = _frac(ec, 8 * e_emu); fe = _frac(np.abs(got.astype(np.float64) - ref), backstop)
    c = int(fc.argmax())
    print("%s: worst channel %d at %.3f of its gate (err %.2e, e_emu %.2e); worst element %.3f of the backstop" % (what, c, fc[c], ec[c], e_emu[c], fe.max()))
    assert (fc <= 1).all(), (what, c, float(ec[c]), float(e_emu[c]))
    assert (fe <= 1).all(), (what, float(fe.max()))
    return c, float(fc[c]), float(fe.max())


def check_stats(pairs, stored, groups, n_p, what, old_tol=False, m=None):
    """pairs (B, groups, 2) against the float64 statistics of the stored float32 tensor (m: those statistics, where the caller has them already)"""
    m = M.groupnorm_stats(stored, groups, C.EPS) if m is None else m; gm, gr = M.stats_gates(m, n_p, C.EPS)
    fm = _frac(np.abs(pairs[..., 0] - m["mean"]), gm); fr = _frac(np.abs(pairs[..., 1] - m["rstd"]), gr); rel = np.abs(pairs[..., 1] / m["rstd"] - 1).max()
    print("%s: n_p %d, mean %.3f of its gate, rstd %.3f of its gate (rel %.2e; the gate allows %.2e)" % (what, n_p, fm.max(), fr.max(), rel, (gr / m["rstd"]).max()))
    assert np.isfinite(pairs).all() and (fm <= 1).all() and (fr <= 1).all(), (what, float(fm.max()), float(fr.max()))
    if old_tol:
        assert rel < 1e-4, (what, rel)
    return float(fm.max()), float(fr.max())


# ---- 3 x 3 ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,H,W", C.CONV3_CASES)
def test_conv3x3_classes_and_sizes(cin, cout, H, W):
    c = C.conv_case(3, cin, cout, H, W); r, _, e_emu, _ = C.conv_reference(3, cin, cout, H, W)
    check_conv(C.run_conv3x3_plain(c), r["out"], e_emu, M.conv_backstop(r), "3x3 %d->%d %dx%d B=%d" % (cin, cout, H, W, c["B"]))


@pytest.mark.parametrize("r", C.RATIOS)
@pytest.mark.parametrize("cin,cout", C.CONV3_ALL_SIZES)
def test_conv3x3_forms(cin, cout, r):
    """every entry point at 24 x 48, B = 3: prologue, out + fin with a residual at a channel offset, fin only, both statistics blocks; calls that differ only in NULL
    arguments are bit-equal.  The convolution's output and the block result both have mean / std = r per group of 32 (encoder_cases.conv3_offset_case)"""
    c = C.conv3_offset_case(cin, cout, 24, 48, r); m, _, e_out, e_fin = C.conv3_offset_reference(cin, cout, 24, 48, r); R = C.run_conv3x3_forms(c)
    what = "3x3 forms %d->%d B=%d r=%d" % (cin, cout, c["B"], r)
    check_conv(R["gn"], m["out"], e_out, M.conv_backstop(m), what + " gn")
    check_conv(R["block_fin"], m["fin"], e_fin, M.conv_backstop(m, fin=True), what + " fin")
    for k in ("gn_stats", "block_out", "bs_out"):
        assert np.array_equal(R[k].view(np.int32), R["gn"].view(np.int32)), k
    for k in ("finonly_fin", "bs_fin"):
        assert np.array_equal(R[k].view(np.int32), R["block_fin"].view(np.int32)), k
    if r == 0:              # without the prologue: the plain convolution of the same slice
        r0 = M.conv3x3(c["x"], c["w"]); e0 = M.per_channel_error(M.emu_conv(c["x"], c["w"])["out"], r0["out"])
        check_conv(R["noprologue"], r0["out"], e0, M.conv_backstop(r0), what + " no prologue")
    check_stats(R["gn_stats_pairs"], R["gn"], 32, C.NP_CONV_OUT, what + " output statistics", old_tol=(r == 0))
    assert np.array_equal(R["bs_pairs"], R["gn_stats_pairs"])
    check_stats(R["bs_fin_pairs"], R["block_fin"], 32, C.NP_CONV_FIN, what + " fin statistics", old_tol=(r == 0))


@pytest.mark.parametrize("k,cin,H,W", C.LATTICE_CASES)
def test_lattice_is_bit_equal(k, cin, H, W):
    c = C.lattice_case(k, cin, H, W); got = C.run_lattice(c)
    assert np.array_equal(got.astype(np.float64), c["ref"]), (np.abs(got - c["ref"]).max(), np.argwhere(got != c["ref"])[:4])


# ---- 1 x 1 ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,H,W", C.CONV1_CASES)
def test_conv1x1_all_pairs(cin, cout, H, W):
    ca, cb = C.conv_case(1, cin, cout, H, W, "bias"), C.conv_case(1, cin, cout, H, W, "gnres")
    ra, _, ea, _ = C.conv_reference(1, cin, cout, H, W, "bias"); rb, _, _, eb = C.conv_reference(1, cin, cout, H, W, "gnres")
    R = C.run_conv1x1(ca, cb); what = "1x1 %d->%d %dx%d B=%d" % (cin, cout, H, W, ca["B"])
    check_conv(R["a"], ra["out"], ea, M.conv_backstop(ra), what + " (a) bias")
    assert np.array_equal(R["a"].view(np.int32), R["a_nostats"].view(np.int32))
    check_conv(R["b"], rb["fin"], eb, M.conv_backstop(rb, fin=True), what + " (b) prologue + residual")
    r0 = M.conv1x1(ca["x"], ca["w"]); e0 = M.per_channel_error(M.emu_conv(ca["x"], ca["w"])["out"], r0["out"])
    check_conv(R["c"], r0["out"], e0, M.conv_backstop(r0), what + " (c) no bias")
    check_stats(R["a_pairs"], R["a"], 32, C.NP_CONV_OUT, what + " output statistics", old_tol=True)
    raw = C.conv_reference(1, cin, cout, H, W, "bias")[1]["raw"]
    for r in C.RATIOS[1:]:          # the output's groups at mean / std = r through the bias; model and emulation follow from the ones without a bias
        b = C.conv1_offset_bias(ca, r0, r); mr = dict(r0, out=r0["out"] + b.astype(np.float64), S=r0["S"] + np.abs(b.astype(np.float64)))
        got, pairs = C.run_conv1x1_stats(ca, b)
        check_conv(got, mr["out"], M.per_channel_error(raw + b, mr["out"]), M.conv_backstop(mr), what + " (a) bias r=%d" % r)
        check_stats(pairs, got, 32, C.NP_CONV_OUT, what + " output statistics r=%d" % r)


# ---- stem ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("cout,cin,H,W", C.STEM_CASES)
def test_stem(cout, cin, H, W, B):
    c = C.stem_case(cout, cin, H, W, B)
    for with_bias, r in ((True, c["ref_bias"]), (False, c["ref_plain"])):
        got = C.run_stem(c, with_bias); f = _frac(np.abs(got.astype(np.float64) - r["out"]), M.stem_backstop(r))
        print("stem %d<-%d %dx%d B=%d bias=%d: worst element %.3f of its gate" % (cout, cin, H, W, B, with_bias, f.max()))
        assert np.isfinite(got).all() and (f <= 1).all(), f.max()


# ---- GroupNorm -------------------------------------------------------------------------------------------------------------------------------------------------------
def _frames(m, B):
    return {k: v[:B] for k, v in m.items()}


@pytest.mark.parametrize("r", C.RATIOS)
@pytest.mark.parametrize("Cc,groups", C.GN_CASES)
def test_groupnorm_statistics(Cc, groups, r):
    """vt_groupnorm_stats on the channel slice [4, 4 + C) of a wider tensor: every HW, B = 1 and 3 (B = 1 is the first frame of the same data)"""
    for HW in C.GN_HW:
        x = C.offset_data(C._rng(21, Cc, groups, HW, r), (3, HW, Cc), groups, r); m = M.groupnorm_stats(x, groups, C.EPS)
        for B in (1, 3):
            check_stats(C.run_gn_stats(x[:B], groups), None, groups, C.np_pass(HW, Cc), "pass C=%d groups=%d HW=%d B=%d r=%d" % (Cc, groups, HW, B, r),
                        old_tol=(r == 0 and HW > 1), m=_frames(m, B))


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("Cc,groups", C.GN_CASES)
def test_groupnorm_nhwc(Cc, groups, relu):
    """vt_groupnorm_nhwc: every HW, B = 1 and 3, every r; the statistics and the apply pass"""
    for HW in C.GN_HW:
        for r in C.RATIOS:
            rng = C._rng(22, Cc, groups, HW, relu, r); x = C.offset_data(rng, (3, HW, Cc), groups, r); m = M.groupnorm_stats(x, groups, C.EPS)
            gamma = (rng.random(Cc) + 0.5).astype(np.float32); beta = (rng.normal(size=Cc) * 0.2).astype(np.float32)
            for B in (1, 3):
                what = "nhwc C=%d groups=%d HW=%d B=%d relu=%d r=%d" % (Cc, groups, HW, B, relu, r)
                pairs, y = C.run_gn_nhwc(x[:B], gamma, beta, groups, relu)
                check_stats(pairs, None, groups, C.np_pass(HW, Cc), what, old_tol=(r == 0 and HW > 1), m=_frames(m, B))
                # the apply pass, given the pairs the kernel computed (gate: the docstring)
                ref = M.groupnorm_apply(x[:B], pairs, gamma, beta, relu); mm = np.repeat(pairs[..., 0], Cc // groups, 1)[:, None]; rs = np.repeat(pairs[..., 1], Cc // groups, 1)[:, None]
                gate = 4 * U * (np.abs((x[:B] - mm) * rs * gamma) + np.abs(beta))
                f = _frac(np.abs(y - ref), gate); print("%s apply: worst element %.3f of its gate" % (what, f.max()))
                assert (f <= 1).all(), (what, f.max())


def test_groupnorm_refusals():
    torch_, L, lib = C._torch(); sp = L.stream_ptr()
    x = C.In(np.zeros((1, 16, 1028 + 8), np.float32)); ws = C.Ws(4096); y = C.Out((1, 16, 1028))
    g = C.dev(np.ones(1028, np.float32))
    bad = [lib.vt_groupnorm_stats(x.ptr, 1028, 0, 1, 16, 1028, 1, C.EPS, ws.ptr, sp),            # C = 1028
           lib.vt_groupnorm_stats(x.ptr, 40, 2, 1, 16, 32, 32, C.EPS, ws.ptr, sp),                # coff = 2
           lib.vt_groupnorm_stats(x.ptr, 38, 4, 1, 16, 32, 32, C.EPS, ws.ptr, sp),                # cstride % 4
           lib.vt_groupnorm_stats(x.ptr, 32, 4, 1, 16, 32, 32, C.EPS, ws.ptr, sp),                # cstride < coff + C
           lib.vt_groupnorm_nhwc(x.ptr, g.data_ptr(), g.data_ptr(), 1, 16, 1028, 4, C.EPS, 1, ws.ptr, y.ptr, sp)]
    torch_.cuda.synchronize()
    assert all(b != 0 for b in bad), bad
    assert y.untouched() and bool(torch_.isnan(ws.full[64:64 + ws.n]).all()), "a refused call wrote"


# ---- sweeps ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _groups(Cc):
    return 32 if Cc % 32 == 0 else Cc


@pytest.mark.parametrize("Cc", C.SWEEP_C)
@pytest.mark.parametrize("h,w", C.SWEEP_OUT)
def test_avgpool(h, w, Cc):
    g = _groups(Cc)
    for B, r in zip((1, 3, 1), C.RATIOS):
        x = C.offset_data(C._rng(31, h, w, Cc, r), (B, 2 * h, 2 * w, Cc), g, r); m = M.avgpool2x2(x)
        got, pairs = C.run_avgpool(x, g, True); got0, _ = C.run_avgpool(x, g, False)
        assert np.array_equal(got.view(np.int32), m["f32"].view(np.int32)) and np.array_equal(got0.view(np.int32), got.view(np.int32))
        assert np.abs(got - m["out"]).max() <= 3 * U * np.abs(x).max()
        assert C._torch()[2].vt_sweep_blocks(h * w) == C.sweep_blocks(h * w)
        check_stats(pairs, got, g, C.np_sweep(h * w, Cc, 0), "avgpool -> %dx%d C=%d B=%d r=%d" % (h, w, Cc, B, r), old_tol=(r == 0))


@pytest.mark.parametrize("Cc", C.SWEEP_C)
@pytest.mark.parametrize("h,w", C.UP_SOURCES)
def test_upsample(h, w, Cc):
    g = _groups(Cc)
    for B, r, with_skip in zip((1, 3, 1), C.RATIOS, (True, True, False)):
        rng = C._rng(32, h, w, Cc, r); low = C.offset_data(rng, (B, h, w, Cc), g, r); skip = rng.normal(size=(B, 2 * h, 2 * w, Cc)).astype(np.float32) if with_skip else None
        m = M.upsample2x_bicubic_add(low, skip); gate = M.upsample_gate(m)
        got, pairs = C.run_upsample(low, skip, g, "stats"); got0, _ = C.run_upsample(low, skip, g, "nostats"); got1, _ = C.run_upsample(low, skip, g, "plain")
        assert np.array_equal(got.view(np.int32), got0.view(np.int32)), "stats_ws NULL and non-NULL differ"
        for nm, a in (("stats form", got), ("plain form", got1)):
            f = _frac(np.abs(a - m["out"]), gate); print("upsample %dx%d C=%d B=%d r=%d %s: worst element %.3f of its gate" % (h, w, Cc, B, r, nm, f.max()))
            assert np.isfinite(a).all() and (f <= 1).all(), (nm, f.max())
        check_stats(pairs, got, g, C.np_sweep(4 * h * w, Cc, 1), "upsample %dx%d C=%d B=%d r=%d" % (h, w, Cc, B, r), old_tol=(r == 0))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_conv_refusals_write_nothing():
    torch_, L, lib = C._torch(); sp = L.stream_ptr(); c = C.conv_case(3, 32, 64, 8, 16, "gn"); g = c["gn"]
    h = C.Conv3(c["w"]); h1 = C.Conv1(C.conv_case(1, 32, 64, 8, 16, "bias")["w"], None)
    x = C.In(np.zeros((1, 24, 48, 40), np.float32)); res = C.In(np.zeros((1, 24, 48, 72), np.float32))
    o, f = C.Out((1, 24, 48, 64), 80, 8), C.Out((1, 24, 48, 64), 80, 8); ws = C.Ws(32 + 9 * 64 * 2)
    st, ga, be = C.dev(g["stats"]), C.dev(g["gamma"]), C.dev(g["beta"]); gn = (st.data_ptr(), ga.data_ptr(), be.data_ptr(), 32)
    blk = lambda H, W, ics, ico, ocs, oco, r, fi, fws: lib.vt_conv3x3_forward_block_stats(h.h, x.ptr, ics, ico, *gn, 1, H, W, o.ptr, ocs, oco, r, 72, 4, fi, 80, 8, None, 0, fws, 32, sp)
    bad = dict(H12=blk(12, 48, 40, 4, 80, 8, None, None, None), W24=blk(8, 24, 40, 4, 80, 8, None, None, None), in_coff2=blk(8, 16, 40, 2, 80, 8, None, None, None),
               out_coff2=blk(8, 16, 40, 4, 80, 2, None, None, None), in_cstride=blk(8, 16, 32, 4, 80, 8, None, None, None), out_cstride=blk(8, 16, 40, 4, 68, 8, None, None, None),
               fin_without_res=blk(8, 16, 40, 4, 80, 8, None, f.ptr, None), fin_stats_without_fin=blk(8, 16, 40, 4, 80, 8, None, None, ws.ptr),
               one_H12=lib.vt_conv1x1_forward(h1.h, x.ptr, 40, 4, None, None, None, 0, 1, 12, 48, o.ptr, 80, 8, None, 0, 0, None, 0, sp),
               one_coff2=lib.vt_conv1x1_forward(h1.h, x.ptr, 40, 2, None, None, None, 0, 1, 8, 16, o.ptr, 80, 8, None, 0, 0, None, 0, sp),
               one_cstride=lib.vt_conv1x1_forward(h1.h, x.ptr, 40, 4, None, None, None, 0, 1, 8, 16, o.ptr, 68, 8, None, 0, 0, None, 0, sp))
    torch_.cuda.synchronize()
    assert all(v != 0 for v in bad.values()), bad
    assert o.untouched() and f.untouched() and bool(torch_.isnan(ws.full[64:64 + ws.n]).all()), "a refused call wrote"
    h.close(); h1.close()
