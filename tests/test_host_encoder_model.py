"""CPU: the float64 model of the encoder's forward operations (tests/encoder_model.py) and the gates of tests/test_gpu_encoder_kernels.py, without a GPU.
1. The model agrees with torch float64 F.conv2d, F.group_norm, F.avg_pool2d and F.interpolate to 1e-12 (relative to the tensor's largest value).
2. The references alone are inside the gates: emu_conv (the kernels' number format in plain index order) and a plain torch float32 convolution stay inside every
   per-element backstop; torch float32 up-sampling, pooling, the stem and float32 statistics in the producers' chain lengths stay inside theirs.
3. Four mutants of emu_conv's output each fail the per-channel gate by at least 10 x; for each, the whole-tensor metric of
   test_gpu_parity.py::test_conv3x3_split_f16_vs_float64 (max |got - ref| < 2e-6 max |ref|) is evaluated and what it says is asserted: it sees all four on these
   cases (the smallest channel's scale is 0.01 of the largest: 5 % of it is 4e-4 of the tensor's maximum), and it passes a fifth, the smallest channel x 1.0002,
   which the per-channel gate fails by more than 10 x."""
import numpy as np
import pytest

import encoder_cases as C
import encoder_model as M

torch = pytest.importorskip("torch")
F = torch.nn.functional

CONV_CASES = [(3,) + c + ("plain",) for c in C.CONV3_CASES] + [(1,) + c + (f,) for c in C.CONV1_CASES for f in ("bias", "gnres")]          # every case of the GPU file


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


def close(a, b):
    return np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


def _torch_ref(c, dtype):
    x = nchw(c["x"]).to(dtype); w = torch.from_numpy(c["w"]).to(dtype); k = c["k"]
    if c["gn"] is not None:
        g = c["gn"]; st = torch.from_numpy(g["stats"]).to(dtype); rep = c["cin"] // g["groups"]
        mean = st[..., 0].repeat_interleave(rep, 1)[:, :, None, None]; rstd = st[..., 1].repeat_interleave(rep, 1)[:, :, None, None]
        x = F.relu((x - mean) * rstd * torch.from_numpy(g["gamma"]).to(dtype)[None, :, None, None] + torch.from_numpy(g["beta"]).to(dtype)[None, :, None, None])
    out = F.conv2d(x, w, None if c["bias"] is None else torch.from_numpy(c["bias"]).to(dtype), 1, k // 2)
    return nhwc(out), None if c["res"] is None else nhwc(out) + c["res"].astype(out.numpy().dtype)


@pytest.mark.parametrize("k,cin,cout,H,W,form", CONV_CASES)
def test_conv_model_and_references_inside_the_backstop(k, cin, cout, H, W, form):
    c = C.conv_case(k, cin, cout, H, W, form); r, e, e_out, e_fin = C.conv_reference(k, cin, cout, H, W, form)
    o64, f64 = _torch_ref(c, torch.float64)
    assert close(r["out"], o64) and (f64 is None or close(r["fin"], f64))
    o32, f32 = _torch_ref(c, torch.float32)
    for nm, got, ref, gate in (("emu", e["out"], r["out"], M.conv_backstop(r)), ("torch float32", o32, r["out"], M.conv_backstop(r))) + \
            ((("emu fin", e["fin"], r["fin"], M.conv_backstop(r, True)), ("torch float32 fin", f32, r["fin"], M.conv_backstop(r, True))) if f64 is not None else ()):
        frac = (np.abs(got.astype(np.float64) - ref) / gate).max(); print("%s: %.4f of the backstop" % (nm, frac))
        assert frac <= 1, (nm, frac)
    assert np.isfinite(e_out).all() and (e_out > 0).all() and e_out.max() < 1e-5


def _about(ratio, r):
    """the offset of a case is one per channel for all frames, set from the statistics over all frames: a frame's own group is about r standard deviations out, not exactly"""
    return np.median(ratio) <= 0.25 if r == 0 else bool(abs(np.median(ratio) / r - 1) <= 0.25 and ratio.min() >= r / 4)


@pytest.mark.parametrize("r", C.RATIOS)
@pytest.mark.parametrize("cin,cout", C.CONV3_ALL_SIZES)
def test_conv3x3_offset_cases_inside_the_backstop(cin, cout, r):
    """the cases of test_conv3x3_forms: model against torch float64, emulation and torch float32 inside the backstop, and the groups of out and fin at mean / std = r"""
    c = C.conv3_offset_case(cin, cout, 24, 48, r); m, e, e_out, e_fin = C.conv3_offset_reference(cin, cout, 24, 48, r)
    o64, f64 = _torch_ref(c, torch.float64); o32, f32 = _torch_ref(c, torch.float32)
    assert close(m["out"], o64) and close(m["fin"], f64)
    for nm, got, ref, gate in (("emu", e["out"], m["out"], M.conv_backstop(m)), ("torch float32", o32, m["out"], M.conv_backstop(m)),
                               ("emu fin", e["fin"], m["fin"], M.conv_backstop(m, True)), ("torch float32 fin", f32, m["fin"], M.conv_backstop(m, True))):
        frac = (np.abs(got.astype(np.float64) - ref) / gate).max(); print("%s: %.4f of the backstop" % (nm, frac))
        assert frac <= 1, (nm, frac)
    assert np.isfinite(e_out).all() and np.isfinite(e_fin).all()
    for t in (m["out"], m["fin"]):
        s = M.groupnorm_stats(t, 32, C.EPS); ratio = np.abs(s["mean"]) * s["rstd"]
        assert _about(ratio, r), (r, ratio.min(), np.median(ratio), ratio.max())


@pytest.mark.parametrize("cin,cout,H,W", C.CONV1_CASES)
def test_conv1x1_offset_bias_puts_the_groups_at_the_ratio(cin, cout, H, W):
    ca = C.conv_case(1, cin, cout, H, W, "bias"); r0 = M.conv1x1(ca["x"], ca["w"]); raw = C.conv_reference(1, cin, cout, H, W, "bias")[1]["raw"]
    for r in C.RATIOS[1:]:
        b = C.conv1_offset_bias(ca, r0, r); out = r0["out"] + b.astype(np.float64); s = M.groupnorm_stats(out, 32, C.EPS)
        assert _about(np.abs(s["mean"]) * s["rstd"], r), r
        mr = dict(r0, out=out, S=r0["S"] + np.abs(b.astype(np.float64)))
        assert (np.abs((raw + b).astype(np.float64) - out) <= M.conv_backstop(mr)).all()


def test_largest_mean_over_std_of_the_encoders_own_groupnorm_inputs():
    """The host path of SIFNetEncoder (one chunk, eager) on tests/golden/encoder.npz with the synthetic weights: the largest |mean| rstd over EVERY GroupNorm input
    (174 of them: image and triplane encoder).  The middle ratio of encoder_cases.RATIOS is at least 4 x that value.  No trained checkpoint is in the repository: a floor."""
    import os
    from vistracker_amd import encoder as E, synthetic as syn
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder.npz"))
    sd = syn.encoder_weights([(str(n), tuple(int(x) for x in s[:d])) for n, s, d in zip(g["names"], g["shapes"], g["ndims"])])
    seen = []; plain = F.group_norm

    def recording(x, groups, w, b, eps):
        t = x.double().reshape(x.shape[0], groups, -1); seen.append(float((t.mean(-1).abs() / torch.sqrt(t.var(-1, unbiased=False) + eps)).max()))
        return plain(x, groups, w, b, eps)

    enc = E.SIFNetEncoder.from_state_dict(sd, device="cpu")
    E.F.group_norm = recording
    try:
        maps = enc._chunk_eager(torch.from_numpy(g["images"]))        # __call__ wraps the maps into ops.FeatureMaps, which takes device tensors only
    finally:
        E.F.group_norm = plain
    for k, t in maps.items():           # the host path reached the last layer of both encoders: these are the golden outputs
        assert np.abs(t.numpy() - g[k]).max() <= 2e-4 * max(1.0, np.abs(g[k]).max()), k
    print("GroupNorm inputs: %d, largest |mean| rstd %.3f" % (len(seen), max(seen)))
    assert len(seen) == 174 and 4 * max(seen) <= C.RATIOS[1] < C.RATIOS[2]


def test_with_float64_statistics_the_prologue_is_group_norm():
    c = C.conv_case(3, 96, 64, 8, 48, "gn"); g = c["gn"]; m = M.groupnorm_stats(c["x"], 32, C.EPS)
    st = np.stack([m["mean"], m["rstd"]], -1)
    ref = F.relu(F.group_norm(nchw(c["x"]), 32, torch.from_numpy(g["gamma"]).double(), torch.from_numpy(g["beta"]).double(), C.EPS))
    assert close(M.groupnorm_apply(c["x"], st, g["gamma"], g["beta"], True), nhwc(ref))
    assert close(M.prologue(c["x"], dict(g, stats=st))[0], nhwc(ref))
    out = F.conv2d(ref, torch.from_numpy(c["w"]).double(), None, 1, 1)
    assert close(M.conv3x3(c["x"], c["w"], gn=dict(g, stats=st))["out"], nhwc(out))
    noaff = F.group_norm(nchw(c["x"]), 32, None, None, C.EPS)
    assert close(M.groupnorm_apply(c["x"], st, np.ones(96), np.zeros(96), False), nhwc(noaff))


@pytest.mark.parametrize("k,cin,H,W", C.LATTICE_CASES)
def test_lattice_cases_are_exact(k, cin, H, W):
    """the case's own assertions (partial sums below 2^24 scaled units, lo = 0) and: emu_conv is bit-equal to the model there"""
    c = C.lattice_case(k, cin, H, W)
    assert np.array_equal(M.emu_conv(c["x"], c["w"])["out"].astype(np.float64), c["ref"])
    assert len({c["w"][:, :, i, j].tobytes() for i in range(k) for j in range(k)}) == k * k and len({c["w"][o].tobytes() for o in range(c["cout"])}) == c["cout"]


@pytest.mark.parametrize("cout,cin,H,W", C.STEM_CASES)
def test_stem_model(cout, cin, H, W):
    c = C.stem_case(cout, cin, H, W, 3)
    for r, b in ((c["ref_bias"], c["bias"]), (c["ref_plain"], None)):
        for dt in (torch.float64, torch.float32):
            t = nhwc(F.conv2d(nchw(c["x"]).to(dt), torch.from_numpy(c["w"]).to(dt), None if b is None else torch.from_numpy(b).to(dt), 2, 3))
            assert close(r["out"], t) if dt == torch.float64 else (np.abs(t - r["out"]) <= M.stem_backstop(r)).all()


@pytest.mark.parametrize("h,w", C.SWEEP_OUT)
def test_avgpool_model(h, w):
    x = C.offset_data(C._rng(31, h, w, 96, 8), (3, 2 * h, 2 * w, 96), 32, 8); m = M.avgpool2x2(x)
    assert close(m["out"], nhwc(F.avg_pool2d(nchw(x), 2, stride=2))) and np.abs(m["f32"] - m["out"]).max() <= 3 * M.U * np.abs(x).max()


@pytest.mark.parametrize("h,w", C.UP_SOURCES)
def test_upsample_model(h, w):
    rng = C._rng(32, h, w, 4, 8); low = C.offset_data(rng, (3, h, w, 4), 4, 8); skip = rng.normal(size=(3, 2 * h, 2 * w, 4)).astype(np.float32)
    for sk in (skip, None):
        m = M.upsample2x_bicubic_add(low, sk); s64 = 0 if sk is None else sk.astype(np.float64)
        assert close(m["out"], nhwc(F.interpolate(nchw(low), scale_factor=2, mode="bicubic", align_corners=True)) + s64)
        f32 = nhwc(F.interpolate(nchw(low).float(), scale_factor=2, mode="bicubic", align_corners=True)) + (0 if sk is None else sk)
        assert (np.abs(f32 - m["out"]) <= M.upsample_gate(m)).all()
    assert np.abs(M.cubic_weights(np.linspace(0, 1, 17)).sum(-1) - 1).max() < 1e-15


@pytest.mark.parametrize("r", C.RATIOS)
@pytest.mark.parametrize("Cc,groups", C.GN_CASES)
def test_statistics_model_and_float32_chains_inside_the_gate(Cc, groups, r):
    HW, B = 257, 2; x = C.offset_data(C._rng(21, Cc, groups, HW, r), (B, HW, Cc), groups, r); m = M.groupnorm_stats(x, groups, C.EPS)
    t = torch.from_numpy(x.astype(np.float64)).permute(0, 2, 1).reshape(B, groups, -1)
    assert close(m["mean"], t.mean(-1).numpy()) and close(m["rstd"], (1 / torch.sqrt(t.var(-1, unbiased=False) + C.EPS)).numpy())
    y = F.group_norm(torch.from_numpy(x.astype(np.float64)).permute(0, 2, 1), groups, None, None, C.EPS).permute(0, 2, 1).numpy()
    assert close(M.groupnorm_apply(x, np.stack([m["mean"], m["rstd"]], -1), np.ones(Cc), np.zeros(Cc), False), y)
    # float32 sums in chains of n_p values per channel (strided over the pixels as a thread of gn_stats_kernel walks them), E[x^2] - mean^2 in float64 from there
    n_p = C.np_pass(HW, Cc); nslot = -(-HW // n_p); s = np.zeros((B, nslot, Cc), np.float32); q = np.zeros_like(s)
    for p in range(HW):
        s[:, p % nslot] += x[:, p]; q[:, p % nslot] += x[:, p] * x[:, p]
    n = HW * (Cc // groups); sm = s.astype(np.float64).sum(1).reshape(B, groups, -1).sum(-1) / n; sq = q.astype(np.float64).sum(1).reshape(B, groups, -1).sum(-1) / n
    mean = sm.astype(np.float32); rstd = (1 / np.sqrt(np.maximum(sq - sm * sm, 0) + C.EPS)).astype(np.float32)
    gm, gr = M.stats_gates(m, n_p, C.EPS)
    assert (np.abs(mean - m["mean"]) <= gm).all() and (np.abs(rstd - m["rstd"]) <= gr).all()


def test_rstd_bound_at_ratio_8_is_not_under_the_old_tolerance():
    """the condition of the issue on the gate at mean / std = 8: stated, with the ratio at which the bound crosses 1e-4"""
    rel = lambda r, n_p: (3 * r * r + 1) * (n_p + 2) * M.U / 2          # E[x^2] = (1 + r^2) var, 2 |mean| E|x| ~ 2 r^2 var; d rstd / rstd = d var / (2 var)
    assert rel(8, C.NP_CONV_OUT) < 1e-4 and rel(8, C.NP_CONV_FIN) < 1e-4 and rel(8, 128) > 1e-4 and rel(2.8, 128) < 1e-4 < rel(2.9, 128)
    assert rel(C.RATIOS[1], C.NP_CONV_FIN) > 1e-4          # at the raised middle ratio (10) the epilogues' bound is over it too: 1e-4 is asserted on centred data only


MUTANT_CASE = (3, 96, 64, 24, 16)


def _mutants():
    c = C.conv_case(*MUTANT_CASE); r, e, e_emu, _ = C.conv_reference(*MUTANT_CASE); out = e["out"]
    small = int(np.abs(c["w"]).reshape(c["cout"], -1).max(1).argmin()); big = int(np.abs(c["w"]).reshape(c["cout"], -1).max(1).argmax())
    m1 = out.copy(); m1[..., big] *= np.float32(1.001)
    m2 = out.copy(); m2[..., small] *= np.float32(1.05)
    m2b = out.copy(); m2b[..., small] *= np.float32(1.0002)
    # the top-left tap (0, 0) of image row 0 reads the zero padding: dropping it there changes nothing but the layer's weight scale (asserted), so the mutant drops the left tap (1, 0) of row 0
    w0 = c["w"].copy(); w0[:, :, 0, 0] = 0; assert np.abs(M.emu_conv(c["x"][:, :2], w0)["out"][:, 0] - out[:, 0]).max() <= 8 * M.U * np.abs(out).max()
    w3 = c["w"].copy(); w3[:, :, 1, 0] = 0; m3 = out.copy(); m3[:, 0] = M.emu_conv(c["x"][:, :2], w3)["out"][:, 0]       # row 0 reads rows -1 .. 1: rows 0, 1 suffice
    return c, r, e_emu, dict(channel_x_1001=(m1, False), smallest_channel_x_105=(m2, False), smallest_channel_x_10002=(m2b, True), left_tap_dropped_in_row_0=(m3, False))


@pytest.mark.parametrize("name", ["channel_x_1001", "smallest_channel_x_105", "smallest_channel_x_10002", "left_tap_dropped_in_row_0"])
def test_mutants_of_the_emulation_fail_the_per_channel_gate(name):
    c, r, e_emu, ms = _mutants(); got, old_passes = ms[name]
    worst = (M.per_channel_error(got, r["out"]) / (8 * e_emu)).max(); old = np.abs(got - r["out"]).max() / np.abs(r["out"]).max()
    print("%s: %.1f x the per-channel gate; whole-tensor metric %.2e (old gate 2e-6)" % (name, worst, old))
    assert worst >= 10
    assert (old < 2e-6) == old_passes, old


def test_swapped_taps_on_the_lattice_are_not_bit_equal():
    c = C.lattice_case(3, 96, 8, 16); got = M.emu_conv(c["x"], np.ascontiguousarray(c["w"].transpose(0, 1, 3, 2)))["out"]
    assert not np.array_equal(got.astype(np.float64), c["ref"])
    c2 = C.conv_case(*MUTANT_CASE); r, _, e_emu, _ = C.conv_reference(*MUTANT_CASE)
    sw = M.emu_conv(c2["x"], np.ascontiguousarray(c2["w"].transpose(0, 1, 3, 2)))["out"]
    assert (M.per_channel_error(sw, r["out"]) / (8 * e_emu)).max() >= 10 and np.abs(sw - r["out"]).max() / np.abs(r["out"]).max() > 2e-6      # the old metric sees this one too
