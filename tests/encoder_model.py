"""Float64 model of the HGFilter encoder's forward operations (csrc/conv.hip, stem.hip, encoder_ops.hip), written from the definitions in numpy.  It imports nothing
from vistracker_amd or oracle/.  Tensors are NHWC; every operation returns its value and what the gates of tests/test_gpu_encoder_kernels.py need.

u = 2^-24 is the unit round-off of float32.  The gates (derivations in the docstring of tests/test_gpu_encoder_kernels.py) are functions at the end of this file."""
import numpy as np

U = 2.0 ** -24
ACT_SCALE = 16.0                      # the kernels' activation scale (2^4)
SPLIT = 3 * 2.0 ** -22                # two operands carried to 22 bits + the dropped lo x lo product


# ---- GroupNorm -------------------------------------------------------------------------------------------------------------------------------------------------
def groupnorm_stats(x, groups, eps=1e-5):
    """x (B, H, W, C) or (B, HW, C).  Per (frame, group), two-pass in float64: mean, rstd = 1 / sqrt(var + eps) (biased variance), E|x|, E[x^2], var."""
    x = np.asarray(x, np.float64); B, C = x.shape[0], x.shape[-1]
    g = x.reshape(B, -1, groups, C // groups)
    mean = g.mean((1, 3)); var = ((g - mean[:, None, :, None]) ** 2).mean((1, 3))
    return dict(mean=mean, rstd=1.0 / np.sqrt(var + eps), var=var, eabs=np.abs(g).mean((1, 3)), esq=(g * g).mean((1, 3)))


def _per_channel(v, C):
    """(B, groups) -> (B, 1, .., C): a group's value for each of its channels"""
    return np.repeat(np.asarray(v, np.float64), C // v.shape[1], axis=1)


def groupnorm_apply(x, stats, gamma, beta, relu):
    """stats (B, groups, 2) {mean, rstd}; the values are used as given (float32 pairs from a kernel or float64 ones from groupnorm_stats)"""
    x = np.asarray(x, np.float64); C = x.shape[-1]; sh = (x.shape[0],) + (1,) * (x.ndim - 2) + (C,)
    st = np.asarray(stats, np.float64)
    y = (x - _per_channel(st[..., 0], C).reshape(sh)) * _per_channel(st[..., 1], C).reshape(sh) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    return np.maximum(y, 0.0) if relu else y


def prologue(x, gn):
    """The GroupNorm + ReLU in front of a convolution, gn = dict(stats (B, groups, 2) float32, gamma, beta float32).  -> act (float64), dact: the bound on what the
    kernel's float32 statement of it can be off by.  The kernel forms a = rstd gamma, s = beta - mean a, v = fma(x, a, s) (the factor 16 is exact): four roundings,
    |dv| <= u (|x a| + |mean a|) [a] + u |mean a| [the product] + u |s| [the difference] + u |v| [the fma]; max(., 0) does not enlarge it."""
    x = np.asarray(x, np.float64)
    if gn is None:
        return x, None
    C = x.shape[-1]; st = np.asarray(gn["stats"], np.float64); sh = (x.shape[0], 1, 1, C)
    a = _per_channel(st[..., 1], C).reshape(sh) * np.asarray(gn["gamma"], np.float64); ma = _per_channel(st[..., 0], C).reshape(sh) * a
    s = np.asarray(gn["beta"], np.float64) - ma; v = x * a + s
    return np.maximum(v, 0.0), U * (np.abs(x * a) + 2 * np.abs(ma) + np.abs(s) + np.abs(v))


# ---- convolutions ------------------------------------------------------------------------------------------------------------------------------------------------
def _corr(act, w, stride, pad):
    """plain cross-correlation, act (B, H, W, Cin) float64, w (Cout, Cin, kh, kw) float64 -> (B, H2, W2, Cout); zero padding of `act`"""
    B, H, W, Cin = act.shape; Cout, _, kh, kw = w.shape
    H2, W2 = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    p = np.zeros((B, H + 2 * pad, W + 2 * pad, Cin)); p[:, pad:pad + H, pad:pad + W] = act
    out = np.zeros((B, H2, W2, Cout))
    for ky in range(kh):
        for kx in range(kw):
            out += p[:, ky:ky + stride * (H2 - 1) + 1:stride, kx:kx + stride * (W2 - 1) + 1:stride] @ w[:, :, ky, kx].T
    return out


def _conv(x, w, bias, gn, res, pad):
    w = np.asarray(w, np.float64); act, dact = prologue(x, gn)
    out = _corr(act, w, 1, pad); S = _corr(np.abs(act), np.abs(w), 1, pad)
    r = dict(act=act, K=w.shape[1] * w.shape[2] * w.shape[3], dpro=None if dact is None else _corr(dact, np.abs(w), 1, pad))
    if bias is not None:
        out = out + np.asarray(bias, np.float64); S = S + np.abs(np.asarray(bias, np.float64))
    r["out"], r["S"] = out, S
    r["fin"] = None if res is None else out + np.asarray(res, np.float64)
    return r


def conv3x3(x, w, bias=None, gn=None, res=None):
    """stride 1, zero pad 1 (the padding pads the rectified activation), w (Cout, Cin, 3, 3).  -> out, fin (= out + res or None), S = sum |w| |act| (+ |bias|) per
    output element, K = 9 Cin, dpro = sum |w| dact (the prologue's rounding propagated; None without one), act"""
    return _conv(x, np.asarray(w).reshape(w.shape[0], w.shape[1], 3, 3), bias, gn, res, 1)


def conv1x1(x, w, bias=None, gn=None, res=None):
    return _conv(x, np.asarray(w).reshape(w.shape[0], w.shape[1], 1, 1), bias, gn, res, 0)


def stem7x7(x, w, bias=None):
    """stride 2, pad 3, output ((H - 1) // 2 + 1, (W - 1) // 2 + 1)"""
    x = np.asarray(x, np.float64); w = np.asarray(w, np.float64).reshape(w.shape[0], w.shape[1], 7, 7)
    out = _corr(x, w, 2, 3); S = _corr(np.abs(x), np.abs(w), 2, 3)
    assert out.shape[1:3] == ((x.shape[1] - 1) // 2 + 1, (x.shape[2] - 1) // 2 + 1)
    if bias is not None:
        out = out + np.asarray(bias, np.float64); S = S + np.abs(np.asarray(bias, np.float64))
    return dict(out=out, S=S, K=49 * w.shape[1])


# ---- the number format of the split-f16 kernels ------------------------------------------------------------------------------------------------------------------
def weight_scale(w):
    """the layer's power of two that puts max |w| into [2^13, 2^14) (1 for an all-zero layer)"""
    m = float(np.abs(np.asarray(w, np.float32)).max())
    return 1.0 if m == 0.0 else float(np.ldexp(1.0, 14 - int(np.frexp(np.float32(m))[1])))


def split_f16(v):
    """float32 array -> hi = float16(v), lo = float16(v - hi), both returned as float32"""
    v = np.asarray(v, np.float32); hi = v.astype(np.float16).astype(np.float32)
    return hi, (v - hi).astype(np.float16).astype(np.float32)


def emu_conv(x, w, bias=None, gn=None, res=None):
    """An emulation of the kernels' NUMBER FORMAT, not of their code: activations x 16 and weights x weight_scale(w), each split into float16 hi + lo, a product
    hi hi + hi lo + lo hi in float32, the products accumulated in float32 in plain (tap, cin) index order, the epilogue fma(acc, 1 / (16 s_W), bias) in float32 and
    the residual added in float32.  The prologue is float32 in the order of its definition ((x - mean) rstd gamma + beta).  w (Cout, Cin, k, k), k = 1 or 3.
    -> out, fin (float32)"""
    import torch
    w = np.asarray(w, np.float32); Cout, Cin, k = w.shape[0], w.shape[1], w.shape[2]; pad = k // 2
    x = np.asarray(x, np.float32); B, H, W, _ = x.shape
    if gn is not None:
        st = np.asarray(gn["stats"], np.float32); sh = (B, 1, 1, Cin)
        mean = np.repeat(st[..., 0], Cin // st.shape[1], 1).reshape(sh); rstd = np.repeat(st[..., 1], Cin // st.shape[1], 1).reshape(sh)
        x = np.maximum((x - mean) * rstd * np.asarray(gn["gamma"], np.float32) + np.asarray(gn["beta"], np.float32), np.float32(0))
    sw = weight_scale(w)
    p = np.zeros((B, H + 2 * pad, W + 2 * pad, Cin), np.float32); p[:, pad:pad + H, pad:pad + W] = x * np.float32(ACT_SCALE)
    ah, al = (torch.from_numpy(a) for a in split_f16(p)); wh, wl = (torch.from_numpy(a) for a in split_f16(w * np.float32(sw)))
    acc = torch.zeros(B * H * W, Cout); t0 = torch.empty_like(acc); t1 = torch.empty_like(acc)
    for ky in range(k):
        for kx in range(k):
            xh = ah[:, ky:ky + H, kx:kx + W].reshape(-1, Cin); xl = al[:, ky:ky + H, kx:kx + W].reshape(-1, Cin)
            for ci in range(Cin):
                a_h, a_l = xh[:, ci:ci + 1], xl[:, ci:ci + 1]; w_h, w_l = wh[:, ci, ky, kx][None], wl[:, ci, ky, kx][None]
                torch.mul(a_h, w_h, out=t0); torch.mul(a_h, w_l, out=t1); t0 += t1; torch.mul(a_l, w_h, out=t1); t0 += t1
                acc += t0
    inv = np.float32(1.0 / (ACT_SCALE * sw))                                    # a power of two: acc * inv is exact, the fma rounds once
    raw = (acc.numpy() * inv).reshape(B, H, W, Cout); out = raw
    if bias is not None:
        out = raw + np.asarray(bias, np.float32)
    return dict(out=out, raw=raw, fin=None if res is None else out + np.asarray(res, np.float32))


# ---- pooling and up-sampling -------------------------------------------------------------------------------------------------------------------------------------------
def avgpool2x2(x):
    """-> out (float64 mean of the window), f32: the float32 statement ((v00 + v01) + v10 + v11) * 0.25f in the kernel's order (numpy float32: bit for bit)"""
    x32 = np.asarray(x, np.float32); x64 = x32.astype(np.float64)
    q = lambda a, i, j: a[:, i::2, j::2]
    return dict(out=(q(x64, 0, 0) + q(x64, 0, 1) + q(x64, 1, 0) + q(x64, 1, 1)) * 0.25,
                f32=(((q(x32, 0, 0) + q(x32, 0, 1)) + q(x32, 1, 0)) + q(x32, 1, 1)) * np.float32(0.25))


def _cubic(t, et=None, A=-0.75):
    """Keys' cubic-convolution weights of taps -1 .. 2 at fraction t, their derivatives in t and -- with et, the absolute error of a float32 t -- a running bound on
    the error of their float32 Horner evaluation (every operation adds u |result| to the propagated error of its operands; the constants are exact in float32)"""
    t = np.asarray(t, np.float64); et = np.zeros_like(t) if et is None else et

    def horner(d, ed, c):                      # ((c0 d + c1) d + c2) d + c3, and the running error bound
        p, e = c[0] * d, abs(c[0]) * ed
        e = e + U * np.abs(p)
        for ck, last in ((c[1], False), (c[2], False), (c[3], True)):
            p = p + ck; e = e + U * np.abs(p)
            if not last:
                q = p * d; e = e * np.abs(d) + np.abs(p) * ed + U * np.abs(q); p = q
        return p, e

    inner = (A + 2, -(A + 3), 0.0, 1.0); outer = (A, -5 * A, 8 * A, -4 * A)
    dinner = lambda d: 3 * (A + 2) * d * d - 2 * (A + 3) * d
    douter = lambda d: 3 * A * d * d - 10 * A * d + 8 * A
    ds = [t + 1, t, 1 - t, 2 - t]; cs = [outer, inner, inner, outer]
    we = [horner(d, et + (U * np.abs(d) if k != 1 else 0), c) for k, (d, c) in enumerate(zip(ds, cs))]
    dw = [douter(ds[0]), dinner(ds[1]), -dinner(ds[2]), -douter(ds[3])]
    return np.stack([x[0] for x in we], -1), np.stack(dw, -1), np.stack([x[1] for x in we], -1)


def cubic_weights(t):
    return _cubic(t)[0]


def upsample2x_bicubic_add(low, skip=None):
    """out = skip + bicubic x2 up-sampling of low (B, h, w, C): align_corners = True (source coordinate dst (h - 1) / (2 h - 1)), A = -0.75, taps clamped to the
    border.  -> out, S = sum |w_y w_x v| per element, skip_abs, and for the gate: Sw = sum (e_y |w_x| + |w_y| e_x) |v| with e the bound on a float32 weight's
    evaluation error at the exact fraction, Sc = 2 u (f_y sum |w_y' w_x v| + f_x sum |w_y w_x' v|): a float32 source coordinate is off by 2 u f (its scale and
    one product are rounded; the fraction's subtraction is exact) and the interpolant is continuously differentiable in it, across tap changes too"""
    low = np.asarray(low, np.float64); B, h, w, C = low.shape; H, W = 2 * h, 2 * w

    def axis(n, N):
        f = np.arange(N) * ((n - 1) / (N - 1)) if N > 1 else np.zeros(N)
        i = np.floor(f).astype(int); wt, dw, ew = _cubic(f - i, np.zeros(N))
        return np.clip(i[:, None] + np.arange(-1, 3)[None], 0, n - 1), wt, dw, ew, f

    iy, wy, dwy, ewy, fy = axis(h, H); ix, wx, dwx, ewx, fx = axis(w, W)
    out, S, Sw, Sc = (np.zeros((B, H, W, C)) for _ in range(4))
    o2 = lambda a, b: (a[:, None] * b[None])[None, :, :, None]
    for i in range(4):
        for k in range(4):
            v = low[:, iy[:, i]][:, :, ix[:, k]]; av = np.abs(v)
            out += o2(wy[:, i], wx[:, k]) * v; S += np.abs(o2(wy[:, i], wx[:, k])) * av
            Sw += (o2(ewy[:, i], np.abs(wx[:, k])) + o2(np.abs(wy[:, i]), ewx[:, k])) * av
            Sc += 2 * U * (o2(fy * np.abs(dwy[:, i]), np.abs(wx[:, k])) + o2(np.abs(wy[:, i]), fx * np.abs(dwx[:, k]))) * av
    sk = np.zeros_like(out) if skip is None else np.asarray(skip, np.float64)
    return dict(out=out + sk, S=S, Sw=Sw, Sc=Sc, skip_abs=np.abs(sk))


# ---- gates -------------------------------------------------------------------------------------------------------------------------------------------------------------
def per_channel_error(got, ref):
    """err_c = max over (b, y, x) |got - ref| / max |ref[..., c]|; a channel without a scale (ref identically 0) must be exactly 0: its error is 0 or inf"""
    got = np.asarray(got, np.float64); C = ref.shape[-1]
    e = np.abs(got - ref).reshape(-1, C).max(0); s = np.abs(ref).reshape(-1, C).max(0)
    return np.where(s > 0, e / np.where(s > 0, s, 1), np.where(e > 0, np.inf, 0.0))


def conv_backstop(r, fin=False):
    """per output element: (3 2^-22 + 3 K u) S -- the operands' 22 bits and the worst case of a sequential float32 sum of the 3 K partial products (which also
    covers the epilogue's one rounding) --, + the prologue's roundings through sum |w|, + u |fin| for the float32 residual add"""
    g = (SPLIT + 3 * r["K"] * U) * r["S"]
    if r["dpro"] is not None:
        g = g + r["dpro"]
    return g + U * np.abs(r["fin"]) if fin else g


def stem_backstop(r):
    return (r["K"] + 2) * U * r["S"]


UPSAMPLE_N = 8
"""float32 roundings on the path of one term w_y w_x v of an up-sampled element in the separable form: the product w_x v (1), the three additions of a four-term row
sum (3; the first addition to 0 and the five-tap form's products with a zero weight are exact), the product w_y row (1), the three additions of the column sum (3).
The issue's form n u sum |w_y w_x v| + u |skip| assumes weights that are exact up to a RELATIVE error; they are not: a weight near 0 (fraction near 0 or 1) carries
the ABSOLUTE error of its Horner evaluation and of the float32 source coordinate.  Both are bounded from the format in upsample2x_bicubic_add (Sw, Sc) and added; the
skip connection's addition rounds the result once more: u |out| <= u (S + |skip|)."""


def upsample_gate(r):
    return (UPSAMPLE_N + 1) * U * r["S"] + r["Sw"] + r["Sc"] + U * r["skip_abs"]


def stats_gates(m, n_p, eps=1e-5):
    """m = groupnorm_stats(...), n_p the longest float32 partial chain of the producer.  mean within n_p u E|x|; var within dv = (n_p + 2) u (E[x^2] + 2 |mean| E|x|),
    so rstd = (var + eps)^-1/2 within rstd ((1 - dv / (var + eps))^-1/2 - 1) (the one-sided worst case; unbounded once dv reaches var + eps) + u rstd for its
    own rounding to float32.  The mean's rounding to float32 adds u |mean|.  -> gate_mean, gate_rstd, both (B, groups)"""
    dv = (n_p + 2) * U * (m["esq"] + 2 * np.abs(m["mean"]) * m["eabs"]); rel = dv / (m["var"] + eps)
    g_r = np.where(rel < 1, m["rstd"] * (1.0 / np.sqrt(np.where(rel < 1, 1 - rel, 1.0)) - 1.0), np.inf) + U * m["rstd"]
    return n_p * U * m["eabs"] + U * np.abs(m["mean"]), g_r
