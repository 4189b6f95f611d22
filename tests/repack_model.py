"""A numpy model of the three packed weight forms of the encoder's forward kernels and of the weight-scale rule, written from the layout comments (csrc/conv.hip:
"fragment (step = chunk * 9 + tap, wave, nt, hi|lo, lane) halves t: W[cout = (wave nt_count + nt) 16 + (lane & 15)][cin = 32 chunk + 8 (lane >> 4) + t][tap]";
csrc/stem.hip: "[Cin][7][7][Cout]" + a bias row) as array reshapes and transposes -- not from the packing loops.  The roundings are numpy's ``astype(np.float16)``
(round to nearest even, denormals kept).  ``unpack_split`` is a second, index-by-index statement of the same layout that the host tests hold against the first.

scale(w)                      (s_W, scale word 1 / (16 s_W)) as float32: s_W = 2^(14 - e) with max |w| = f 2^e, f in [0.5, 1); NaN entries do not take part in
                              the maximum; a zero or non-finite maximum gives s_W = 1
pack3x3(w) / pack1x1(w)       (uint16 halves of the packed weight -- the parts of a 256-output 1 x 1 one after the other --, scale word)
pack_stem(w, bias)            float32 [Cin][7][7][Cout] + the bias row (zeros without a bias)
``mutant`` exists for tests/test_host_repack.py only.
"""
import numpy as np

ACT_SCALE = np.float32(16.0)


def scale(w):
    a = np.abs(np.asarray(w, np.float32)).ravel()
    m = np.float32(np.fmax.reduce(a, initial=np.float32(0)))            # fmax drops a NaN operand
    sw = np.float32(1)
    if m > 0 and np.isfinite(m):
        _, e = np.frexp(m)
        with np.errstate(over="ignore"):
            sw = np.float32(np.ldexp(np.float32(1), 14 - int(e)))
    with np.errstate(divide="ignore", over="ignore"):
        return sw, np.float32(1) / (ACT_SCALE * sw)


def split(x):
    """hi = f16(x), lo = f16(x - f32(hi))"""
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def _fragments(x, nt, ntap, mutant=None):
    """x (rows = 64 nt, Cin, ntap) float32, already scaled and zero-padded -> uint16 halves in fragment order [chunk][tap][wave][nt][hi|lo][lane][8]"""
    rows, cin, _ = x.shape
    assert rows == 64 * nt and cin % 32 == 0
    hi, lo = split(x)
    out = []
    for plane in ((lo, hi) if mutant == "hilo" else (hi, lo)):
        # rows = (wave, nt, lane & 15); cin = (chunk, lane >> 4, t)
        if mutant == "quad_k":
            f = plane.reshape(4, nt, 16, cin // 32, 8, 4, ntap).transpose(0, 1, 2, 3, 5, 4, 6)
        else:
            f = plane.reshape(4, nt, 16, cin // 32, 4, 8, ntap)
        # -> [chunk][tap][wave][nt][lane >> 4][lane & 15][t]
        out.append(f.transpose((6, 3, 0, 1, 4, 2, 5) if mutant == "tap_major" else (3, 6, 0, 1, 4, 2, 5)))
    return np.ascontiguousarray(np.stack(out, axis=4)).view(np.uint16).ravel()


def pack3x3(w, mutant=None):
    w = np.asarray(w, np.float32)
    cout, cin = w.shape[:2]
    assert cout in (32, 64, 128) and cin % 32 == 0 and w.shape[2:] == (3, 3)
    nt = 2 if cout == 128 else 1
    sw, word = scale(w)
    x = np.zeros((64 * nt, cin, 9), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        x[:cout] = w.reshape(cout, cin, 9) * sw            # tap = 3 ky + kx; rows beyond Cout = 32 stay zero
    return _fragments(x, nt, 9, mutant), word


def pack1x1(w, mutant=None):
    w = np.asarray(w, np.float32)
    cout, cin = w.shape[:2]
    assert cout in (64, 128, 256) and cin in (32, 64, 128, 256)
    parts = 2 if cout == 256 else 1
    pcout = cout // parts
    nt = 2 if pcout == 128 else 1
    sw, word = scale(w)
    with np.errstate(over="ignore", invalid="ignore"):
        x = (w.reshape(cout, cin, 1) * sw).astype(np.float32)
    return np.concatenate([_fragments(x[p * pcout:(p + 1) * pcout], nt, 1, mutant) for p in range(parts)]), word


def pack_stem(w, bias=None):
    w = np.asarray(w, np.float32)
    cout = w.shape[0]
    assert w.shape[2:] == (7, 7)
    b = np.zeros(cout, np.float32) if bias is None else np.asarray(bias, np.float32)
    return np.concatenate([np.ascontiguousarray(w.transpose(1, 2, 3, 0)).ravel(), b])


def unpack_split(halves, cout, cin, ksize):
    """the weights (cout, cin, k, k) as float64 hi + lo (still scaled by s_W) read back element by element at the documented position:
    uint4 index ((((chunk ntap + tap) 4 + wave) nt + n) 2 + hi|lo) 64 + lane, half t"""
    ntap = ksize * ksize
    parts = 2 if (ksize == 1 and cout == 256) else 1
    pcout = cout // parts
    nt = 2 if pcout == 128 else 1
    n16 = (cin // 32) * ntap * 4 * nt * 2 * 64
    h = np.asarray(halves, np.uint16).view(np.float16).astype(np.float64).reshape(parts, n16, 8)
    co, ci, tap = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(ntap), indexing="ij")
    part, r = co // pcout, co % pcout
    wave, n, lane = r // (16 * nt), (r // 16) % nt, (r % 16) + 16 * ((ci % 32) // 8)
    base = ((((ci // 32) * ntap + tap) * 4 + wave) * nt + n) * 2 * 64
    return (h[part, base + lane, ci % 8] + h[part, base + 64 + lane, ci % 8]).reshape(cout, cin, ksize, ksize)


# ---- the weight sets of the tests -------------------------------------------------------------------------------------------------------------------------------
WEIGHT_SETS = ("gauss", "zero", "pow2", "below_pow2", "subnormal", "inf", "nan")


def weights(kind, shape, seed):
    """float32 weights of ``shape`` = (cout, cin, k, k): Gaussian x 0.05, with the named feature planted.  Plain Gaussian weights almost never have an f16-denormal
    low half (the residual of x ~ 2^11 is a multiple of 2^-12), so every third weight is replaced by (H + d) / s_W with H an f16 value in [2^-4, 1) and d a non-zero
    multiple of 2^-24 below 2^-16: its high half is H, its low half exactly the denormal d (s_W of the set is unchanged: these weights are tiny)."""
    r = np.random.RandomState(seed)
    w = (0.05 * r.randn(*shape)).astype(np.float32)
    f = w.reshape(-1)
    n3 = f[1::3].size
    H = (r.uniform(2.0 ** -4, 1.0, n3) * np.where(r.rand(n3) < 0.5, -1, 1)).astype(np.float16).astype(np.float32)
    d = (r.randint(1, 256, n3) * np.where(r.rand(n3) < 0.5, -1, 1)).astype(np.float32) * np.float32(2.0 ** -24)
    f[1::3] = 0
    f[1::3] = (H + d) / scale(w)[0]
    i = 3 * int(r.randint(f.size // 3))             # a position that is not a planted one
    if kind == "zero":
        f[:] = 0
    elif kind == "pow2":                # the maximum exactly 2^-2: frexp's exponent is one higher than just below it
        f[i] = -0.25
    elif kind == "below_pow2":
        f[i] = np.nextafter(np.float32(0.25), np.float32(0))
    elif kind == "subnormal":
        f[::7] = (r.randint(1, 1 << 23, f[::7].size).astype(np.uint32)).view(np.float32) * np.where(r.rand(f[::7].size) < 0.5, -1, 1).astype(np.float32)
    elif kind == "inf":
        f[i] = -np.inf
    elif kind == "nan":
        f[i] = np.nan
        f[(i + 11) % f.size] = np.nan
    else:
        assert kind == "gauss"
    return w
