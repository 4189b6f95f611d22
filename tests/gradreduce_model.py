"""The float64 model of ``vt_grad_rank_mean`` (include/vistracker.h) and the cases its tests run.

Definition: parts holds W rows; out[i] = (float32)((((float64)parts[0][i] + parts[1][i]) + ... + parts[W-1][i]) / (float64)W): the rows added in rank order, left to
right, in float64; one float64 division; one rounding to float32.

``mean`` is the model (an explicit loop over ranks in numpy float64).  ``mean_python`` restates it element by element on Python floats (IEEE binary64 as well, none
of numpy's array arithmetic).  The three mutants are what the case set must tell from the model: a float32 accumulator, the reversed rank order, a multiplication
by float32(1 / W) in place of the float64 division."""
import numpy as np

NS = (0, 1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4 * 256 * 3 + 2)
WS = (1, 2, 3, 5, 8)
PADS = (0, 7)                  # stride = n + pad
OFFSETS = (0, 1, 2, 3)         # floats into a 16-byte aligned allocation, for parts and out independently


def mean(parts):
    """parts (W, n) float32 -> (n,) float32"""
    parts = np.asarray(parts, np.float32)
    with np.errstate(all="ignore"):
        s = parts[0].astype(np.float64)
        for r in range(1, parts.shape[0]):
            s = s + parts[r].astype(np.float64)
        return (s / np.float64(parts.shape[0])).astype(np.float32)


def mean_python(parts):
    """the same definition, one element at a time on Python floats"""
    import struct
    parts = np.asarray(parts, np.float32)
    W, n = parts.shape
    rows = [[float(v) for v in parts[r]] for r in range(W)]
    out = np.empty(n, np.float32)
    for i in range(n):
        s = rows[0][i]
        for r in range(1, W):
            s = s + rows[r][i]
        q = s / float(W)
        try:
            out[i] = struct.unpack("f", struct.pack("f", q))[0]            # round to nearest even, as the conversion instruction
        except OverflowError:                                              # beyond float32's range: the conversion gives an infinity
            out[i] = np.float32(np.inf) if q > 0 else np.float32(-np.inf)
    return out


def mutant_fp32_accumulator(parts):
    parts = np.asarray(parts, np.float32)
    with np.errstate(all="ignore"):
        s = parts[0].copy()
        for r in range(1, parts.shape[0]):
            s = (s + parts[r]).astype(np.float32)
        return (s.astype(np.float64) / np.float64(parts.shape[0])).astype(np.float32)


def mutant_reversed_order(parts):
    return mean(np.asarray(parts, np.float32)[::-1])


def mutant_reciprocal(parts):
    parts = np.asarray(parts, np.float32)
    with np.errstate(all="ignore"):
        s = parts[0].astype(np.float64)
        for r in range(1, parts.shape[0]):
            s = s + parts[r].astype(np.float64)
        return (s * np.float64(np.float32(1.0) / np.float32(parts.shape[0]))).astype(np.float32)


MUTANTS = {"fp32 accumulator": mutant_fp32_accumulator, "reversed rank order": mutant_reversed_order, "multiplication by float32(1/W)": mutant_reciprocal}


def _special(k, W):
    """column k of the hand-made values: one value per rank"""
    c = np.zeros(W, np.float32)
    if k == 0:          # the float64 sum depends on the order (W >= 3); float32 overflows where float64 does not (W = 2)
        c[:] = [2.0 ** 60, -2.0 ** 60, 1.0][:W] + [0.0] * max(0, W - 3) if W >= 3 else [3.0e38] * W
    elif k == 1:        # cancels to +0
        c[0] = 1.2345678
        if W > 1:
            c[1] = -c[0]
        else:
            c[0] = 0.0
    elif k == 2:        # every rank -0 -> -0
        c[:] = -0.0
    elif k == 3:        # the float32 left-to-right sum loses the 1 (W >= 3) or overflows (W = 2)
        c[:] = [1.0e8, 1.0, -1.0e8][:W] + [0.0] * max(0, W - 3) if W >= 3 else [3.0e38, 2.5e38][:W]
    elif k == 4:        # a NaN from the last rank
        c[:] = 1.0
        c[W - 1] = np.nan
    elif k == 5:        # an infinity from the first rank
        c[:] = -2.0
        c[0] = np.inf
    elif k == 6:        # inf - inf -> NaN (W >= 2)
        c[0] = np.inf
        c[W - 1] = -np.inf if W > 1 else np.inf
    elif k == 7:        # the smallest denormal from every rank
        c[:] = np.float32(1e-45)
    elif k == 8:        # cancels to +0 from the far end
        c[W - 1] = 7.0
        c[0] = -7.0 if W > 1 else 0.0
    return c


N_SPECIAL, PERIOD = 9, 13


def values(W, n, seed=0):
    """(W, n) float32: magnitudes spanning 30 binades inside every row, both signs; columns j with j % 13 < 9 carry the hand-made values"""
    rng = np.random.default_rng([seed, W, n])
    v = (rng.uniform(1.0, 2.0, (W, n)) * 2.0 ** rng.uniform(-15.0, 15.0, (W, n)) * rng.choice([-1.0, 1.0], (W, n))).astype(np.float32)
    free = [j for j in range(n) if j % PERIOD >= N_SPECIAL]
    if len(free) >= 2:                                                     # the span is reached in every row that has room for it
        v[:, free[0]] = np.sign(v[:, free[0]]) * np.float32(1.5 * 2.0 ** -15)
        v[:, free[-1]] = np.sign(v[:, free[-1]]) * np.float32(1.5 * 2.0 ** 15)
    for j in range(n):
        if j % PERIOD < N_SPECIAL:
            v[:, j] = _special(j % PERIOD, W)
    return v


def cases():
    """(W, n, pad) of every case; the offsets are the GPU test's"""
    return [(W, n, pad) for W in WS for n in NS for pad in PADS]


def same_bits(got, want):
    """float32 arrays equal as bits, NaN payloads excluded: where the model has a NaN any NaN will do"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.isnan(got[nan]).all()) and np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32))
