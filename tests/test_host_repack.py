"""CPU: the numpy model of the packed weight forms (tests/repack_model.py) against itself: the transposed statement of the layout against the index-by-index one,
the scale rule at its edges, and mutants of the layout that must not go unnoticed.  The GPU tests hold the device packing against this model byte for byte."""
import numpy as np
import pytest

import repack_model as RM

SPLIT_SHAPES = [(32, 32, 3), (64, 32, 3), (128, 32, 3), (64, 64, 3), (128, 96, 3), (64, 32, 1), (128, 64, 1), (256, 32, 1), (256, 256, 1)]


def pack(w):
    return (RM.pack3x3 if w.shape[2] == 3 else RM.pack1x1)(w)


@pytest.mark.parametrize("cout,cin,k", SPLIT_SHAPES)
def test_unpacking_returns_the_weights(cout, cin, k):
    """(hi + lo) / s_W at the documented position of every (cout, cin, tap) is the weight to 2^-21 max |w|: hi leaves at most half an f16 ulp of 2^13 <= |x| < 2^14
    (4), lo keeps that to 2^-11 relative (2^-9 absolute, 2^-22 of 2^13) or, as a denormal, to 2^-25 absolute."""
    w = RM.weights("gauss", (cout, cin, k, k), 7 * cout + cin + k)
    halves, word = pack(w)
    sw, word2 = RM.scale(w)
    assert word == word2 and halves.size == (2 if cout == 256 and k == 1 else 1) * (cin // 32) * k * k * 4 * (2 if min(cout, 128) == 128 else 1) * 2 * 64 * 8
    back = RM.unpack_split(halves, cout, cin, k) / float(sw)
    m = float(np.abs(w).max())
    err = float(np.abs(back - w.astype(np.float64)).max())
    print(f"\n[{cout}x{cin}x{k}x{k}] s_W = 2^{int(np.log2(sw))}, largest error {err:.3e} = {err / m:.3e} max|w| (bound {2.0 ** -21:.3e})", end="")
    assert err <= 2.0 ** -21 * m
    if cout == 32:          # the rows beyond Cout = 32 are zero
        assert not RM.unpack_split(halves, 64, cin, k)[32:].any()


def test_low_halves_are_often_denormal():
    """a third of the Gaussian set's low halves are f16 denormals (a device that flushed them would differ in a third of the low bytes)"""
    for kind in RM.WEIGHT_SETS[:1] + ("pow2", "below_pow2"):
        w = RM.weights(kind, (64, 64, 3, 3), 3)
        x = w * RM.scale(w)[0]
        _, lo = RM.split(x)
        den = (np.abs(lo.astype(np.float32)) < 2.0 ** -14) & (lo != 0)
        print(f"\n{kind}: denormal low halves {den.mean():.3f}", end="")
        assert 0.33 < den.mean() < 0.35


def test_scale_rule():
    f = np.float32
    one = (f(1), f(1) / f(16))
    assert RM.scale(np.zeros((64, 32, 3, 3), f)) == one
    for k in (-20, -2, 0, 5):
        p = f(2.0 ** k)
        w = np.full(8, 0.3 * p, f); w[3] = -p                                     # exactly 2^k: f = 0.5, e = k + 1, the maximum lands on 2^13
        sw, word = RM.scale(w)
        assert sw == f(2.0 ** (13 - k)) and p * sw == 2.0 ** 13 and word == f(2.0 ** (k - 17))
        w[3] = np.nextafter(p, f(0))                                                # one ulp below: e = k, just under 2^14
        sw, word = RM.scale(w)
        assert sw == f(2.0 ** (14 - k)) and 2.0 ** 14 > w[3] * sw > 2.0 ** 14 - 1 and word == f(2.0 ** (k - 18))
    w = np.array([0.1, -np.inf, 0.2], f)
    assert RM.scale(w) == one                                                       # a non-finite maximum
    w = np.array([0.1, np.nan, -0.2, np.nan], f)
    assert RM.scale(w) == RM.scale(np.array([0.1, -0.2], f)) == (f(2.0 ** 16), f(2.0 ** -20))     # NaN beside finite values: dropped
    assert RM.scale(np.array([np.nan, np.nan], f)) == one


def test_weight_sets_plant_what_they_name():
    shape = (64, 32, 3, 3)
    g = RM.weights("gauss", shape, 1)
    assert not RM.weights("zero", shape, 1).any()
    assert np.abs(RM.weights("pow2", shape, 1)).max() == 0.25 and np.abs(RM.weights("below_pow2", shape, 1)).max() == np.nextafter(np.float32(0.25), np.float32(0))
    assert RM.scale(RM.weights("pow2", shape, 1))[0] == 2.0 ** 15 and RM.scale(RM.weights("below_pow2", shape, 1))[0] == 2.0 ** 16
    s = RM.weights("subnormal", shape, 1)
    assert ((s != 0) & (np.abs(s) < np.finfo(np.float32).tiny)).sum() >= s.size // 8 and RM.scale(s)[0] == RM.scale(g)[0]
    assert np.isinf(RM.weights("inf", shape, 1)).sum() == 1 and np.isnan(RM.weights("nan", shape, 1)).sum() == 2


@pytest.mark.parametrize("mutant", ["quad_k", "hilo", "tap_major"])
def test_mutants_of_the_layout_change_the_bytes(mutant):
    """lane quad and k swapped, the hi and lo planes swapped, tap-major instead of chunk-major order: each moves bytes, so the byte comparison on the GPU sees it"""
    w = RM.weights("gauss", (64, 64, 3, 3), 5)
    good, _ = RM.pack3x3(w)
    bad, _ = RM.pack3x3(w, mutant=mutant)
    assert good.shape == bad.shape and (good != bad).mean() > 0.5
    if mutant != "tap_major":           # one tap: nothing to reorder
        w1 = RM.weights("gauss", (128, 64, 1, 1), 6)
        assert (RM.pack1x1(w1)[0] != RM.pack1x1(w1, mutant=mutant)[0]).mean() > 0.5
    if mutant != "hilo":                # hi + lo does not care which plane is which; the bytes above do
        back = RM.unpack_split(bad, 64, 64, 3) / float(RM.scale(w)[0])
        assert np.abs(back - w).max() > 2.0 ** -21 * np.abs(w).max()


def test_stem_form():
    r = np.random.RandomState(2)
    w, b = r.randn(64, 5, 7, 7).astype(np.float32), r.randn(64).astype(np.float32)
    p = RM.pack_stem(w, b)
    assert p.size == 5 * 49 * 64 + 64 and np.array_equal(p[-64:], b) and not RM.pack_stem(w)[-64:].any()
    for co, ci, ky, kx in ((0, 0, 0, 0), (63, 4, 6, 6), (17, 2, 3, 5)):
        assert p[((ci * 7 + ky) * 7 + kx) * 64 + co] == w[co, ci, ky, kx]
