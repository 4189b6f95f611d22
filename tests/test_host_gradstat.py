"""CPU: the float64 model of the gradient record and the step guard (tests/gradstat_model.py) against a naive restatement, the four mutants its cases and gates
must reject, the library's exports, and the constructor's refusal of clipping without the guard."""
import ctypes
import math
import os

import numpy as np
import pytest

import gradstat_model as GS


@pytest.fixture(scope="module")
def ref():
    g, segs = GS.case()
    return g, segs, GS.seg_stats(g, segs)


def naive_stats(g, segs, square_all=False, end_shift=0, to_next_begin=False):
    """element by element in Python floats, added left to right; the switches are the mutants"""
    out = ([], [], [])
    for s, (b, e) in enumerate(segs):
        if to_next_begin and s + 1 < len(segs):
            e = segs[s + 1][0]
        e += end_shift
        tot, mx, nf = 0.0, 0.0, 0
        for x in g[b:e].tolist():
            if math.isnan(x) or math.isinf(x):
                nf += 1
                if square_all:
                    tot += x * x
                continue
            tot += x * x
            mx = max(mx, abs(x))
        out[0].append(tot); out[1].append(np.float32(mx)); out[2].append(nf)
    return out


def test_model_against_the_restatement(ref):
    g, segs, want = ref
    assert GS.stats_failures(naive_stats(g, segs), want, segs) == []
    # the case holds what it promises
    lens = [e - b for b, e in segs]
    assert set(GS.LENGTHS) <= set(lens) and lens.count(1) == 4 and all(np.isnan(g[e:(segs[s + 1][0] if s + 1 < len(segs) else None)]).all() for s, (b, e) in enumerate(segs))
    assert sorted({segs[s + 1][0] - segs[s][1] for s in range(len(segs) - 1)}) == [0, 1, 64]
    fin = g[np.isfinite(g) & (g != 0)].astype(np.float64)
    assert np.log2(np.abs(fin).max() / np.abs(fin[np.abs(fin) >= 1e-30]).min()) >= 30 and (np.abs(fin) < 1.2e-38).any() and (np.abs(fin) > 2.9e38).any()
    s, m, n = want
    assert n[lens.index(70)] == 70 and s[lens.index(70)] == 0 and m[lens.index(70)] == 0 and s[lens.index(130)] == 0 and n[lens.index(130)] == 0
    assert n[lens.index(GS.CHUNK + 1)] == 2 and n[lens.index(65)] == 2 and n[lens.index(600001)] == 2 and s[lens.index(600001)] > 0
    assert all(np.isfinite(s))                                     # a NaN does not erase the norm of its tensor


def test_close_and_scale_of_the_model():
    assert GS.coef_of(3.0, None) == 1 and GS.coef_of(3.0, 0.0) == 1 and GS.coef_of(0.5, 1.0) == 1
    assert GS.coef_of(2.0, 1.0) == np.float32(1.0 / (2.0 + 1e-6))
    c = GS.close([np.array([9.0, 16.0])], [np.array([0, 0])], 1.5, 2.5)
    assert c["norm"] == 5.0 and c["skip"] is False and c["coef"] == np.float32(2.5 / (5.0 + 1e-6))
    assert GS.close([np.array([1.0])], [np.array([1])], 1.5, None)["skip"] and GS.close([np.array([1.0])], [np.array([0])], float("inf"), None)["skip"]
    assert GS.close([np.array([1.0])], [np.array([0])], float("nan"), None)["skip"]
    g = np.array([1.0, -3.0, 1e-40], np.float32)
    assert np.array_equal(GS.scaled(g, np.float32(0.3), False), g * np.float32(0.3)) and np.array_equal(GS.scaled(g, np.float32(0.3), True), g)


MUTANTS = {
    "non-finite elements squared into the sum": dict(square_all=True),
    "padding counted": dict(to_next_begin=True),
    "a segment end one too far": dict(end_shift=1),
    "a segment end one short": dict(end_shift=-1),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_the_gates_reject_the_mutant(ref, name):
    g, segs, want = ref
    bad = GS.stats_failures(naive_stats(g, segs, **MUTANTS[name]), want, segs)
    print(f"\n[{name}] fails {len(bad)} gates, the first: {bad[:1]}", end="")
    assert bad, name


def test_the_gates_reject_a_coefficient_without_its_epsilon():
    norm, max_norm = 1e-3, 5e-4
    want = GS.close([np.array([norm * norm])], [np.array([0])], 0.0, max_norm)
    mutant = dict(want, coef=np.float32(min(1.0, max_norm / want["norm"])))
    assert GS.close_failures(want, want, GS.coef_of(want["norm"], max_norm), 2) == []
    assert [b[0] for b in GS.close_failures(mutant, want, GS.coef_of(want["norm"], max_norm), 2)] == ["coef"]


def test_library_exports_the_guard():
    from vistracker_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vt_grad_stats", "vt_grad_stats_workspace_bytes", "vt_grad_guard_close", "vt_grad_scale", "vt_grad_guard_record_bytes"):
        assert hasattr(l, name) and name in _lib.SIGNATURES, name
    fn = l.vt_grad_stats_workspace_bytes
    fn.restype, fn.argtypes = ctypes.c_long, [ctypes.c_long, ctypes.c_int]
    # room for every chunk partial (8 + 4 + 4 bytes and a table entry) of any segmentation of n elements into n_seg segments
    n, n_seg = 10 * GS.CHUNK + 5, 7
    assert fn(n, n_seg) >= 20 * (n // GS.CHUNK + n_seg) and fn(0, 0) >= 0
    rec = l.vt_grad_guard_record_bytes
    rec.restype, rec.argtypes = ctypes.c_long, [ctypes.c_int, ctypes.c_int]
    assert rec(5, 0) == 16 + 32 + 16 * 5 and rec(5, 3) == 16 + 4 * (32 + 16 * 5)


def test_clipping_without_the_guard_raises():
    """the check comes before anything touches a device"""
    from vistracker_amd import _lib as L
    from vistracker_amd.training import SIFNetTrainer
    with pytest.raises(L.VtError, match="guard"):
        SIFNetTrainer({}, None, clip_norm=1.0)
    with pytest.raises(L.VtError, match="guard"):
        SIFNetTrainer({}, None, record=4)
