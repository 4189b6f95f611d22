"""GPU: vt_grad_stats, vt_grad_guard_close and vt_grad_scale against the float64 model tests/gradstat_model.py.  One buffer of 17 segments (lengths 1 .. 600 001
around the 4096-element chunk, gaps of 0, 1 and 64 elements filled with NaN, NaN / Inf at segment ends and chunk edges) at the four base alignments.
Gates (gradstat_model.stats_failures / close_failures): counts and largest magnitude exact, sums within len . 2^-53 relative, every output the same bits on a second
call and at every alignment; the coefficient is the model's float32 value at the kernel's own norm; the scaled gradient is one float32 multiplication per element."""
import numpy as np
import pytest
import torch

import gradstat_model as GS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ref():
    g, segs = GS.case()
    return g, segs, GS.seg_stats(g, segs)


def at_base(g, base):
    """the values on the device, ``base`` floats past a 16-byte boundary"""
    buf = torch.empty(g.size + 4, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[base:base + g.size]
    view.copy_(torch.as_tensor(g))
    return view


def bits(out):
    return [o.cpu().numpy().view(np.int64 if o.dtype == torch.float64 else np.int32).copy() for o in out]


def test_stats_against_the_model_at_every_alignment(ref):
    from vistracker_amd import ops
    g, segs, want = ref
    first = None
    for base in range(4):
        d = at_base(g, base)
        out = ops.grad_stats(d, segs)
        got = [o.cpu().numpy() for o in out]
        assert out[0].dtype == torch.float64 and out[1].dtype == torch.float32 and out[2].dtype == torch.int32
        bad = GS.stats_failures(got, want, segs)
        rel = max(abs(float(a) - float(b)) / float(b) / ((e - s) * GS.EPS) for a, b, (s, e) in zip(got[0], want[0], segs) if b > 0)
        print(f"\n[base {base}] largest sumsq error {rel:.3f} of its bound len . 2^-53", end="")
        assert not bad, (base, bad[:4])
        b0, again = bits(out), bits(ops.grad_stats(d, torch.as_tensor(segs, device=DEV)))
        assert all(np.array_equal(x, y) for x, y in zip(b0, again)), ("second call", base)
        first = b0 if first is None else first
        assert all(np.array_equal(x, y) for x, y in zip(b0, first)), ("against base 0", base)


def test_segments_and_gaps_that_hold_nothing(ref):
    from vistracker_amd import _lib as L, ops
    d = torch.full((300,), float("nan"), device=DEV)
    s, m, n = ops.grad_stats(d, [(0, 0), (7, 7), (300, 300)])          # empty segments: zeros, and nothing of the NaN around them
    assert s.tolist() == [0.0] * 3 and m.tolist() == [0.0] * 3 and n.tolist() == [0] * 3
    assert all(o.numel() == 0 for o in ops.grad_stats(d, []))
    with pytest.raises(L.VtError):
        ops.grad_stats(d, [(0, 10), (5, 20)])                           # not ascending
    with pytest.raises(L.VtError):
        ops.grad_stats(d, [(0, 301)])


def guard_of(bufs, segs, **kw):
    from vistracker_amd import ops
    return ops.StepGuard(bufs, [[(b, e - b) for b, e in s] for s in segs], [[f"b{k}.{i}" for i in range(len(s))] for k, s in enumerate(segs)], **kw)


CLOSE_SEGS = [[(0, 5), (64, 64 + GS.CHUNK + 3)], [(1, 2), (2, 131)], [(3, 70)]]
CLOSE_SIZES = (64 + GS.CHUNK + 3 + 2, 140, 70)


def close_buffers(seed):
    rng = np.random.default_rng(seed)
    return [rng.normal(0, 1e-3, n).astype(np.float32) for n in CLOSE_SIZES]


def want_close(hs, error, max_norm):
    st = [GS.seg_stats(h, s) for h, s in zip(hs, CLOSE_SEGS)]
    return st, GS.close([x[0] for x in st], [x[2] for x in st], error, max_norm)


@pytest.mark.parametrize("K", [1, 3])
def test_close_counters_ring_and_decision(K):
    """K + 2 steps: clean, a NaN in buffer 1, clean, a non-finite error alone, clean (the first K + 2 of them)"""
    plan = [("clean", 1.25), ("nan", 0.5), ("clean", 2.0), ("error", float("inf")), ("clean", 3.0)][:K + 2]
    n_el = sum(e - b for s in CLOSE_SEGS for b, e in s)
    max_norm = 0.02                                                     # below the norm of the buffers (about 0.065): clipping bites
    guard = guard_of([torch.empty(n, device=DEV) for n in CLOSE_SIZES], CLOSE_SEGS, max_norm=max_norm, record=K)
    assert guard.read()["steps"] == 0 and guard.read()["ring"] == []
    wants, skipped = [], 0
    for t, (kind, error) in enumerate(plan):
        hs = close_buffers(t)
        if kind == "nan":
            hs[1][5] = np.nan
        ds = [torch.as_tensor(h, device=DEV) for h in hs]
        skip = guard.close(ds, torch.tensor(error, dtype=torch.float64, device=DEV))
        st, want = want_close(hs, error, max_norm)
        assert want["skip"] == (kind != "clean") and (kind != "clean" or want["coef"] < 1)
        skipped += want["skip"]
        rec = guard.read()
        assert skip.dtype == torch.int32 and bool(skip.item()) == want["skip"] == rec["skip"]
        assert rec["steps"] == t + 1 and rec["skipped"] == skipped and rec["step"] == t and (rec["error"] == error)
        bad = GS.close_failures(rec, want, GS.coef_of(rec["norm"], max_norm), n_el)
        assert not bad, (t, bad)
        names = guard.names
        flat = [np.concatenate([x[i] for x in st]) for i in range(3)]
        assert [rec["nonfinite"][k] for k in names] == flat[2].tolist() and [np.float32(rec["maxabs"][k]) for k in names] == flat[1].tolist()
        assert not GS.stats_failures(([rec["sumsq"][k] for k in names], flat[1], flat[2]), flat, [s for ss in CLOSE_SEGS for s in ss])
        # the scaled gradients: one float32 multiplication per element by the coefficient the kernel chose; untouched on a skipped step
        for d, h in zip(ds, hs):
            assert np.array_equal(d.cpu().numpy().view(np.int32), GS.scaled(h, np.float32(rec["coef"]), want["skip"]).view(np.int32)), (t, kind)
        wants.append(rec)
        ring = rec["ring"]
        assert [r["step"] for r in ring] == list(range(max(0, t + 1 - K), t + 1))                     # the last K steps, oldest first
        for r in ring:
            assert all(r[k] == wants[r["step"]][k] or (k == "error" and np.isinf(r[k])) for k in ("norm", "coef", "skip", "error", "sumsq", "maxabs", "nonfinite")), (t, r["step"])


def test_no_clipping_and_no_error():
    guard = guard_of([torch.empty(n, device=DEV) for n in CLOSE_SIZES], CLOSE_SEGS)
    hs = close_buffers(9)
    ds = [torch.as_tensor(h, device=DEV) for h in hs]
    skip = guard.close(ds)
    rec = guard.read()
    assert not bool(skip.item()) and rec["coef"] == 1.0 and rec["error"] == 0.0 and rec["ring"] == []
    assert all(np.array_equal(d.cpu().numpy().view(np.int32), h.view(np.int32)) for d, h in zip(ds, hs))
    assert guard.launches_per_close == 10 and guard_of([torch.empty(70, device=DEV)], [CLOSE_SEGS[2]], max_norm=1.0).launches_per_close == 5


@pytest.mark.parametrize("n,base", [(1, 0), (3, 1), (5, 3), (1027, 0), (1027, 2), (70001, 1)])
def test_scale_is_one_multiplication_per_element(n, base):
    from vistracker_amd import ops
    h = GS.values(np.random.default_rng(n), n)
    coef = np.float32(0.3)
    for skip in (0, 1):
        d = at_base(h, base)
        ops.grad_scale(d, torch.tensor([coef], device=DEV), torch.tensor([skip], dtype=torch.int32, device=DEV))
        assert np.array_equal(d.cpu().numpy().view(np.int32), GS.scaled(h, coef, bool(skip)).view(np.int32)), (n, base, skip)
    d = at_base(h, base)
    ops.grad_scale(d, torch.tensor([coef], device=DEV))                # no flag: never skipped
    assert np.array_equal(d.cpu().numpy().view(np.int32), GS.scaled(h, coef, False).view(np.int32))
