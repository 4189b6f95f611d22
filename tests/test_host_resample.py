"""CPU: the models of the hourglass's joining operators (tests/resample_model.py) and of the hourglass (tests/hourglass_model.py) against torch float64 and the
recorded reference; the gate of tests/test_gpu_resample_bwd.py (4 e32) shown to pass the float32 run and to reject four wrong operators."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hourglass_model as HM
import resample_model as R
from conftest import ROOT, golden

SIZES = [(1, 1), (1, 5), (2, 3), (5, 7), (8, 16)]


def _rand(seed, *shape):
    return np.random.RandomState(seed).randn(*shape)


@pytest.mark.parametrize("h,w", SIZES)
def test_upsample_model_is_torch_float64(h, w):
    low, d = _rand(1, 2, 4, h, w), _rand(2, 2, 4, 2 * h, 2 * w)
    lt = torch.tensor(low, requires_grad=True)
    up = F.interpolate(lt, scale_factor=2, mode="bicubic", align_corners=True)
    up.backward(torch.tensor(d))
    tol = 64 * np.finfo(np.float64).eps * max(1.0, float(np.abs(d).max()) * 4)
    assert np.abs(up.detach().numpy() - R.upsample(low)).max() <= tol
    assert np.abs(lt.grad.numpy() - R.upsample_backward(d)).max() <= tol
    # the operator matrix is the same map
    U = R.operator_2d(h, w)
    assert np.abs((U @ low.reshape(8, -1).T).T.reshape(2, 4, 2 * h, 2 * w) - up.detach().numpy()).max() <= tol


def test_pool_model_is_torch_float64():
    x, d = _rand(3, 2, 4, 6, 10), _rand(4, 2, 4, 3, 5)
    xt = torch.tensor(x, requires_grad=True)
    p = F.avg_pool2d(xt, 2, stride=2)
    p.backward(torch.tensor(d))
    assert np.abs(p.detach().numpy() - R.avgpool(x)).max() <= 1e-15
    assert np.array_equal(xt.grad.numpy(), R.avgpool_backward(d))           # 0.25 d: exact
    assert np.array_equal(R.avgpool_backward(d.astype(np.float32), np.float32), np.float32(0.25) * np.repeat(np.repeat(d.astype(np.float32), 2, 2), 2, 3))


MUTANTS = {"zero padding instead of clamped taps": dict(border="zero"), "align_corners=False scaling": dict(align_corners=False), "A = -0.5": dict(a=-0.5),
           "a clamped duplicate tap counted once": dict(border="once")}


@pytest.mark.parametrize("h,w", [(2, 3), (5, 7), (8, 16)])
def test_gate_passes_float32_and_rejects_mutants(h, w):
    d = _rand(10 * h + w, 2, 4, 2 * h, 2 * w).astype(np.float32)
    g64, e32 = R.backward_and_e32(d)
    assert e32 > 0
    g32 = R.upsample_backward(d, np.float32).astype(np.float64)
    assert np.abs(g32 - g64).max() <= 4 * e32               # trivially: it defines e32
    for name, kw in MUTANTS.items():
        err = float(np.abs(R.upsample_backward(d, np.float64, **kw) - g64).max())
        print(f"\n[{h}x{w}] {name}: error {err:.3e} = {err / e32:.1f} e32", end="")
        assert err > 4 * e32, name


def test_gather_window_in_float32():
    """what vt_upsample2x_bicubic_backward relies on, with the forward's float32 coordinates: every output row that reads low row l lies in [2l - 4, 2l + 4], a
    low row has at most 9 readers, and no tap base exceeds n - 1 (all weight lands inside the matrix)"""
    for n in list(range(1, 130)) + [256, 512]:
        U = R.upsample_matrix(n, np.float32)
        for l in range(n):
            rows = np.nonzero(U[:, l])[0]
            assert len(rows) <= 9 and rows.min() >= 2 * l - 4 and rows.max() <= 2 * l + 4, (n, l, rows)
        # a partition of unity, so nothing was dropped: four float32 Horner polynomials of three steps with intermediates below 8, 4 x 3 x 8 x 2^-24 = 5.7e-6
        assert np.abs(U.sum(1) - 1).max() < 1e-5, n


def test_hourglass_model_forward_is_the_recorded_reference():
    gold = golden("hourglass")
    P = HM.make_params(2, 128, 61)
    x, _ = HM.make_inputs(1, 32, 64, 128, 161)
    out64 = HM.forward(P, x)
    e32 = float(np.abs(HM.forward(P, x, torch.float32) - out64).max())
    err = float(np.abs(gold["out"] - out64.reshape(-1)[::HM.GOLDEN_OUT_STEP]).max())
    print(f"\nhourglass out: the model's float32 error {e32:.3e}, |reference - model64| {err:.3e} of {np.abs(out64).max():.3e}", end="")
    assert e32 > 0 and err <= 4 * e32


def test_hourglass_manual_grads_are_autograd():
    """the explicit chain at the model's own saved activations equals float64 autograd (small: depth 2, 128 features, 8 x 16)"""
    P = HM.make_params(2, 128, 5)
    x, dy = HM.make_inputs(1, 8, 16, 128, 6)
    g = HM.autograd_grads(P, x, dy)
    m = HM.manual_grads(P, x, dy)
    assert set(m) == set(g) - {"out"}
    for n in m:
        assert np.abs(m[n] - g[n]).max() <= 1e-10 * max(1.0, np.abs(g[n]).max()), n


def test_header_declares_the_entry_points():
    src = open(os.path.join(ROOT, "include", "vistracker.h")).read()
    for name in ("vt_avgpool2x2_backward", "vt_upsample2x_bicubic_backward"):
        assert re.search(r"\bint\s+" + name + r"\s*\(const float \*d_out, int B, int \w+, int \w+, int C, float \*\w+, void \*stream\);", src), name
