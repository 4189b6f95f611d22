"""GPU: the backward of 2 x 2 average pooling and of the bicubic x2 up-sampling (csrc/resample_bwd.hip, ops.avgpool2x2_train / upsample2x_bicubic_add_train)
against the numpy float64 model of tests/resample_model.py.  Bounds follow tests/test_gpu_convblock.py: e32 = the float32 run of the model against its float64
run on the test's own inputs, the kernel gets 4 e32; the pooling backward is exact and compared bit for bit."""
import numpy as np
import pytest
import torch

import resample_model as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def L():
    from vistracker_amd import _lib
    return _lib


def cl(a):
    """NCHW numpy -> channels-last float32 device tensor"""
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).to(DEV).contiguous(memory_format=torch.channels_last)


def nchw(t):
    return t.detach().double().cpu().numpy()


def report(what, name, err, e32, scale):
    print(f"\n[{what}] {name:>12}: e32 {e32:.3e} | kernel error {err:.3e} ({err / e32 if e32 > 0 else 0.0:.2f} e32) | largest element {scale:.3e}", end="")


def nan_like(B, C, H, W):
    return torch.full((B, C, H, W), float("nan"), device=DEV).contiguous(memory_format=torch.channels_last)


def raw_up_bwd(d, out=None):
    """vt_upsample2x_bicubic_backward on a channels-last device tensor d (B,C,2h,2w), into ``out`` (NaN-filled when not given)"""
    B, C, H, W = d.shape
    d = d.contiguous(memory_format=torch.channels_last)
    out = nan_like(B, C, H // 2, W // 2) if out is None else out
    L().check(L().lib().vt_upsample2x_bicubic_backward(d.data_ptr(), B, H // 2, W // 2, C, out.data_ptr(), L().stream_ptr()))
    return out


@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 4), (2, 6, 10, 36), (1, 16, 32, 256)])
def test_a_pool_backward_bit_for_bit(B, H, W, C):
    d = np.random.RandomState(B + H + W + C).randn(B, C, H // 2, W // 2).astype(np.float32)
    got = nan_like(B, C, H, W)
    dt = cl(d)
    L().check(L().lib().vt_avgpool2x2_backward(dt.data_ptr(), B, H, W, C, got.data_ptr(), L().stream_ptr()))
    want = np.float32(0.25) * np.repeat(np.repeat(d, 2, 2), 2, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(want.astype(np.float64), R.avgpool_backward(d))           # and that is the model


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C", [4, 36, 256])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (2, 3), (5, 7), (8, 16), (16, 32)])
def test_b_bicubic_backward(h, w, C, B):
    d = np.random.RandomState(1000 + 97 * h + w + C + B).randn(B, C, 2 * h, 2 * w).astype(np.float32)
    g64, e32 = R.backward_and_e32(d)
    err = float(np.abs(nchw(raw_up_bwd(cl(d))) - g64).max())
    report(f"b {h}x{w} C{C} B{B}", "d_low", err, e32, float(np.abs(g64).max()))
    assert np.isfinite(err) and err <= 4 * e32


@pytest.mark.parametrize("h,w", [(3, 4), (1, 1), (2, 2)])
def test_c_whole_operator(h, w):
    """output pixel k's one-hot in channel k: d_low[..., k] is row k of U"""
    n = 4 * h * w
    d = np.zeros((1, n, 2 * h, 2 * w), np.float32)
    d[0, np.arange(n), np.arange(n) // (2 * w), np.arange(n) % (2 * w)] = 1.0
    got = nchw(raw_up_bwd(cl(d)))[0].reshape(n, h * w)
    U64 = R.operator_2d(h, w)
    e32 = float(np.abs(R.operator_2d(h, w, np.float32).astype(np.float64) - U64).max())
    err = float(np.abs(got - U64).max())
    report(f"c operator {h}x{w}", "U", err, e32, float(np.abs(U64).max()))
    assert np.isfinite(err) and err <= 4 * e32
    assert np.all(got[U64 == 0] == 0), "an entry outside the operator's support: wrong window or clamp"


def test_d_adjoint():
    """<U a, b> == <a, U^T b> with U a from the forward kernel (vt_upsample2x_bicubic_add, NULL skip)"""
    B, C, h, w = 2, 8, 5, 7
    r = np.random.RandomState(7)
    a, b = r.randn(B, C, h, w).astype(np.float32), r.randn(B, C, 2 * h, 2 * w).astype(np.float32)
    at = cl(a)
    Ua = nan_like(B, C, 2 * h, 2 * w)
    L().check(L().lib().vt_upsample2x_bicubic_add(at.data_ptr(), None, B, h, w, C, Ua.data_ptr(), L().stream_ptr()))
    Utb = raw_up_bwd(cl(b))
    lhs, rhs = float((nchw(Ua) * b.astype(np.float64)).sum()), float((a.astype(np.float64) * nchw(Utb)).sum())
    # each side's own 4 e32 against the float64 model, carried through the inner product: sum |b| e32(U a) + sum |a| e32(U^T b)
    e_fwd = float(np.abs(R.upsample(a, np.float32).astype(np.float64) - R.upsample(a)).max())
    e_bwd = R.backward_and_e32(b)[1]
    bound = 4 * (e_fwd * float(np.abs(b).sum()) + e_bwd * float(np.abs(a).sum()))
    print(f"\n[d adjoint] <U a, b> {lhs:.9e} | <a, U^T b> {rhs:.9e} | difference {abs(lhs - rhs):.3e} | bound {bound:.3e}", end="")
    assert abs(lhs - rhs) <= bound


def test_e_calling_conventions():
    lib = L().lib()
    B, C, h, w = 2, 36, 5, 7
    d = cl(np.random.RandomState(11).randn(B, C, 2 * h, 2 * w))
    g0 = raw_up_bwd(d)
    assert torch.equal(raw_up_bwd(d), g0), "two calls, equal bits"
    for k in (-40, 40):
        assert torch.equal(raw_up_bwd(d * 2.0 ** k), g0 * 2.0 ** k), k          # no range assumption
    pre = nan_like(B, C, h, w)
    assert torch.equal(raw_up_bwd(d, out=pre), g0) and not torch.isnan(g0).any()         # NaN-filled output: every element written
    dp = cl(np.random.RandomState(12).randn(B, C, h, w))
    p0, p1 = nan_like(B, C, 2 * h, 2 * w), nan_like(B, C, 2 * h, 2 * w)
    for p in (p0, p1):
        L().check(lib.vt_avgpool2x2_backward(dp.data_ptr(), B, 2 * h, 2 * w, C, p.data_ptr(), L().stream_ptr()))
    assert torch.equal(p0, p1) and not torch.isnan(p0).any()
    # refused without a launch: the outputs keep their NaN fill
    out = nan_like(B, C, 6, 6)
    assert lib.vt_avgpool2x2_backward(dp.data_ptr(), B, 5, 6, C, out.data_ptr(), L().stream_ptr()) == L().VT_ERR_ARG          # odd H
    assert lib.vt_avgpool2x2_backward(dp.data_ptr(), B, 6, 6, 6, out.data_ptr(), L().stream_ptr()) == L().VT_ERR_ARG          # C = 6
    assert lib.vt_upsample2x_bicubic_backward(d.data_ptr(), B, 3, 3, 6, out.data_ptr(), L().stream_ptr()) == L().VT_ERR_ARG   # C = 6
    assert lib.vt_upsample2x_bicubic_backward(d.data_ptr(), B, 0, 3, C, out.data_ptr(), L().stream_ptr()) == L().VT_ERR_ARG   # h = 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_f_autograd_ops():
    from vistracker_amd import encoder, ops
    B, C, H, W = 2, 64, 8, 12
    r = np.random.RandomState(21)
    # pooling
    x = cl(r.randn(B, C, H, W)).requires_grad_(True)
    y = ops.avgpool2x2_train(x)
    want = encoder.avgpool2x2(x.detach())
    assert torch.equal(y.detach(), want)
    assert y._vt_stats[1] == want._vt_stats[1] and y._vt_stats[2] is False and torch.equal(y._vt_stats[0][B * 32:], want._vt_stats[0][B * 32:])      # the partial sums
    dy = cl(r.randn(B, C, H // 2, W // 2))
    y.backward(dy)
    assert torch.equal(x.grad, ops.avgpool2x2_backward(dy))
    assert np.array_equal(x.grad.cpu().numpy(), np.float32(0.25) * np.repeat(np.repeat(dy.cpu().numpy(), 2, 2), 2, 3))
    # up-sampling + skip
    low, skip = cl(r.randn(B, C, H // 2, W // 2)).requires_grad_(True), cl(r.randn(B, C, H, W)).requires_grad_(True)
    z = ops.upsample2x_bicubic_add_train(low, skip)
    want = encoder.upsample2x_bicubic_add(low.detach(), skip.detach())
    assert torch.equal(z.detach(), want)
    assert z._vt_stats[1] == want._vt_stats[1] and z._vt_stats[2] is False and torch.equal(z._vt_stats[0][B * 32:], want._vt_stats[0][B * 32:])
    dz = cl(r.randn(B, C, H, W))
    z.backward(dz)
    assert torch.equal(low.grad, ops.upsample2x_bicubic_backward(dz)) and torch.equal(low.grad, raw_up_bwd(dz))
    assert torch.equal(skip.grad, dz)
    # no CPU path
    for fn, args in ((ops.avgpool2x2_train, (torch.zeros(1, 32, 4, 4),)), (ops.upsample2x_bicubic_add_train, (torch.zeros(1, 32, 2, 2), torch.zeros(1, 32, 4, 4))),
                     (ops.avgpool2x2_backward, (torch.zeros(1, 32, 2, 2),)), (ops.upsample2x_bicubic_backward, (torch.zeros(1, 32, 4, 4),))):
        with pytest.raises(L().VtError):
            fn(*args)
