"""GPU: ``vt_grad_rank_mean`` (csrc/gradreduce.hip) against its float64 model tests/gradreduce_model.py, bit for bit: every n, W, stride and base offset of the
case set, into a fresh ``out`` and in place into each row; W = 1 is the identity; a power-of-two scale goes through; two calls give equal bits; the error returns.
The comparison runs on the int32 view on the device, NaN payloads excluded (where the model has a NaN any NaN will do); one read-back per W."""
import numpy as np
import pytest
import torch

import gradreduce_model as GM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def placed(host, pad, off):
    """the (W, n) array in device memory with rows n + pad apart, starting ``off`` floats into an aligned allocation -> the (W, n) view"""
    W, n = host.shape
    stride = n + pad
    buf = torch.full((W * stride + off + 4,), 777.0, device=DEV)
    view = buf[off:off + W * stride].view(W, stride)
    view[:, :n] = torch.as_tensor(host, device=DEV)
    return view[:, :n], buf


def agree(got, want_bits, want_nan):
    """device bool: got (n,) equals the model as bits outside its NaNs and is NaN inside them"""
    return (torch.where(want_nan, torch.isnan(got), got.view(torch.int32) == want_bits)).all()


@pytest.mark.parametrize("W", GM.WS)
def test_kernel_is_the_model_bit_for_bit(W):
    from vistracker_amd import ops
    flags, names = [], []
    for n in GM.NS:
        host = GM.values(W, n)
        want = GM.mean(host)
        want_bits, want_nan = torch.as_tensor(want.view(np.int32), device=DEV), torch.as_tensor(np.isnan(want), device=DEV)
        for pad in GM.PADS:
            for poff in GM.OFFSETS:
                parts, buf = placed(host, pad, poff)
                before = buf.clone()
                for ooff in GM.OFFSETS:                                                   # a fresh out, its own base offset
                    obuf = torch.full((n + ooff + 4,), 555.0, device=DEV)
                    out = ops.grad_rank_mean(parts, out=obuf[ooff:ooff + n])
                    flags.append(agree(out, want_bits, want_nan)); names.append((n, pad, poff, ooff, "fresh"))
                    flags.append((obuf[:ooff] == 555.0).all() & (obuf[ooff + n:] == 555.0).all()); names.append((n, pad, poff, ooff, "fresh: nothing written outside out"))
                flags.append((buf.view(torch.int32) == before.view(torch.int32)).all()); names.append((n, pad, poff, "parts untouched"))
                for r in range(W):                                                        # in place into row r
                    parts, buf = placed(host, pad, poff)
                    ops.grad_rank_mean(parts, out=parts[r])
                    flags.append(agree(parts[r], want_bits, want_nan)); names.append((n, pad, poff, r, "in place"))
                    others = torch.as_tensor(np.delete(host, r, 0).view(np.int32), device=DEV)
                    rest = torch.cat([parts[:r], parts[r + 1:]], 0).view(torch.int32)
                    flags.append((rest == others).all()); names.append((n, pad, poff, r, "in place: the other rows untouched"))
    ok = torch.stack([torch.as_tensor(f, device=DEV).reshape(()) for f in flags]).cpu().numpy()
    assert ok.all(), [names[i] for i in np.flatnonzero(~ok)][:20]


def test_w1_returns_its_input():
    from vistracker_amd import ops
    for n in (1, 5, 1025, 4 * 256 * 3 + 2):
        host = GM.values(1, n)
        finite = ~np.isnan(host[0])
        parts, _ = placed(host, 0, 0)
        out = ops.grad_rank_mean(parts).cpu().numpy()
        assert np.array_equal(out[finite].view(np.int32), host[0][finite].view(np.int32)) and np.isnan(out[~finite]).all()


def test_power_of_two_scale_and_repeatability():
    from vistracker_amd import ops
    for W in GM.WS:
        host = GM.values(W, 4 * 256 * 3 + 2)
        keep = np.isfinite(host).all(0) & (np.abs(host) < 1e30).all(0) & ((np.abs(host) > 1e-30) | (host == 0)).all(0)          # short of overflow and underflow
        host = np.ascontiguousarray(host[:, keep])
        parts, _ = placed(host, 0, 0)
        a, b = ops.grad_rank_mean(parts), ops.grad_rank_mean(parts)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))                                                        # two calls, equal bits
        scaled = ops.grad_rank_mean(parts * 2.0 ** -7)
        assert torch.equal(scaled.view(torch.int32), (a * 2.0 ** -7).view(torch.int32)), W


def test_error_returns():
    from vistracker_amd import _lib as L, ops
    lib = L.lib()
    x, out = torch.zeros(2, 8, device=DEV), torch.zeros(8, device=DEV)
    st = L.stream_ptr()
    assert lib.vt_grad_rank_mean(x.data_ptr(), 0, 8, 8, out.data_ptr(), st) == L.VT_ERR_ARG and b"W" in lib.vt_last_error()
    assert lib.vt_grad_rank_mean(x.data_ptr(), -3, 8, 8, out.data_ptr(), st) == L.VT_ERR_ARG
    assert lib.vt_grad_rank_mean(None, 2, 8, 8, out.data_ptr(), st) == L.VT_ERR_ARG and b"NULL" in lib.vt_last_error()
    assert lib.vt_grad_rank_mean(x.data_ptr(), 2, 8, 8, None, st) == L.VT_ERR_ARG
    assert lib.vt_grad_rank_mean(x.data_ptr(), 2, 8, 7, out.data_ptr(), st) == L.VT_ERR_ARG and b"stride" in lib.vt_last_error()
    assert lib.vt_grad_rank_mean(x.data_ptr(), 2, 8, 8, x.data_ptr() + 4, st) == L.VT_ERR_ARG                                # overlaps the rows, is none of them
    assert lib.vt_grad_rank_mean(None, 2, 0, 0, None, st) == L.VT_OK                                                        # n = 0: a successful no-op
    out.fill_(3.0)
    assert lib.vt_grad_rank_mean(x.data_ptr(), 2, 0, 8, out.data_ptr(), st) == L.VT_OK and bool((out == 3.0).all())
    with pytest.raises(L.VtError):
        ops.grad_rank_mean(x.double())
    with pytest.raises(L.VtError):
        ops.grad_rank_mean(x, out=torch.zeros(7, device=DEV))
    with pytest.raises(L.VtError):
        ops.grad_rank_mean(x.cpu())
    assert ops.grad_rank_mean(torch.zeros(3, 0, device=DEV)).shape == (0,)
