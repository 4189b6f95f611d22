"""A numpy model of the two operators that join the ConvBlocks of an hourglass (model/HGFilters.py:32, 47) and of their backward, written from the definitions:

    F.avg_pool2d(x, 2, stride=2)                                               out = Py x Px^T,   P (n/2, n) with 1/2 at [i, 2i] and [i, 2i+1]
    F.interpolate(x, scale_factor=2, mode='bicubic', align_corners=True)       out = Uy x Ux^T,   U (2n, n):

output index o reads the source coordinate f = o (n - 1) / (2n - 1), the four taps floor(f) - 1 + i (i = 0..3) CLAMPED to [0, n - 1], with the cubic convolution
weights of t = f - floor(f) for A = -0.75; a tap that the clamp moves onto a neighbour adds to that neighbour's entry.  The backward of a linear operator is its
transpose.  Everything is computed in ``dtype``: float64 is the model, float32 (coordinates, weights and sums) the run that defines e32.  It shares no code with
the product (vistracker_amd/csrc/resample_bwd.hip, encoder_ops.hip).  Tensors are NCHW numpy arrays.

``a``, ``align_corners`` and ``border`` exist for the mutants of tests/test_host_resample.py only."""
import numpy as np


def cubic_weights(t, a, dtype):
    """the four weights of the taps at distance t + 1, t, 1 - t, 2 - t (Keys' cubic convolution kernel with parameter a)"""
    c = dtype
    near = lambda d: ((a + c(2)) * d - (a + c(3))) * d * d + c(1)                    # noqa: E731  |d| <= 1
    far = lambda d: ((a * d - c(5) * a) * d + c(8) * a) * d - c(4) * a                # noqa: E731  1 < |d| < 2
    return [far(t + c(1)), near(t), near(c(1) - t), far(c(2) - t)]


def upsample_matrix(n, dtype=np.float64, a=-0.75, align_corners=True, border="clamp"):
    """U (2n, n).  border: 'clamp' (the definition), 'zero' (taps outside dropped), 'once' (a clamped duplicate tap counted once)"""
    c = dtype
    N = 2 * n
    U = np.zeros((N, n), dtype)
    scale = c(n - 1) / c(N - 1) if N > 1 else c(0)
    for o in range(N):
        f = scale * c(o) if align_corners else (c(o) + c(0.5)) * c(0.5) - c(0.5)
        i0 = int(np.floor(f))
        w = cubic_weights(f - c(i0), c(a), c)
        seen = set()
        for i in range(4):
            k = i0 - 1 + i
            if border == "zero" and not 0 <= k < n:
                continue
            k = min(max(k, 0), n - 1)
            if border == "once" and k in seen:
                continue
            seen.add(k)
            U[o, k] = U[o, k] + w[i]
    return U


def pool_matrix(n, dtype=np.float64):
    """P (n/2, n)"""
    assert n % 2 == 0
    P = np.zeros((n // 2, n), dtype)
    for i in range(n // 2):
        P[i, 2 * i] = P[i, 2 * i + 1] = dtype(0.5)
    return P


def _apply(My, Mx, x, dtype):
    """My x Mx^T over the last two axes, in dtype"""
    return np.einsum("oy,bcyx,px->bcop", My, np.asarray(x, dtype), Mx).astype(dtype)


def upsample(low, dtype=np.float64, **kw):
    h, w = low.shape[2:]
    return _apply(upsample_matrix(h, dtype, **kw), upsample_matrix(w, dtype, **kw), low, dtype)


def upsample_backward(d_out, dtype=np.float64, **kw):
    """d_low = Uy^T d_out Ux"""
    h, w = d_out.shape[2] // 2, d_out.shape[3] // 2
    return _apply(upsample_matrix(h, dtype, **kw).T, upsample_matrix(w, dtype, **kw).T, d_out, dtype)


def avgpool(x, dtype=np.float64):
    H, W = x.shape[2:]
    return _apply(pool_matrix(H, dtype), pool_matrix(W, dtype), x, dtype)


def avgpool_backward(d_out, dtype=np.float64):
    h, w = d_out.shape[2:]
    return _apply(pool_matrix(2 * h, dtype).T, pool_matrix(2 * w, dtype).T, d_out, dtype)


def operator_2d(h, w, dtype=np.float64, **kw):
    """the whole up-sampling operator as a matrix (2h 2w, h w): row = output pixel oy 2w + ox, column = low pixel yy w + xx"""
    return np.kron(upsample_matrix(h, dtype, **kw), upsample_matrix(w, dtype, **kw)).astype(dtype)


def backward_and_e32(d_out):
    """(float64 d_low, e32 = the largest |float32 run - float64 run|)"""
    g64 = upsample_backward(d_out, np.float64)
    g32 = upsample_backward(np.asarray(d_out, np.float32), np.float32)
    return g64, float(np.abs(g32.astype(np.float64) - g64).max())
