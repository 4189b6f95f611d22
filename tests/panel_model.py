"""Test helper (not a test file): the camera panel of step 7 -- the bilinear resize of an (h, w) image to (H, size) with half-pixel centres and rounding to
grey levels, the contract of vt_resize_panel_u8 in csrc/inputs.hip and of ``sequence_io.resize_bilinear_hw`` -- restated in exact integer arithmetic.

Per axis, output pixel d of ``out`` samples the ``n`` source pixels at src = n / out * (d + 0.5) - 0.5 = (n (2 d + 1) - out) / (2 out), clamped at 0
(``inputs_model.axis_taps``): tap weights are integers over 2 out, the blend of the four uint8 taps is an integer V over D = (2 size) (2 H), and rounding to
the nearest grey level, floor(V / D + 1 / 2), is (2 V + D) // (2 D).  No floating point anywhere.
"""
from __future__ import annotations

import numpy as np

from inputs_model import axis_taps


def resize_hw(img, H, size):
    """uint8 image (h,w) or (h,w,C) -> (grey levels (H,size[,C]) uint8, distance (H,size[,C]) of the exact blend from the nearest half-way point, in grey levels)"""
    c = np.asarray(img).astype(np.int64)
    ix0, ix1, wx0, wx1 = axis_taps(c.shape[1], size)
    iy0, iy1, wy0, wy1 = axis_taps(c.shape[0], H)
    ex = (lambda a: a[..., None]) if c.ndim == 3 else (lambda a: a)
    row = lambda iy: c[iy][:, ix0] * ex(wx0[None, :]) + c[iy][:, ix1] * ex(wx1[None, :])
    V = row(iy0) * ex(wy0[:, None]) + row(iy1) * ex(wy1[:, None])
    D = (2 * size) * (2 * H)
    q = np.clip((2 * V + D) // (2 * D), 0, 255).astype(np.uint8)
    r = (2 * V + D) % (2 * D)
    return q, np.minimum(r, 2 * D - r) / (2 * D)


def panel(img, H, size, cs, ce):
    """columns [cs, ce) of ``resize_hw``: the panel's grey levels and distances"""
    q, d = resize_hw(img, H, size)
    return q[:, cs:ce], d[:, cs:ce]


def tap_extent(w, size, cs, ce):
    """first and last source column that the exact taps of output columns [cs, ce) read (weight-0 taps included)"""
    i0, i1, _, _ = axis_taps(w, size)
    return int(i0[cs:ce].min()), int(i1[cs:ce].max())


def image(seed, h, w):
    """seeded random (h,w,3) uint8 image"""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# the panel of image_size 64: H = int(0.75 * 64), columns int(0.2 * 64) .. int(0.8 * 64)
SIZE, H, CS, CE = 64, 48, 12, 51
# ratio 2 on both axes: every weight is 1 / 4 or 3 / 4, every blend exact in fp32
EXACT = (96, 128)
# non-dyadic with a different ratio per axis; another one; up-scaling (both clamps of the tap rule live)
ROUNDING = [(83, 110), (75, 101), (30, 40)]
