"""Test helper (not a test file): the two contracts of csrc/overlay.hip restated in float64 / integer numpy.  Nothing here is shared with the product, and
both take the rasteriser's outputs (rgb / alpha, owner maps) as INPUTS, so neither depends on the rasteriser.

Overlay (vt_overlay_panel_u8): per pixel and channel, p the panel's byte, v = 255 opacity clip(rgb, 0, 1) + (1 - opacity alpha) p, q = clip(floor(v + 1/2), 0, 255).
Score (vt_mask_score): owner d -> face d (d < F) or d - F (d < 2 F) or none; face -> body (< nf_body), object (< nf_body + nf_obj) or neither; raster sample
(yi, xi) of rows [0, rows) x [0, is) reads mask pixel (((2 yi + 1) h) // (2 rows), ((2 xi + 1) w) // (2 is)), channel 0, on when > thres.
"""
from __future__ import annotations

import numpy as np


def overlay(rgb, alpha, panel, opacity):
    """rgb (..., 3) and alpha (...) float32 as rendered, panel (..., 3) uint8 -> (grey levels uint8, distance of v from the nearest half-way point).  The opacity
    is the float32 the C ABI receives."""
    o = np.float64(np.float32(opacity))
    v = 255.0 * o * np.clip(np.asarray(rgb, np.float64), 0.0, 1.0) + (1.0 - o * np.asarray(alpha, np.float64)[..., None]) * np.asarray(panel).astype(np.float64)
    q = np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)
    return q, np.abs(v - np.floor(v) - 0.5)


def assert_overlay(got, rgb, alpha, panel, opacity, band=1e-3, max_share=0.01, tag=""):
    """the band rule: equal to the model wherever v is more than ``band`` from a half-way point, within one level there, and at most ``max_share`` of the
    values may be that close"""
    q, d = overlay(rgb, alpha, panel, opacity)
    clear = d > band
    share = 1.0 - clear.mean()
    print(f"{tag}: device differs from the model in {int((got != q).sum())} of {q.size} values; {100 * share:.2f} % within {band} of a half-way point")
    np.testing.assert_array_equal(got[clear], q[clear])
    assert np.abs(got.astype(int) - q.astype(int)).max(initial=0) <= 1
    assert share <= max_share, share


def classes(fidx, F, nf_body, nf_obj):
    """owner map -> 0 body, 1 object, -1 neither"""
    d = np.asarray(fidx).astype(np.int64)
    face = np.where((d >= 0) & (d < F), d, np.where((d >= F) & (d < 2 * F), d - F, -1))
    return np.where((face >= 0) & (face < nf_body), 0, np.where((face >= nf_body) & (face < nf_body + nf_obj), 1, -1))


def sample(mask, rows, is_):
    """(h,w) or (h,w,C) mask -> (rows, is) values at the contract's nearest-neighbour positions, channel 0"""
    m = np.asarray(mask)
    m = m if m.ndim == 2 else m[..., 0]
    h, w = m.shape
    sy = ((2 * np.arange(rows, dtype=np.int64) + 1) * h) // (2 * rows)
    sx = ((2 * np.arange(is_, dtype=np.int64) + 1) * w) // (2 * is_)
    return m[sy][:, sx]


def score(fidx, rows, F, nf_body, nf_obj, pm, om, thres=127):
    """fidx (is,is) owners, pm / om masks -> (2,4) int64: per class inter, fit, mask, hidden"""
    is_ = fidx.shape[1]
    cls = classes(fidx[:rows], F, nf_body, nf_obj)
    out = np.zeros((2, 4), np.int64)
    for c, m in enumerate((pm, om)):
        on = sample(m, rows, is_).astype(np.int64) > thres
        out[c] = ((cls == c) & on).sum(), (cls == c).sum(), on.sum(), (on & (cls == 1 - c)).sum()
    return out


def iou(count):
    c = np.asarray(count).astype(np.int64)
    union = c[..., 1] + c[..., 2] - c[..., 0]
    return np.where(union > 0, c[..., 0] / np.maximum(union, 1), np.nan)


def masks_of_owners(fidx, rows, F, nf_body, nf_obj):
    """(rows, is) uint8 masks that are on exactly where the owner is body / object"""
    cls = classes(fidx[:rows], F, nf_body, nf_obj)
    return ((cls == 0) * 255).astype(np.uint8), ((cls == 1) * 255).astype(np.uint8)


def random_owners(rng, is_, F, nf_body, nf_obj):
    """an (is,is) owner map with every kind of id: faces, their reversed copies [F, 2 F), -1, a third face range (neither class), ids >= 2 F"""
    kind = rng.integers(0, 6, (is_, is_))
    face = rng.integers(0, F, (is_, is_))
    third = rng.integers(nf_body + nf_obj, F, (is_, is_))
    d = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4], [face, F + face, -1, third + F * rng.integers(0, 2, (is_, is_)), 2 * F + face], face)
    d[0, 0], d[0, 1], d[1, 0] = 2 * F, 2 * F - 1, 0x7fffffff
    return d.astype(np.int32)


def random_mask(rng, h, w, c=None):
    """values around the threshold as well as 0 / 255"""
    m = rng.choice(np.array([0, 255, 127, 128, 1, 200], np.uint8), (h, w) if c is None else (h, w, c))
    return np.ascontiguousarray(m)
