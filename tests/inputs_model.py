"""Test helper (not a test file): the crop + bilinear resize + rounding contract of csrc/inputs.hip restated in exact integer arithmetic, and the seeded
frames the host and GPU tests of the network inputs share.

Per axis the crop has n = br - tl pixels (tl, br rounded as data/base_data.py:204-233 rounds them) and output pixel d samples the crop at
src = n / S * (d + 0.5) - 0.5 = (n (2 d + 1) - S) / (2 S), clamped at 0: tap weights are integers over 2 S, the blend of the four uint8 taps is an integer V
over D = (2 S)^2, and rounding to the nearest grey level, floor(V / D + 1 / 2), is (2 V + D) // (2 D).  No floating point anywhere.
"""
from __future__ import annotations

import numpy as np


def corners(center, crop_size):
    """tl, br of the crop around ``center``: numpy's round (halves to even), as the reference rounds them"""
    c = np.asarray(center, np.float64)
    return np.round(c - crop_size / 2).astype(np.int64), np.round(c + crop_size / 2).astype(np.int64)


def padded_crop(img, tl, br):
    """the crop as int64: image pixels x in [max(0, tl.x), min(W - 1, br.x)), y likewise (the last image column / row is dropped when the crop reaches it), 0 elsewhere"""
    h, w = img.shape[:2]
    out = np.zeros((int(br[1] - tl[1]), int(br[0] - tl[0])) + img.shape[2:], np.int64)
    x1, y1, x2, y2 = max(0, int(tl[0])), max(0, int(tl[1])), min(w - 1, int(br[0])), min(h - 1, int(br[1]))
    if x2 > x1 and y2 > y1:
        out[y1 - tl[1]:y2 - tl[1], x1 - tl[0]:x2 - tl[0]] = img[y1:y2, x1:x2]
    return out


def axis_taps(n, S):
    """i0, i1 (S,) and the integer weights w0, w1 over 2 S of every output index of an axis with n crop pixels"""
    num = np.maximum(n * (2 * np.arange(S, dtype=np.int64) + 1) - S, 0)          # src * 2 S
    i0 = np.minimum(num // (2 * S), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    w1 = np.clip(num - i0 * 2 * S, 0, 2 * S)
    return i0, i1, 2 * S - w1, w1


def crop_resize(img, center, crop_size, S):
    """uint8 image (H,W) or (H,W,C) -> (grey levels (S,S[,C]) uint8, distance (S,S[,C]) of the exact blend from the nearest half-way point, in grey levels)"""
    tl, br = corners(center, crop_size)
    c = padded_crop(np.asarray(img), tl, br)
    ix0, ix1, wx0, wx1 = axis_taps(c.shape[1], S)
    iy0, iy1, wy0, wy1 = axis_taps(c.shape[0], S)
    ex = (lambda a: a[..., None]) if c.ndim == 3 else (lambda a: a)
    row = lambda iy: c[iy][:, ix0] * ex(wx0[None, :]) + c[iy][:, ix1] * ex(wx1[None, :])
    V = row(iy0) * ex(wy0[:, None]) + row(iy1) * ex(wy1[:, None])
    D = (2 * S) ** 2
    q = np.clip((2 * V + D) // (2 * D), 0, 255).astype(np.uint8)
    r = (2 * V + D) % (2 * D)
    return q, np.minimum(r, 2 * D - r) / (2 * D)


def compose(q_rgb, q_pm, q_om, table):
    """(5,S,S) float32 from grey levels: rgb * (pm >= 128 | om >= 128), pm, om, each through the / 255 table"""
    comb = (q_pm >= 128) | (q_om >= 128)
    return np.concatenate([table[np.where(comb[..., None], q_rgb, 0)].transpose(2, 0, 1), table[q_pm][None], table[q_om][None]], 0)


def frames(seed, B, H, W):
    """seeded test frames: random rgb (B,H,W,3); masks (B,H,W) of 0 / 255 blocks with grey ramps at the block borders and a sprinkle of 127 / 128, so
    that resized values on both sides of the 127 / 128 threshold of the composition occur"""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    masks = []
    for _ in range(2):
        m = np.zeros((B, H, W), np.uint8)
        for b in range(B):
            y0, x0 = int(rng.integers(0, H // 2)), int(rng.integers(0, W // 2))
            m[b, y0:y0 + H // 2, x0:x0 + W // 2] = 255
            m[b, y0:y0 + H // 2, x0:x0 + 4] = np.array([40, 100, 127, 128], np.uint8)
            m[b, y0:y0 + 3, x0:x0 + W // 2] = np.array([90, 128, 200], np.uint8)[:, None]
            m[b, y0 + 8:y0 + 14, x0:x0 + W // 2] = 127; m[b, y0 + 16:y0 + 22, x0:x0 + W // 2] = 128          # bands wide enough for all four taps
        grey = rng.random((B, H, W)) < 0.05
        m[grey] = rng.choice(np.array([127, 128, 1, 254], np.uint8), int(grey.sum()))
        masks.append(m)
    return rgb, masks[0], masks[1]
