"""CPU: the float64 map gradients of tests/mapgrad_model.py (the hand-written bilinear sampler under autograd) against torch's own
F.grid_sample(align_corners=True, padding_mode="zeros") autograd in float64, on the inputs every GPU test of the map gradient uses -- the points outside the
image, outside each plane and on exact texel coordinates included; the recorded reference gradients (tests/golden/mapgrad.npz) against the model; and the two
new entries of the C ABI."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dectrain_model as M
import mapgrad_model as G
from conftest import golden

B, N = 2, 150


@pytest.fixture(scope="module")
def case():
    from vistracker_amd import synthetic as syn
    dec, maps = syn.sifnet_decoders(3), syn.feature_maps(B, res_scale=0.125)
    pts, cc, bc = M.make_inputs(B, N, 11)
    up = M.make_upstream(B, N, seed=12)
    return dec, maps, pts, cc, bc, up, G.run(dec, [maps], pts, cc, bc, upstream=[up])


def test_model_map_gradients_are_grid_sample_autograd(case):
    dec, maps, pts, cc, bc, up, r64 = case
    cls = M.point_classes(maps, pts, cc, bc)
    for k in ("outside_image", "outside_right", "outside_back", "outside_top", "exact_texel", "bulk"):
        assert cls[k].any(), k
    dt = torch.float64
    params = M.make_params(dec, dt)
    p, c, b = M._t(pts, dt), M._t(cc, dt), M._t(bc, dt)
    pr = M.projections(p, c, b)
    leaves = {n: M._t(maps[n], dt).clone().requires_grad_(True) for n in G.MAPS}
    cols = []
    for name, kind in M.CONCAT:
        if kind is None:
            cols.append(torch.stack([p[..., 0], p[..., 1], p[..., 2] - 2.2], 1))
        else:
            grid = torch.stack(pr[kind], -1)[:, :, None, :]
            cols.append(torch.nn.functional.grid_sample(leaves[name], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[..., 0])
    u, v = pr["persp"]
    preds = M.decode(params, torch.cat(cols, 1), (u >= -1) & (u <= 1) & (v >= -1) & (v <= 1))
    sum((preds[M.HEADS.index(h)] * M._t(g, dt)).sum() for h, g in up.items()).backward()
    for n in G.MAPS:
        want, got = leaves[n].grad.numpy(), r64["dmaps"][0][n]
        assert np.abs(want).max() > 0
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), n


def test_recorded_reference_map_gradients(case):
    """the reference ran in float32: its autograd map gradients are within float32 round-off of the float64 model, relative to each tensor's largest element.
    The file stores the touched texel rows of every map (index + every third channel); every other row is an exact zero there and of round-off size in the model."""
    g = golden("mapgrad")
    dec, maps, pts, cc, bc, up, r64 = case
    assert np.array_equal(g["pts"], pts) and np.array_equal(g["cc"], cc) and np.array_equal(g["bc"], bc)
    for n in G.MAPS:
        want = r64["dmaps"][0][n]
        C, R = want.shape[1], want.shape[2]
        rows = want.transpose(0, 2, 3, 1).reshape(-1, C)
        idx, val = g["idx_" + n], g["val_" + n]
        assert val.shape == (len(idx), len(range(0, C, G.GOLDEN_CHANNEL_STEP)))
        assert np.abs(val - rows[idx][:, ::G.GOLDEN_CHANNEL_STEP]).max() <= 2e-5 * np.abs(rows).max(), n
        untouched = np.ones(len(rows), bool); untouched[idx] = False
        # a texel coordinate that is an integer in float32 need not be one in float64: the model may put a weight of round-off size on a neighbour
        assert np.abs(rows[untouched]).max(initial=0.0) <= 2e-5 * np.abs(rows).max(), n


def test_library_exports_the_map_gradient_entries():
    from vistracker_amd import _lib
    assert os.path.exists(_lib.LIB_PATH)
    l = ctypes.CDLL(_lib.LIB_PATH)
    for s in ("vt_decoder_grads", "vt_decoder_grads_ws_bytes"):
        assert hasattr(l, s) and s in _lib.SIGNATURES, s
    lib = _lib.lib()
    assert lib.vt_decoder_grads_ws_bytes(2, 150, 0, 0) == lib.vt_decoder_weight_grads_ws_bytes(2, 150, 0)
    assert lib.vt_decoder_grads_ws_bytes(2, 150, 0, 1) > lib.vt_decoder_grads_ws_bytes(2, 150, 0, 0)
    assert lib.vt_decoder_grads_ws_bytes(2, 150, 100, 1) == -1 and lib.vt_decoder_grads_ws_bytes(0, 150, 0, 1) == -1
