"""CPU: the float64 model of tests/dectrain_model.py against the reference's recorded predictions and autograd gradients (tests/golden/dectrain.npz), and what
of ops.DecoderParams needs no device: the flat layout as the library states it, the state_dict keys and shapes, the round trips."""
import numpy as np
import pytest
import torch

import dectrain_model as M
from conftest import golden

B, N = 2, 150


@pytest.fixture(scope="module")
def case():
    from vistracker_amd import synthetic as syn
    g = golden("dectrain")
    dec, maps = syn.sifnet_decoders(3), syn.feature_maps(B, res_scale=0.125)
    up = {h: g["up_" + h] for h in M.HEADS}
    return g, dec, maps, up, M.run(dec, [maps], g["pts"], g["cc"], g["bc"], upstream=[up])


def test_inputs_regenerate_from_their_seeds(case):
    g = case[0]
    pts, cc, bc = M.make_inputs(B, N, seed=11)
    assert np.array_equal(pts, g["pts"]) and np.array_equal(cc, g["cc"]) and np.array_equal(bc, g["bc"])
    up = M.make_upstream(B, N, seed=12)
    assert all(np.array_equal(up[h], g["up_" + h]) for h in M.HEADS)
    assert tuple(g["rows"]) == M.GOLDEN_ROWS


def test_model_matches_the_recorded_reference(case):
    """the reference ran in float32: the float64 model is within float32 round-off of it, relative to each tensor's largest element"""
    g, _, _, _, r64 = case
    for i, h in enumerate(M.HEADS):
        np.testing.assert_allclose(g["pred_" + h], r64["preds"][0][i], atol=5e-5, rtol=0)
        for l in range(4):
            for kind in ("weight", "bias"):
                want = r64["grads"][(h, l, kind)]
                sub = want[list(M.GOLDEN_ROWS)] if kind == "weight" and l < 3 else want
                got = g[f"g_{h}_{l}_{kind}"]
                assert got.shape == sub.shape
                assert np.abs(got - sub).max() <= 2e-5 * np.abs(want).max(), (h, l, kind)


def test_model_point_classes_and_df_override(case):
    g, _, maps, _, r64 = case
    cls = M.point_classes(maps, g["pts"], g["cc"], g["bc"])
    for k in ("outside_image", "outside_right", "outside_back", "outside_top", "exact_texel", "bulk"):
        assert cls[k].any(), k
    assert cls["bulk"].mean() > 0.7
    out = cls["outside_image"]
    df = r64["preds"][0][0]
    assert (df.transpose(0, 2, 1)[out] == M.OUT_DIST).all() and (df.transpose(0, 2, 1)[~out] != M.OUT_DIST).all()
    assert cls["outside_image"][:, 128:].any() and cls["exact_texel"][:, 128:].any()          # the ragged last tile holds special points too


def test_bilinear_is_grid_sample():
    """the hand-written sampler against F.grid_sample(align_corners=True, padding_mode='zeros'), in float64"""
    rng = np.random.default_rng(0)
    m = torch.tensor(rng.normal(size=(2, 3, 7, 7)))
    uv = torch.tensor(rng.uniform(-1.4, 1.4, (2, 50, 2)))
    uv[0, 0] = torch.tensor([-1.0, 1.0]); uv[0, 1] = torch.tensor([1.0, 0.0])
    want = torch.nn.functional.grid_sample(m, uv[:, :, None, :], mode="bilinear", padding_mode="zeros", align_corners=True)[..., 0]
    np.testing.assert_allclose(M.bilinear(m, uv[..., 0], uv[..., 1]).numpy(), want.numpy(), atol=1e-13)


def test_flat_layout_and_state_dict_round_trip():
    from vistracker_amd import _lib as L, ops
    from vistracker_amd.sifnet import SIFNetQuery
    from vistracker_amd import synthetic as syn
    lib = L.lib()
    n = lib.vt_decoder_param_floats()
    assert n == sum(128 * 611 + 128 + 2 * (128 * 128 + 128) + k * 128 + k for k in M.DIMS)
    # the offsets tile [0, n) in head, layer, weight-then-bias order
    at = 0
    for h, k in enumerate(M.DIMS):
        for l in range(4):
            out, inn = (k if l == 3 else 128), (611 if l == 0 else 128)
            assert lib.vt_decoder_param_offset(h, l, 0) == at; at += out * inn
            assert lib.vt_decoder_param_offset(h, l, 1) == at; at += out
    assert at == n
    assert lib.vt_decoder_param_offset(5, 0, 0) == -1 and lib.vt_decoder_param_offset(0, 4, 0) == -1 and lib.vt_decoder_param_offset(-1, 0, 1) == -1
    assert lib.vt_decoder_weight_grads_ws_bytes(0, 5, 0) == -1 and lib.vt_decoder_weight_grads_ws_bytes(2, 150, 100) == -1
    assert lib.vt_decoder_weight_grads_ws_bytes(65536, 5, 0) == -1 and lib.vt_decoder_weight_grads_ws_bytes(2, 150, 64) > 0
    dec = syn.sifnet_decoders(3)
    p = ops.DecoderParams.from_decoders(dec, device="cpu")
    assert p.flat.requires_grad and p.flat.is_leaf and tuple(p.flat.shape) == (n,) and len(p.views) == 40
    for name in M.HEADS:
        for l, (w, b) in enumerate(dec[name]):
            o = lib.vt_decoder_param_offset(M.HEADS.index(name), l, 0)
            assert np.array_equal(p.flat.detach().numpy()[o:o + w.size].reshape(w.shape), w)
            assert np.array_equal(p.views[(name, l, "bias")].numpy(), b)
    back = p.to_decoders()
    for name in M.HEADS:
        for (w, b), (w2, b2) in zip(dec[name], back[name]):
            assert np.array_equal(w, w2) and np.array_equal(b, b2) and w2.dtype == np.float32
    sd = p.state_dict()
    assert len(sd) == 40 and tuple(sd["df.0.weight"].shape) == (128, 611, 1) and tuple(sd["df.0.bias"].shape) == (128,)
    assert tuple(sd["pca_predictor.6.weight"].shape) == (9, 128, 1) and tuple(sd["part_predictor.6.bias"].shape) == (14,)
    assert tuple(sd["center_predictor.4.weight"].shape) == (128, 128, 1) and tuple(sd["visib_predictor.6.weight"].shape) == (1, 128, 1)
    assert set(k.split(".")[0] for k in sd) == {"df", "pca_predictor", "part_predictor", "center_predictor", "visib_predictor"}
    # identity, bit for bit; with the module. prefix and foreign keys as a reference checkpoint carries them; and the way into SIFNetQuery's host form
    q = ops.DecoderParams(torch.zeros(n))
    q.load_state_dict({"module." + k: v for k, v in sd.items()} | {"module.image_filter.conv1.weight": torch.zeros(3)})
    assert torch.equal(q.flat, p.flat)
    assert all(torch.equal(a, b) for a, b in zip(q.load_state_dict(q.state_dict()).state_dict().values(), sd.values()))
    host = SIFNetQuery.decoders_from_state_dict(p.state_dict("module."))
    for name in M.HEADS:
        for (w, b), (w2, b2) in zip(dec[name], host[name]):
            assert np.array_equal(w, w2) and np.array_equal(b, b2)
    with pytest.raises(KeyError):
        q.load_state_dict({k: v for k, v in sd.items() if k != "df.2.bias"})
    with pytest.raises(L.VtError):
        ops.DecoderParams(torch.zeros(n - 1))


def test_no_cpu_path():
    from vistracker_amd import _lib as L, ops
    from vistracker_amd import synthetic as syn
    p = ops.DecoderParams.from_decoders(syn.sifnet_decoders(3), device="cpu")
    with pytest.raises(L.VtError):
        ops.sifnet_query_train(p, [], torch.zeros(1, 4, 3), torch.zeros(1, 2), torch.zeros(1, 3))
