"""CPU: the float64 model of SIF-Net's training objective (tests/losshead_model.py) against the reference's own float32 values and autograd gradients
(tests/golden/losshead.npz, tools/gen_golden_losshead.py), and the argument errors of the Python shim that need no GPU.

The golden is a float32 evaluation, the model a float64 one, so they differ by the golden's rounding (u = 2^-24 per operation):
* a loss is a mean of non-negative float32 summands, each the result of at most 5 rounded operations, added up by torch in float32 (at most B 9 N = 8991
  summands: a blocked sum, error below (log2(8991) + 8) u of the sum), then weighted and averaged over the stacks (3 more): below 32 u RELATIVE to the value;
* a gradient element is a product of at most 6 rounded factors; the softmax's (p - onehot) cancels, so its error is relative to 1 x the element's factor,
  not to the element: below 8 u of the tensor's largest magnitude.
"""
import numpy as np
import pytest
import torch

import losshead_model as M
from conftest import golden

U = 2.0 ** -24
CASES, golden_case = M.CASES, M.golden_case


@pytest.mark.parametrize("S,vis_loss", CASES)
def test_model_matches_the_reference(S, vis_loss):
    args, kw, want = golden_case(golden("losshead"), S, vis_loss)
    got = M.loss_head(*args, **kw)
    np.testing.assert_allclose(got["losses_all"], want["losses_all"], rtol=32 * U, atol=0)
    np.testing.assert_allclose(got["error"], want["error"], rtol=32 * U, atol=0)
    for k in ("d_df", "d_pca", "d_parts", "d_centers", "d_vis"):
        assert got[k].shape == want[k].shape
        err = np.abs(got[k] - want[k]).max()
        print(f"S = {S} {vis_loss} {k}: max |model - golden| = {err:.3e}, bound {8 * U * np.abs(want[k]).max():.3e}")
        assert err <= 8 * U * np.abs(want[k]).max()
        assert np.array_equal(got[k] == 0, want[k] == 0)                # the same elements carry no gradient: clamp, mask and sign(0) agree exactly


def test_golden_covers_the_edges():
    g = golden("losshead")
    md, df, df_h, df_o = float(g["max_dist"]), g["df"].astype(np.float32), g["df_h"], g["df_o"]
    assert (df_h > md).any() and (df_h < md).any() and (df[:, :, 0] > md).any() and (df[:, :, 0] < md).any()
    assert (df_o < np.float32(0.05)).any() and (df_o > np.float32(0.05)).any() and (df_o == np.float32(0.05)).any()
    assert (df[:, :, 0] == md).any() and (df[:, :, 0] == df_h[None]).any()
    d_df = g["S3_d_df"]
    at_md = (df[:, :, 0] == md) & (df_h[None] < md)                       # p == max_dist with the label below it: |p - g| > 0 and the gradient passes
    assert at_md.any() and (d_df[:, :, 0][at_md] > 0).all()
    assert (d_df[:, :, 0][df[:, :, 0] > md] == 0).all()
    assert (d_df[:, :, 0][df[:, :, 0] == df_h[None]] == 0).all()          # sign(0) = 0
    assert (g["S3_d_pca"][:, :, :, 5] == 0).all()                         # df_o == 0.05 exactly is masked out ...
    assert (g["S3_d_pca"][:, :, :, 6] != 0).any()                         # ... the float below it is not


def test_float32_run_of_the_model_is_close_to_the_float64_run():
    args, kw, _ = golden_case(golden("losshead"), 3, "l2")
    r64, e32 = M.reference_and_e32(*args, **kw)
    assert (e32["losses_all"] <= 32 * U * r64["losses_all"]).all()
    for k in ("d_df", "d_pca", "d_parts", "d_centers", "d_vis"):
        assert e32[k] <= 8 * U * np.abs(r64[k]).max()


def test_shim_argument_errors():
    from vistracker_amd import _lib as L, ops, training
    assert "vt_sifnet_loss_head" in L.SIGNATURES and "vt_sifnet_loss_head_ws_bytes" in L.SIGNATURES
    B, N = 2, 5
    preds = tuple(torch.zeros(B, k, N) for k in ops.HEAD_DIMS)
    labels = (torch.zeros(B, N), torch.zeros(B, N), torch.zeros(B, N, dtype=torch.int32), torch.zeros(B, 9), torch.zeros(B, 3), torch.zeros(B))
    with pytest.raises(L.VtError):
        ops.sifnet_loss_head([preds], *labels)                         # host tensors: no CPU path
    with pytest.raises(L.VtError):
        ops.sifnet_loss_head(preds, *labels)
    with pytest.raises(L.VtError):
        ops.sifnet_loss_head([], *labels)
    with pytest.raises(L.VtError):
        ops.sifnet_loss_head([preds[:4]], *labels)
    with pytest.raises(L.VtError):
        ops.sifnet_loss_head(preds[:4], *labels)
    assert ops.LOSS_SLOTS == M.SLOTS and ops.LOSS_SLOT_WEIGHT == M.SLOT_WEIGHT and ops.LOSS_WEIGHTS == M.WEIGHTS
    # the reference's sampling set-up (config/tri-vis-l2.json: 20000 samples, ratios 0.01 / 0.49 / 0.5) adds up; one that does not is an error
    assert training.sample_counts([0.01, 0.49, 0.5], 20000) == (200, [198, 9702, 9900])
    assert training.sample_counts([0.2, 0.8], 500) == (5, [99, 396])
    with pytest.raises(L.VtError):
        training.sample_counts([0.5, 0.5], 500)                        # 5 + 247 + 247 = 499
