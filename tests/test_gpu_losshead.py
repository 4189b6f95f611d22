"""GPU: vt_sifnet_loss_head (csrc/losshead.hip), SIFNetQuery.get_errors and vistracker_amd.training against the float64 model of tests/losshead_model.py and the
reference's recorded values (tests/golden/losshead.npz).

The bound of every comparison is MEASURED, not chosen: e32 = the float32 run of the objective against its float64 run on the inputs of the test, per output
(per slot for the six losses, the largest element error for a gradient tensor), and the kernel gets 4 e32 -- the convention of tests/test_gpu_boundary.py.  For
the recorded cases the float32 run is the reference's own (the golden), otherwise the model's.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import losshead_model as M
from conftest import golden

pytestmark = pytest.mark.gpu
GRADS = tuple("d_" + h for h in M.HEADS)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def make_case(S, B, N, seed=0, md=0.5):
    """float32 inputs with distances on both sides of max_dist and df_o on both sides of 0.05; per-frame pca_gt, obj_center, visibility"""
    rng = np.random.default_rng(seed)
    df_h = rng.uniform(0.0, 2 * md, (B, N)).astype(np.float32)
    df_o = np.where(rng.random((B, N)) < 0.5, rng.uniform(0.0, 0.05, (B, N)), rng.uniform(0.05, 2 * md, (B, N))).astype(np.float32)
    c = {"df_h": df_h, "df_o": df_o, "parts_gt": rng.integers(0, 14, (B, N)).astype(np.int32),
         "pca_gt": np.linalg.qr(rng.normal(size=(B, 3, 3)))[0].reshape(B, 9).astype(np.float32), "obj_center": rng.normal(0, 0.4, (B, 3)).astype(np.float32),
         "visibility": rng.uniform(0.1, 1.0, (B,)).astype(np.float32), "max_dist": md,
         "df": (np.stack([df_h, df_o], 1)[None] + rng.normal(0, 0.2, (S, B, 2, N))).astype(np.float32),
         "parts": rng.normal(0, 3.0, (S, B, 14, N)).astype(np.float32), "vis": rng.uniform(0, 1, (S, B, 1, N)).astype(np.float32)}
    c["pca"] = (c["pca_gt"][None, :, :, None] + rng.normal(0, 0.3, (S, B, 9, N))).astype(np.float32)
    c["centers"] = (c["obj_center"][None, :, :, None] + rng.normal(0, 0.2, (S, B, 3, N))).astype(np.float32)
    return c


def model_args(c):
    N = c["df"].shape[-1]
    return ([c[h] for h in M.HEADS], c["df_h"], c["df_o"], c["parts_gt"], *M.per_point((c["pca_gt"], c["obj_center"], c["visibility"]), N), c["max_dist"])


def run_kernel(c, vis_loss="l2", weights=M.WEIGHTS, per_frame=True, grads=True):
    """the op on a case -> dict of numpy arrays: terms, losses_all, error and (with ``grads``) d_df .. d_vis through autograd"""
    from vistracker_amd import ops
    N = c["df"].shape[-1]
    heads = [dev(c[h]).requires_grad_(grads) for h in M.HEADS]
    lab = (c["pca_gt"], c["obj_center"], c["visibility"]) if per_frame else M.per_point((c["pca_gt"], c["obj_center"], c["visibility"]), N)
    error, losses_all, terms = ops.sifnet_loss_head(heads, dev(c["df_h"]), dev(c["df_o"]), dev(c["parts_gt"], torch.int32), *[dev(a) for a in lab],
                                                    max_dist=c["max_dist"], weights=weights, vis_loss=vis_loss, want_terms=True)
    assert error.dtype == torch.float64 and losses_all.dtype == torch.float64 and tuple(losses_all.shape) == (6,)
    out = {"terms": terms.cpu().numpy(), "losses_all": losses_all.detach().cpu().numpy(), "error": float(error.detach())}
    if grads:
        error.backward()
        out.update({"d_" + h: t.grad.cpu().numpy() for h, t in zip(M.HEADS, heads)})
    else:
        assert not error.requires_grad
    return out


def check(got, ref, e32, what, outputs=M.OUTPUTS):
    lines = []
    for k in outputs:
        assert np.isfinite(got[k]).all(), (what, k)
        err = np.abs(np.asarray(got[k], np.float64) - ref[k])
        bound = 4 * np.asarray(e32[k])
        lines.append(f"{k}: e32 {np.max(e32[k]):.2e} kernel {err.max():.2e}")
        assert (err.reshape(-1, *np.shape(bound)) <= bound).all(), (what, k, err.max(), bound)
    print(f"\n[{what}] " + "; ".join(lines))


# ---- 1: the reference's recorded values ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,vis_loss", M.CASES)
def test_golden_parity(S, vis_loss):
    """|kernel - golden| <= 4 e32 with e32 = |golden - float64 model|: the reference's own float32 error on these inputs"""
    g = golden("losshead")
    args, kw, want = M.golden_case(g, S, vis_loss)
    r64 = M.loss_head(*args, **kw)
    c = {k: g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k] for k in g}
    c.update({h: c[h][:S] for h in M.HEADS}); c["max_dist"] = float(g["max_dist"])
    got = run_kernel(c, vis_loss=vis_loss, weights=tuple(g["weights"]))
    for k in ("losses_all", "error") + GRADS:
        w = np.asarray(want[k], np.float64)
        e32 = np.abs(w - r64[k]) if k == "losses_all" else np.abs(w - r64[k]).max()
        err = np.abs(np.asarray(got[k], np.float64) - w)
        print(f"\n[golden S = {S} {vis_loss}] {k}: e32 {np.max(e32):.3e}, |kernel - golden| {err.max():.3e}, |kernel - model| {np.abs(got[k] - r64[k]).max():.3e}")
        assert (err.reshape(-1, *np.shape(e32)) <= 4 * e32).all(), (k, err.max(), e32)


# ---- 2: shapes -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1027])
def test_shapes_against_the_model(N, B, S):
    c = make_case(S, B, N, seed=1000 * N + 10 * B + S)
    vis_loss = "l1" if (N + B + S) % 2 else "l2"
    ref, e32 = M.reference_and_e32(*model_args(c), vis_loss=vis_loss)
    check(run_kernel(c, vis_loss=vis_loss, per_frame=bool(N % 2)), ref, e32, f"N = {N} B = {B} S = {S} {vis_loss}")


# ---- 3: crafted edges ----------------------------------------------------------------------------------------------------------------------------------------
def test_crafted_edges():
    S, B, N, md = 2, 2, 70, 0.5
    c = make_case(S, B, N, seed=3, md=md)
    c["df"][:, :, 0, 0] = 0.25; c["df_h"][:, 0] = 0.25                            # p == g: sign(0) = 0
    c["df"][:, :, 0, 1] = md; c["df_h"][:, 1] = 0.125                             # p == max_dist exactly, the label below: the gradient passes
    c["df"][:, :, 0, 2] = np.nextafter(np.float32(md), np.float32(1)); c["df_h"][:, 2] = 0.125      # the float above max_dist: clamped, no gradient
    c["df"][:, :, 1, 3] = 0.75; c["df_o"][:, 3] = 0.875                           # both beyond max_dist: zero value, zero gradient
    c["df_o"][:, 4] = np.float32(0.05)                                            # exactly the threshold: masked out (strict <)
    c["df_o"][:, 5] = np.nextafter(np.float32(0.05), np.float32(0))               # the float below: in
    c["parts"][:, :, :, 6] = 80.0; c["parts"][:, :, 3, 6] = -80.0; c["parts"][:, :, 5, 7] = 80.0; c["parts"][:, :, :5, 7] = -80.0
    c["parts_gt"][:, 6] = 3; c["parts_gt"][:, 7] = 5                              # the label on the -80 logit (loss 160 + log 13) and on the +80 one (loss ~ 0)
    ref, e32 = M.reference_and_e32(*model_args(c), vis_loss="l1")
    got = run_kernel(c, vis_loss="l1")
    check(got, ref, e32, "crafted edges")
    g0 = np.float32(1.0 / (B * S))
    d = got["d_df"]
    assert (d[:, :, 0, 0] == 0).all() and (d[:, :, 0, 1] == g0).all() and (d[:, :, 0, 2] == 0).all() and (d[:, :, 1, 3] == 0).all()
    for k in ("d_pca", "d_centers", "d_vis"):
        assert (got[k][..., 4] == 0).all() and (got[k][..., 5] != 0).all()
    assert np.abs(got["d_parts"][:, :, :, 7]).max() < 1e-30                         # softmax within 1e-30 of onehot: no gradient to speak of, no NaN
    # an all-false mask: exactly zero masked terms and gradients
    c2 = dict(c); c2["df_o"] = np.maximum(c["df_o"], np.float32(0.05))
    got2 = run_kernel(c2)
    assert (got2["terms"][3:] == 0).all() and got2["terms"][:3].min() > 0
    for k in ("d_pca", "d_centers", "d_vis"):
        assert (got2[k] == 0).all()
    assert np.isfinite(got2["d_df"]).all() and np.isfinite(got2["d_parts"]).all()
    # part labels outside [0, 14) are clamped: the call completes and equals, bit for bit, the call with the clamped labels -- every other point included
    bad, ok = dict(c), dict(c)
    bad["parts_gt"] = c["parts_gt"].copy(); bad["parts_gt"][:, 10] = -1; bad["parts_gt"][:, 11] = 14; bad["parts_gt"][0, 12] = 2 ** 31 - 1
    ok["parts_gt"] = np.clip(bad["parts_gt"], 0, 13)
    gb, gk = run_kernel(bad), run_kernel(ok)
    for k in M.OUTPUTS:
        assert np.array_equal(gb[k], gk[k]), k
    from vistracker_amd import _lib as L, ops
    with pytest.raises(L.VtError):                                                  # ... and the shim rejects them on request
        ops.sifnet_loss_head([dev(c[h]) for h in M.HEADS], dev(c["df_h"]), dev(c["df_o"]), dev(bad["parts_gt"], torch.int32), dev(c["pca_gt"]),
                             dev(c["obj_center"]), dev(c["visibility"]), validate=True)
    assert L.lib().vt_sifnet_loss_head_ws_bytes(0, 5) == -1 and L.lib().vt_sifnet_loss_head_ws_bytes(2, 257) == 2 * 2 * 48


# ---- 4: determinism ------------------------------------------------------------------------------------------------------------------------------------------
def test_determinism_and_label_forms():
    c = make_case(3, 2, 1027, seed=4)
    a, b = run_kernel(c), run_kernel(c)
    for k in M.OUTPUTS:
        assert np.array_equal(a[k], b[k]), k                                        # two calls: the same bits
    nograd = run_kernel(c, grads=False)                                             # all five gradient pointers NULL
    assert np.array_equal(nograd["terms"], a["terms"]) and nograd["error"] == a["error"]
    pp = run_kernel(c, per_frame=False)                                             # per-point labels: the same bits as per-frame ones
    for k in M.OUTPUTS:
        assert np.array_equal(pp[k], a[k]), k
    # one gradient pointer at a time: only that head's gradient is computed, with the same bits
    from vistracker_amd import ops
    heads = [dev(c[h]) for h in M.HEADS]; heads[2].requires_grad_(True)
    err, _ = ops.sifnet_loss_head(heads, dev(c["df_h"]), dev(c["df_o"]), dev(c["parts_gt"], torch.int32), dev(c["pca_gt"]), dev(c["obj_center"]),
                                  dev(c["visibility"]), max_dist=c["max_dist"])
    (2.0 * err).backward()
    assert float(err.detach()) == a["error"] and np.array_equal(heads[2].grad.cpu().numpy(), 2 * a["d_parts"])       # the incoming gradient scales it (x2 is exact)


# ---- 5: autograd through the query ---------------------------------------------------------------------------------------------------------------------------
def torch_get_errors(preds, df_h, df_o, parts_gt, pca_gt, max_dist, obj_center, vis_gt, weights, vis_loss, dtype):
    """the expression of get_errors (chore_tri_vis.py:52-99) for one stack in torch, in ``dtype``, per-point labels -> losses_all (6,)"""
    import torch.nn.functional as F
    df, pca, parts, centers, vis = (t.to(dtype) for t in preds)
    df_h, df_o, pca_gt, obj_center, vis_gt = (t.to(dtype) for t in (df_h, df_o, pca_gt, obj_center, vis_gt))
    dfl = lambda g, p: F.l1_loss(torch.clamp(p, max=max_dist), torch.clamp(g, max=max_dist), reduction="none").sum(-1).mean()      # noqa: E731
    loss_h, loss_o = dfl(df_h, df[:, 0]) * weights[0], dfl(df_o, df[:, 1]) * weights[1]
    loss_parts = (F.cross_entropy(parts, parts_gt.long(), reduction="none") * weights[2]).sum(-1).mean()
    mask_o = (df_o < 0.05).unsqueeze(1)
    loss_pca = ((F.mse_loss(pca, pca_gt, reduction="none") * mask_o) * weights[3]).mean()        # pca as (B,9,N): the mask broadcasts over the 9
    loss_obj = (F.mse_loss(centers, obj_center, reduction="none") * mask_o).mean() * weights[4]
    fn = F.l1_loss if vis_loss == "l1" else F.mse_loss
    loss_vis = (fn(vis, vis_gt.unsqueeze(1), reduction="none") * mask_o).mean() * weights[5]
    return torch.stack([loss_h, loss_o, loss_parts, loss_pca, loss_vis, loss_obj])


def test_get_errors_reaches_the_points(synth):
    from vistracker_amd import _lib as L, ops, synthetic as syn
    from vistracker_amd.sifnet import SIFNetQuery
    B, N = 2, 300
    net = SIFNetQuery(synth["decoders"])
    net.set_feature_maps(syn.feature_maps(B, 4, res_scale=1 / 8))
    assert net.loss_weights == [1.0, 1.0, 0.006, 500, 1000, 1000] and net.vis_loss_name == "l2" and net.error_buffer is None
    c = make_case(1, B, N, seed=5, md=5.0)
    rng = np.random.default_rng(6)
    pts = dev(rng.normal(0, 0.25, (B, N, 3)) + [0, 0, 2.2]).requires_grad_(True)
    cc = dev([[1018.952, 779.486]] * B); bc = dev([[0, 0, 2.2]] * B)
    lab = M.per_point((c["pca_gt"], c["obj_center"], c["visibility"]), N)
    df_h, df_o, parts_gt = dev(c["df_h"]), dev(c["df_o"]), dev(c["parts_gt"])                    # parts_gt float, as the reference's loader delivers it
    pca_gt, oc, vg = dev(lab[0]).view(B, 3, 3, N), dev(lab[1]), dev(lab[2])
    net.query(pts, crop_center=cc, body_center=bc)
    assert len(net.intermediate_preds_list) == 1 and net.intermediate_preds_list[0] is net.preds
    error, losses_all = net.get_errors(df_h, df_o, parts_gt, pca_gt, 5.0, bc, oc, visibility=vg)
    assert net.error_buffer is losses_all
    error.backward()
    grad = pts.grad.clone()
    assert torch.isfinite(grad).all() and float(grad.abs().max()) > 0
    # by hand: the loss head's gradients at the kernel's own predictions, pushed through vt_query_backward two heads a call (as ops.sifnet_query's backward does)
    preds = [t.detach().reshape(B, k, N) for t, k in zip(net.preds, ops.HEAD_DIMS)]
    leaves = [p.clone().requires_grad_(True) for p in preds]
    e2, l2 = ops.sifnet_loss_head([tuple(leaves)], df_h, df_o, parts_gt, pca_gt, oc, vg, max_dist=5.0)
    assert float(e2) == float(error) and torch.equal(l2, losses_all)
    e2.backward()
    parts_d = []
    for s in range(0, 5, 2):
        args = [None] * 5
        for i in range(s, min(s + 2, 5)):
            args[i] = leaves[i].grad.contiguous()
        dp = torch.empty(B, N, 3, device="cuda")
        L.check(L.lib().vt_query_backward(net.handle.h, C.byref(net.maps.c), L.dptr(pts.detach()), L.dptr(cc), L.dptr(bc), B, N, *[L.dptr(a) for a in args],
                                          L.dptr(dp), L.stream_ptr()))
        parts_d.append(dp)
    by_hand64 = sum(d.double() for d in parts_d)
    by_hand32 = (parts_d[0] + parts_d[1]) + parts_d[2]
    e32 = float((by_hand32.double() - by_hand64).abs().max())                       # what adding the three partial gradients in float32 costs: all the two can differ by
    err = float((grad.double() - by_hand64).abs().max())
    print(f"\npoints.grad: e32 {e32:.3e}, |autograd - by hand| {err:.3e}, largest element {float(grad.abs().max()):.3e}")
    assert err <= 4 * e32
    # losses_all against the torch expression of get_errors on the kernel's own predictions
    targs = (preds, df_h, df_o, parts_gt, dev(lab[0]), 5.0, oc, vg, net.loss_weights, "l2")
    t64, t32 = torch_get_errors(*targs, torch.float64), torch_get_errors(*targs, torch.float32)
    e32 = (t32.double() - t64).abs()
    err = (losses_all - t64).abs()
    print(f"losses_all: e32 {e32.tolist()}, kernel {err.tolist()}")
    assert bool((err <= 4 * e32).all())
    # the compact per-frame labels: the same bits
    e3, l3 = net.get_errors(df_h, df_o, parts_gt, dev(c["pca_gt"]).view(B, 3, 3), 5.0, bc, dev(c["obj_center"]), visibility=dev(c["visibility"]))
    assert torch.equal(l3, losses_all) and float(e3) == float(error)
    with pytest.raises(ValueError):
        net.get_errors(df_h, df_o, parts_gt, pca_gt, 5.0, bc, oc)


# ---- 6: batch assembly and validation ------------------------------------------------------------------------------------------------------------------------
def test_training_batch_and_validate(synth):
    from pmdist_cases import body_object_case
    from vistracker_amd import synthetic as syn, training
    from vistracker_amd.boundary_sampler import BoundarySampler
    from vistracker_amd.sifnet import SIFNetQuery
    case = body_object_case(n_surface=8, n_box=8)
    B, total = 2, 500
    sv, sf = dev(case["body"][:B]), dev(case["body_faces"], torch.int32); ov, of = dev(case["obj"][:B]), dev(case["obj_faces"], torch.int32)
    bs = BoundarySampler(case["labels"], seed=3)
    body_center = torch.stack([v.mean(0) for v in sv]); visibility = dev([0.8, 0.3])
    kw = dict(sigmas=[0.08, 0.02], ratios=[0.2, 0.8], total_sample_num=total)
    batch = training.make_training_batch(bs, (sv, sf), (ov, of), body_center, visibility, **kw)
    assert set(batch) == {"points", "df_h", "df_o", "labels", "pca_axis", "body_center", "obj_center", "visibility"}
    n_grid, nums = training.sample_counts(kw["ratios"], total)
    assert n_grid + sum(nums) == total and (n_grid, nums) == (5, [99, 396])          # check_sample_num
    shapes = {"points": (B, total, 3), "df_h": (B, total), "df_o": (B, total), "labels": (B, total), "pca_axis": (B, 3, 3), "body_center": (B, 3),
              "obj_center": (B, 3), "visibility": (B,)}
    for k, s in shapes.items():
        assert tuple(batch[k].shape) == s and batch[k].is_cuda, k
    assert batch["labels"].dtype == torch.int32 and int(batch["labels"].min()) >= 0 and int(batch["labels"].max()) < 14
    # a frame's entries alone and in the batch: the same bits
    one = training.make_training_batch(bs, (sv[1:], sf), (ov[1:], of), body_center[1:], visibility[1:], keys=[1], **kw)
    for k in batch:
        assert torch.equal(one[k][0], batch[k][1]), k
    assert not torch.equal(batch["points"][0], batch["points"][1])
    # 5 points of the box, then sigma 0.08, then 0.02, scattered by a permutation: most samples are near a surface; the ones farther than 0.5 m can only be box
    # points (6 sigma of the widest noise is 0.48 m), and they are no longer the first five
    d_min = torch.minimum(batch["df_h"], batch["df_o"])
    assert float((d_min < 0.1).float().mean()) > 0.7
    far = d_min > 0.5
    assert int(far.sum(1).max()) <= n_grid and bool(far[:, n_grid:].any())
    # the labels are compute_labels' on those points
    d_h, d_o, _, _, parts = bs.compute_labels((ov, of), batch["points"], (sv, sf))
    assert torch.equal(d_h, batch["df_h"]) and torch.equal(d_o, batch["df_o"]) and torch.equal(parts, batch["labels"])
    np.testing.assert_allclose(batch["obj_center"].cpu().numpy(), case["obj"][:B].mean(1) - body_center.cpu().numpy(), atol=2e-6)
    np.testing.assert_allclose(batch["pca_axis"].cpu().numpy(), bs.compute_pca(case["obj"][:B]).astype(np.float32), atol=1e-6)
    # depth-dependent scaling (traindata_online.py:147-151): the body's centre lands on `depth`, distances scale with it
    scaled = training.make_training_batch(bs, (sv, sf), (ov, of), body_center, visibility, depth=2.0, **kw)
    np.testing.assert_allclose(scaled["body_center"][:, 2].cpu().numpy(), 2.0, atol=1e-6)
    np.testing.assert_allclose(scaled["obj_center"].cpu().numpy(), (batch["obj_center"] * (2.0 / body_center[:, 2:3])).cpu().numpy(), atol=1e-5)
    # validate = query + get_errors, composed by hand
    net = SIFNetQuery(synth["decoders"])
    net.set_feature_maps(syn.feature_maps(B, 4, res_scale=1 / 8))
    cc = dev([[1018.952, 779.486]] * B)
    val = training.validate(net, batch, cc, max_dist=5.0)
    assert list(val) == ["df_h", "df_o", "parts", "pca", "vis", "obj_center", "total"] and all(isinstance(v, float) and np.isfinite(v) for v in val.values())
    with torch.no_grad():
        net.query(batch["points"], crop_center=cc, body_center=batch["body_center"])
        error, losses_all = net.get_errors(batch["df_h"], batch["df_o"], batch["labels"], batch["pca_axis"], 5.0, batch["body_center"], batch["obj_center"],
                                           visibility=batch["visibility"])
    assert [float(x) for x in losses_all] + [float(error)] == list(val.values())
    assert val["total"] == pytest.approx(sum(list(val.values())[:6]), rel=1e-12)
