"""Golden vectors of SIF-Net's training objective: the reference's own CHORETriplaneVisibility.get_errors (model/chore_tri_vis.py:52-99) with CHORE.get_df_loss
(model/chore.py:312-325), run in float32 on the CPU on a stub that carries what the two methods read -- intermediate_preds_list, loss_weights, part_loss_func,
dfloss_func, vis_loss_name and a silent print_errors (the model's constructor would build the encoder and call .cuda()) -- and torch's autograd gradient of
`error` to every prediction.

Cases: S = 3 and S = 1 stacks (the first of the three), B = 3, N = 333, max_dist = 0.5, vis_loss l1 and l2.  Predictions are drawn on the float16 grid (stored
as float16: every value is exact in float32) with distances and labels on both sides of max_dist and df_o on both sides of 0.05; a few are placed exactly: p == g,
p == max_dist, df_o == float32(0.05).  pca_gt, obj_center and visibility are per frame, repeated over the points for the reference as its loader does
(data/traindata_online.py:102,177-183).  vis_loss changes the vis term and d_vis only (asserted here), so the other gradients are stored once per S.
Build container only: writes tests/golden/losshead.npz (data only)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

torch = rh.enter_reference()
import contextlib  # noqa: E402
import io  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    from model import CHORETriplaneVisibility  # noqa: E402
    from model.chore import CHORE  # noqa: E402

S, B, N, MD = 3, 3, 333, 0.5
WEIGHTS = [1.0, 1.0, 0.006, 500, 1000, 1000]
rng = np.random.default_rng(20)
f16 = lambda a: np.asarray(a, np.float16)      # noqa: E731
df_h = rng.uniform(0.0, 1.0, (B, N)).astype(np.float32)                          # half of them beyond max_dist
df_o = np.where(rng.random((B, N)) < 0.4, rng.uniform(0.0, 0.05, (B, N)), rng.uniform(0.05, 1.2, (B, N))).astype(np.float32)
df_o[:, 5] = np.float32(0.05)                                                    # exactly on the mask's threshold: masked out
df_o[:, 6] = np.nextafter(np.float32(0.05), np.float32(0))                       # the float below it: in
parts_gt = rng.integers(0, 14, (B, N)).astype(np.int32)
pca_gt = np.linalg.qr(rng.normal(size=(B, 3, 3)))[0].reshape(B, 9).astype(np.float32)
obj_center = rng.normal(0, 0.4, (B, 3)).astype(np.float32)
visibility = rng.uniform(0.1, 1.0, (B,)).astype(np.float32)
df = f16(np.stack([df_h, df_o], 1)[None] + rng.normal(0, 0.2, (S, B, 2, N)))
df[:, :, 0, 0] = f16(0.5)                                                        # p == max_dist: the gradient passes
df[:, :, 1, 1] = f16(0.75); df_o[:, 1] = 0.75                                    # p == g beyond max_dist: both clamp, zero value, zero gradient
df[:, :, 0, 2] = f16(0.25); df_h[:, 2] = 0.25                                    # p == g below max_dist: sign(0) = 0
pca = f16(pca_gt[None, :, :, None] + rng.normal(0, 0.3, (S, B, 9, N)))
parts = f16(rng.normal(0, 3.0, (S, B, 14, N)))
centers = f16(obj_center[None, :, :, None] + rng.normal(0, 0.2, (S, B, 3, N)))
vis = f16(1.0 / (1.0 + np.exp(-rng.normal(0, 1.5, (S, B, 1, N)))))
vis[:, :, 0, 6] = f16(visibility)[None]                                          # p == g (to float16) inside the mask: |p - g| tiny or zero


class Stub:
    pass


def run(n_stacks, vis_loss):
    heads = [torch.tensor(a[:n_stacks].astype(np.float32), requires_grad=True) for a in (df, pca, parts, centers, vis)]
    net = Stub()
    net.intermediate_preds_list = [(heads[0][s], heads[1][s].view(B, 3, 3, N), heads[2][s], heads[3][s], heads[4][s]) for s in range(n_stacks)]
    net.loss_weights = WEIGHTS
    net.part_loss_func = torch.nn.CrossEntropyLoss(reduction="none")
    net.dfloss_func = torch.nn.L1Loss(reduction="none")
    net.vis_loss_name = vis_loss
    net.print_errors = lambda errors: None
    net.get_df_loss = lambda *a: CHORE.get_df_loss(net, *a)
    rep = lambda a: torch.tensor(np.repeat(a[..., None], N, -1))       # noqa: E731
    error, losses_all = CHORETriplaneVisibility.get_errors(net, torch.tensor(df_h), torch.tensor(df_o), torch.tensor(parts_gt).long(), rep(pca_gt).view(B, 3, 3, N),
                                                           MD, None, rep(obj_center), visibility=rep(visibility))
    assert net.error_buffer is losses_all
    error.backward()
    return np.float32(error.item()), losses_all.numpy().astype(np.float32), [h.grad.numpy() for h in heads]


out = dict(df=df, pca=pca, parts=parts, centers=centers, vis=vis, df_h=df_h, df_o=df_o, parts_gt=parts_gt, pca_gt=pca_gt, obj_center=obj_center,
           visibility=visibility, max_dist=np.float32(MD), weights=np.array(WEIGHTS, np.float64))
for n_stacks in (3, 1):
    e2, l2, g2 = run(n_stacks, "l2")
    e1, l1, g1 = run(n_stacks, "l1")
    for i in range(4):
        assert np.array_equal(g1[i], g2[i])
    assert np.array_equal(np.delete(l1, 4), np.delete(l2, 4))
    tag = f"S{n_stacks}"
    for name, g in zip(("d_df", "d_pca", "d_parts", "d_centers"), g2):
        out[f"{tag}_{name}"] = g
    out[f"{tag}_l2_d_vis"], out[f"{tag}_l1_d_vis"] = g2[4], g1[4]
    out[f"{tag}_l2_error"], out[f"{tag}_l1_error"] = e2, e1
    out[f"{tag}_l2_losses_all"], out[f"{tag}_l1_losses_all"] = l2, l1
    print(tag, "l2", e2, l2.tolist(), "\n   l1", e1, l1.tolist())
mask = df_o < np.float32(0.05)
print(f"mask true for {mask.mean():.2f} of the points; df_h > max_dist for {(df_h > MD).mean():.2f}; df_h prediction > max_dist for "
      f"{(df[:, :, 0].astype(np.float32) > MD).mean():.2f}")
path = os.path.join(ROOT, "tests", "golden", "losshead.npz")
np.savez_compressed(path, **out)
print("wrote tests/golden/losshead.npz", os.path.getsize(path), "bytes")
