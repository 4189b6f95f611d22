"""Golden vectors of the gradient to the feature maps: the reference's own CHORETriplaneVisibility.query (model/chore_triplane.py:97-164, sampling through
model/geometry.py:4-14) run in float32 on the CPU through tools/ref_harness.py with the eight feature maps as LEAVES, and torch autograd's .grad of each for
sum(prediction * upstream).

Inputs: those of tools/gen_golden_dectrain.py (synthetic.sifnet_decoders(3), synthetic.feature_maps(2, res_scale=0.125), regenerated from their seeds by the
tests; the points, centres and upstream of tests/dectrain_model.py make_inputs(2, 150, 11) / make_upstream(2, 150, 12)).  Recorded per map: the texel rows
(frame, y, x) that received anything, as an index into the (B R R) rows of the channel-last gradient, and every third channel (0, 3, 6, ...: mapgrad_model.
GOLDEN_CHANNEL_STEP, which keeps the file near dectrain.npz's size) of their values; every other row is an exact zero.
Build container only: writes tests/golden/mapgrad.npz (data only)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as rh  # noqa: E402

torch = rh.enter_reference()
import dectrain_model as M  # noqa: E402
import mapgrad_model as G  # noqa: E402
from vistracker_amd import synthetic as syn  # noqa: E402

B, N = 2, 150
dec, maps = syn.sifnet_decoders(3), syn.feature_maps(B, res_scale=0.125)
pts, cc, bc = M.make_inputs(B, N, seed=11)
up = M.make_upstream(B, N, seed=12)
net, _ = rh.make_sifnet(dec, maps)
t = {k: torch.tensor(maps[k]).requires_grad_(True) for k in G.MAPS}
net.im_feat_list = [t["im_feat"]]
net.tmpx = t["tmpx"]
net.triplane_tmpx = [t["tri_tmpx0"], t["tri_tmpx1"], t["tri_tmpx2"]]
net.triplane_feat_list = [[t["tri_feat0"]], [t["tri_feat1"]], [t["tri_feat2"]]]
net.query(torch.tensor(pts), crop_center=torch.tensor(cc), body_center=torch.tensor(bc))
preds = net.get_preds()
sum((p.reshape(B, k, N) * torch.tensor(up[h])).sum() for p, h, k in zip(preds, M.HEADS, M.DIMS)).backward()
out = dict(pts=pts, cc=cc, bc=bc)
r64 = G.run(dec, [maps], pts, cc, bc, upstream=[up])
for n in G.MAPS:
    g = t[n].grad.numpy()
    rows = g.transpose(0, 2, 3, 1).reshape(-1, g.shape[1])
    idx = np.flatnonzero((rows != 0).any(1)).astype(np.int32)
    out["idx_" + n], out["val_" + n] = idx, rows[idx][:, ::G.GOLDEN_CHANNEL_STEP]
    print(n, g.shape, "touched rows", len(idx), "of", len(rows), "|ref - model64|", np.abs(g - r64["dmaps"][0][n]).max(), "of", np.abs(g).max())
path = os.path.join(ROOT, "tests", "golden", "mapgrad.npz")
np.savez_compressed(path, **out)
print("wrote tests/golden/mapgrad.npz", os.path.getsize(path), "bytes")
