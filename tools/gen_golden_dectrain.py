"""Golden vectors of the decoder training step: the reference's own CHORETriplaneVisibility.query (model/chore_triplane.py:97-164) with its make_decoder
decoders (model/chore.py:113-126), run in float32 on the CPU through tools/ref_harness.py, and torch's autograd gradient of sum(prediction * upstream) to the
decoders' weights and biases.

Inputs: synthetic.sifnet_decoders(3) and synthetic.feature_maps(2, res_scale=0.125) (regenerated from their seeds by the tests, not stored); the points, crop
centres, body centres and upstream gradients of tests/dectrain_model.py (make_inputs, make_upstream: small, stored).  Recorded: the five predictions; the
gradients of all biases, of all layer-4 weights, and of the rows dectrain_model.GOLDEN_ROWS of every other weight matrix.
Build container only: writes tests/golden/dectrain.npz (data only)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as rh  # noqa: E402

torch = rh.enter_reference()
import dectrain_model as M  # noqa: E402
from vistracker_amd import synthetic as syn  # noqa: E402

B, N = 2, 150
dec, maps = syn.sifnet_decoders(3), syn.feature_maps(B, res_scale=0.125)
pts, cc, bc = M.make_inputs(B, N, seed=11)
up = M.make_upstream(B, N, seed=12)
net, _ = rh.make_sifnet(dec, maps)
mods = {"df": net.df, "pca": net.pca_predictor, "parts": net.part_predictor, "centers": net.center_predictor, "vis": net.visib_predictor}
convs = {n: [m for m in mods[n] if isinstance(m, torch.nn.Conv1d)] for n in M.HEADS}
for n in M.HEADS:
    for c in convs[n]:
        c.weight.requires_grad_(True); c.bias.requires_grad_(True)
net.query(torch.tensor(pts), crop_center=torch.tensor(cc), body_center=torch.tensor(bc))
preds = net.get_preds()
loss = sum((p.reshape(B, k, N) * torch.tensor(up[h])).sum() for p, h, k in zip(preds, M.HEADS, M.DIMS))
loss.backward()
out = dict(pts=pts, cc=cc, bc=bc, rows=np.array(M.GOLDEN_ROWS, np.int32))
for h, p, k in zip(M.HEADS, preds, M.DIMS):
    out["pred_" + h] = p.detach().numpy().reshape(B, k, N)
    out["up_" + h] = up[h]
    for l, c in enumerate(convs[h]):
        w = c.weight.grad.numpy()[:, :, 0]
        out[f"g_{h}_{l}_weight"] = w if l == 3 else w[list(M.GOLDEN_ROWS)]
        out[f"g_{h}_{l}_bias"] = c.bias.grad.numpy()
r64 = M.run(dec, [maps], pts, cc, bc, upstream=[up])
for i, h in enumerate(M.HEADS):
    print(h, "pred |ref - model64|", np.abs(out["pred_" + h] - r64["preds"][0][i]).max())
    for l in range(4):
        g = r64["grads"][(h, l, "weight")]
        print("   layer", l, "dW", np.abs(out[f"g_{h}_{l}_weight"] - (g if l == 3 else g[list(M.GOLDEN_ROWS)])).max(), "of", np.abs(g).max(),
              " db", np.abs(out[f"g_{h}_{l}_bias"] - r64["grads"][(h, l, "bias")]).max())
path = os.path.join(ROOT, "tests", "golden", "dectrain.npz")
np.savez_compressed(path, **out)
print("wrote tests/golden/dectrain.npz", os.path.getsize(path), "bytes")
