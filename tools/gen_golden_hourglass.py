"""Golden vectors of the hourglass backward: the reference's own ``HourGlass(1, 2, 128, norm='group')`` (model/HGFilters.py:4-53), run in float32 on the CPU
through tools/ref_harness.py with torch autograd; B = 1, 32 x 64 pixels.

Inputs are regenerated from their seeds by the tests and are NOT stored: tests/hourglass_model.py make_params(2, 128, SEED) (synthetic weights, one seed per block,
loaded into the reference module with load_state_dict) and make_inputs(1, 32, 64, 128, SEED + 100) (the input and the upstream gradient).
Recorded: the gradient to the input whole, every GroupNorm gamma / beta gradient in full, every GOLDEN_WEIGHT_STEP-th element of each convolution's flattened
weight gradient and every GOLDEN_OUT_STEP-th element of the flattened output.  A committed file stays under 1 MiB, so the convolutions' weight gradients go to a
second file.  Build container only: writes tests/golden/hourglass.npz and tests/golden/hourglass_wgrad.npz (data only)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as rh  # noqa: E402

torch = rh.enter_reference()
import hourglass_model as HM  # noqa: E402
from model.HGFilters import HourGlass  # noqa: E402

DEPTH, FEATURES, B, H, W, SEED = 2, 128, 1, 32, 64, 61          # tests/test_host_resample.py and test_gpu_hourglass.py use the same numbers
P = HM.make_params(DEPTH, FEATURES, SEED)
x, dy = HM.make_inputs(B, H, W, FEATURES, SEED + 100)
hg = HourGlass(1, DEPTH, FEATURES, norm="group")
hg.load_state_dict({k: torch.tensor(v) for k, v in P.items()}, strict=True)
xt = torch.tensor(x).requires_grad_(True)
y = hg(xt)
(y * torch.tensor(dy)).sum().backward()
g64 = HM.autograd_grads(P, x, dy)
small = {"out": y.detach().numpy().reshape(-1)[::HM.GOLDEN_OUT_STEP], "d_x": xt.grad.numpy()}
wgrad = {}
print(f"out |ref - model64| {np.abs(y.detach().numpy() - g64['out']).max():.3e}; d_x {np.abs(small['d_x'] - g64['d_x']).max():.3e} of {np.abs(g64['d_x']).max():.3e}")
for n, p in hg.named_parameters():
    if p.grad is None:          # bn4 of an identity block (net_util.py:371-372)
        continue
    g = p.grad.numpy()
    if g.ndim == 4:
        wgrad[n] = g.reshape(-1)[::HM.GOLDEN_WEIGHT_STEP]
    else:
        small[n] = g
    print(f"{n:26s} {str(g.shape):18s} |ref - model64| {np.abs(g - g64[n]).max():.3e} of {np.abs(g).max():.3e}")
for name, data in (("hourglass.npz", small), ("hourglass_wgrad.npz", wgrad)):
    path = os.path.join(ROOT, "tests", "golden", name)
    np.savez_compressed(path, **data)
    print("wrote tests/golden/" + name, os.path.getsize(path), "bytes")
