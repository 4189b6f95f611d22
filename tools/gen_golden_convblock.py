"""Golden vectors of the ConvBlock backward: the reference's own ``ConvBlock(64, 128, 'group')`` (1x1-projected residual) and ``ConvBlock(128, 128, 'group')``
(identity residual), model/net_util.py:346-396, run in float32 on the CPU through tools/ref_harness.py with torch autograd.

Inputs are regenerated from their seeds by the tests and are NOT stored: tests/convblock_model.py make_params(cin, cout, seed) (synthetic weights, loaded into the
reference module with load_state_dict) and make_inputs(1, 8, 16, cin, cout, seed + 1) (the block input and the upstream gradient; B = 1, 8 x 16 pixels).
Recorded per block: the output, the gradient to the input, every GroupNorm gamma / beta gradient in full and every GOLDEN_WEIGHT_STEP-th element of each
convolution's flattened weight gradient.  Build container only: writes tests/golden/convblock.npz (data only)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as rh  # noqa: E402

torch = rh.enter_reference()
import convblock_model as M  # noqa: E402
from model.net_util import ConvBlock  # noqa: E402

BLOCKS = ((64, 128, 21), (128, 128, 23))       # (cin, cout, seed); tests/test_host_convblock.py and test_gpu_convblock.py use the same table
out = {}
for cin, cout, seed in BLOCKS:
    P = M.make_params(cin, cout, seed)
    x, dy = M.make_inputs(1, 8, 16, cin, cout, seed + 1)
    blk = ConvBlock(cin, cout, "group")
    missing = blk.load_state_dict({k: torch.tensor(v) for k, v in P.items()}, strict=True)
    xt = torch.tensor(x).requires_grad_(True)
    y = blk(xt)
    (y * torch.tensor(dy)).sum().backward()
    tag = f"b{cin}_{cout}."
    out[tag + "out"] = y.detach().numpy()
    out[tag + "d_x"] = xt.grad.numpy()
    g64 = M.autograd_grads(P, x, dy)
    names = {n: p for n, p in blk.named_parameters() if p.grad is not None}
    for n, p in names.items():
        if n.startswith("downsample.0"):        # the same module as bn4 (net_util.py:362-366)
            continue
        g = p.grad.numpy()
        out[tag + n] = g.reshape(-1)[::M.GOLDEN_WEIGHT_STEP] if g.ndim == 4 else g
        print(f"{tag}{n:22s} {str(g.shape):18s} |ref - model64| {np.abs(g - g64[n]).max():.3e} of {np.abs(g).max():.3e}")
    print(f"{tag}out |ref - model64| {np.abs(out[tag + 'out'] - g64['out']).max():.3e}; d_x {np.abs(out[tag + 'd_x'] - g64['d_x']).max():.3e}")
path = os.path.join(ROOT, "tests", "golden", "convblock.npz")
np.savez_compressed(path, **out)
print("wrote tests/golden/convblock.npz", os.path.getsize(path), "bytes")
