"""Golden vectors of one whole-network training step: the reference's own ``CHORETriplaneVisibility`` (model/chore_tri_vis.py, model/chore_triplane.py:60-164) in
train mode, run in FLOAT64 on the CPU (torch's default dtype set to float64 before the module is built, float64 inputs) through tools/ref_harness.py: ``filter`` on the (B,8,H,W) input, ``query`` at the labelled points, ``get_errors`` and torch
autograd's ``error.backward()``.  Options: config tri-vis-l2 with num_stack, triplane_encoder_stack and num_hourglass set to the case's (2 stacks of depth 1).

Inputs are regenerated from their seeds by the tests and are NOT stored: sifnet_step_model.case() (synthetic weights loaded into the reference module with
load_state_dict, the images, the points and centres, the labels).  Recorded: the six losses and the total, and the gradients sifnet_step_model.gated() lists (every
decoder tensor, the last stack's tail and the stem of each encoder) in the form of sifnet_step_model.golden_sub.  Also writes the parameter NAMES of the shipped
configuration (3 stacks of depth 2) to tests/golden/sifnet_state_dict_keys.txt.  Build container only: writes data only."""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as rh  # noqa: E402

torch = rh.enter_reference()
import sifnet_step_model as SM  # noqa: E402
from config.config_loader import load_configs  # noqa: E402
from model import CHORETriplaneVisibility  # noqa: E402


def build(num_stack, depth):
    with contextlib.redirect_stdout(io.StringIO()):
        cfg = load_configs("tri-vis-l2")
        cfg.gpu_id = "cpu"
        cfg.num_stack = cfg.triplane_encoder_stack = num_stack
        cfg.num_hourglass = depth
        return CHORETriplaneVisibility(cfg).train(), cfg


shipped, _ = build(3, 2)
path = os.path.join(ROOT, "tests", "golden", "sifnet_state_dict_keys.txt")
with open(path, "w") as f:
    f.write("\n".join(shipped.state_dict().keys()) + "\n")
print("wrote tests/golden/sifnet_state_dict_keys.txt", len(shipped.state_dict()), "names")

# float64: the recording then carries no rounding of its own to speak of, and the tests can hold the GPU to it at the bound they hold it to the float64 model at
torch.set_default_dtype(torch.float64)
net, cfg = build(SM.NUM_STACK, SM.DEPTH)
c = SM.case()
f64 = lambda a: torch.tensor(np.asarray(a, np.float64))        # noqa: E731
res = net.load_state_dict({k: f64(v) for k, v in SM.state_dict(c).items()}, strict=False)
assert all(p.dtype == torch.float64 for p in net.parameters())
assert not res.unexpected_keys and all(".bn4." in k for k in res.missing_keys), (res.unexpected_keys, res.missing_keys)      # an identity block never uses bn4
lab, n = c["labels"], c["pts"].shape[1]
rep = lambda a: f64(np.ascontiguousarray(np.repeat(np.asarray(a)[..., None], n, -1)))      # noqa: E731  what the reference's loader repeats per point
net.filter(f64(c["images"]))
net.query(f64(c["pts"]), crop_center=f64(c["cc"]), body_center=f64(c["bc"]))
with contextlib.redirect_stdout(io.StringIO()):
    error, losses_all = net.get_errors(f64(lab["df_h"]), f64(lab["df_o"]), torch.tensor(lab["labels"]).long(), rep(lab["pca_axis"]), SM.MAX_DIST,
                                       f64(c["bc"]), rep(lab["obj_center"]), visibility=rep(lab["visibility"]))
assert error.dtype == losses_all.dtype == torch.float64
error.backward()
r64 = SM.run(c)
data = {"losses_all": losses_all.detach().numpy().astype(np.float64), "error": np.float64(error.detach())}
print("losses", data["losses_all"], "|ref - model64|", np.abs(data["losses_all"] - r64["losses_all"]))
named = dict(net.named_parameters())
for k in SM.gated():
    g = named[k].grad.numpy()
    assert g.dtype == np.float64
    g = g[:, :, 0] if g.ndim == 3 else g            # Conv1d weights (out, in, 1)
    data[k] = SM.golden_sub(k)(g)
    print(f"{k:40s} {str(g.shape):18s} |ref - model64| {np.abs(g - r64['grads'][k]).max():.3e} of {np.abs(g).max():.3e}")
path = os.path.join(ROOT, "tests", "golden", "sifnet_step.npz")
np.savez_compressed(path, **data)
print("wrote tests/golden/sifnet_step.npz", os.path.getsize(path), "bytes")
