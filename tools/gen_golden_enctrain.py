"""Golden vectors of the whole-encoder backward: the reference's own ``HGFilter`` (model/HGFilters.py:56-203), run in float32 on the CPU through
tools/ref_harness.py with torch autograd, in the two configurations of tests/enctrain_model.py FILTER_CASES (image encoder: Cin 5, tmpx 64, hourglass_dim 256;
triplane encoder: Cin 1, tmpx 32, hourglass_dim 64), 2 stacks of depth 1, B = 1, 64 x 128 pixels.  The options are built as tools/gen_golden_encoder.py builds
them (config tri-vis-l2; the triplane encoder's Namespace), with num_stack and num_hourglass set to the case's.

Inputs are regenerated from their seeds by the tests and are NOT stored: enctrain_model.filter_case(tag) (synthetic weights loaded into the reference module with
load_state_dict, the image, the upstream gradients of the two outputs and of normx).  Recorded per case: every bias / gamma / beta gradient whole and every
GOLDEN_WEIGHT_STEP-th element of each convolution's flattened weight gradient.  Build container only: writes tests/golden/enctrain_image.npz and
tests/golden/enctrain_triplane.npz (data only)."""
import contextlib
import io
import os
import sys
from argparse import Namespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as rh  # noqa: E402

torch = rh.enter_reference()
import enctrain_model as EM  # noqa: E402
from config.config_loader import load_configs  # noqa: E402
from model.HGFilters import HGFilter  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    cfg = load_configs("tri-vis-l2")
for tag in EM.FILTER_CASES:
    cin, tmpx, hg, _ = EM.FILTER_CASES[tag]
    with contextlib.redirect_stdout(io.StringIO()):
        if tag == "image":
            opt = cfg
            opt.num_stack, opt.num_hourglass = EM.FILTER_NUM_STACK, EM.FILTER_DEPTH
        else:
            opt = Namespace(input_type="mask", num_stack=EM.FILTER_NUM_STACK, hourglass_dim=cfg.triplane_hg_dim, tmpx_dim=cfg.triplane_tmpx_dim, hg_down=cfg.hg_down,
                            norm=cfg.norm, num_hourglass=EM.FILTER_DEPTH)
        enc = HGFilter(opt)
    assert (enc.conv1.weight.shape[1], enc.conv1.weight.shape[0], enc.l0.weight.shape[0]) == (cin, tmpx, hg), tag
    P, x, d_outs, d_normx = EM.filter_case(tag)
    res = enc.load_state_dict({k: torch.tensor(v) for k, v in P.items()}, strict=False)
    assert not res.unexpected_keys and all(".bn4." in k for k in res.missing_keys), (res.unexpected_keys, res.missing_keys)      # an identity block never uses bn4
    outs, tmpx_t, normx = enc(torch.tensor(x))
    assert tmpx_t.grad_fn is None
    loss = sum((o * torch.tensor(d)).sum() for o, d in zip(outs, d_outs)) + (normx * torch.tensor(d_normx)).sum()
    loss.backward()
    g64 = EM.filter_autograd_grads(P, x, d_outs, d_normx)
    data = {}
    for n, p in enc.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.numpy()
        data[n] = g.reshape(-1)[::EM.GOLDEN_WEIGHT_STEP] if g.ndim == 4 else g
        if n in g64:
            print(f"{tag} {n:34s} {str(g.shape):18s} |ref - model64| {np.abs(g - g64[n]).max():.3e} of {np.abs(g).max():.3e}")
    # the reference registers a projection's norm twice (bn4 and downsample.0 are one module): the model's name is bn4
    data = {k: v for k, v in data.items() if ".downsample.0." not in k}
    assert set(data) == {k for k in g64 if k not in ("tmpx", "normx") and not k.startswith("out")}, sorted(set(data) ^ set(g64))
    path = os.path.join(ROOT, "tests", "golden", f"enctrain_{tag}.npz")
    np.savez_compressed(path, **data)
    print("wrote tests/golden/enctrain_" + tag + ".npz", os.path.getsize(path), "bytes")
