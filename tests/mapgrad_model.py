"""float64 model of the gradient SIF-Net's decoder training step sends to the eight feature maps: the run of tests/dectrain_model.py (projection, the
hand-written bilinear sampler, the 611-channel concatenation, the five decoders, the upstream gradient or get_errors) with the MAPS AS LEAVES beside the decoder
parameters, differentiated by torch autograd.  Like dectrain_model.py it shares no code with the product.  Runs in any dtype: the float32 run against the float64
run on a test's own inputs is that test's e32 PER MAP TENSOR (the largest element difference), and the kernels get 4 e32.

Stacks that share a tensor (the tmpx maps, chore_triplane.py:139-149) share its array OBJECT in ``maps_list``: one leaf is made per distinct array, so the
gradient of a shared map is the sum over its stacks, as ``t.grad`` of the shared tensor is.
"""
import numpy as np
import torch

import dectrain_model as M

MAPS = tuple(name for name, kind in M.CONCAT if kind is not None)        # the eight maps, concatenation order
GOLDEN_CHANNEL_STEP = 3                                                  # tests/golden/mapgrad.npz records the channels 0, 3, 6, ... of every touched texel row


def _leaves(maps_list, dtype):
    """-> [S] dicts name -> leaf tensor; arrays that are the same object share one leaf"""
    made = {}
    out = []
    for maps in maps_list:
        d = {}
        for name in MAPS:
            if id(maps[name]) not in made:
                made[id(maps[name])] = M._t(maps[name], dtype).clone().requires_grad_(True)
            d[name] = made[id(maps[name])]
        out.append(d)
    return out


def _grad(t):
    return (t.grad if t.grad is not None else torch.zeros_like(t)).detach().numpy().astype(np.float64)


def run(decoders, maps_list, pts, cc, bc, upstream=None, labels=None, max_dist=5.0, dtype=torch.float64):
    """dectrain_model.run with the maps as leaves -> its dict and "dmaps": [S][name] (B,C,R,R), the gradient of the same scalar to every map"""
    params = M.make_params(decoders, dtype)
    p, c, b = M._t(pts, dtype), M._t(cc, dtype), M._t(bc, dtype)
    leaves = _leaves(maps_list, dtype)
    preds_list = []
    for maps in leaves:
        feat, in_img = M.features(maps, p, c, b)
        preds_list.append(M.decode(params, feat, in_img))
    out = {"preds": [[t.detach().numpy().astype(np.float64) for t in preds] for preds in preds_list]}
    if upstream is not None:
        loss = sum((preds[M.HEADS.index(h)] * M._t(g, dtype)).sum() for preds, up in zip(preds_list, upstream) for h, g in up.items())
        if torch.is_tensor(loss):
            loss.backward()
    elif labels is not None:
        lab = {k: M._t(v, torch.int64 if k == "labels" else dtype) for k, v in labels.items()}
        loss, losses_all = M.get_errors(preds_list, lab, max_dist)
        loss.backward()
        out["error"], out["losses_all"] = float(loss.detach()), losses_all.detach().numpy().astype(np.float64)
    out["grads"] = M.grads_of(params)
    out["dmaps"] = [{name: _grad(t) for name, t in maps.items()} for maps in leaves]
    return out


def reference_and_e32(*args, **kw):
    """-> (float64 run, e32): dectrain_model's e32 entries and e32["dmaps"][s][name] = the largest element error of the float32 run"""
    r64, r32 = run(*args, dtype=torch.float64, **kw), run(*args, dtype=torch.float32, **kw)
    e32 = {"preds": [[np.abs(a - b).max() for a, b in zip(p64, p32)] for p64, p32 in zip(r64["preds"], r32["preds"])],
           "grads": {k: np.abs(r64["grads"][k] - r32["grads"][k]).max() for k in r64["grads"]},
           "dmaps": [{n: np.abs(d64[n] - d32[n]).max() for n in d64} for d64, d32 in zip(r64["dmaps"], r32["dmaps"])]}
    return r64, e32


def train_maps_model(decoders, maps, pts, cc, bc, labels, steps, lr, max_dist=5.0, dtype=torch.float64):
    """``steps`` steps of torch.optim.Adam on the eight maps of one stack, decoders fixed, one fixed batch -> the total error before every step"""
    params = M.make_params(decoders, dtype)
    leaves = _leaves([maps], dtype)[0]
    opt = torch.optim.Adam(list(leaves.values()), lr=lr)
    p, c, b = M._t(pts, dtype), M._t(cc, dtype), M._t(bc, dtype)
    lab = {k: M._t(v, torch.int64 if k == "labels" else dtype) for k, v in labels.items()}
    errors = []
    for _ in range(steps):
        opt.zero_grad()
        feat, in_img = M.features(leaves, p, c, b)
        error, _ = M.get_errors([M.decode(params, feat, in_img)], lab, max_dist)
        error.backward()
        opt.step()
        errors.append(float(error.detach()))
    return errors
