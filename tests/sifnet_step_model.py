"""A float64 model of one optimisation step of the whole SIF-Net (model/chore_triplane.py:60-164, model/chore_tri_vis.py:52-99, trainer/trainer.py:97-106): the
existing models composed, no new arithmetic.  tests/enctrain_model.py (EM) runs the image encoder on channels 0..4 and the shared triplane encoder on the 3B
single-channel renders; tests/dectrain_model.py (DM) samples the S per-stack map sets, decodes and evaluates get_errors; tests/mapgrad_model.py (G) is the same run
with the maps as leaves, the form used AT a GPU forward's saved activations; tests/losshead_model.py (LH) restates the six losses in numpy and is held against DM's
here.  It shares no code with the product (vistracker_amd/training.py SIFNetTrainer).  Tensors are NCHW numpy / torch arrays.

case()               the inputs of tests/test_gpu_sifnet_trainer.py and tools/gen_golden_sifnet_step.py, regenerated from seeds: B = 2, two stacks of depth 1, a
                     128 x 128 input (32 x 32 maps, 64 x 64 tmpx), N = 150 points, the shipped channel widths, weights at the scale of EM.filter_make_params
state_dict(c)        the case's parameters under the reference's checkpoint keys
run(c, dtype)        the step's objective and its gradient to EVERY parameter by torch autograd through the whole composition, in dtype; run in float32 against
                     float64 it gives e32, the unit of the bounds
at_saved(c, ...)     the float64 chain at a GPU forward's saved activations: G.run at the GPU's maps, then EM.filter_manual_grads from the maps' gradients
train(c, steps, lr)  ``steps`` steps of torch.optim.Adam on everything, one fixed batch -> the objective before every step
"""
import concurrent.futures

import numpy as np
import torch

import dectrain_model as DM
import enctrain_model as EM
import losshead_model as LH
import mapgrad_model as G

B, N, H, W = 2, 150, 128, 128
NUM_STACK, DEPTH = 2, 1
SEED = 7                    # chosen with train(): see tests/golden/sifnet_step.md
MAX_DIST = 5.0
IMAGE, TRIPLANE = "image_filter.", "triplane_encoder."
MODULES = {"df": "df", "pca": "pca_predictor", "parts": "part_predictor", "centers": "center_predictor", "vis": "visib_predictor"}
GOLDEN_ROWS = DM.GOLDEN_ROWS          # rows of a decoder's 128-row weight gradients kept in tests/golden/sifnet_step.npz


def make_decoders(seed):
    rng = np.random.default_rng(seed)
    dec = {}
    for name, k in zip(DM.HEADS, DM.DIMS):
        dec[name] = [((rng.normal(0, np.sqrt(2.0 / i), (o, i))).astype(np.float32), rng.normal(0, 0.05, (o,)).astype(np.float32))
                     for o, i in ((128, 611), (128, 128), (128, 128), (k, 128))]
    return dec


def case(seed=SEED):
    cin_i, tmpx_i, hg_i, _ = EM.FILTER_CASES["image"]
    cin_t, tmpx_t, hg_t, _ = EM.FILTER_CASES["triplane"]
    r = np.random.RandomState(seed)
    pts, cc, bc = DM.make_inputs(B, N, seed=seed + 4)
    return dict(P_img=EM.filter_make_params(cin_i, tmpx_i, hg_i, NUM_STACK, DEPTH, seed + 1), P_tri=EM.filter_make_params(cin_t, tmpx_t, hg_t, NUM_STACK, DEPTH, seed + 2),
                dec=make_decoders(seed + 3), images=r.rand(B, 8, H, W).astype(np.float32), pts=pts, cc=cc, bc=bc, labels=DM.make_labels(B, N, seed + 5))


def state_dict(c):
    sd = {IMAGE + k: v for k, v in c["P_img"].items()}
    sd.update({TRIPLANE + k: v for k, v in c["P_tri"].items()})
    for name, layers in c["dec"].items():
        for i, (w, b) in zip((0, 2, 4, 6), layers):
            sd[f"{MODULES[name]}.{i}.weight"], sd[f"{MODULES[name]}.{i}.bias"] = w[:, :, None], b
    return sd


def triplane_input(images):
    """(B,8,H,W) -> (3B,1,H,W): view v's B renders at [vB, (v+1)B), as CHORETriplane.filter feeds one shared encoder three times"""
    return np.ascontiguousarray(np.asarray(images)[:, 5:8].transpose(1, 0, 2, 3).reshape(-1, 1, *np.asarray(images).shape[2:]))


def stack_maps(outs_img, tmpx, outs_tri, tmpx_tri, b):
    """the S map sets of the query (chore_triplane.py:127-149); the tmpx entries are the SAME objects in every stack"""
    shared = {"tmpx": tmpx}
    shared.update({f"tri_tmpx{v}": tmpx_tri[v * b:(v + 1) * b] for v in range(3)})
    maps = []
    for s in range(len(outs_img)):
        d = dict(shared)
        d["im_feat"] = outs_img[s]
        d.update({f"tri_feat{v}": outs_tri[s][v * b:(v + 1) * b] for v in range(3)})
        maps.append(d)
    return maps


def _labels(c, dtype):
    return {k: DM._t(v, torch.int64 if k == "labels" else dtype) for k, v in c["labels"].items()}


def _objective(c, params, dtype, run_filter):
    b = c["images"].shape[0]
    oi, tmpx = run_filter(c["P_img"], c["images"][:, :5])
    ot, ttmpx = run_filter(c["P_tri"], triplane_input(c["images"]))
    maps = stack_maps(oi, tmpx.detach(), ot, ttmpx.detach(), b)           # tmpx is detached (HGFilters.py:203)
    p, cc, bc = DM._t(c["pts"], dtype), DM._t(c["cc"], dtype), DM._t(c["bc"], dtype)
    preds_list = []
    for m in maps:
        feat, in_img = DM.features(m, p, cc, bc)
        preds_list.append(DM.decode(params, feat, in_img))
    error, losses_all = DM.get_errors(preds_list, _labels(c, dtype), MAX_DIST)
    return error, losses_all, preds_list


def run(c, dtype=torch.float64):
    """-> {"error", "losses_all" (6,), "preds" [S][5], "grads": {reference checkpoint key: gradient}} of the pure model in dtype"""
    leaves = {}

    def run_filter(P, x):
        outs, tmpx, _, p, _ = EM.filter_run(P, x, dtype, leaves=True)
        leaves[id(P)] = p
        return outs, tmpx

    params = DM.make_params(c["dec"], dtype)
    error, losses_all, preds_list = _objective(c, params, dtype, run_filter)
    error.backward()
    g = {}
    for prefix, P in ((IMAGE, c["P_img"]), (TRIPLANE, c["P_tri"])):
        g.update({prefix + k: v.grad.double().numpy() for k, v in leaves[id(P)].items() if v.grad is not None})
    for (name, l, kind), v in DM.grads_of(params).items():
        g[f"{MODULES[name]}.{2 * l}.{kind}"] = v
    return {"error": float(error.detach()), "losses_all": losses_all.detach().double().numpy(), "grads": g,
            "preds": [[t.detach().double().numpy() for t in preds] for preds in preds_list]}


def losshead_losses(c, preds):
    """losses_all of tests/losshead_model.py on a run's predictions: the numpy restatement of the objective, held against DM.get_errors"""
    n = c["pts"].shape[1]
    stacked = [np.stack([p[h] for p in preds]) for h in range(5)]
    lab = c["labels"]
    pca, oc, vis = LH.per_point((lab["pca_axis"].reshape(-1, 9), lab["obj_center"], lab["visibility"]), n)
    return LH.loss_head(stacked, lab["df_h"], lab["df_o"], lab["labels"], pca, oc, vis, MAX_DIST)["losses_all"]


def gated(num_stack=NUM_STACK):
    """the parameter tensors the GPU test gates: every decoder tensor, the last stack's tail and the stem of each encoder"""
    last = num_stack - 1
    enc = list(EM.stem_make_params(1, 32, 0)) + [f"{n}{last}.{s}" for n in ("conv_last", "bn_end", "l") for s in ("weight", "bias")]
    return [f"{m}.{i}.{kind}" for m in MODULES.values() for i in (0, 2, 4, 6) for kind in ("weight", "bias")] + [p + k for p in (IMAGE, TRIPLANE) for k in enc]


def golden_sub(key):
    """what tests/golden/sifnet_step.npz keeps of a gated gradient: the GOLDEN_ROWS of a decoder's 128-row weight, every EM.GOLDEN_WEIGHT_STEP-th element of a
    convolution's flattened weight, everything else whole"""
    def sub(a):
        a = np.asarray(a)
        if a.ndim == 4:
            return a.reshape(-1)[::EM.GOLDEN_WEIGHT_STEP]
        return a[list(GOLDEN_ROWS)] if a.ndim == 2 and a.shape[0] == 128 else a
    return sub


def reference_and_e32(c):
    """-> (float64 run, e32): e32["losses_all"] (6,) and e32["grads"][key] = the largest element error of the float32 run"""
    r64, r32 = run(c, torch.float64), run(c, torch.float32)
    return r64, {"losses_all": np.abs(r64["losses_all"] - r32["losses_all"]), "error": abs(r64["error"] - r32["error"]),
                 "grads": {k: float(np.abs(r64["grads"][k] - r32["grads"][k]).max()) for k in r64["grads"]}}


def at_saved(c, gpu_maps, saved_img, saved_tri):
    """The float64 chain at a GPU forward's saved activations.  ``gpu_maps``: the S map sets as the GPU computed them (NCHW float64 arrays; shared tensors are
    shared objects, as stack_maps builds them); ``saved_*``: the tape of each encoder in EM.filter_saved_from_model's layout.  G.run gives the losses, the decoder
    gradients and the gradient to every map; the maps' gradients are the upstream of EM.filter_manual_grads.  -> run()'s dict (no "preds")"""
    b = c["images"].shape[0]
    r = G.run(c["dec"], gpu_maps, c["pts"], c["cc"], c["bc"], labels=c["labels"], max_dist=MAX_DIST)
    g = {f"{MODULES[name]}.{2 * l}.{kind}": v for (name, l, kind), v in r["grads"].items()}
    d_img = [r["dmaps"][s]["im_feat"] for s in range(len(gpu_maps))]
    d_tri = [np.concatenate([r["dmaps"][s][f"tri_feat{v}"] for v in range(3)], 0) for s in range(len(gpu_maps))]
    assert d_tri[0].shape[0] == 3 * b
    with concurrent.futures.ThreadPoolExecutor(2) as pool:            # the two encoders' chains are independent: side by side
        fi = pool.submit(EM.filter_manual_grads, c["P_img"], c["images"][:, :5], d_img, None, saved_img)
        ft = pool.submit(EM.filter_manual_grads, c["P_tri"], triplane_input(c["images"]), d_tri, None, saved_tri)
        gi, gt = fi.result(), ft.result()
    g.update({IMAGE + k: v for k, v in gi.items()})
    g.update({TRIPLANE + k: v for k, v in gt.items()})
    return {"error": r["error"], "losses_all": r["losses_all"], "grads": g}


def train(c, steps, lr=1e-3, dtype=torch.float64):
    """``steps`` steps of torch.optim.Adam on every parameter of both encoders and the decoders, one fixed batch -> the objective before every step"""
    pp = {id(P): {k: DM._t(v, dtype).requires_grad_(True) for k, v in P.items() if ".downsample.0" not in k} for P in (c["P_img"], c["P_tri"])}
    params = DM.make_params(c["dec"], dtype)
    opt = torch.optim.Adam([t for d in pp.values() for t in d.values()] + [t for n in DM.HEADS for wb in params[n] for t in wb], lr=lr)
    errors = []
    for _ in range(steps):
        opt.zero_grad()
        leaves = {}

        def run_filter(P, x):           # EM.filter_run makes its own leaves from arrays: run it on the current values, hand the gradients over afterwards
            outs, tmpx, _, p, _ = EM.filter_run({k: v.detach().numpy() for k, v in pp[id(P)].items()}, x, dtype, leaves=True)
            leaves[id(P)] = p
            return outs, tmpx

        error, _, _ = _objective(c, params, dtype, run_filter)
        error.backward()
        for i, d in pp.items():
            for k, v in d.items():
                v.grad = leaves[i][k].grad
        opt.step()
        errors.append(float(error.detach()))
    return errors
