"""One whole training step of the SIF-Net, training.SIFNetTrainer.train_step (both encoders, the five decoders, the loss, the backward, the three optimiser
steps), at B = 16, a 512 x 512 input, 3 stacks of depth 2 and the shipped sample count (num_samples_train = 20 000 points a frame, config tri-vis-l2), against the
torch composition of the same network on the same device in the same run: the encoders written with F.conv2d / F.group_norm / F.interpolate (channels-last), the
query with F.grid_sample, the decoders with torch.einsum, get_errors as tests/dectrain_model.py states it, autograd and ONE torch.optim.Adam over everything.

Synthetic weights (tests/sifnet_step_model.py's scale) and a synthetic labelled batch: the cost of a step does not depend on the values.  Median of 5 rounds after
warm-up, device time by events around `iters` back-to-back steps.

    python tools/bench_scripts/trainstepbench.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import dectrain_model as DM  # noqa: E402
import enctrain_model as EM  # noqa: E402
import sifnet_step_model as SM  # noqa: E402
from vistracker_amd.training import SIFNetTrainer  # noqa: E402

DEV, B, S, N, STACKS, DEPTH = "cuda:0", 16, 512, 20000, 3, 2
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def timed(fn, iters, rounds=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ms), min(ms), max(ms)


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def torch_filter(tp, x, stacks, depth):
    def blk(n, t):
        return EM._block({k[len(n) + 1:]: v for k, v in tp.items() if k.startswith(n + ".")}, t)[0]

    def level(i, n, t):
        up1 = blk(f"m{i}.b1_{n}", t)
        low = blk(f"m{i}.b2_{n}", F.avg_pool2d(t, 2, stride=2))
        low = level(i, n - 1, low) if n > 1 else blk(f"m{i}.b2_plus_1", low)
        return up1 + F.interpolate(blk(f"m{i}.b3_{n}", low), scale_factor=2, mode="bicubic", align_corners=True)

    t, _ = EM.stem_forward(tp, x)
    previous = blk("conv4", blk("conv3", F.avg_pool2d(blk("conv2", t), 2, stride=2)))
    outs = []
    for i in range(stacks):
        o, p2, _ = EM.tail_forward(EM.filter_tail_params(tp, i), blk(f"top_m_{i}", level(i, depth, previous)), previous)
        outs.append(o)
        previous = p2 if p2 is not None else previous
    return outs, t.detach()


def main():
    say(f"trainstepbench: B = {B}, input {S} x {S}, {STACKS} stacks of depth {DEPTH}, N = {N} points a frame, {torch.cuda.get_device_name(0)}; median (min .. max) of 5 rounds")
    cin_i, tmpx_i, hg_i, _ = EM.FILTER_CASES["image"]
    cin_t, tmpx_t, hg_t, _ = EM.FILTER_CASES["triplane"]
    c = dict(P_img=EM.filter_make_params(cin_i, tmpx_i, hg_i, STACKS, DEPTH, 1), P_tri=EM.filter_make_params(cin_t, tmpx_t, hg_t, STACKS, DEPTH, 2), dec=SM.make_decoders(3))
    rng = np.random.default_rng(0)
    bc = np.tile(np.array([[0.0, 0.0, 2.2]], np.float32), (B, 1))
    pts = (bc[:, None] + rng.normal(0, 0.3, (B, N, 3))).astype(np.float32)
    cc = np.tile(np.array([[1018.952, 779.486]], np.float32), (B, 1))
    lab = DM.make_labels(B, N, 5)
    dev = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=DEV)      # noqa: E731
    batch = {"points": dev(pts), "df_h": dev(lab["df_h"]), "df_o": dev(lab["df_o"]), "labels": dev(lab["labels"], torch.int32), "pca_axis": dev(lab["pca_axis"]),
             "body_center": dev(bc), "obj_center": dev(lab["obj_center"]), "visibility": dev(lab["visibility"])}
    images, ccd = torch.rand(B, 8, S, S, device=DEV), dev(cc)

    tr = SIFNetTrainer(SM.state_dict(c), None, num_stack=STACKS, num_hourglass=DEPTH, triplane_stack=STACKS, device=DEV)
    ours = timed(lambda: tr.train_step(batch, images, ccd), 2)
    say(f"SIFNetTrainer.train_step: {ours[0]:.1f} ms ({ours[1]:.1f} .. {ours[2]:.1f})")
    del tr
    torch.cuda.empty_cache()

    def leaves(P):
        return {k: (cl(torch.as_tensor(v).to(DEV)) if v.ndim == 4 else torch.as_tensor(v).to(DEV)).requires_grad_(True) for k, v in P.items() if ".downsample.0" not in k}

    p_img, p_tri = leaves(c["P_img"]), leaves(c["P_tri"])
    params = {n: [(dev(w).requires_grad_(True), dev(b).requires_grad_(True)) for w, b in c["dec"][n]] for n in DM.HEADS}
    opt = torch.optim.Adam(list(p_img.values()) + list(p_tri.values()) + [t for n in DM.HEADS for wb in params[n] for t in wb], lr=1e-3)
    labt = {k: dev(v, torch.int64 if k == "labels" else torch.float32) for k, v in lab.items()}
    xi, xt = cl(images[:, :5]), cl(images[:, 5:8].transpose(0, 1).reshape(3 * B, 1, S, S))
    p, bcd = batch["points"], batch["body_center"]

    def sample(m, u, v):
        return F.grid_sample(m, torch.stack([u, v], -1)[:, :, None], mode="bilinear", padding_mode="zeros", align_corners=True)[..., 0]

    def torch_step():
        opt.zero_grad(set_to_none=True)
        oi, tmpx = torch_filter(p_img, xi, STACKS, DEPTH)
        ot, ttmpx = torch_filter(p_tri, xt, STACKS, DEPTH)
        pr = DM.projections(p, ccd, bcd)
        z = torch.stack([p[..., 0], p[..., 1], p[..., 2] - 2.2], 1)
        u, v = pr["persp"]
        in_img = (u >= -1) & (u <= 1) & (v >= -1) & (v <= 1)
        kinds = ("right", "back", "top")
        shared = [sample(tmpx, u, v)] + [sample(ttmpx[k * B:(k + 1) * B], *pr[kinds[k]]) for k in range(3)]
        preds_list = []
        for s in range(STACKS):
            feat = torch.cat([sample(oi[s], u, v), z] + shared + [sample(ot[s][k * B:(k + 1) * B], *pr[kinds[k]]) for k in range(3)], 1)
            preds_list.append(DM.decode(params, feat, in_img))
        error, _ = DM.get_errors(preds_list, labt, 5.0)
        error.backward()
        opt.step()

    ref = timed(torch_step, 2)
    say(f"torch composition (autograd, torch.optim.Adam): {ref[0]:.1f} ms ({ref[1]:.1f} .. {ref[2]:.1f}) | ratio torch / ours {ref[0] / ours[0]:.2f}")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
