"""Cost of training SIF-Net's five point decoders (feature maps frozen) at the reference's training shape: csrc/dectrain.hip -- the forward from plain weights
(vt_decoder_train_forward), the weight-gradient call (vt_decoder_weight_grads: features, taped forward, delta propagation, split-K weight-gradient GEMMs, fp64
finish) and a whole training.DecoderTrainer.train_step -- against the torch composition of the same expression on the same box: F.grid_sample + conv1d +
autograd (+ torch.optim.Adam for the step).  The parent of this kernel file has no such path, so the composition is the only honest comparison.

Shape: batch_size = 8 (config/tri-vis-l2.json:14), num_samples_train = 20000 (:18), full-resolution maps, S = 1 and S = 3 stacks (num_stack, :59).

Flop count per point and stack, multiply-add = 2 (layer sizes 611-128-128-128-k, k = 2, 9, 14, 3, 1, sum 29):
    forward             2 x (5 x (611 x 128 + 2 x 128 x 128) + 128 x 29) = 1 117 184
    delta propagation   2 x (5 x 2 x 128 x 128 + 128 x 29)               =   335 104      (no layer-1 backward to the features)
    weight gradients    = forward                                        = 1 117 184
x 160 000 points = 0.179 + 0.054 + 0.179 = 0.411 TFLOP per stack for the gradient call (its forward is inside it), 0.179 for the forward alone; a train step
runs both (the forward that yields the predictions, then the gradient call): 0.590 TFLOP per stack.  Rates are quoted against 157.3 TFLOP/s (fp32-input MFMA).

Timing: device events around `--reps` back-to-back calls after `--warmup`, `--rounds` rounds alternating kernel and composition; median round [min .. max].

usage: python tools/bench_scripts/dectrainbench.py [--batch 8] [--points 20000] [--out profiles/r15_dectrain.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vistracker_amd import _lib as L, ops, synthetic as syn, training  # noqa: E402
from vistracker_amd.sifnet import SIFNetQuery  # noqa: E402

PEAK = 157.3e12
FWD, DELTA = 1117184, 335104


def event_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record(); torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


class Composition:
    """the decoders as torch leaves and the query as the reference composes it (chore_triplane.py:97-164) on NCHW maps"""

    def __init__(self, params: ops.DecoderParams, cam):
        self.w = {k: v.clone().requires_grad_(True) for k, v in params.views.items()}
        self.cam = cam
        self.opt = torch.optim.Adam(list(self.w.values()), lr=1e-3)

    def query(self, maps_list, pts, cc, bc):
        fx, fy, cx, cy, crop = self.cam
        x, y, z = pts[..., 0], pts[..., 1], pts[..., 2]
        u = 2 * (crop / 2 + fx * x / z + cx - cc[:, 0:1]) / crop - 1
        v = 2 * (crop / 2 + fy * y / z + cy - cc[:, 1:2]) / crop - 1
        c = pts - bc[:, None]
        grids = {"persp": torch.stack([u, v], -1), "right": torch.stack([c[..., 2], c[..., 1]], -1), "back": torch.stack([-c[..., 0], c[..., 1]], -1),
                 "top": torch.stack([c[..., 0], -c[..., 2]], -1)}
        idx = lambda m, k: F.grid_sample(m, grids[k][:, :, None, :], mode="bilinear", padding_mode="zeros", align_corners=True)[..., 0]      # noqa: E731
        in_img = (u >= -1) & (u <= 1) & (v >= -1) & (v <= 1)
        z_feat = torch.stack([x, y, z - 2.2], 1)
        out = []
        for m in maps_list:
            feat = torch.cat([idx(m["im_feat"], "persp"), z_feat, idx(m["tmpx"], "persp"), idx(m["tri_tmpx0"], "right"), idx(m["tri_tmpx1"], "back"),
                              idx(m["tri_tmpx2"], "top"), idx(m["tri_feat0"], "right"), idx(m["tri_feat1"], "back"), idx(m["tri_feat2"], "top")], 1)
            preds = []
            for name in ops.HEADS:
                h = feat
                for l in range(4):
                    h = F.conv1d(h, self.w[(name, l, "weight")].unsqueeze(-1), self.w[(name, l, "bias")])
                    h = torch.relu(h) if l < 3 else h
                if name == "vis":
                    h = torch.sigmoid(h)
                if name == "df":
                    h = torch.where(in_img[:, None], h, torch.full_like(h, 5.0))
                preds.append(h)
            out.append(tuple(preds))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--res-scale", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dectrainbench: needs the GPU; nothing here can be timed without it")
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    B, N = a.batch, a.points
    say(f"dectrainbench: B = {B}, N = {N}, maps at res_scale {a.res_scale:g}, {torch.cuda.get_device_name(0)}")
    say(f"  {a.rounds} rounds of {a.reps} calls after {a.warmup} warm-up calls, device events; median round [min .. max]; rates against {PEAK / 1e12:.1f} TFLOP/s")
    rng = np.random.default_rng(0)
    dev = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")      # noqa: E731
    base = {k: dev(v) for k, v in syn.feature_maps(B, res_scale=a.res_scale).items()}
    nchw = [base] + [{k: (v if "tmpx" in k else torch.randn_like(v)) for k, v in base.items()} for _ in range(2)]
    fms = [ops.FeatureMaps.from_nchw(m) for m in nchw]
    bc = dev(rng.normal(0, 0.05, (B, 3)) + [0, 0, 2.2]); cc = dev([[1018.952, 779.486]] * B)
    pts = dev(rng.normal(0, 0.3, (B, N, 3))) + bc[:, None]
    net = SIFNetQuery(syn.sifnet_decoders(3))
    net.set_feature_maps(fms[0])
    batch = {"points": pts, "body_center": bc, "df_h": dev(rng.uniform(0, 0.6, (B, N))),
             "df_o": dev(np.where(rng.random((B, N)) < 0.5, rng.uniform(0, 0.05, (B, N)), rng.uniform(0.05, 0.8, (B, N)))),
             "labels": dev(rng.integers(0, 14, (B, N)), torch.int32), "pca_axis": dev(np.linalg.qr(rng.normal(size=(B, 3, 3)))[0]),
             "obj_center": dev(rng.normal(0, 0.4, (B, 3))), "visibility": dev(rng.uniform(0.1, 1, (B,)))}
    lib = L.lib()
    for S in (1, 3):
        tr = training.DecoderTrainer(net)
        p = tr.params
        comp = Composition(p, net.camera.as_cam5())
        outs = [[torch.empty(B, k, N, device="cuda") for k in ops.HEAD_DIMS] for _ in range(S)]
        ups = [[torch.randn(B, k, N, device="cuda") for k in ops.HEAD_DIMS] for _ in range(S)]
        dflat = torch.empty_like(p.flat.detach())
        ws = torch.empty(lib.vt_decoder_weight_grads_ws_bytes(B, N, 0) // 4 + 4, device="cuda")
        common = (p.cam.ctypes.data,)

        def k_forward():
            for s in range(S):
                L.check(lib.vt_decoder_train_forward(p.flat.data_ptr(), *common, C.byref(fms[s].c), pts.data_ptr(), cc.data_ptr(), bc.data_ptr(), B, N,
                                                     *[t.data_ptr() for t in outs[s]], L.stream_ptr()))

        def k_grads():
            for s in range(S):
                L.check(lib.vt_decoder_weight_grads(p.flat.data_ptr(), *common, C.byref(fms[s].c), pts.data_ptr(), cc.data_ptr(), bc.data_ptr(), B, N,
                                                    *[t.data_ptr() for t in ups[s]], dflat.data_ptr(), 1 if s else 0, 0, ws.data_ptr(), L.stream_ptr()))

        def k_step():
            tr.train_step(batch, cc, maps=fms[:S])

        def c_forward():
            with torch.no_grad():
                return comp.query(nchw[:S], pts, cc, bc)

        def c_grads():
            for t in comp.w.values():
                t.grad = None
            preds = comp.query(nchw[:S], pts, cc, bc)
            sum((t * g).sum() for ps, gs in zip(preds, ups) for t, g in zip(ps, gs)).backward()

        def c_step():
            comp.opt.zero_grad()
            preds = comp.query(nchw[:S], pts, cc, bc)
            error, _ = ops.sifnet_loss_head([(d, q.view(B, 3, 3, N), pa, ce, vi) for d, q, pa, ce, vi in preds], batch["df_h"], batch["df_o"], batch["labels"],
                                            batch["pca_axis"], batch["obj_center"], batch["visibility"], max_dist=5.0)
            error.backward()
            comp.opt.step()

        # the same numbers first
        k_forward(); ref = c_forward()
        ferr = max(float((x - y).abs().max()) for x, y in zip(outs[0], ref[0]))
        k_grads(); c_grads()
        got = ops.DecoderParams(dflat.clone()).views
        gerr = max(float((got[k] - comp.w[k].grad).abs().max() / comp.w[k].grad.abs().max()) for k in got)
        say(f"S = {S}: kernel against composition: predictions max |difference| {ferr:.2e}; weight gradients, worst tensor max |difference| / max |gradient| {gerr:.2e}")
        res = {k: [] for k in ("k_forward", "c_forward", "k_grads", "c_grads", "k_step", "c_step")}
        fns = dict(k_forward=k_forward, c_forward=c_forward, k_grads=k_grads, c_grads=c_grads, k_step=k_step, c_step=c_step)
        for _ in range(a.rounds):
            for k in res:
                res[k].append(event_ms(fns[k], a.warmup, a.reps))
        med = {k: float(np.median(v)) for k, v in res.items()}
        pts_all = B * N * S
        for what, flops, kk, ck, note in (("forward      ", FWD * pts_all, "k_forward", "c_forward", "C call, preallocated outputs"),
                                          ("gradient call", (2 * FWD + DELTA) * pts_all, "k_grads", "c_grads", "C call; composition = forward + backward"),
                                          ("train_step   ", (3 * FWD + DELTA) * pts_all, "k_step", "c_step", "DecoderTrainer; composition = torch forward, fused loss head, backward, optim.Adam")):
            say(f"  {what}: kernel {med[kk]:8.3f} ms [{min(res[kk]):.3f} .. {max(res[kk]):.3f}]   torch composition {med[ck]:8.3f} ms [{min(res[ck]):.3f} .. {max(res[ck]):.3f}]"
                f"   x{med[ck] / med[kk]:.2f}   {flops / 1e12:.3f} TFLOP -> {flops / (med[kk] * 1e-3) / 1e12:.1f} TFLOP/s = {100 * flops / (med[kk] * 1e-3) / PEAK:.1f} % of the fp32-MFMA rate   ({note})")
        del comp, tr
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
