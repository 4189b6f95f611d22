"""Cost of the gradient to SIF-Net's feature maps at the reference's training shape: vt_decoder_grads (csrc/dectrain.hip, section 5) with weights + maps, maps
only (dparams NULL) and weights only (d_maps NULL), each against the torch composition dectrainbench.py builds (F.grid_sample + conv1d + autograd, here with
the maps requiring grad where the kernel computes them), and weights only also against vt_decoder_weight_grads, the entry the parent already had (the same
kernels behind it: it must not have become slower beyond the run-to-run spread).

Shape: batch_size = 8, num_samples_train = 20000, full-resolution maps, S = 1 and S = 3 stacks (stacks share their tmpx tensors; the kernel adds into one
buffer with accumulate_maps, autograd adds for the composition).

Timing: device events around `--reps` back-to-back calls after `--warmup`, `--rounds` rounds alternating all variants; median round [min .. max].

usage: python tools/bench_scripts/mapgradbench.py [--batch 8] [--points 20000] [--out profiles/r16_mapgrad.txt]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dectrainbench import Composition, event_ms  # noqa: E402
from vistracker_amd import _lib as L, ops, synthetic as syn, training  # noqa: E402
from vistracker_amd.sifnet import SIFNetQuery  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--res-scale", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mapgradbench: needs the GPU; nothing here can be timed without it")
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    B, N = a.batch, a.points
    say(f"mapgradbench: B = {B}, N = {N}, maps at res_scale {a.res_scale:g}, {torch.cuda.get_device_name(0)}")
    say(f"  {a.rounds} rounds of {a.reps} calls after {a.warmup} warm-up calls, device events; median round [min .. max]")
    rng = np.random.default_rng(0)
    dev = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")      # noqa: E731
    base = {k: dev(v) for k, v in syn.feature_maps(B, res_scale=a.res_scale).items()}
    nchw = [base] + [{k: (v if "tmpx" in k else torch.randn_like(v)) for k, v in base.items()} for _ in range(2)]
    fms = [ops.FeatureMaps.from_nchw(m) for m in nchw]
    bc = dev(rng.normal(0, 0.05, (B, 3)) + [0, 0, 2.2]); cc = dev([[1018.952, 779.486]] * B)
    pts = dev(rng.normal(0, 0.3, (B, N, 3))) + bc[:, None]
    net = SIFNetQuery(syn.sifnet_decoders(3))
    net.set_feature_maps(fms[0])
    lib = L.lib()
    shared = [i for i, k in enumerate(ops.MAP_ORDER) if "tmpx" in k]
    for S in (1, 3):
        p = training.DecoderTrainer(net).params
        comp = Composition(p, net.camera.as_cam5())
        ups = [[torch.randn(B, k, N, device="cuda") for k in ops.HEAD_DIMS] for _ in range(S)]
        dflat = torch.empty_like(p.flat.detach())
        ws = torch.empty(lib.vt_decoder_grads_ws_bytes(B, N, 0, 1) // 4 + 4, device="cuda")
        # gradient buffers: one set per stack, the tmpx ones shared (stack s > 0 adds into stack 0's)
        dbuf = [[torch.empty_like(t) for t in fms[s].t] for s in range(S)]
        for s in range(1, S):
            for i in shared:
                dbuf[s][i] = dbuf[0][i]
        dms = []
        for s in range(S):
            dm = L.VtMaps()
            for i, t in enumerate(dbuf[s]):
                dm.maps[i] = t.data_ptr(); dm.res[i] = t.shape[1]
            dms.append(dm)
        # accumulate_maps is one flag per call: a stack s > 0 takes two calls' worth of semantics in one by zeroing its own buffers first
        own = [[t for i, t in enumerate(dbuf[s]) if i not in shared] for s in range(S)]

        def grads(weights, maps, old=False):
            for s in range(S):
                args = (p.flat.data_ptr(), p.cam.ctypes.data, C.byref(fms[s].c), pts.data_ptr(), cc.data_ptr(), bc.data_ptr(), B, N, *[t.data_ptr() for t in ups[s]],
                        dflat.data_ptr() if weights else None, 1 if s else 0)
                if old:
                    L.check(lib.vt_decoder_weight_grads(*args, 0, ws.data_ptr(), L.stream_ptr()))
                    continue
                if maps and s:
                    for t in own[s]:
                        t.zero_()
                L.check(lib.vt_decoder_grads(*args, C.byref(dms[s]) if maps else None, 1 if s else 0, 0, ws.data_ptr(), L.stream_ptr()))

        leaves = [{k: v.clone().requires_grad_(True) for k, v in nchw[0].items()}]
        leaves += [{k: (leaves[0][k] if "tmpx" in k else v.clone().requires_grad_(True)) for k, v in nchw[s].items()} for s in range(1, S)]

        def comp_grads(weights, maps):
            for t in comp.w.values():
                t.grad = None; t.requires_grad_(weights)
            for m in leaves:
                for t in m.values():
                    t.grad = None
            preds = comp.query(leaves if maps else nchw[:S], pts, cc, bc)
            sum((t * g).sum() for ps, gs in zip(preds, ups) for t, g in zip(ps, gs)).backward()

        # the same numbers first
        grads(True, True); comp_grads(True, True)
        worst = 0.0
        for s in range(S):
            for i, k in enumerate(ops.MAP_ORDER):
                want = leaves[s][k].grad.permute(0, 2, 3, 1)
                worst = max(worst, float((dbuf[s][i] - want).abs().max() / want.abs().max()))
        say(f"S = {S}: kernel against composition, map gradients: worst tensor max |difference| / max |gradient| {worst:.2e}")
        fns = {"k_both": lambda: grads(True, True), "c_both": lambda: comp_grads(True, True), "k_maps": lambda: grads(False, True),
               "c_maps": lambda: comp_grads(False, True), "k_weights": lambda: grads(True, False), "c_weights": lambda: comp_grads(True, False),
               "k_weights_old": lambda: grads(True, False, old=True)}
        res = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k in res:
                res[k].append(event_ms(fns[k], a.warmup, a.reps))
        med = {k: float(np.median(v)) for k, v in res.items()}
        fmt = lambda k: f"{med[k]:8.3f} ms [{min(res[k]):.3f} .. {max(res[k]):.3f}]"      # noqa: E731
        for what, kk, ck in (("weights + maps", "k_both", "c_both"), ("maps only     ", "k_maps", "c_maps"), ("weights only   ", "k_weights", "c_weights")):
            say(f"  {what}: vt_decoder_grads {fmt(kk)}   torch composition {fmt(ck)}   x{med[ck] / med[kk]:.2f}")
        say(f"  weights only   : vt_decoder_weight_grads (the parent's entry) {fmt('k_weights_old')}   vt_decoder_grads / it = {med['k_weights'] / med['k_weights_old']:.3f}")
        del comp, leaves
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
