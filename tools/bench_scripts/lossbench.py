"""Cost of SIF-Net's training objective at the reference's training shape: the fused loss head (csrc/losshead.hip: values and the gradient to every prediction in
one launch + a small reduction launch) against the torch composition of the same expression on the same box -- the only way to compute the objective without
the kernel: the expression of get_errors (model/chore_tri_vis.py:52-99) in float32 torch ops followed by error.backward() -- and against the floor

    bytes the kernel must move / 6.29 TB/s (the delivered bandwidth DESIGN.md uses)

Shape: batch_size = 8 (config/tri-vis-l2.json:14), total_sample_num = num_samples_train = 20000 (:18, train_launch.py:63), at S = 3 stacks (num_stack, :59: the
training forward) and S = 1 (the eval-mode query).  Bytes per point: 29 S predictions read + 29 S gradients written + 3 labels read (df_h, df_o, parts_gt; the
per-frame labels are 13 floats per FRAME), 4 bytes each; the values-only call moves half of the first two.

Timing: device events around `--reps` back-to-back calls after `--warmup` calls, repeated `--rounds` times alternating kernel and composition; the median
round is reported with the spread.  Both sides produce the same outputs (error, six losses, five gradient tensors); allocation of the outputs is inside both.

usage: python tools/bench_scripts/lossbench.py [--batch 8] [--points 20000] [--out profiles/r14_losshead.txt]
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
from vistracker_amd import _lib as L, ops  # noqa: E402

BW = 6.29e12
WEIGHTS = ops.LOSS_WEIGHTS


def torch_objective(stacks, df_h, df_o, parts_gt, pca_gt, obj_center, vis_gt, max_dist):
    """get_errors (chore_tri_vis.py:52-99, vis_loss l2) as the reference writes it, per-point labels as its loader delivers them"""
    error, losses_all = 0.0, 0.0
    mask_o = (df_o < 0.05).unsqueeze(1)
    for df, pca, parts, centers, vis in stacks:
        dfl = lambda g, p: F.l1_loss(torch.clamp(p, max=max_dist), torch.clamp(g, max=max_dist), reduction="none").sum(-1).mean()      # noqa: E731
        loss_h, loss_o = dfl(df_h, df[:, 0]) * WEIGHTS[0], dfl(df_o, df[:, 1]) * WEIGHTS[1]
        loss_parts = (F.cross_entropy(parts, parts_gt, reduction="none") * WEIGHTS[2]).sum(-1).mean()
        loss_pca = ((F.mse_loss(pca, pca_gt, reduction="none") * mask_o) * WEIGHTS[3]).mean()
        loss_obj = (F.mse_loss(centers, obj_center, reduction="none") * mask_o).mean() * WEIGHTS[4]
        loss_vis = (F.mse_loss(vis, vis_gt.unsqueeze(1), reduction="none") * mask_o).mean() * WEIGHTS[5]
        error = error + loss_h + loss_o + loss_parts + loss_pca + loss_vis + loss_obj
        losses_all = losses_all + torch.stack([loss_h, loss_o, loss_parts, loss_pca, loss_vis, loss_obj]).detach()
    return error / len(stacks), losses_all / len(stacks)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lossbench: needs the GPU; nothing here can be timed without it")
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    B, N = a.batch, a.points
    say(f"lossbench: B = {B} (batch_size, config/tri-vis-l2.json:14), N = {N} (num_samples_train = total_sample_num, :18), {torch.cuda.get_device_name(0)}")
    say(f"  {a.rounds} rounds of {a.reps} calls after {a.warmup} warm-up calls, device events; median round [min .. max]")
    rng = np.random.default_rng(0)
    dev = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")      # noqa: E731
    df_h, df_o = dev(rng.uniform(0, 1, (B, N))), dev(np.where(rng.random((B, N)) < 0.4, rng.uniform(0, 0.05, (B, N)), rng.uniform(0.05, 1, (B, N))))
    parts_i = dev(rng.integers(0, 14, (B, N)), torch.int32); parts_l = parts_i.long()
    pca_f, oc_f, vis_f = dev(rng.normal(size=(B, 9))), dev(rng.normal(0, 0.4, (B, 3))), dev(rng.uniform(0.1, 1, (B,)))
    pca_p, oc_p, vis_p = (t.unsqueeze(-1).expand(*t.shape, N).contiguous() for t in (pca_f, oc_f, vis_f))
    for S in (3, 1):
        heads = [dev(rng.normal(0, 1, (S, B, k, N))).requires_grad_(True) for k in ops.HEAD_DIMS]
        heads_ng = [h.detach() for h in heads]

        def fused():
            for h in heads:
                h.grad = None
            err, la = ops.sifnet_loss_head(heads, df_h, df_o, parts_i, pca_f, oc_f, vis_f, max_dist=5.0)
            err.backward()
            return err, la

        def fused_values():
            return ops.sifnet_loss_head(heads_ng, df_h, df_o, parts_i, pca_f, oc_f, vis_f, max_dist=5.0)

        def composed():
            for h in heads:
                h.grad = None
            err, la = torch_objective([tuple(h[s] for h in heads) for s in range(S)], df_h, df_o, parts_l, pca_p, oc_p, vis_p, 5.0)
            err.backward()
            return err, la

        def composed_values():
            with torch.no_grad():
                return torch_objective([tuple(h[s] for h in heads_ng) for s in range(S)], df_h, df_o, parts_l, pca_p, oc_p, vis_p, 5.0)

        terms = torch.empty(6, dtype=torch.float64, device="cuda"); gbuf = [torch.empty_like(h) for h in heads_ng]
        ws = torch.empty(L.lib().vt_sifnet_loss_head_ws_bytes(B, N) // 8, dtype=torch.float64, device="cuda")
        w6 = (C.c_double * 6)(*WEIGHTS)

        def raw(grads=True):
            L.check(L.lib().vt_sifnet_loss_head(*[h.data_ptr() for h in heads_ng], S, B, N, df_h.data_ptr(), df_o.data_ptr(), parts_i.data_ptr(), pca_f.data_ptr(),
                                                oc_f.data_ptr(), vis_f.data_ptr(), 1, 5.0, w6, 1, 1.0, terms.data_ptr(),
                                                *[(g.data_ptr() if grads else None) for g in gbuf], ws.data_ptr(), L.stream_ptr()))

        # the same numbers first (float32 composition against the fp64-accumulating kernel: relative differences of float32 rounding)
        e_k, l_k = fused(); g_k = [h.grad.clone() for h in heads]
        e_t, l_t = composed(); g_t = [h.grad.clone() for h in heads]
        rel = float(((l_k - l_t.double()).abs() / l_t.double().abs()).max())
        gerr = max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(g_k, g_t))
        say(f"S = {S}: kernel against composition: losses max relative difference {rel:.2e}, gradients max |difference| / max |gradient| {gerr:.2e}")
        moved = B * N * (29 * S * 2 + 3) * 4 + B * 13 * 4
        moved_v = B * N * (29 * S + 3) * 4 + B * 13 * 4
        res = {k: [] for k in ("raw", "raw_values", "fused", "composed", "fused_values", "composed_values")}
        for _ in range(a.rounds):
            for k, fn in (("raw", raw), ("raw_values", lambda: raw(False)), ("fused", fused), ("composed", composed), ("fused_values", fused_values), ("composed_values", composed_values)):
                res[k].append(event_ms(fn, a.warmup, a.reps))
        med = {k: float(np.median(v)) for k, v in res.items()}
        for k, label, byt in (("raw", "values + gradients, C call  ", moved), ("fused", "values + gradients, op + bwd", moved),
                              ("raw_values", "values only, C call         ", moved_v), ("fused_values", "values only, op             ", moved_v)):
            floor = byt / BW * 1e3
            comp = "composed_values" if "values" in k else "composed"
            say(f"  {label}: kernel {med[k] * 1e3:8.1f} us [{min(res[k]) * 1e3:.1f} .. {max(res[k]) * 1e3:.1f}]   torch composition {med[comp] * 1e3:8.1f} us "
                f"[{min(res[comp]) * 1e3:.1f} .. {max(res[comp]) * 1e3:.1f}]   x{med[comp] / med[k]:.1f}   floor {floor * 1e3:.1f} us ({byt / 1e6:.1f} MB): "
                f"{100 * floor / med[k]:.0f} % of the floor's rate reached")
    say("  (C call = vt_sifnet_loss_head on preallocated buffers: the two launches; op = ops.sifnet_loss_head: the shim, the allocation of its outputs and, with")
    say("   gradients, autograd's backward -- host time is in those numbers, as it is in the composition's)")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
