"""What the step guard and the gradient record add to a step of training.SIFNetTrainer, at the README's training size (B = 16, a 512 x 512 input, 3 stacks of
depth 2, 20 000 points a frame: the sizes of trainstepbench.py and ddpbench.py), on ONE GPU.  Cross-GPU behaviour is not measured.

  (a) vt_grad_stats over the image encoder's flat gradient with its leaves as segments, against two read rates measured in the same run: vt_grad_rank_mean with
      W = 1 (reads and writes n floats) and a float4 copy (torch's copy_ of the same buffer);
  (b) StepGuard.close over the three buffers: without clipping, with a norm that never bites (the scale launches return at once), with one that bites;
  (c) train_step with the guard off, on, and on with clipping, ALTERNATING in one process: every round runs the three once, in turn.

Synthetic weights and batch as trainstepbench.py.  Median (min .. max) of the rounds after warm-up, device time by events.

    python tools/bench_scripts/guardbench.py [out.txt]
    python tools/bench_scripts/guardbench.py --plain-step [--root CHECKOUT] [out.txt]     # only the unguarded train_step, from the package of another checkout
                                                                                         # (the parent commit's): run in turn with this one's for the A/B"""
import os
import statistics
import sys

args = sys.argv[1:]
plain_only = "--plain-step" in args
if plain_only:
    args.remove("--plain-step")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HERE = ROOT
if "--root" in args:
    i = args.index("--root")
    ROOT = os.path.abspath(args[i + 1])
    del args[i:i + 2]
OUT = args[0] if args else None

import numpy as np  # noqa: E402
import torch  # noqa: E402

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


def alternating(fns, rounds=6, warm=1):
    """every round runs each of ``fns`` once, in turn -> [(median, min, max)] in ms"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def fmt(t, unit="ms"):
    k = 1e3 if unit == "us" else 1.0
    return f"{t[0] * k:.1f} {unit} ({t[1] * k:.1f} .. {t[2] * k:.1f})"


def main():
    torch.cuda.set_device(0)
    say(f"guardbench: B = {B}, input {S} x {S}, {STACKS} stacks of depth {DEPTH}, N = {N} points a frame, {torch.cuda.get_device_name(0)}; median (min .. max)"
        + (f"; package of {ROOT}" if plain_only else ""))
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
    sd = SM.state_dict(c)

    def make(**kw):
        return SIFNetTrainer(sd, None, num_stack=STACKS, num_hourglass=DEPTH, triplane_stack=STACKS, device=DEV, lr=1e-5, **kw)

    if plain_only:
        tr = make()
        say(f"train_step, no guard: {fmt(timed(lambda: tr.train_step(batch, images, ccd), 2, rounds=6))}")
        return

    from vistracker_amd import ops
    off, on = make(), make(guard=True, record=8)
    # (a) the kernel alone, on a real gradient
    on.backward(batch, images, ccd)
    grads = [g.detach().clone() for g in on.flat_grads()]
    g, seg = grads[0], on.guard._seg[0]
    n, n_seg = g.numel(), seg.shape[0]
    say(f"flat gradient buffers: image encoder {n} floats in {n_seg} leaves, triplane encoder {grads[1].numel()} in {on.guard._seg[1].shape[0]}, decoders "
        f"{grads[2].numel()} in {on.guard._seg[2].shape[0]} ({sum(x.numel() for x in grads) * 4 / 1e6:.1f} MB)")
    out, ws = on.guard._out[0], on.guard._ws[0]
    st = timed(lambda: ops.grad_stats(g, seg, ws=ws, out=out), 50)
    dst = torch.empty_like(g)
    mean = timed(lambda: ops.grad_rank_mean(g.view(1, -1), out=dst), 50)
    cp = timed(lambda: dst.copy_(g), 50)
    say(f"(a) vt_grad_stats, n = {n}, {n_seg} segments (three launches): {fmt(st, 'us')} | reads {4 * n / 1e6:.1f} MB at {4 * n / st[0] / 1e9:.2f} TB/s")
    say(f"    vt_grad_rank_mean W = 1 (reads n, writes n): {fmt(mean, 'us')} | reads at {4 * n / mean[0] / 1e9:.2f} TB/s, moves {8 * n / mean[0] / 1e9:.2f} TB/s")
    say(f"    float4 copy of the same buffer: {fmt(cp, 'us')} | reads at {4 * n / cp[0] / 1e9:.2f} TB/s, moves {8 * n / cp[0] / 1e9:.2f} TB/s"
        + (" (the buffer fits the 256 MiB Infinity Cache: cache rates, not HBM's)" if 8 * n < 256 * 2 ** 20 else ""))

    # (b) the whole close
    err = torch.tensor(1.0, dtype=torch.float64, device=DEV)
    norm = None
    for label, kw in (("no clipping", {}), ("clip_norm 1e30 (never bites)", dict(max_norm=1e30)), ("clip_norm = half the norm (bites)", "half")):
        if kw == "half":
            kw = dict(max_norm=0.5 * norm)
        guard = ops.StepGuard(grads, [[(int(b), int(e - b)) for b, e in s.cpu().tolist()] for s in on.guard._seg],
                              [[f"{k}.{i}" for i in range(s.shape[0])] for k, s in enumerate(on.guard._seg)], record=8, **kw)
        work = [x.clone() for x in grads]

        def close():
            for w, x in zip(work, grads):
                w.copy_(x)
            guard.close(work, err)

        def copies():
            for w, x in zip(work, grads):
                w.copy_(x)

        t, t0 = timed(close, 20), timed(copies, 20)
        norm = guard.read()["norm"]
        say(f"(b) StepGuard.close, {label}: {guard.launches_per_close} launches, {(t[0] - t0[0]) * 1e3:.1f} us (with the three restoring copies {fmt(t, 'us')}, the copies alone"
            f" {fmt(t0, 'us')}); norm {norm:.4e}")
    del guard, work, grads, dst

    # (c) the step
    clip = make(guard=True, clip_norm=0.5 * norm, record=8)
    trs = (("guard off", off), ("guard on, record 8", on), ("guard on, clip_norm = half the first norm", clip))
    res = alternating([lambda t=t: t.train_step(batch, images, ccd) for _, t in trs])
    for (label, t), r in zip(trs, res):
        say(f"(c) train_step, {label}: {fmt(r)} | against guard off: {r[0] - res[0][0]:+.2f} ms ({(r[0] / res[0][0] - 1) * 100:+.2f} %)")
    rec = clip.guard.read()
    say(f"    the clipped trainer's record: {rec['steps']} steps, {rec['skipped']} skipped, last norm {rec['norm']:.4e}, coef {rec['coef']:.4f}")


if __name__ == "__main__":
    main()
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")
