"""What data-parallel training adds to a step of training.SIFNetTrainer, at the README's training size: B = 16, a 512 x 512 input, 3 stacks of depth 2, 20 000
points a frame (config tri-vis-l2), on ONE GPU (no multi-GPU node has been available: the cross-GPU cost of the gather is NOT measured here).

  (a) vt_grad_rank_mean alone for W = 2, 4, 8 rows of the image encoder's flat gradient length, into the gradient buffer as RankMean.reduce runs it:
      microseconds and (W + 1) . 4 . n bytes per second, against the 6.29 TB/s a float4 copy reaches on this chip;
  (b) train_step with an RCCL group of ONE rank (VT_FORCE_DIST=1: all_gather_into_tensor of the three flat gradients onto itself, then the kernel with W = 1)
      against train_step without a group: the difference is what the reducer adds to a step on every rank, the wire excluded;
  (c) train_step_micro over 2 x 8 frames against one step of 16.

Synthetic weights and batch as tools/bench_scripts/trainstepbench.py.  Median (min .. max) of 5 rounds after warm-up, device time by events.

    python tools/bench_scripts/ddpbench.py [out.txt]
    python tools/bench_scripts/ddpbench.py --plain-step [--root CHECKOUT] [out.txt]      # only train_step without a group, from the package of another checkout
                                                                                        # (the parent commit's), for the A/B of (b)"""
import os
import statistics
import sys

args = sys.argv[1:]
plain_only = "--plain-step" in args
if plain_only:
    args.remove("--plain-step")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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
HBM_COPY_TBS = 6.29
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


def fmt(t):
    return f"{t[0]:.1f} ms ({t[1]:.1f} .. {t[2]:.1f})"


def main():
    torch.cuda.set_device(0)
    say(f"ddpbench: B = {B}, input {S} x {S}, {STACKS} stacks of depth {DEPTH}, N = {N} points a frame, {torch.cuda.get_device_name(0)}; median (min .. max) of 5 rounds"
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
        return SIFNetTrainer(sd, None, num_stack=STACKS, num_hourglass=DEPTH, triplane_stack=STACKS, device=DEV, **kw)

    tr = make()
    plain = timed(lambda: tr.train_step(batch, images, ccd), 2)
    say(f"train_step, no group: {fmt(plain)}")
    if plain_only:
        return

    # (a) the kernel alone
    from vistracker_amd import ops
    n = tr.image_optimizer.n
    sizes = [tr.image_optimizer.n, tr.tri_optimizer.n, tr.params.flat.numel()]
    say(f"flat gradient buffers: image encoder {sizes[0]} floats, triplane encoder {sizes[1]}, decoders {sizes[2]} ({sum(sizes) * 4 / 1e6:.1f} MB a rank)")
    out = torch.empty(n, device=DEV)
    for W in (2, 4, 8):
        parts = torch.randn(W, n, device=DEV)
        t = timed(lambda: ops.grad_rank_mean(parts, out=out), 20)
        byts = (W + 1) * 4 * n
        say(f"(a) vt_grad_rank_mean W = {W}, n = {n}: {t[0] * 1e3:.1f} us ({t[1] * 1e3:.1f} .. {t[2] * 1e3:.1f}) | {byts / 1e6:.1f} MB moved, {byts / t[0] / 1e9:.2f} TB/s"
            f" = {byts / t[0] / 1e9 / HBM_COPY_TBS * 100:.0f} % of the {HBM_COPY_TBS} TB/s float4 copy" + (" (the rows fit the 256 MiB Infinity Cache)" if byts < 256 * 2 ** 20 else ""))
        del parts
    del out

    # (c) two micro-batches of 8 against the step of 16
    from vistracker_amd.training import slice_batch
    halves = [(slice_batch(batch, slice(k, k + B // 2)), images[k:k + B // 2], ccd[k:k + B // 2]) for k in (0, B // 2)]
    mic = timed(lambda: tr.train_step_micro(halves), 2)
    say(f"(c) train_step_micro, 2 x {B // 2} frames: {fmt(mic)} | against the step of {B}: {mic[0] - plain[0]:+.1f} ms ({mic[0] / plain[0]:.3f} x)")
    del tr
    torch.cuda.empty_cache()

    # (b) an RCCL group of one rank
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29621")
    os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
    os.environ["VT_FORCE_DIST"] = "1"
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    trg = make(group=True)
    assert trg.reducer.collective and trg.reducer.backend == "nccl"
    grp = timed(lambda: trg.train_step(batch, images, ccd), 2)
    say(f"(b) train_step, RCCL group of one rank (three all_gather_into_tensor + three vt_grad_rank_mean, W = 1): {fmt(grp)} | against no group: {grp[0] - plain[0]:+.2f} ms"
        f" ({(grp[0] / plain[0] - 1) * 100:+.2f} %)")
    red = timed(lambda: trg.reducer.reduce(trg.flat_grads()), 20)
    say(f"    RankMean.reduce alone on that group, back to back: {red[0] * 1e3:.0f} us ({red[1] * 1e3:.0f} .. {red[2] * 1e3:.0f})")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
    if OUT:
        os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
        with open(OUT, "w") as f:
            f.write("\n".join(lines) + "\n")
