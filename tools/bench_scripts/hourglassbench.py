"""Forward + backward of one hourglass (depth 2, 256 features) at B = 16, 128 x 128 (the encoder's own size), and the two kernels of csrc/resample_bwd.hip alone.

1. encoder.TrainableHourglass (fused split-f16 forward; backward = 7 vt_conv_block_backward + 2 vt_avgpool2x2_backward + 2 vt_upsample2x_bicubic_backward) against
   the torch composition F.group_norm / F.relu / F.conv2d / F.avg_pool2d / F.interpolate + autograd in channels-last on the same device, in the same run.
2. vt_avgpool2x2_backward / vt_upsample2x_bicubic_backward at 128 x 128 and 64 x 64 results against the autograd backward of F.avg_pool2d / F.interpolate on
   channels-last tensors, with the bytes each must move (read d_out once, write the result once) per second next to the 6.29 TB/s the other scripts of this
   directory use as the HBM figure.  These are memory-bound gathers: the byte rate is the whole story.

Median of 5 rounds after warm-up, device time by events around `iters` back-to-back calls.

    python tools/bench_scripts/hourglassbench.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import hourglass_model as HM  # noqa: E402
from vistracker_amd import ops  # noqa: E402
from vistracker_amd.encoder import TrainableHourglass  # noqa: E402

DEV, B, FEAT, DEPTH, S, HBM_TBS = "cuda:0", 16, 256, 2, 128, 6.29
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


def cl(shape, seed):
    return torch.tensor(np.random.RandomState(seed).randn(*shape), dtype=torch.float32, device=DEV).contiguous(memory_format=torch.channels_last)


def torch_block(p, n, x):
    g = lambda k: p[f"{n}.{k}"]         # noqa: E731
    o1 = F.conv2d(F.relu(F.group_norm(x, 32, g("bn1.weight"), g("bn1.bias"), 1e-5)), g("conv1.weight"), None, 1, 1)
    o2 = F.conv2d(F.relu(F.group_norm(o1, 32, g("bn2.weight"), g("bn2.bias"), 1e-5)), g("conv2.weight"), None, 1, 1)
    o3 = F.conv2d(F.relu(F.group_norm(o2, 32, g("bn3.weight"), g("bn3.bias"), 1e-5)), g("conv3.weight"), None, 1, 1)
    return torch.cat((o1, o2, o3), 1) + x


def torch_hourglass(p, n, x):
    up1 = torch_block(p, f"b1_{n}", x)
    low = torch_block(p, f"b2_{n}", F.avg_pool2d(x, 2, stride=2))
    low = torch_hourglass(p, n - 1, low) if n > 1 else torch_block(p, "b2_plus_1", low)
    low = torch_block(p, f"b3_{n}", low)
    return up1 + F.interpolate(low, scale_factor=2, mode="bicubic", align_corners=True)


say(f"{torch.cuda.get_device_name(0)}; median [min, max] of 5 rounds")
P = HM.make_params(DEPTH, FEAT, 7)
hg = TrainableHourglass.from_state_dict(P, "", depth=DEPTH, device=DEV)
tp = {k: torch.tensor(v, device=DEV) for k, v in P.items() if ".bn4." not in k}
tp = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v).requires_grad_(True) for k, v in tp.items()}
x, dy = cl((B, FEAT, S, S), 1).requires_grad_(True), cl((B, FEAT, S, S), 2)


def ours():
    x.grad = None
    for t in hg.parameters():
        t.grad = None
    hg(x).backward(dy)


def theirs():
    x.grad = None
    for t in tp.values():
        t.grad = None
    torch_hourglass(tp, DEPTH, x).backward(dy)


t_o, t_t = timed(ours, 2), timed(theirs, 2)
say(f"hourglass depth {DEPTH}, {FEAT} features, B = {B}, {S} x {S}, forward + backward: this library {t_o[0]:.2f} ms [{t_o[1]:.2f}, {t_o[2]:.2f}]; "
    f"torch composition (MIOpen, autograd) {t_t[0]:.2f} ms [{t_t[1]:.2f}, {t_t[2]:.2f}]; ratio torch / this = {t_t[0] / t_o[0]:.2f}")
del hg, tp
for R in (S, S // 2):           # the size of the result of the pooling backward = of the input of the up-sampling backward
    d_small, d_big = cl((B, FEAT, R // 2, R // 2), 3), cl((B, FEAT, R, R), 4)
    nbytes = 4 * B * FEAT * (R * R + R * R // 4)
    xs = cl((B, FEAT, R, R), 5).requires_grad_(True)
    pooled = F.avg_pool2d(xs, 2, stride=2)
    ls = cl((B, FEAT, R // 2, R // 2), 6).requires_grad_(True)
    up = F.interpolate(ls, scale_factor=2, mode="bicubic", align_corners=True)
    for name, fn, ref in (("vt_avgpool2x2_backward", lambda: ops.avgpool2x2_backward(d_small), lambda: torch.autograd.grad(pooled, xs, d_small, retain_graph=True)),
                          ("vt_upsample2x_bicubic_backward", lambda: ops.upsample2x_bicubic_backward(d_big), lambda: torch.autograd.grad(up, ls, d_big, retain_graph=True))):
        a, b = timed(fn, 20), timed(ref, 20)
        verdict = "faster than" if a[0] < b[0] else "SLOWER than"
        say(f"{name}, B = {B}, {FEAT} channels, {R} x {R} on the large side: {1e3 * a[0]:.1f} us [{1e3 * a[1]:.1f}, {1e3 * a[2]:.1f}] for {nbytes / 1e6:.1f} MB = "
            f"{nbytes / a[0] / 1e9:.2f} TB/s of {HBM_TBS} TB/s ({nbytes / a[0] / 1e9 / HBM_TBS:.0%}); torch autograd {1e3 * b[0]:.1f} us [{1e3 * b[1]:.1f}, {1e3 * b[2]:.1f}]: "
            f"{verdict} torch's, ratio torch / this = {b[0] / a[0]:.2f}")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
