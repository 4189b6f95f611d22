"""The encoder-training rows of csrc/enctrain.hip at B = 16 and a 512 x 512 input, each against the torch composition (F.conv2d / F.group_norm / autograd,
channels-last) on the same device in the same run:

1. vt_stem7x7_wgrad alone (Cin 5 -> 64, d_y 256 x 256) against torch.nn.grad.conv2d_weight, with its share of the fp32 MFMA roof (2 M N K FLOP of the GEMM
   M = 64, N = 245, K = B 256 256 against 157.3 TFLOP/s) and of the HBM roof (read d_y and x once: 6.29 TB/s).
2. vt_stack_tail_backward alone (256 / 256 channels at 128 x 128, a middle stack) against autograd through the four 1 x 1 convolutions and the GroupNorm.
3. one whole-encoder forward + backward, encoder.TrainableHGFilter (3 stacks, depth 2) against the same network written with torch modules.

Median of 5 rounds after warm-up, device time by events around `iters` back-to-back calls.

    python tools/bench_scripts/enctrainbench.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import enctrain_model as EM  # noqa: E402
from vistracker_amd import ops  # noqa: E402
from vistracker_amd.encoder import TrainableHGFilter, TrainableStackTail, _leaf  # noqa: E402

DEV, B, S, HBM_TBS, MFMA_F32_TFLOPS = "cuda:0", 16, 512, 6.29, 157.3
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


def main():
    torch.manual_seed(0)
    say(f"enctrainbench: B = {B}, input {S} x {S}, {torch.cuda.get_device_name(0)}; median (min .. max) of 5 rounds")
    # 1. the stem's weight gradient
    cin, cout, h2 = 5, 64, S // 2
    x = cl(torch.rand(B, cin, S, S, device=DEV)); dy = cl(torch.randn(B, cout, h2, h2, device=DEV))
    ours = timed(lambda: ops.stem7x7_wgrad(dy, x), 10)
    ref = timed(lambda: torch.nn.grad.conv2d_weight(x, (cout, cin, 7, 7), dy, stride=2, padding=3), 10)
    flop = 2.0 * cout * 49 * cin * B * h2 * h2
    byts = 4.0 * (dy.numel() + x.numel())
    say(f"stem wgrad {cin}->{cout}: {ours[0]:.3f} ms ({ours[1]:.3f} .. {ours[2]:.3f}) | torch conv2d_weight {ref[0]:.3f} ms | ratio torch / ours {ref[0] / ours[0]:.2f} | "
        f"{flop / ours[0] / 1e9:.1f} TFLOP/s = {100 * flop / ours[0] / 1e9 / MFMA_F32_TFLOPS:.1f} % of the fp32 MFMA roof | {byts / ours[0] / 1e9:.2f} TB/s = "
        f"{100 * byts / ours[0] / 1e9 / HBM_TBS:.1f} % of the HBM roof")
    # 2. the tail of a middle stack
    C, Co, hq = 256, 256, S // 4
    P = EM.tail_make_params(C, Co, False, 3)
    tail = TrainableStackTail({k: _leaf(v, DEV) for k, v in P.items()}, False, DEV)
    ll = cl(torch.randn(B, C, hq, hq, device=DEV)); prev = cl(torch.randn(B, C, hq, hq, device=DEV))
    d_out = cl(torch.randn(B, Co, hq, hq, device=DEV)); d_prev = cl(torch.randn(B, C, hq, hq, device=DEV))
    out, prev2 = tail(ll, prev)
    s_ll, s_raw, s_out, s_ws = out.grad_fn.saved_tensors[:4]
    params = dict(zip(ops.STACK_TAIL_PARAMS, [t.detach() for t in tail.tensors()]))
    ours = timed(lambda: ops.stack_tail_backward_raw(d_out, d_prev, s_ll, s_raw, s_out, s_ws, params), 5)
    tp = {k: cl(torch.as_tensor(v).to(DEV)).requires_grad_(True) if v.ndim == 4 else torch.as_tensor(v).to(DEV).requires_grad_(True) for k, v in P.items()}
    llr = ll.clone().requires_grad_(True)

    def torch_tail():
        o, p2, _ = EM.tail_forward(tp, llr, prev)
        return o, p2

    o, p2 = torch_tail()
    ref = timed(lambda: torch.autograd.grad([o, p2], [llr] + list(tp.values()), [d_out, d_prev], retain_graph=True), 5)
    say(f"stack tail backward {C}/{Co} at {hq} x {hq}: {ours[0]:.3f} ms ({ours[1]:.3f} .. {ours[2]:.3f}) | torch autograd backward {ref[0]:.3f} ms | ratio torch / ours {ref[0] / ours[0]:.2f}")
    del o, p2, out, prev2
    # 3. the whole encoder, forward + backward
    P = EM.filter_make_params(5, 64, 256, 3, 2, 9)
    enc = TrainableHGFilter.from_state_dict(P, "", num_stack=3, num_hourglass=2, device=DEV)
    d_outs = [cl(torch.randn(B, 256, hq, hq, device=DEV)) for _ in range(3)]

    def ours_step():
        outs, _, _ = enc(x)
        torch.autograd.backward(outs, d_outs)
        for p in enc.parameters():
            p.grad = None

    tp = {k: (cl(torch.as_tensor(v).to(DEV)) if v.ndim == 4 else torch.as_tensor(v).to(DEV)).requires_grad_(True) for k, v in P.items() if ".downsample.0" not in k}

    def torch_filter(xx):
        def blk(n, t):
            return EM._block({k[len(n) + 1:]: v for k, v in tp.items() if k.startswith(n + ".")}, t)[0]

        def level(i, n, t):
            up1 = blk(f"m{i}.b1_{n}", t)
            low = blk(f"m{i}.b2_{n}", F.avg_pool2d(t, 2, stride=2))
            low = level(i, n - 1, low) if n > 1 else blk(f"m{i}.b2_plus_1", low)
            return up1 + F.interpolate(blk(f"m{i}.b3_{n}", low), scale_factor=2, mode="bicubic", align_corners=True)

        t, _ = EM.stem_forward(tp, xx)
        previous = blk("conv4", blk("conv3", F.avg_pool2d(blk("conv2", t), 2, stride=2)))
        outs = []
        for i in range(3):
            o, p2, _ = EM.tail_forward(EM.filter_tail_params(tp, i), blk(f"top_m_{i}", level(i, 2, previous)), previous)
            outs.append(o)
            previous = p2 if p2 is not None else previous
        return outs

    def torch_step():
        torch.autograd.backward(torch_filter(x), d_outs)
        for p in tp.values():
            p.grad = None

    ours = timed(ours_step, 2, rounds=5, warm=2)
    ref = timed(torch_step, 2, rounds=5, warm=2)
    say(f"whole encoder forward + backward (3 stacks, depth 2): {ours[0]:.1f} ms ({ours[1]:.1f} .. {ours[2]:.1f}) | torch modules + autograd {ref[0]:.1f} ms | ratio torch / ours {ref[0] / ours[0]:.2f}")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
