"""Forward + backward of one 256 -> 256 ConvBlock (the hourglass shape) at B = 16: 128 x 128 (the hourglass's top level) and 32 x 32.
TrainableConvBlock (fused split-f16 forward, csrc/convtrain.hip backward) against the torch composition F.group_norm / F.relu / F.conv2d + autograd in
channels-last on the same device, measured in the same run.  Median of 5 rounds after warm-up, device time by events around `iters` back-to-back steps.

FLOPs of a step (2 per multiply-add), per pixel: the three convolutions are 9 (256 128 + 128 64 + 64 64) = 405 504 MACs; forward 1x, data gradient 1x, weight
gradient 1x -> 3 x 2 x 405 504 = 2 433 024 flop per pixel and frame.  The two GEMM kernels of the backward (dgrad, wgrad) do 2 x 405 504 each; their fraction of
the fp32-input MFMA roof (v_mfma_f32_16x16x4_f32: 256 flop / cycle / CU x 256 CUs x 2.4 GHz = 157.3 TFLOP/s) comes from timing the primitives alone.

    python tools/bench_scripts/convblockbench.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import convblock_model as M  # noqa: E402
from vistracker_amd import _lib as L  # noqa: E402
from vistracker_amd.encoder import TrainableConvBlock  # noqa: E402

DEV, B, ROOF = "cuda:0", 16, 157.3e12
MACS = 9 * (256 * 128 + 128 * 64 + 64 * 64)
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


def torch_block(p, x):
    o1 = F.conv2d(F.relu(F.group_norm(x, 32, p["bn1.weight"], p["bn1.bias"], 1e-5)), p["conv1.weight"], None, 1, 1)
    o2 = F.conv2d(F.relu(F.group_norm(o1, 32, p["bn2.weight"], p["bn2.bias"], 1e-5)), p["conv2.weight"], None, 1, 1)
    o3 = F.conv2d(F.relu(F.group_norm(o2, 32, p["bn3.weight"], p["bn3.bias"], 1e-5)), p["conv3.weight"], None, 1, 1)
    return torch.cat((o1, o2, o3), 1) + x


P = M.make_params(256, 256, 7)
say(f"ConvBlock 256 -> 256 forward + backward, B = {B}; {torch.cuda.get_device_name(0)}; median [min, max] of 5 rounds")
for S in (128, 32):
    r = np.random.RandomState(S)
    x = torch.tensor(r.randn(B, 256, S, S), dtype=torch.float32, device=DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    dy = torch.tensor(r.randn(B, 256, S, S), dtype=torch.float32, device=DEV).contiguous(memory_format=torch.channels_last)
    blk = TrainableConvBlock.from_state_dict(P, "", device=DEV)
    tp = {k: torch.tensor(v, device=DEV).requires_grad_(True) for k, v in P.items() if not k.startswith("bn4")}
    tp = {k: (v.detach().contiguous(memory_format=torch.channels_last).requires_grad_(True) if v.dim() == 4 else v) for k, v in tp.items()}

    def ours():
        x.grad = None
        for t in blk.parameters():
            t.grad = None
        blk(x).backward(dy)

    def ours_fwd():
        with torch.no_grad():
            blk(x)

    def theirs():
        x.grad = None
        for t in tp.values():
            t.grad = None
        torch_block(tp, x).backward(dy)

    iters = 3 if S == 128 else 20
    flop = 3 * 2 * MACS * B * S * S
    t_o, t_f, t_t = timed(ours, iters), timed(ours_fwd, iters), timed(theirs, iters)
    say(f"{S} x {S}: this library {t_o[0]:.3f} ms [{t_o[1]:.3f}, {t_o[2]:.3f}] (forward alone {t_f[0]:.3f} ms) = {flop / t_o[0] / 1e9:.1f} TFLOP/s of {flop / 1e9:.1f} GFLOP; "
        f"torch composition {t_t[0]:.3f} ms [{t_t[1]:.3f}, {t_t[2]:.3f}]; ratio torch / this = {t_t[0] / t_o[0]:.2f}")
    # the two GEMM kernels alone on the widest layer (256 -> 128, 3 x 3)
    lib = L.lib()
    w = torch.tensor(P["conv1.weight"], device=DEV)
    d_o = dy[:, :128].contiguous(memory_format=torch.channels_last)
    g = torch.empty_like(x); dW = torch.empty_like(w)
    ws_d = torch.empty(int(lib.vt_conv_dgrad_workspace_bytes(128, 256, 9)) // 4 + 4, device=DEV)
    ws_w = torch.empty(int(lib.vt_conv_wgrad_workspace_bytes(B, S, S, 128, 256, 9)) // 4 + 4, device=DEV)
    st = torch.stack([torch.zeros(B * 32, device=DEV), torch.ones(B * 32, device=DEV)], -1).contiguous()
    ga, be = torch.ones(256, device=DEV), torch.zeros(256, device=DEV)
    xd = x.detach()
    t_d = timed(lambda: L.check(lib.vt_conv3x3_dgrad(w.data_ptr(), 128, 256, d_o.data_ptr(), 128, 0, B, S, S, g.data_ptr(), 256, 0, ws_d.data_ptr(), L.stream_ptr())), iters)
    t_w = timed(lambda: L.check(lib.vt_conv3x3_wgrad(d_o.data_ptr(), 128, 0, xd.data_ptr(), 256, 0, st.data_ptr(), ga.data_ptr(), be.data_ptr(), 32, B, S, S, 256, 128,
                                                     dW.data_ptr(), 0, ws_w.data_ptr(), L.stream_ptr())), iters)
    fl = 2 * 9 * 256 * 128 * B * S * S
    say(f"    256 -> 128 layer alone: dgrad {t_d[0]:.3f} ms = {fl / t_d[0] / 1e9:.1f} TFLOP/s = {fl / t_d[0] / 1e-3 / ROOF:.1%} of the fp32-MFMA roof; "
        f"wgrad (+ finish) {t_w[0]:.3f} ms = {fl / t_w[0] / 1e9:.1f} TFLOP/s = {fl / t_w[0] / 1e-3 / ROOF:.1%}")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
