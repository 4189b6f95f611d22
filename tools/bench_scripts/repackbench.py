"""What an optimiser step of one encoder costs between the end of backward() and the next forward, for encoder.TrainableHGFilter (3 stacks, depth 2) at B = 16 and
a 512 x 512 input, on the two paths:

  host    ops.FusedAdam per leaf (one launch each) + the packed forward handles rebuilt on the host (VT_ENCODER_HOST_REPACK: synchronise, destroy, copy down, pack
          on the CPU, hipMalloc, copy up, synchronise -- per convolution, at its first use in the next forward)
  device  encoder.EncoderAdam: one Adam launch over the flat buffers + one repack plan (two launches), no host wait

Per path, wall clock from a synchronised end of backward():
  to_first_conv   optimiser step + zero_grad + the next forward up to and including its first convolution (the stem), synchronised
  to_forward_end  optimiser step + zero_grad + the whole next forward, synchronised; `forward` is that forward alone, so the difference is what the step adds
Median (min .. max) of 5 rounds after 2 warm-up rounds.

    python tools/bench_scripts/repackbench.py [out.txt]"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import enctrain_model as EM  # noqa: E402
from vistracker_amd import encoder as E, ops  # noqa: E402

DEV, B, S = "cuda:0", 16, 512
lines = []


def say(s):
    print(s, flush=True); lines.append(s)


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def med(v):
    return f"{statistics.median(v):8.2f} ms ({min(v):.2f} .. {max(v):.2f})"


def measure(name, host):
    E._PackedHandles.host_repack = host
    torch.manual_seed(0)
    P = EM.filter_make_params(5, 64, 256, 3, 2, 9)
    enc = E.TrainableHGFilter.from_state_dict(P, "", num_stack=3, num_hourglass=2, device=DEV)
    x = cl(torch.rand(B, 5, S, S, device=DEV))
    d_outs = [cl(torch.randn(B, 256, S // 4, S // 4, device=DEV)) for _ in range(3)]
    if host:
        opt = ops.FusedAdam(enc.parameters(), lr=1e-4)

        def step():
            opt.step()
            E.invalidate_handles(enc)           # FusedAdam writes through data_ptr(): the version counters do not see it
            opt.zero_grad()
        launches = len(enc.parameters())
    else:
        opt = E.EncoderAdam(enc, lr=1e-4)

        def step():
            opt.step()
            opt.zero_grad()
        launches = opt.launches_per_step
    n_handles = sum(len(o._handles) for o in E._handle_owners(enc)) if not host else None
    res = {"to_first_conv": [], "to_forward_end": [], "forward": [], "step_host_ms": []}
    for rnd in range(7):
        for what in ("to_first_conv", "to_forward_end"):
            outs, _, _ = enc(x)
            torch.autograd.backward(outs, d_outs)
            del outs
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            t1 = time.perf_counter()
            with torch.no_grad():
                if what == "to_first_conv":
                    enc.stem(x)
                else:
                    enc(x)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if rnd >= 2:
                res[what].append(1e3 * (t2 - t0))
                if what == "to_forward_end":
                    res["step_host_ms"].append(1e3 * (t1 - t0))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            enc(x)
        torch.cuda.synchronize()
        if rnd >= 2:
            res["forward"].append(1e3 * (time.perf_counter() - t0))
    if n_handles is None:
        n_handles = sum(len(o._handles) for o in E._handle_owners(enc))
    say(f"{name}: {len(enc.parameters())} leaves, {n_handles} packed handles, optimiser launches per step {launches}")
    say(f"  to_first_conv   {med(res['to_first_conv'])}")
    say(f"  to_forward_end  {med(res['to_forward_end'])}")
    say(f"  forward         {med(res['forward'])}")
    say(f"  step adds       {statistics.median(res['to_forward_end']) - statistics.median(res['forward']):8.2f} ms (median to_forward_end - median forward); "
        f"host time inside step() {statistics.median(res['step_host_ms']):.2f} ms")
    return statistics.median(res["to_forward_end"]) - statistics.median(res["forward"]), statistics.median(res["to_first_conv"])


def main():
    say(f"repackbench: B = {B}, input {S} x {S}, 3 stacks of depth 2, {torch.cuda.get_device_name(0)}; wall clock, median (min .. max) of 5 rounds")
    h = measure("host   (ops.FusedAdam per leaf + host rebuild)", True)
    d = measure("device (encoder.EncoderAdam)", False)
    say(f"step overhead host / device: {h[0]:.2f} / {d[0]:.2f} ms; to the first convolution: {h[1]:.2f} / {d[1]:.2f} ms")
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
