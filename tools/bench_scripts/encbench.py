import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT)        # the tree this file lies in
import numpy as np, torch
from vistracker_amd import _lib, synthetic as syn
from vistracker_amd.encoder import SIFNetEncoder
g = np.load(os.path.join(ROOT, 'tests', 'golden', 'encoder.npz'))
ks = [(str(n), tuple(int(x) for x in s[:d])) for n, s, d in zip(g["names"], g["shapes"], g["ndims"])]
enc = SIFNetEncoder.from_state_dict(syn.encoder_weights(ks))
torch.backends.cudnn.benchmark = (len(sys.argv) > 2)
B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
img = torch.rand(B, 8, 512, 512, device="cuda")
_lib.lib(); torch.cuda.synchronize()               # the library is loaded and the weights are on the device: what the first call adds is the encoder's own
t0 = time.perf_counter()
enc(img); torch.cuda.synchronize()                 # warm-up: one packed handle per convolution, MIOpen kernel selection where a route falls back, the graph capture of a full chunk
print(f"encoder B={B}: first call {(time.perf_counter() - t0)*1e3:.1f} ms")
REPS = 8
t0 = time.perf_counter()
for _ in range(REPS): m = enc(img)
torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / REPS
print(f"encoder B={B}: {dt*1e3:.1f} ms -> {B/dt:.1f} frames/s, {613e9*B/dt/1e12:.1f} TFLOP/s (613 GFLOP/frame)")
if len(sys.argv) > 3:
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        enc(img); torch.cuda.synchronize()
    print(prof.key_averages().table(sort_by="cuda_time_total", row_limit=14, max_name_column_width=60))
