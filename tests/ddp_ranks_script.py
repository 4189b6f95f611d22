"""TEST INFRASTRUCTURE (launched by tests/test_gpu_ddp_trainer.py under torch.distributed.run): ``training.SIFNetTrainer(group=True)`` on the case of
tests/sifnet_step_model.py with WORLD_SIZE ranks that all use cuda:0.

    ddp_ranks_script.py OUT BACKEND MODE

BACKEND gloo (several ranks on the one GPU, the gather through host copies) or nccl (RCCL).  With more than one rank, rank r trains on frame r of the case; a single
rank trains on the whole batch.  MODE ``train``: three steps, ``in_sync()`` asserted after each, the final state and the returned errors written to
OUT.rank<r>.npz; over nccl one further step runs with every host wait barred.  MODE ``mismatch``: rank 1 perturbs one weight before construction; the constructor
must raise on every rank, and the script then exits with status 3."""
import datetime
import os
import sys

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
os.environ.setdefault("ROCBLAS_DEFAULT_ATOMICS_MODE", "0")

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sifnet_step_model as SM                                     # noqa: E402
from vistracker_amd import _lib as L                               # noqa: E402
from vistracker_amd.training import SIFNetTrainer, slice_batch     # noqa: E402

out_path, backend, mode = sys.argv[1], sys.argv[2], sys.argv[3]
world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
DEV = "cuda:0"
torch.cuda.set_device(0)
torch.backends.cudnn.benchmark = False
# a lost peer ends the run after 120 s instead of hanging it
kw = {"device_id": torch.device("cuda", 0)} if backend == "nccl" else {}
dist.init_process_group(backend, timeout=datetime.timedelta(seconds=120), **kw)


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


c = SM.case()
lab = c["labels"]
batch = {"points": dev(c["pts"]), "df_h": dev(lab["df_h"]), "df_o": dev(lab["df_o"]), "labels": dev(lab["labels"], torch.int32), "pca_axis": dev(lab["pca_axis"]),
         "body_center": dev(c["bc"]), "obj_center": dev(lab["obj_center"]), "visibility": dev(lab["visibility"])}
images, cc = dev(c["images"]), dev(c["cc"])
if world > 1:
    sl = slice(rank, rank + 1)
    batch, images, cc = slice_batch(batch, sl), images[sl], cc[sl]

sd = SM.state_dict(c)
if mode == "mismatch" and rank == 1:
    key = sorted(k for k in sd if k.startswith("image_filter.") and k.endswith(".weight"))[0]
    w = np.array(sd[key], copy=True)
    w.reshape(-1)[0] = np.nextafter(w.reshape(-1)[0], np.float32(np.inf))          # one weight, one ulp
    sd = dict(sd, **{key: w})

try:
    tr = SIFNetTrainer(sd, None, num_stack=SM.NUM_STACK, num_hourglass=SM.DEPTH, triplane_stack=SM.NUM_STACK, device=DEV, group=True)
except L.VtError as e:
    if mode != "mismatch":
        raise
    print("MISMATCH_CAUGHT", rank, str(e)[:80], flush=True)
    dist.destroy_process_group()
    sys.exit(3)
assert mode == "train", "the constructor accepted ranks built from different weights"
assert tr.reducer.world == world and tr.reducer.backend == backend and tr.reducer.collective

errors, losses = [], []
for step in range(3):
    e, l = tr.train_step(batch, images, cc)
    errors.append(e); losses.append(l)
    assert tr.in_sync(), (rank, step)

state = {}
for name, o in (("image", tr.image_optimizer), ("tri", tr.tri_optimizer)):
    state.update({f"{name}_p": o.flat, f"{name}_m": o.m, f"{name}_v": o.v})
state.update(dec_p=tr.params.flat.detach(), dec_m=tr.optimizer.m[0], dec_v=tr.optimizer.v[0])
np.savez(f"{out_path}.rank{rank}.npz", errors=torch.stack(errors).cpu().numpy(), losses=torch.stack(losses).cpu().numpy(),
         grad_dec=tr.params.flat.grad.cpu().numpy(), **{k: v.cpu().numpy() for k, v in state.items()})

if backend == "nccl":
    def barred(*a, **k):
        raise AssertionError("train_step with an RCCL group went to the host")

    saved = torch.Tensor.cpu, torch.Tensor.numpy, torch.Tensor.item, torch.cuda.synchronize
    torch.Tensor.cpu = torch.Tensor.numpy = torch.Tensor.item = torch.cuda.synchronize = barred
    try:
        e, l = tr.train_step(batch, images, cc)
    finally:
        torch.Tensor.cpu, torch.Tensor.numpy, torch.Tensor.item, torch.cuda.synchronize = saved
    assert e.is_cuda and bool(torch.isfinite(e))
    print("NO_HOST_WAIT_OK", flush=True)

print("RANK_OK", rank, flush=True)
dist.barrier()
dist.destroy_process_group()
