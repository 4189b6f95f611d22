"""TEST INFRASTRUCTURE (launched by tests/test_gpu_step_guard.py under torch.distributed.run): ``training.SIFNetTrainer(group=True, guard=True, record=3)`` on the
case of tests/sifnet_step_model.py with two gloo ranks that share cuda:0; rank r trains on frame r.

    guard_ranks_script.py OUT

Three steps, each ``train_step`` written out (backward, the gradient mean over the ranks, apply) so that rank 1 can overwrite one element of ITS gradient with a NaN
before the mean of the second step.  Both ranks must skip that step and stay in sync; each writes its final state and its ``guard.read()`` to OUT.rank<r>.npz."""
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

import gradstat_model as GS                                        # noqa: E402
import sifnet_step_model as SM                                     # noqa: E402
from vistracker_amd.training import SIFNetTrainer, slice_batch     # noqa: E402

out_path = sys.argv[1]
world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
DEV = "cuda:0"
torch.cuda.set_device(0)
# a lost peer ends the run after 120 s instead of hanging it
dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


c = SM.case()
lab = c["labels"]
batch = {"points": dev(c["pts"]), "df_h": dev(lab["df_h"]), "df_o": dev(lab["df_o"]), "labels": dev(lab["labels"], torch.int32), "pca_axis": dev(lab["pca_axis"]),
         "body_center": dev(c["bc"]), "obj_center": dev(lab["obj_center"]), "visibility": dev(lab["visibility"])}
images, cc = dev(c["images"]), dev(c["cc"])
sl = slice(rank, rank + 1)
batch, images, cc = slice_batch(batch, sl), images[sl], cc[sl]

tr = SIFNetTrainer(SM.state_dict(c), None, num_stack=SM.NUM_STACK, num_hourglass=SM.DEPTH, triplane_stack=SM.NUM_STACK, device=DEV, group=True, guard=True, record=3)
assert tr.reducer.world == world == 2 and tr.reducer.collective
named = tr.image.named_parameters()
name, leaf = named[len(named) // 2]
index = (leaf.data_ptr() - tr.image_optimizer.flat.data_ptr()) // 4 + leaf.numel() - 1          # the last element of the image encoder's middle leaf

skipped = []
for step in range(3):
    error, _ = tr.backward(batch, images, cc)
    if step == 1 and rank == 1:
        tr.flat_grads()[0][index] = float("nan")
    tr.reducer.reduce(tr.flat_grads())
    tr.apply(tr._guard_error(error))
    assert tr.in_sync(), (rank, step)
    skipped.append(bool(tr.guard.skip.item()))
assert skipped == [False, True, False], (rank, skipped)

rec = tr.guard.read()
assert rec["skipped"] == 1 and {k: v for r in rec["ring"] for k, v in r["nonfinite"].items() if v} == {"image_filter." + name: 1}, rank
arrays = GS.record_arrays(rec)
state = []
for o in (tr.image_optimizer, tr.tri_optimizer):
    state += [o.flat, o.m, o.v]
state += [tr.params.flat.detach(), tr.optimizer.m[0], tr.optimizer.v[0]]
arrays.update({f"state{i}": t.cpu().numpy().view(np.int32).astype(np.int64) for i, t in enumerate(state)})
np.savez(f"{out_path}.rank{rank}.npz", **arrays)
print("RANK_OK", rank, flush=True)
dist.barrier()
dist.destroy_process_group()
