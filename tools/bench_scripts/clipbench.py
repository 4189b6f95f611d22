"""HVOP-Net's clip data set at the size of config/cmf-k4-lrot.json: B = 128 clips of T = 180 frames, multi_kinects, obj_repre '6d', aug_num 4.

1. ``HVOPClipData.batch`` (vt_clip_draw + vt_clip_build and the two index gathers around them) per batch, and ``vt_clip_build`` alone with its effective
   bandwidth from the bytes it writes.  Against it: the numpy model of tests/clipdata_model.py building the same batch on the host in float32, the clips split
   over at most 16 threads.  That comparison is OUR restatement of the reference's data set in numpy, not the reference's loader with its 32 workers.
2. A training step fed from the device (``data.batch`` + ``train_step`` per step, as ``train_epoch`` runs them) against ``train_step`` on a batch that is already
   on the device, and against ``train_step`` fed a host-built batch uploaded per step (the model's arrays, built beforehand: only the upload is in the time).

Median of 5 rounds after warm-up, device time by events around ``iters`` back-to-back calls; min and max alongside.  The file records what was measured.

    python tools/bench_scripts/clipbench.py [out.txt]"""
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import clipdata_cases as CC  # noqa: E402
import clipdata_model as M  # noqa: E402
import former_cases as FC  # noqa: E402
from conftest import golden  # noqa: E402
from vistracker_amd import infill_training as IT, ops  # noqa: E402
from vistracker_amd.infill_data import HVOPClipData  # noqa: E402

DEV, B, T, AUG, THREADS = "cuda:0", 128, 180, 4, 16
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
    return f"{t[0]:8.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def main():
    torch.cuda.set_device(0)
    say(f"HVOP-Net clip data set, {torch.cuda.get_device_name(0)}: B = {B}, T = {T}, multi_kinects, '6d', aug_num {AUG}; ms = median (min .. max) of 5 rounds")
    names = [f"Date0{1 + 2 * (i % 2)}_Sub0{i}_seq{i}" for i in range(6)]
    seqs = [CC.sequence(n, 1500, 50 + i) for i, n in enumerate(names)]
    kw = dict(start_fr_min=10, start_fr_max=50, min_drop_len=10, max_drop_len=40, obj_repre="6d", aug_num=AUG, multi_kinects=True, kinect=CC.kinect())
    data = HVOPClipData.from_packed(seqs, names, T, 10, device=DEV, **kw)
    say(f"   {data.tables['poses'].shape[0]} frames in {len(seqs)} sequences, {data.num_clips} clips")
    idx = torch.randperm(data.num_clips, generator=torch.Generator().manual_seed(0))[:B].to(torch.int32)
    didx = idx.to(DEV)
    say("")
    say("1. one batch")
    a = timed(lambda: data.batch(didx, 5, 1), 20)
    dec = data.draw(didx, 5, 1)
    start, date = data.clip_start.index_select(0, didx.long()), data.clip_date.index_select(0, didx.long())
    d = timed(lambda: ops.clip_draw(didx, 5, 1, *data.draw_args), 50)
    b = timed(lambda: ops.clip_build(data.tables, data.w2c_R, data.w2c_t, start, date, dec, T, 6, None, didx, 5, 1), 50)
    written = B * T * (2 * 147 * 4 + 2 * 6 * 4 + 2)
    read = B * T * (72 + 12) * 4
    say(f"   HVOPClipData.batch (draw + build + gathers)   {fmt(a)}")
    say(f"   vt_clip_draw alone                            {fmt(d)}")
    say(f"   vt_clip_build alone                           {fmt(b)}  writes {written / 1e6:.1f} MB, reads {read / 1e6:.1f} MB: {written / b[0] / 1e6:.1f} GB/s written, "
        f"{(written + read) / b[0] / 1e6:.1f} GB/s moved")
    tab, starts, dates, _ = CC.clip_table(seqs, names, T, 10)[:4]
    K = CC.kinect()
    date_names = sorted({n.split("_")[0] for n in names})
    tab["w2c_R"], tab["w2c_t"] = np.stack([K[x][0] for x in date_names]), np.stack([K[x][1] for x in date_names])
    hidx = idx.numpy()
    hdec = {k: v.cpu().numpy() for k, v in dec.items()}

    def host_batch():
        noise = M.hashed_noise(hidx, 5, 1, AUG, np.float32)
        parts = np.array_split(np.arange(B), THREADS)
        with ThreadPoolExecutor(THREADS) as ex:
            outs = list(ex.map(lambda p: M.build(tab, starts[hidx[p]], dates[hidx[p]], {k: v[p] for k, v in hdec.items()}, T, 6, noise[p], np.float32), parts))
        return {k: np.concatenate([o[k] for o in outs]) for k in ("data_smpl", "data_obj", "gt_smpl", "gt_obj", "mask_obj", "mask_smpl")}

    host_batch()
    hs = []
    for _ in range(3):
        t0 = time.perf_counter(); hb = host_batch(); hs.append((time.perf_counter() - t0) * 1e3)
    say(f"   numpy model (float32, {THREADS} threads), same batch {statistics.median(hs):8.1f} ({min(hs):.1f} .. {max(hs):.1f})  -- our restatement on the host, not the reference's loader")
    say("")
    say("2. one training step (8 layers + projections + predictor + motion losses + Adam), dropout 0.05")
    tr = IT.HVOPTrainer(FC.seeded_weights(golden("infill"), 31), FC.hvop_opt(0.05), lr=1e-4)
    fixed = data.batch(didx, 5, 1)
    keys = ("data_smpl", "mask_smpl", "data_obj", "mask_obj", "gt_obj")

    def fed_from_device():
        tr.train_step(data.batch(didx, 5, 1), seed=1)

    def fed_from_host():
        tr.train_step({k: torch.from_numpy(hb[k]).to(DEV) for k in keys}, seed=1)

    s0, s1, s2 = timed(lambda: tr.train_step(fixed, seed=1), 3), timed(fed_from_device, 3), timed(fed_from_host, 3)
    say(f"   train_step, batch resident on the device      {fmt(s0)}")
    say(f"   data.batch + train_step (as train_epoch)      {fmt(s1)}")
    say(f"   upload of a host-built batch + train_step     {fmt(s2)}  (the {statistics.median(hs):.0f} ms of building it on the host are not in this time)")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
