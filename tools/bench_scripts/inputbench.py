"""Network-input throughput from a sequence folder (data/testdata_triplane.py:42-74 -> vistracker_amd.sequence_io.SequenceLoader): what the two loader
options buy.  Writes --frames synthetic 1536 x 2048 frames (a photo-like noisy JPEG + two PNG masks each) to a temporary folder and times the loader per
frame in four settings, in one process, one after the other:

  today's path   device_prep off, decode_workers 0      (PIL decode, numpy crop, torch resize, compose, copy: one frame after another on the host)
  device only    device_prep on,  decode_workers 0      (csrc/inputs.hip: vt_mask_bbox + vt_crop_resize_compose on uploaded uint8 frames)
  threads only   device_prep off, decode_workers 16
  both           device_prep on,  decode_workers 16

Every setting also runs the loader's SMPL-H forward and triplane render of the batch.  For the device path the parts are timed on their own on one batch:
decode, staging into the pinned buffer, upload, the two kernels (device events) against their HBM byte floor, the read-back of the boxes.

usage: python tools/bench_scripts/inputbench.py [--frames 96] [--bs 16] [--workers 16] [--out DIR]
"""
import argparse
import os
import shutil
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vistracker_amd import _lib as L  # noqa: E402
from vistracker_amd import ops, sequence_io as SIO, synthetic as syn  # noqa: E402

HBM_TBS = 6.29
H, W, CROP, S = 1536, 2048, 1200, 512


def write_frames(root, T):
    """photo-like frames (smooth colour fields + noise of sigma 12, shifted per frame) and moving rectangular masks"""
    from PIL import Image
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([128 + 90 * np.sin(x / 150 + c) * np.cos(y / 110 - c) for c in range(3)], -1)
    base = np.clip(np.rint(base + rng.normal(0, 12, base.shape).astype(np.float32)), 0, 255).astype(np.uint8)
    seq = os.path.join(root, "Date03_Sub03_chairwood")
    frames, files = [], []
    for i in range(T):
        name = f"t{i:04d}.000"; frames.append(name)
        ff = os.path.join(seq, name); os.makedirs(ff)
        u0, v0 = 500 + (37 * i) % 1100, 500 + (23 * i) % 500
        pm = np.zeros((H, W), np.uint8); pm[v0 - 400:v0 + 400, u0 - 120:u0 + 120] = 255
        om = np.zeros((H, W), np.uint8); om[v0 - 50:v0 + 250, u0 + 100:u0 + 400] = 255
        Image.fromarray(np.roll(base, 17 * i, axis=1)).save(os.path.join(ff, "k1.color.jpg"), quality=90)
        Image.fromarray(pm).save(os.path.join(ff, "k1.person_mask.png")); Image.fromarray(om).save(os.path.join(ff, "k1.obj_rend_mask.png"))
        files.append(os.path.join(ff, "k1.color.jpg"))
    return frames, files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--bs", type=int, default=16)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=None, help="directory for the report (r10_inputs.txt)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "inputbench needs the GPU"
    torch.cuda.set_device(0)
    lines = []
    say = lambda x: (print(x, flush=True), lines.append(x))
    T, bs = a.frames, a.bs
    root = tempfile.mkdtemp(prefix="vt_inputbench_")
    try:
        t0 = time.perf_counter()
        frames, files = write_frames(root, T)
        nbytes = sum(os.path.getsize(os.path.join(os.path.dirname(f), n)) for f in files for n in os.listdir(os.path.dirname(f)))
        say(f"{T} frames of {H} x {W} written in {time.perf_counter() - t0:.1f} s ({nbytes / T / 1e6:.2f} MB of files per frame: JPEG q90 + two PNG masks); "
            f"crop {CROP} -> {S}, loader batches of {bs}, torch threads {torch.get_num_threads()}")
        model = syn.smplh_model(0)
        sp = syn.sequence_params(T, seed=7)
        smplt = {"poses": sp["pose"], "betas": sp["betas"], "trans": sp["trans"], "frames": frames}
        ctx = SimpleNamespace(smpl=ops.SmplhHandle(model), b25=ops.LandmarkHandle(syn.landmark_regressors(model, 1)["body25"]))
        make = lambda fl, **kw: SIO.SequenceLoader(fl, bs, smplt, ctx, model["f"], image_size=S, crop_size=CROP, **kw)
        settings = [("today's path", False, 0), ("device only", True, 0), ("threads only", False, a.workers), ("both", True, a.workers)]
        first = {}
        for name, dp, dw in settings:                                    # warm-up: code objects, pinned buffers, the page cache of the first batch
            first[name] = next(iter(make(files[:bs], device_prep=dp, decode_workers=dw)))["images"].clone()
        torch.cuda.synchronize()
        same = all(torch.equal(first["today's path"], v) for v in first.values())
        say(f"first batch of the four settings bit-identical: {same}")
        base_ms = None
        for name, dp, dw in settings:
            torch.cuda.synchronize(); t0 = time.perf_counter(); n = 0
            for batch in make(files, device_prep=dp, decode_workers=dw):
                n += batch["images"].shape[0]
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            ms = 1e3 * dt / n
            base_ms = ms if base_ms is None else base_ms
            say(f"SequenceLoader [{name:13s}] device_prep={str(dp):5s} decode_workers={dw:2d}: {n} frames in {dt:6.2f} s = {ms:7.2f} ms per frame "
                f"({n / dt:6.1f} frames/s, x{base_ms / ms:.2f} of today's path)")

        # ---- the parts of the device path, one batch ------------------------------------------------------------------------------------------------
        part = files[:bs]
        t0 = time.perf_counter(); decoded = [SIO.decode_frame(f) for f in part]; t_dec = time.perf_counter() - t0
        pool = SIO._decode_pool(a.workers)
        t0 = time.perf_counter(); list(pool.map(SIO.decode_frame, part)); t_decp = time.perf_counter() - t0
        pool.shutdown()
        say(f"decode (PIL, JPEG + two PNG): {1e3 * t_dec / bs:.2f} ms per frame on one thread, {1e3 * t_decp / bs:.2f} ms per frame with {a.workers} threads")
        t0 = time.perf_counter(); host = [SIO.host_crop(d, f, CROP, S) for d, f in zip(decoded, part)]; t_host = time.perf_counter() - t0
        say(f"host path behind the decode (bbox, crop, resize, compose): {1e3 * t_host / bs:.2f} ms per frame")
        g, hw = bs, H * W
        stage = torch.empty(5 * g * hw, dtype=torch.uint8, pin_memory=True)
        hn = stage.numpy()
        t0 = time.perf_counter()
        for k, (rgb, pm, om) in enumerate(decoded):
            hn[k * hw:(k + 1) * hw] = pm.reshape(-1); hn[(g + k) * hw:(g + k + 1) * hw] = om.reshape(-1)
            hn[2 * g * hw + 3 * k * hw:2 * g * hw + 3 * (k + 1) * hw] = rgb.reshape(-1)
        t_stage = time.perf_counter() - t0
        say(f"staging into the pinned buffer: {1e3 * t_stage / bs:.2f} ms per frame ({5 * hw / 1e6:.1f} MB per frame)")
        ev = lambda: torch.cuda.Event(enable_timing=True)
        reps = 10
        dev = stage.to("cuda", non_blocking=True); torch.cuda.synchronize()
        e0, e1 = ev(), ev(); e0.record()
        for _ in range(reps):
            dev = stage.to("cuda", non_blocking=True)
        e1.record(); torch.cuda.synchronize()
        t_up = e0.elapsed_time(e1) / reps
        say(f"upload: {t_up / bs:.3f} ms per frame = {5 * g * hw / t_up / 1e6:.1f} GB/s host to device")
        d_pm, d_om, d_rgb = dev[:g * hw].view(g, H, W), dev[g * hw:2 * g * hw].view(g, H, W), dev[2 * g * hw:].view(g, H, W, 3)
        boxes = ops.mask_bbox(d_pm, d_om).cpu().numpy()
        centers = np.stack([sum(SIO.bbox_from_device(b)) // 2 for b in boxes])
        assert np.array_equal(centers.astype(np.float32), np.stack([h[1] for h in host]))
        corners = np.concatenate([np.round(centers - CROP / 2), np.round(centers + CROP / 2)], 1).astype(np.int64)
        out = torch.zeros(g, 8, S, S, device="cuda")
        ops.crop_resize_compose(d_rgb, d_pm, d_om, corners, CROP, S, out=out); torch.cuda.synchronize()
        assert torch.equal(out[:, :5].cpu(), torch.from_numpy(np.stack([h[0] for h in host]))), "device crops differ from the host path"
        # the kernels alone: the C entry points with every argument already on the device, between two device events
        lib, st = L.lib(), L.stream_ptr()
        box = torch.empty(g, 4, dtype=torch.int32, device="cuda")
        d_corners = torch.as_tensor(corners.astype(np.int32), device="cuda")
        table = torch.as_tensor(ops.div255_table(), device="cuda")
        bbox = lambda: L.check(lib.vt_mask_bbox(d_pm.data_ptr(), d_om.data_ptr(), g, H, W, 127, box.data_ptr(), st))
        cropk = lambda: L.check(lib.vt_crop_resize_compose(d_rgb.data_ptr(), d_pm.data_ptr(), d_om.data_ptr(), g, H, W, d_corners.data_ptr(), CROP, S,
                                                           table.data_ptr(), out.data_ptr(), out.stride(0), st))
        reps = 50

        def timed(fn):
            fn(); torch.cuda.synchronize()
            e0, e1 = ev(), ev(); e0.record()
            for _ in range(reps):
                fn()
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps

        t_bb = timed(bbox)
        assert np.array_equal(box.cpu().numpy(), boxes)
        fl_bb = 2 * hw / (HBM_TBS * 1e12) * 1e3
        say(f"vt_mask_bbox ({g} frames a call, two launches): {1e3 * t_bb / g:.2f} us per frame; reads {2 * hw / 1e6:.2f} MB per frame = {2 * g * hw / t_bb / 1e9:.2f} TB/s; "
            f"floor at {HBM_TBS} TB/s {1e3 * fl_bb:.2f} us per frame")
        t_cr = timed(cropk)
        by_cr = 5 * CROP * CROP + 20 * S * S
        say(f"vt_crop_resize_compose ({g} frames a call, one launch): {1e3 * t_cr / g:.2f} us per frame; at most {5 * CROP * CROP / 1e6:.2f} MB read "
            f"+ {20 * S * S / 1e6:.2f} MB written per frame = {g * by_cr / t_cr / 1e9:.2f} TB/s; floor at {HBM_TBS} TB/s {by_cr / (HBM_TBS * 1e12) * 1e6:.2f} us per frame")
        t_w = timed(lambda: ops.crop_resize_compose(d_rgb, d_pm, d_om, corners, CROP, S, out=out))
        say(f"ops.crop_resize_compose (the wrapper: checks and uploads the corners, then the kernel): {1e3 * t_w / g:.2f} us per frame")
        t0 = time.perf_counter()
        for _ in range(reps):
            ops.mask_bbox(d_pm, d_om).cpu()
        t_rb = (time.perf_counter() - t0) / reps
        say(f"vt_mask_bbox + read-back of the boxes (the one synchronisation of a batch): {1e3 * t_rb:.3f} ms per batch")
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            open(os.path.join(a.out, "r10_inputs.txt"), "w").write("\n".join(lines) + "\n")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
