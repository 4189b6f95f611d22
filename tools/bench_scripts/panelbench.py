"""Step 7 with a real camera panel (render/render_recon.py:157-159 resizes the camera image into the left panel of every frame): the video path
``SequencePipeline.render(video=...)`` on the synthetic sequence of videobench.py, camera images read from 1536 x 2048 JPEGs on disk, four settings one after the
other in one process:

  default        device_panel off                     (PIL decode and sequence_io.resize_bilinear_hw on the host, frame by frame, then one upload per frame)
  device         device_panel on,  decode_workers 0   (PIL decode on the calling thread; csrc/inputs.hip vt_resize_panel_u8 on the staged columns of a chunk)
  device+pool    device_panel on,  decode_workers 16  (the next chunk is decoded in the pool while this one renders)
  black          no camera image                      (the ceiling of the video path)

and, for the device path's parts per frame: staging into the pinned buffer, the upload, the kernel.  Device and host panels are compared on the first images:
they may differ by one grey level where fp32 puts a blend on the other side of a rounding boundary (the host path itself differs from the exact model there);
anything more is an error.  --settings default,black runs on a tree without the device path.

usage: python tools/bench_scripts/panelbench.py [--frames 480] [--files 96] [--chunk 8] [--settings default,device,device+pool,black] [--out DIR]
"""
import argparse
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vistracker_amd import ops, sequence_io as SIO, synthetic as syn  # noqa: E402
from vistracker_amd import visualize as V  # noqa: E402

HBM_TBS = 6.29


def write_images(folder, n, H=1536, W=2048):
    """n camera-image stand-ins (smooth colour fields + per-pixel noise, shifted from frame to frame) as JPEG q90"""
    from PIL import Image
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([128 + 90 * np.sin(x / 150 + c) * np.cos(y / 110 - c) for c in range(3)], -1) + rng.normal(0, 12, (H, W, 3)).astype(np.float32)
    base = np.clip(np.rint(base), 0, 255).astype(np.uint8)
    files = []
    for k in range(n):
        files.append(os.path.join(folder, f"t{k:04d}.k1.color.jpg"))
        Image.fromarray(np.roll(base, (7 * k, 13 * k), (0, 1))).save(files[-1], quality=90)
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=480)
    ap.add_argument("--files", type=int, default=96)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--settings", default="default,device,device+pool,black")
    ap.add_argument("--out", default=None, help="directory for the report (panelbench.txt)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "panelbench needs the GPU"
    torch.cuda.set_device(0)
    T = a.frames
    model = syn.smplh_model(0); h = ops.SmplhHandle(model)
    sp = syn.sequence_params(T, 7)
    tv, tf = syn.object_template()
    recon = {"poses": sp["pose"], "betas": sp["betas"], "trans": sp["trans"], "obj_angles": sp["obj_R"].transpose(0, 2, 1),
             "obj_trans": sp["obj_t"], "obj_scales": np.ones(T, np.float32)}
    c, s = np.cos(0.35), np.sin(0.35)
    kin = V.KinectTransform(world2local_R=[np.eye(3), np.eye(3), np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])],
                            world2local_t=[np.zeros(3), np.zeros(3), np.array([0.8, 0, 0.3])])
    lines = []
    say = lambda x: (print(x, flush=True), lines.append(x))
    out_dir = a.out or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    files = write_images(tmp, min(a.files, T))
    say(f"{len(files)} JPEGs of 1536 x 2048 (q90, {np.mean([os.path.getsize(f) for f in files]) / 1e6:.2f} MB each) written in {time.perf_counter() - t0:.1f} s; "
        f"frame i shows file i % {len(files)}; {T} frames, chunks of {a.chunk}, step 7 -> Motion-JPEG .avi at q{a.quality}")
    path_of = lambda i: files[i % len(files)]
    r = V.RendererSide2side(image_size=1200)
    size, (cs, ce) = r.image_size, r.get_xcuts(r.image_size)
    H, W, _ = r.frame_shape(1)
    settings = a.settings.split(",")

    # ---- device against host panels ----------------------------------------------------------------------------------------------------------------
    if "device" in settings or "device+pool" in settings:
        imgs = [SIO._load_image(f) for f in files[:4]]
        buf = torch.zeros(len(imgs), H, W, 3, dtype=torch.uint8, device="cuda")
        SIO.device_panels(imgs, buf, size, cs, ce)
        got = buf[:, :, :ce - cs].cpu().numpy().astype(np.int16)
        ref = np.stack([SIO.resize_bilinear_hw(im, H, size)[:, cs:ce] for im in imgs]).astype(np.int16)
        diff = np.abs(got - ref)
        assert diff.max() <= 1, f"device and host panels differ by {int(diff.max())} grey levels"
        assert not buf[:, :, ce - cs:].any()
        say(f"device panel against resize_bilinear_hw on {len(imgs)} images (2048 -> 1200: ratio 128 / 75): {int((diff > 0).sum())} of {diff.size} values differ "
            f"({100 * (diff > 0).mean():.4f} %), all by one grey level")

    # ---- end to end ------------------------------------------------------------------------------------------------------------------------------------
    from vistracker_amd.pipeline import SequencePipeline
    fake = SimpleNamespace(device="cuda:0", ctx=SimpleNamespace(smpl=h))
    kw = {"default": dict(rgb=lambda i: SIO._load_image(path_of(i))), "device": dict(rgb=path_of, device_panel=True),
          "device+pool": dict(rgb=path_of, device_panel=True, decode_workers=16), "black": dict(rgb=None)}
    warm = SequencePipeline.render(fake, {"recon": recon}, kin, template=(tv, tf), chunk=a.chunk, end=2 * a.chunk, video=os.path.join(out_dir, "warm.avi"),
                                   quality=a.quality, **kw[settings[0]])
    os.remove(warm)
    base = None
    for name in settings:
        path = os.path.join(out_dir, f"panel_{name.replace('+', '_')}.avi")
        torch.cuda.synchronize(); t0 = time.perf_counter()
        p = SequencePipeline.render(fake, {"recon": recon}, kin, template=(tv, tf), chunk=a.chunk, video=path, quality=a.quality, **kw[name])
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        base = dt if base is None else base
        say(f"step 7 -> .avi [{name:11s}]: {T} frames in {dt:6.2f} s = {1e3 * dt / T:6.2f} ms per frame ({T / dt:7.1f} frames/s, x{base / dt:.2f} of {settings[0]}), "
            f"file {os.path.getsize(p) / 1e6:.1f} MB")
        os.remove(p)

    # ---- where a frame's time goes -------------------------------------------------------------------------------------------------------------------
    t0 = time.perf_counter()
    imgs = [SIO._load_image(f) for f in files[:a.chunk]]
    t_dec = (time.perf_counter() - t0) / len(imgs)
    say(f"PIL decode of one JPEG on one thread: {1e3 * t_dec:.2f} ms")
    t0 = time.perf_counter()
    for im in imgs:
        SIO.resize_bilinear_hw(im, H, size)
    say(f"resize_bilinear_hw (the default path's resize, host): {1e3 * (time.perf_counter() - t0) / len(imgs):.2f} ms per frame")
    if "device" in settings or "device+pool" in settings:
        reps = 10
        SIO.stage_panels(imgs, size, cs, ce)
        t0 = time.perf_counter()
        for _ in range(reps):
            stage, desc = SIO.stage_panels(imgs, size, cs, ce)
        t_st = (time.perf_counter() - t0) / reps / len(imgs)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(reps):
            dev = stage.to("cuda", non_blocking=True)
        torch.cuda.synchronize(); t_up = (time.perf_counter() - t0) / reps / len(imgs)
        buf = torch.zeros(len(imgs), H, W, 3, dtype=torch.uint8, device="cuda")
        off = torch.arange(len(imgs), device="cuda") * (H * W * 3)
        run = lambda: ops.resize_panel_u8(dev, desc, H, size, cs, ce - cs, buf, off, W * 3)
        run(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            run()
        e1.record(); torch.cuda.synchronize()
        t_k = e0.elapsed_time(e1) / 50 / len(imgs) * 1e-3
        nb = stage.numel() / len(imgs)
        rd, wr = nb, H * (ce - cs) * 3
        say(f"device path per frame ({len(imgs)} frames a chunk): staging {nb / 1e6:.2f} MB of {imgs[0].nbytes / 1e6:.2f} MB ({100 * nb / imgs[0].nbytes:.1f} % of the image, "
            f"columns {SIO.panel_columns(imgs[0].shape[1], size, cs, ce)}) into the pinned buffer {1e3 * t_st:.3f} ms, upload {1e3 * t_up:.3f} ms "
            f"({nb / t_up / 1e9:.1f} GB/s), vt_resize_panel_u8 {1e6 * t_k:.2f} us for {rd / 1e6:.2f} MB read + {wr / 1e6:.2f} MB written = "
            f"{(rd + wr) / t_k / 1e12:.2f} TB/s; floor at {HBM_TBS} TB/s {(rd + wr) / (HBM_TBS * 1e12) * 1e6:.2f} us")
    if a.out:
        open(os.path.join(out_dir, "panelbench.txt"), "w").write("\n".join(lines) + "\n")
    for f in files:
        os.remove(f)
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
