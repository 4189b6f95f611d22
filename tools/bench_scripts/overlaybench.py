"""Step 7 with the fit drawn on the camera image and scored on the masks (csrc/overlay.hip): the video path ``SequencePipeline.render(video=...)`` on the
synthetic sequence of panelbench.py, camera images from 1536 x 2048 JPEGs and person / object masks from 1536 x 2048 PNGs on disk, one setting after the other
in one process:

  default          device_panel off, overlay off          (the parent commit's default path)
  overlay          device_panel off, overlay on
  device+pool      device_panel on, decode_workers 16     (the decode out of the way)
  overlay+pool     the same with overlay on
  scores           mask_scores from the masks on disk, decode_workers 0
  scores+pool      mask_scores, decode_workers 16

--kernels times the two kernels alone at the production shape (image_size 1200: panels of 900 x 720, owner maps of 2400 x 2400, 1800 rows scored, masks of
1536 x 2048) with events, next to their byte floors: overlay 16 B + 3 B read and 3 B written per pixel; score 4 B of owners per sample plus the mask bytes.  Run
that mode under a kernel trace for the per-kernel time.  --settings default,device+pool runs on a tree without the overlay.

usage: python tools/bench_scripts/overlaybench.py [--frames 240] [--files 48] [--chunk 8] [--settings ...] [--kernels] [--out DIR]
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
from vistracker_amd import ops, sequence_io as SIO, synthetic as syn  # noqa: E402
from vistracker_amd import visualize as V  # noqa: E402

HBM_TBS = 6.29


def write_frames(folder, n, H=1536, W=2048):
    """n frame folders <folder>/tNNNN.000 with k1.color.jpg (q90), k1.person_mask.png, k1.obj_rend_mask.png (ellipses that move from frame to frame)"""
    from PIL import Image
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([128 + 90 * np.sin(x / 150 + c) * np.cos(y / 110 - c) for c in range(3)], -1) + rng.normal(0, 12, (H, W, 3)).astype(np.float32)
    base = np.clip(np.rint(base), 0, 255).astype(np.uint8)
    files = []
    for k in range(n):
        d = os.path.join(folder, f"t{k:04d}.000"); os.makedirs(d)
        files.append(os.path.join(d, "k1.color.jpg"))
        Image.fromarray(np.roll(base, (7 * k, 13 * k), (0, 1))).save(files[-1], quality=90)
        pm = (((x - 900 - 3 * k) / 160) ** 2 + ((y - 760) / 420) ** 2 < 1).astype(np.uint8) * 255
        om = (((x - 1200 + 2 * k) / 150) ** 2 + ((y - 900) / 130) ** 2 < 1).astype(np.uint8) * 255
        Image.fromarray(pm).save(os.path.join(d, "k1.person_mask.png")); Image.fromarray(om).save(os.path.join(d, "k1.obj_rend_mask.png"))
    return files


def kernels(say):
    size, H, pw, cs, n = 1200, 900, 720, 240, 8
    rs, rows, h, w = 2 * size, 2 * H, 1536, 2048
    rng = np.random.default_rng(1)
    rgb = torch.rand(n, size, size, 3, device="cuda"); alpha = torch.rand(n, size, size, device="cuda")
    buf = torch.randint(0, 256, (n, H, 2 * pw, 3), dtype=torch.uint8, device="cuda")
    src = torch.arange(n, device="cuda") * (H * 2 * pw * 3); dst = src + pw * 3
    F, nb, no = 16000, 13776, 2000
    fidx = torch.as_tensor(rng.integers(-1, 2 * F, (n, rs, rs)).astype(np.int32)).cuda()
    masks = torch.randint(0, 256, (n, 2, h, w), dtype=torch.uint8, device="cuda")
    desc = [[(2 * k) * h * w, (2 * k + 1) * h * w, h, w, 1, w, 1, w] for k in range(n)]
    count = torch.empty(n, 2, 4, dtype=torch.int32, device="cuda")
    runs = {"vt_overlay_panel_u8": (lambda: ops.overlay_panel_u8(rgb, alpha, buf, src, dst, 0, H, cs, pw, 2 * pw * 3, 0.6), 22 * H * pw),
            "vt_mask_score": (lambda: ops.mask_score(fidx, rows, F, nb, no, masks, masks, desc, count=count), 4 * rows * rs + 2 * h * w)}
    for name, (run, nbytes) in runs.items():
        run(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            run()
        e1.record(); torch.cuda.synchronize()
        t = e0.elapsed_time(e1) / 50 / n * 1e-3
        say(f"{name}: {1e6 * t:.2f} us per view ({n} views a call, events over 50 calls) for {nbytes / 1e6:.2f} MB = {nbytes / t / 1e12:.2f} TB/s; "
            f"floor at {HBM_TBS} TB/s {nbytes / (HBM_TBS * 1e12) * 1e6:.2f} us")
    c = count.cpu().numpy()
    say(f"vt_mask_score counts of view 0: {c[0].tolist()}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--files", type=int, default=48)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--settings", default="default,overlay,device+pool,overlay+pool,scores,scores+pool")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None, help="directory for the report (overlaybench.txt)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "overlaybench needs the GPU"
    torch.cuda.set_device(0)
    lines = []
    say = lambda x: (print(x, flush=True), lines.append(x))
    out_dir = a.out or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    report = lambda: open(os.path.join(out_dir, "overlaybench_kernels.txt" if a.kernels else "overlaybench.txt"), "w").write("\n".join(lines) + "\n")
    if a.kernels:
        kernels(say)
        report()
        return
    T = a.frames
    model = syn.smplh_model(0); h = ops.SmplhHandle(model)
    sp = syn.sequence_params(T, 7)
    tv, tf = syn.object_template()
    recon = {"poses": sp["pose"], "betas": sp["betas"], "trans": sp["trans"], "obj_angles": sp["obj_R"].transpose(0, 2, 1),
             "obj_trans": sp["obj_t"], "obj_scales": np.ones(T, np.float32)}
    c, s = np.cos(0.35), np.sin(0.35)
    kin = V.KinectTransform(world2local_R=[np.eye(3), np.eye(3), np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])],
                            world2local_t=[np.zeros(3), np.zeros(3), np.array([0.8, 0, 0.3])])
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    files = write_frames(tmp, min(a.files, T))
    say(f"{len(files)} frames of 1536 x 2048 on disk (JPEG q90 + two PNG masks) written in {time.perf_counter() - t0:.1f} s; frame i shows file i % {len(files)}; "
        f"{T} frames, chunks of {a.chunk}, step 7 -> Motion-JPEG .avi at q{a.quality}")
    path_of = lambda i: files[i % len(files)]
    from vistracker_amd.pipeline import SequencePipeline
    fake = SimpleNamespace(device="cuda:0", ctx=SimpleNamespace(smpl=h))
    host = dict(rgb=lambda i: SIO._load_image(path_of(i)))
    pool = dict(rgb=path_of, device_panel=True, decode_workers=16)
    kw = {"default": host, "overlay": dict(host, overlay=True), "device+pool": pool, "overlay+pool": dict(pool, overlay=True)}
    settings = a.settings.split(",")
    warm = SequencePipeline.render(fake, {"recon": recon}, kin, template=(tv, tf), chunk=a.chunk, end=2 * a.chunk, video=os.path.join(out_dir, "warm.avi"),
                                   quality=a.quality, **kw[settings[0]])
    os.remove(warm)
    for name in settings:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        if name.startswith("scores"):
            res = SequencePipeline.mask_scores(fake, {"recon": recon}, kin, path_of, (tv, tf), chunk=a.chunk, decode_workers=16 if name.endswith("pool") else 0)
            dt = time.perf_counter() - t0
            iou = res["iou"][:, 0]
            say(f"mask_scores    [{name:12s}]: {T} frames in {dt:6.2f} s = {1e3 * dt / T:6.2f} ms per frame ({T / dt:7.1f} frames/s); IoU body {np.nanmin(iou[:, 0]):.3f}.."
                f"{np.nanmax(iou[:, 0]):.3f}, object {np.nanmin(iou[:, 1]):.3f}..{np.nanmax(iou[:, 1]):.3f}; counts of frame 0: {res['count'][0, 0].tolist()}")
            continue
        path = os.path.join(out_dir, f"overlay_{name.replace('+', '_')}.avi")
        p = SequencePipeline.render(fake, {"recon": recon}, kin, template=(tv, tf), chunk=a.chunk, video=path, quality=a.quality, **kw[name])
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        say(f"step 7 -> .avi [{name:12s}]: {T} frames in {dt:6.2f} s = {1e3 * dt / T:6.2f} ms per frame ({T / dt:7.1f} frames/s), file {os.path.getsize(p) / 1e6:.1f} MB")
        os.remove(p)
    t0 = time.perf_counter()
    for f in files[:a.chunk]:
        SIO.decode_masks(f)
    say(f"PIL decode of one frame's two PNG masks on one thread: {1e3 * (time.perf_counter() - t0) / a.chunk:.2f} ms")
    report()
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
