"""Step-7 video throughput (demo.sh: render/render_side_comp.py -> render_recon.py's FFMPEG writer; here video.write_video, Motion-JPEG AVI encoded by
csrc/jpeg.hip).  Two measurements on the synthetic sequence of renderbench.py (two views x one recon, 900 x 2160 frames):

  encoder alone   JpegEncoder.encode on device frames (q90, 4:2:0; 8 frames per call): ms per frame, compressed bytes per frame, PSNR of libjpeg's
                  decoding against the input; for rendered frames with a black camera panel and with a photo-like noisy camera panel;
  end to end      SequencePipeline.render's video path (render_frames(on_device=True) -> write_video) for --frames frames into an .avi, and the PNG
                  path (render_frames -> write_frames) on --png-frames frames in the same run (scaled to frames/s).

--encode-only runs just the encoder on --frames frames (for `rocprofv3 --kernel-trace --stats` in a run of its own).

usage: python tools/bench_scripts/videobench.py [--frames 1500] [--png-frames 100] [--out DIR] [--encode-only]
"""
import argparse
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vistracker_amd import ops, synthetic as syn  # noqa: E402
from vistracker_amd import video as VID  # noqa: E402
from vistracker_amd import visualize as V  # noqa: E402

HBM_TBS = 6.29


def photo_panel(seed=0, H=1536, W=2048):
    """camera-image stand-in: smooth colour fields + per-pixel noise (sigma 12): the hard case for the encoder's bytes"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([128 + 90 * np.sin(x / 150 + c) * np.cos(y / 110 - c) for c in range(3)], -1)
    img += rng.normal(0, 12, img.shape).astype(np.float32)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--png-frames", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", default=None, help="directory for the report (r07_video.txt) and the .avi")
    ap.add_argument("--encode-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "videobench needs the GPU"
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
    r = V.RendererSide2side(image_size=1200)
    cam = photo_panel()
    lines = []
    say = lambda x: (print(x, flush=True), lines.append(x))
    out_dir = a.out or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    H, W, _ = r.frame_shape(1)

    # ---- encoder alone ---------------------------------------------------------------------------------------------------------------------------
    sets = {"rendered, black camera panel": None, "rendered, noisy photo camera panel": (lambda i: cam)}
    enc = VID.JpegEncoder(H, W, quality=a.quality, subsampling="420")
    n_enc = T if a.encode_only else min(T, 96)
    say(f"step-7 frames {H} x {W} (1 recon, two views), JPEG q{a.quality} 4:2:0, {a.chunk} frames per vt_jpeg_encode call")
    for name, rgb in sets.items():
        chunks = list(r.render_frames([recon], tv, tf, h, kin, rgb=rgb, end=min(T, 2 * a.chunk), chunk=a.chunk, on_device=True))
        frames = torch.cat(chunks)
        jp = enc.encode(frames)                                    # warm-up (buffers, code objects)
        reps = max(1, n_enc // len(frames))
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(reps):
            jp = enc.encode(frames)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        nfr = reps * len(frames)
        nbytes = np.mean([len(j) for j in jp])
        try:
            from PIL import Image
            ps = []
            host = frames.cpu().numpy()
            for k, j in enumerate(jp):
                d = np.asarray(Image.open(io.BytesIO(j)).convert("RGB")).astype(np.float64)
                ps.append(10 * np.log10(255.0 ** 2 / np.mean((d - host[k]) ** 2)))
            psnr = f"PSNR (libjpeg decode vs input) min {min(ps):.2f} / mean {np.mean(ps):.2f} dB"
        except ImportError:
            psnr = "PSNR not measured (no PIL)"
        say(f"encoder alone [{name}]: {nfr} frames in {dt:.3f} s = {1e3 * dt / nfr:.3f} ms per frame ({nfr / dt:.0f} frames/s), "
            f"{nbytes / 1e3:.0f} kB per frame, {psnr}")
        if a.encode_only:
            break
    rd = H * W * 3
    say(f"byte floor: read {rd / 1e6:.2f} MB of rgb + fp32 planes {H * W * 1.5 * 4 * 2 / 1e6:.1f} MB written and read + < 1 MB of output per frame = "
        f"{(rd + H * W * 12 + 1e6) / (HBM_TBS * 1e12) * 1e3:.4f} ms at {HBM_TBS} TB/s; DCT: {H * W * 1.5 * 16 / 1e6:.0f} M FMAs per frame")
    if a.encode_only:
        if a.out:
            open(os.path.join(out_dir, "videobench_encode_only.txt"), "w").write("\n".join(lines) + "\n")
        return

    # ---- end to end ------------------------------------------------------------------------------------------------------------------------------
    from vistracker_amd.pipeline import SequencePipeline
    from types import SimpleNamespace
    fake = SimpleNamespace(device="cuda:0", ctx=SimpleNamespace(smpl=h))
    V.write_frames([np.zeros((1, 8, 8, 3), np.uint8)], os.path.join(out_dir, "png_warm"))
    for rgb_name, rgb in (("black camera panel", None), ("photo camera panel (host resize per frame)", lambda i: cam)):
        path = os.path.join(out_dir, "step7.avi" if rgb is None else "step7_photo.avi")
        torch.cuda.synchronize(); t0 = time.perf_counter()
        p = SequencePipeline.render(fake, {"recon": recon}, kin, rgb=rgb, template=(tv, tf), chunk=a.chunk, video=path, quality=a.quality)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        size = os.path.getsize(p)
        say(f"step 7 -> .avi [{rgb_name}]: SequencePipeline.render(video=...) {T} frames in {dt:.2f} s = {T / dt:.1f} frames/s, "
            f"file {size / 1e6:.1f} MB ({size / T / 1e3:.0f} kB per frame)")
        torch.cuda.synchronize(); t0 = time.perf_counter(); n = 0
        for ch in r.render_frames([recon], tv, tf, h, kin, rgb=rgb, chunk=a.chunk, on_device=True):
            n += len(ch)
        torch.cuda.synchronize(); dt2 = time.perf_counter() - t0
        say(f"  render_frames(on_device=True) alone, same frames: {n / dt2:.1f} frames/s -> encoding + AVI add {1e3 * (dt - dt2) / T:.3f} ms per frame")
        P = min(a.png_frames, T)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        paths = V.write_frames(r.render_frames([recon], tv, tf, h, kin, rgb=rgb, end=P, chunk=a.chunk), os.path.join(out_dir, "png"))
        dt3 = time.perf_counter() - t0
        say(f"  PNG path (render_frames -> write_frames, PIL) on the first {len(paths)} frames: {dt3:.2f} s = {len(paths) / dt3:.1f} frames/s "
            f"(scaled to {T} frames: {T * dt3 / len(paths):.1f} s)")
        for q in paths:
            os.remove(q)
    if a.out:
        open(os.path.join(out_dir, "r07_video.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
