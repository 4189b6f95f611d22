"""Step-7 throughput (demo.sh: render/render_side_comp.py) of a synthetic sequence: two views x one recon per frame, SMPL-H + object + the 80 x 80 m
xz checkerboard ground, 1200^2 with anti-aliasing (2400^2 raster), through RendererSide2side.render_frames (uint8 frames to the host) and through
vt_render_rgb alone.  Prints ms per view, frames/s, the tile-list size and a VALU bound for the resolve:

    resolve work  = sum over tiles of 256 pixels x list length   (every pixel runs the inside test against every face binned to its tile)
    bound         = work x VALU_PER_TEST / (256 CU x 4 SIMD x 32 lanes x clock)

VALU_PER_TEST = 16 (three edge functions: 6 sub, 6 mul, 3 compare, 1 branch mask; the depth of covered pixels and the LDS reads are extra).
With --kernels the per-kernel split comes from `rocprofv3 --kernel-trace --stats` in a separate run of this script (pass its stats CSV).

usage: python tools/bench_scripts/renderbench.py [--frames 1500] [--chunk 8] [--out profiles/r07_render.txt] [--kernel-stats stats.csv]
"""
import argparse
import csv
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vistracker_amd import ops, synthetic as syn  # noqa: E402
from vistracker_amd import visualize as V  # noqa: E402

VALU_PER_TEST = 16
CLOCK_GHZ = 2.4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--chunk", type=int, default=8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats.csv of a run of this script")
    ap.add_argument("--render-only", action="store_true", help="vt_render_rgb only (for the profiler run)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "renderbench needs the GPU"
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
    lines = []
    say = lambda x: (print(x), lines.append(x))
    nf = len(model["f"]) + len(tf)
    say(f"step-7 workload: {T} frames x 2 views x 1 recon, {nf} mesh faces (SMPL-H {len(model['f'])} + object {len(tf)}) per view + "
        f"{r.ground_xz.faces.shape[1]} ground faces (static layer), 1200^2 anti-aliased (2400^2 raster), chunk {a.chunk} frames = {2 * a.chunk} views per call")
    # static layer set-up (once per camera)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    layer = r.nrwrapper.static_layer(r.nrwrapper.front_renderer, r.ground_xz)
    torch.cuda.synchronize(); say(f"static layer (ground set-up + binning + resolve, once): {1e3 * (time.perf_counter() - t0):.1f} ms")
    # warm-up
    for _ in r.render_frames([recon], tv, tf, h, kin, start=0, end=2 * a.chunk, chunk=a.chunk):
        pass
    if not a.render_only:
        torch.cuda.synchronize(); t0 = time.perf_counter(); n = 0
        for fr in r.render_frames([recon], tv, tf, h, kin, chunk=a.chunk):
            n += len(fr)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        say(f"render_frames end to end (SMPL-H forward, object, camera transforms, vt_render_rgb, uint8 panels, frames to host): {n} frames in {dt:.2f} s "
            f"= {n / dt:.1f} frames/s, {1e3 * dt / (2 * n):.3f} ms per view")
    # vt_render_rgb alone on the views of the first chunks (built once)
    dev = torch.device("cuda")
    ii = torch.arange(a.chunk, device=dev)
    g = lambda k, w: torch.as_tensor(np.asarray(recon[k], np.float32).reshape(T, w), device=dev)[ii].contiguous()
    sv, _, _ = ops.smplh_forward(h, g("poses", 156), g("betas", 10), g("trans", 3))
    ov = (torch.tensor(tv, device=dev)[None] @ g("obj_angles", 9).reshape(-1, 3, 3) + g("obj_trans", 3)[:, None])
    verts = torch.cat([sv.detach(), ov], 1)
    views = torch.stack([kin.world2local_torch(verts, k) for k in (1, 2)], 1).reshape(2 * a.chunk, -1, 3).contiguous()
    faces = np.concatenate([model["f"], tf + 6890]).astype(np.int32)
    cols = np.concatenate([np.tile(V.COLOR_LIST3[0], (len(model["f"]), 1)), np.tile(V.COLOR_LIST3[1], (len(tf), 1))]).astype(np.float32)
    fd, cd = torch.tensor(faces, device=dev), torch.tensor(cols, device=dev)
    ras, p = r.nrwrapper.raster, r.nrwrapper.front_renderer
    ras.render(views, fd, cd, p, static=layer)
    reps = max(1, (2 * T) // (2 * a.chunk))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        ras.render(views, fd, cd, p, static=layer)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    nv = reps * 2 * a.chunk
    ms_view = 1e3 * dt / nv
    entries = ras.last_entries
    say(f"vt_render_rgb alone: {nv} views in {dt:.2f} s = {ms_view:.3f} ms per view ({1e3 / ms_view / 2:.1f} frames/s at two views per frame); "
        f"1500 frames x 2 views: {1.5 * 2 * ms_view:.2f} s")
    work = 256.0 * entries / (2 * a.chunk)
    bound_ms = work * VALU_PER_TEST / (256 * 4 * 32 * CLOCK_GHZ * 1e9) * 1e3
    say(f"tile lists: {entries / (2 * a.chunk):.0f} entries per view (16 x 16 tiles, 22500 per view) -> {work / 1e6:.1f} M pixel-face inside tests per view")
    say(f"VALU bound of the resolve: {work / 1e6:.1f} M tests x {VALU_PER_TEST} VALU / (256 CU x 4 SIMD x 32 lanes x {CLOCK_GHZ} GHz) = {bound_ms:.4f} ms per view; "
        f"the whole call runs at {bound_ms / ms_view:.3f} of it")
    out_px = 2400 * 2400
    say(f"output floor: rgb + alpha fp32 at 1200^2 = {1200 * 1200 * 16 / 1e6:.1f} MB written per view ({1200 * 1200 * 16 / 6.29e12 * 1e3:.4f} ms at 6.29 TB/s), "
        f"{out_px / 1e6:.2f} M raster pixels")
    if a.kernel_stats and os.path.exists(a.kernel_stats):
        rows = list(csv.DictReader(open(a.kernel_stats)))
        tot = {}
        for row in rows:
            nm = row.get("Name", row.get("KernelName", ""))
            for key, grp in (("rnd_setup", "setup"), ("rnd_count", "binning"), ("rnd_scan", "binning"), ("rnd_fill", "binning"),
                             ("rnd_resolve_kernel<true>", "resolve"), ("rnd_resolve_kernel<false>", "static layer"), ("rnd_panel", "panels")):
                if key in nm.replace("ILb1E", "<true>").replace("ILb0E", "<false>"):
                    tot[grp] = tot.get(grp, 0.0) + float(row.get("TotalDurationNs", 0))
        s_ = sum(v for k, v in tot.items() if k != "static layer")
        if s_ > 0:
            say("kernel time split (rocprofv3, per-view calls): " + ", ".join(f"{k} {100 * v / s_:.1f} %" for k, v in sorted(tot.items()) if k != "static layer"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
