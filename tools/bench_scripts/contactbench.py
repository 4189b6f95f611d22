"""Cost of the contact step of demo step 7 (csrc/contact.hip) on renderbench.py's workload: a synthetic sequence, two views x one recon per frame,
1200^2 anti-aliased, 16-frame chunks, with the object posed to touch the body in every second frame (tests/contact_model.place_object's rule,
restated here on device vertices).  Prints vt_contact_regions per frame against its VALU bound

    pair tests = NVo x NVs per frame, ~8 lane-ops each (3 sub, 3 mul, 2 add; compare and select extra) at 78.6 T lane-ops/s

vt_render_rgb per view with and without the 14 spheres in the face list, the tile-list growth, and render_frames end to end with and without
viz_contact.  Compare with renderbench.py run on the parent commit in the same session.

usage: python tools/bench_scripts/contactbench.py [--frames 1500] [--chunk 16] [--out profiles/r08_contact.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from vistracker_amd import ops, synthetic as syn  # noqa: E402
from vistracker_amd import visualize as V  # noqa: E402

LANE_OPS_PER_TEST = 8
LANE_OPS_PER_S = 78.6e12


def touching_poses(sv, tv, sp, rng):
    """object poses (obj_angles, obj_trans): even frames touch the body (an object vertex 1 cm outside a random SMPL vertex), odd frames keep the
    sequence's own object pose (renderbench.py's), which stays in front of both cameras"""
    T = len(sv)
    A, t = np.zeros((T, 3, 3), np.float32), np.zeros((T, 3), np.float32)
    R = syn.random_rotations(T, rng).astype(np.float64)
    for b in range(T):
        if b % 2:
            A[b] = sp["obj_R"][b].T; t[b] = sp["obj_t"][b]
            continue
        a = int(rng.integers(sv.shape[1]))
        d = sv[b, a] - sv[b].mean(0); d /= np.linalg.norm(d)
        rv = tv.astype(np.float64) @ R[b].T
        k = int(np.argmin(rv @ d))
        A[b] = R[b].T; t[b] = sv[b, a] + 0.01 * d - rv[k]
    return A, t


def timed(fn, reps):
    fn(); torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "contactbench needs the GPU"
    torch.cuda.set_device(0)
    dev = torch.device("cuda")
    T, ch = a.frames, a.chunk
    model = syn.smplh_model(0); h = ops.SmplhHandle(model)
    labels = syn.part_labels(model)
    sp = syn.sequence_params(T, 7)
    tv, tf = syn.object_template()
    sv = torch.cat([ops.smplh_forward(h, *(torch.tensor(sp[k][i:i + 64], device=dev) for k in ("pose", "betas", "trans")))[0].detach() for i in range(0, T, 64)])
    A, t = touching_poses(sv.cpu().numpy().astype(np.float64), tv, sp, np.random.default_rng(107))
    recon = {"poses": sp["pose"], "betas": sp["betas"], "trans": sp["trans"], "obj_angles": A, "obj_trans": t, "obj_scales": np.ones(T, np.float32)}
    c, s = np.cos(0.35), np.sin(0.35)
    kin = V.KinectTransform(world2local_R=[np.eye(3), np.eye(3), np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])],
                            world2local_t=[np.zeros(3), np.zeros(3), np.array([0.8, 0, 0.3])])
    lines = []
    say = lambda x: (print(x, flush=True), lines.append(x))
    NVs, NVo = 6890, len(tv)
    say(f"contact workload: {T} frames, {ch}-frame chunks, SMPL-H {NVs} vertices searched by {NVo} object vertices per frame = {NVs * NVo / 1e6:.2f} M pair tests, "
        f"even frames posed to touch, odd frames in renderbench.py's pose; 1200^2 anti-aliased, two views per frame")
    cv = V.ContactVisualizer(labels, thres=0.04, radius=0.06)
    # vt_contact_regions on one chunk
    sv_c = sv[:ch].contiguous()
    ov_c = (torch.tensor(tv, device=dev)[None] @ torch.tensor(A[:ch], device=dev) + torch.tensor(t[:ch], device=dev)[:, None]).contiguous()
    reg = cv.regions(sv_c, ov_c)
    touching = int((reg["count"].sum(1) > 0).sum())
    dt = timed(lambda: cv.regions(sv_c, ov_c), 200)
    bound = NVs * NVo * LANE_OPS_PER_TEST / LANE_OPS_PER_S
    say(f"vt_contact_regions ({ch} frames a call, output allocation included, {touching} of {ch} frames touch): {1e3 * dt:.3f} ms per call = {1e6 * dt / ch:.2f} us per frame; "
        f"VALU bound {NVs * NVo / 1e6:.2f} M x {LANE_OPS_PER_TEST} / 78.6 T lane-ops/s = {1e6 * bound:.3f} us per frame -> {bound / (dt / ch):.3f} of it "
        f"({(NVo + 31) // 32 * ch} workgroups of 256 threads on 256 CUs: a call this small is mostly fixed cost -- allocations and two launches -- not arithmetic)")
    dt_s = timed(lambda: cv.spheres(reg), 200)
    say(f"vt_contact_spheres ({ch} x 14 x 162 vertices): {1e3 * dt_s:.3f} ms per call")
    # vt_render_rgb per view without / with the sphere faces
    r = V.RendererSide2side(image_size=1200, part_labels=labels)
    layer = r.nrwrapper.static_layer(r.nrwrapper.front_renderer, r.ground_xz)
    ras, p = r.nrwrapper.raster, r.nrwrapper.front_renderer
    faces = np.concatenate([model["f"], tf + NVs]).astype(np.int32)
    cols = np.concatenate([np.tile(V.COLOR_LIST3[0], (len(model["f"]), 1)), np.tile(V.COLOR_LIST3[1], (len(tf), 1))]).astype(np.float32)
    sf, sc = cv.sphere_faces_colors(NVs + NVo)
    mesh = torch.cat([sv_c, ov_c], 1); withs = torch.cat([mesh, cv.spheres(reg)], 1)
    res = {}
    for name, vb, fb, cb in (("mesh faces only", mesh, faces, cols), ("with 14 spheres per view", withs, np.concatenate([faces, sf]), np.concatenate([cols, sc]))):
        views = torch.stack([kin.world2local_torch(vb, k) for k in (1, 2)], 1).reshape(2 * ch, -1, 3).contiguous()
        fd, cd = torch.tensor(fb, device=dev), torch.tensor(cb, device=dev)
        dtv = timed(lambda: ras.render(views, fd, cd, p, static=layer), max(1, T // ch)) / (2 * ch)
        res[name] = (dtv, ras.last_entries / (2 * ch), len(fb))
        say(f"vt_render_rgb, {name}: {len(fb)} faces per view, {1e3 * dtv:.3f} ms per view, {ras.last_entries / (2 * ch):.0f} tile-list entries per view")
    (d0, e0, _), (d1, e1, _) = res["mesh faces only"], res["with 14 spheres per view"]
    say(f"spheres drawn: render call x {d1 / d0:.3f}, tile list x {e1 / e0:.3f} (4480 sphere faces next to {len(faces)} mesh faces, absent spheres culled at set-up); "
        f"contact search per frame / render call per frame (two views) = {(dt / ch) / (2 * d1):.4f}")
    # end to end
    for _ in r.render_frames([recon], tv, tf, h, kin, start=0, end=2 * ch, chunk=ch, viz_contact=True):
        pass
    for name, kw in (("viz_contact=False", {}), ("viz_contact=True, spheres", {"viz_contact": True})):
        torch.cuda.synchronize(); t0 = time.perf_counter(); n = 0
        for fr in r.render_frames([recon], tv, tf, h, kin, chunk=ch, **kw):
            n += len(fr)
        torch.cuda.synchronize(); dte = time.perf_counter() - t0
        say(f"render_frames end to end, {name}: {n} frames in {dte:.2f} s = {n / dte:.1f} frames/s, {1e3 * dte / (2 * n):.3f} ms per view")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
