"""Cost and accuracy of the training-sample labels (csrc/pmdist.hip): distance and closest point to the body (13776 faces) and to the object (2500 faces),
nearest body vertex, for B = 16 frames of N = 110 000 points each (100 000 surface samples at sigma = 0.05 + 10 000 box points: boundary_sampling's
defaults at grid_ratio 0.1).  No earlier GPU code does this, so there is no parent time; the yardstick is the arithmetic floor

    point-triangle tests EXECUTED (counted by vt_point_mesh_distance_ex) x LANE_OPS_FULL + sphere tests (all B N NF) x LANE_OPS_SPHERE, over the fp32
    vector rate without contraction or packing (78.6 T lane-ops/s; the build uses -ffp-contract=off -fno-slp-vectorize)

The floor is INDICATIVE: the lane-ops per test are estimated from the source (LANE_OPS_FULL below), not counted in the gfx950 instruction stream, the rate is
the project's convention for un-packed fp32 VALU without fused multiply-add and is not measured here, and the fp64 re-evaluations of the near-minimal
triangles are not in it.  The culling hit rate is the share of the B N NF tests the kernel skipped.  The accuracy section repeats the measurement of
tests/test_gpu_boundary.py on its inputs (tests/pmdist_cases.py: e32 of the float64 / float32 model, the kernel's own error).

usage: python tools/bench_scripts/pmdbench.py [--frames 16] [--points 100000] [--grid 10000] [--out profiles/r13_pmdist.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from vistracker_amd import ops, synthetic as syn  # noqa: E402
from vistracker_amd.boundary_sampler import BoundarySampler  # noqa: E402

LANE_OPS_FULL = 105       # ESTIMATE from the source of pm_closest<float>: 15 sub, 6 dots x 5, 3 x 3 for va vb vc, ~15 compares / selects, 2 divisions (~10 each), 9 for the point, 8 for the distance
LANE_OPS_SPHERE = 11      # 3 sub, 5 for the dot, add, mul, compare
LANE_OPS_PER_S = 78.6e12


def timed(fn, reps):
    fn(); torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--grid", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    B, N = a.frames, a.points + a.grid
    model = syn.smplh_model(0); sp = syn.sequence_params(B)
    h = ops.SmplhHandle(model)
    dev = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device="cuda")      # noqa: E731
    body, _, _ = ops.smplh_forward(h, dev(sp["pose"]), dev(sp["betas"]), dev(sp["trans"]))
    body = body.detach().contiguous(); bf = dev(np.asarray(model["f"]), torch.int32)
    ov0, of_np = syn.object_template()
    obj = torch.einsum("bij,nj->bni", dev(sp["obj_R"]), dev(ov0)) + dev(sp["obj_t"])[:, None]
    obj = obj.contiguous(); of = dev(of_np, torch.int32)
    bs = BoundarySampler(syn.part_labels(model))
    t0 = time.perf_counter()
    samples = bs.boundary_sampling((body, bf), (obj, of), sigma=0.05, sample_num=a.points, grid_ratio=a.grid / a.points)[0]
    torch.cuda.synchronize()
    say(f"pmdbench: B = {B} frames, N = {N} points per frame ({a.points} surface at sigma 0.05 + {a.grid} box), body {bf.shape[0]} faces, object {of.shape[0]} faces")
    say(f"boundary_sampling (sampling in torch + labels, first call): {1e3 * (time.perf_counter() - t0) / B:.2f} ms per frame")

    for name, v, f in (("body", body, bf), ("object", obj, of)):
        NF = f.shape[0]; total = B * N * NF
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        ops.point_mesh_distance(samples, v, f, validate=False, n_tests=cnt)
        done = int(cnt)
        floor = (done * LANE_OPS_FULL + total * LANE_OPS_SPHERE) / LANE_OPS_PER_S
        floor_nocull = total * LANE_OPS_FULL / LANE_OPS_PER_S
        t_c = timed(lambda: ops.point_mesh_distance(samples, v, f, validate=False), a.reps)
        t_d = timed(lambda: ops.point_mesh_distance(samples, v, f, want_closest=False, want_face=False, validate=False), a.reps)
        t_n = timed(lambda: ops.point_mesh_distance(samples, v, f, validate=False, culling=False), 1)
        say(f"{name}: point-triangle tests executed {done} of {total} = culling skipped {100 * (1 - done / total):.2f} %")
        say(f"{name}: dist + closest + face_id {1e3 * t_c / B:.3f} ms per frame, dist only {1e3 * t_d / B:.3f} ms per frame; estimated arithmetic floor of the executed fp32 tests "
            f"{1e3 * floor / B:.3f} ms per frame ({100 * floor / t_c:.0f} % of it reached; indicative, see the docstring); culling off {1e3 * t_n / B:.3f} ms per frame (floor {1e3 * floor_nocull / B:.3f})")
    t_v = timed(lambda: ops.nearest_vertex(samples, body, want_dist=False), a.reps)
    say(f"nearest body vertex: {1e3 * t_v / B:.3f} ms per frame (floor {1e3 * B * N * body.shape[1] * 9 / LANE_OPS_PER_S / B:.3f} at 9 lane-ops per pair)")
    t_l = timed(lambda: bs.compute_labels((obj, of), samples, (body, bf)), a.reps)
    say(f"compute_labels (body + object with closest points, parts): {1e3 * t_l / B:.3f} ms per frame")

    # accuracy on the inputs of tests/test_gpu_boundary.py
    import pmdist_cases as T
    c = T.body_object_case()
    p = dev(c["points"])
    for name, vk, fk in (("body", "body", "body_faces"), ("object", "obj", "obj_faces")):
        ref, e32 = T.model_reference(c["points"], c[vk], c[fk])
        dist, closest, _ = ops.point_mesh_distance(p, dev(c[vk]), dev(c[fk], torch.int32))
        err = np.abs(dist.cpu().numpy() - ref["dist"])
        tie = (ref["dist2"] - ref["dist"]) < 4 * e32
        dq = np.linalg.norm(closest.cpu().numpy() - ref["closest"], axis=-1)
        say(f"accuracy, {name} (3 x 512 points of the GPU test): e32 (float32 model - float64 model) = {e32:.3e} m, kernel |dist - float64 model| max = "
            f"{err.max():.3e} m, |closest - model closest| max = {dq[~tie].max():.3e} m ({int(tie.sum())} equidistant points excluded)")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
