"""Inputs shared by tests/test_gpu_boundary.py and tools/bench_scripts/pmdbench.py: the posed body / object case with its query points, and the float64
model's answer with the measured float32 error e32 (tests/pmdist_model.py)."""
import numpy as np
import torch

import pmdist_model as M


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def body_object_case(n_surface=448, n_box=64, seed=0):
    """B = 3 posed frames of the synthetic body and of the object, and N = n_surface + n_box points per frame: area-weighted samples of both meshes, one half
    perturbed by sigma = 0.01, the other by 0.15, plus uniform points of the sampling box (far from everything: the culling's case)"""
    from vistracker_amd import ops, synthetic as syn
    from vistracker_amd.boundary_sampler import BoundarySampler
    model = syn.smplh_model(0); sp = syn.sequence_params(3)
    h = ops.SmplhHandle(model)
    verts, _, _ = ops.smplh_forward(h, dev(sp["pose"]), dev(sp["betas"]), dev(sp["trans"]))
    body = verts.detach().cpu().numpy()
    bf = np.asarray(model["f"]).astype(np.int32)
    ov0, of = syn.object_template()
    obj = (np.einsum("bij,nj->bni", sp["obj_R"], ov0) + sp["obj_t"][:, None]).astype(np.float32)
    rng = np.random.default_rng(seed)
    bmin, bmax = BoundarySampler.get_bounds()
    pts = []
    for b in range(3):
        s = syn.sample_surface(np.concatenate([body[b], obj[b]]), np.concatenate([bf, of + body.shape[1]]), n_surface, seed=seed + b)
        sig = np.where(np.arange(n_surface) % 2 == 0, 0.01, 0.15)[:, None]
        pts.append(np.concatenate([s + sig * rng.normal(size=s.shape), rng.uniform(bmin, bmax, (n_box, 3))]))
    return {"body": body, "body_faces": bf, "obj": obj, "obj_faces": of, "points": np.stack(pts).astype(np.float32), "labels": syn.part_labels(model)}


def model_reference(points, verts, faces):
    """per-frame float64 model, and e32 = max |float32 model - float64 model| of the distances"""
    ref = [M.point_mesh(points[b], verts[b], faces, second=True) for b in range(len(points))]
    r32 = [M.point_mesh(points[b], verts[b], faces, dtype=np.float32) for b in range(len(points))]
    e32 = max(float(np.abs(r["dist"].astype(np.float64) - q["dist"]).max()) for r, q in zip(r32, ref))
    return {k: np.stack([r[k] for r in ref]) for k in ref[0]}, e32
