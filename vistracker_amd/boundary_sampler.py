"""Training samples of SIF-Net and their ground-truth labels, on the device, for a batch of frames at once.

Mirrors ``preprocess/boundary_sampler.py`` (BoundarySampler, :20-218) method by method: ``boundary_sampling``, ``compute_labels``, ``flip_part_labels``,
``get_sample_num``, ``boundary_sample_all``, ``compute_pca``, ``get_grid_samples``, ``get_bounds``.  Differences, all forced by working on the GPU:

* a mesh is ``(verts, faces)``: verts a (B,NV,3) device tensor -- one pose per frame -- or (NV,3) for a single frame, faces (NF,3) integers shared by the
  frames (the reference takes one trimesh / psbody mesh per call).  Per-frame results carry the frame axis exactly when the vertices do.
* the labels -- unsigned distance and closest surface point to both meshes, body part of the nearest SMPL vertex -- are the HIP kernels of
  ``csrc/pmdist.hip`` (``ops.point_mesh_distance``, ``ops.nearest_vertex``) instead of ``igl.signed_distance`` and trimesh's kd-tree.  PARITY UNPINNED,
  restated from the geometric definition: igl, trimesh and psbody are not installed; the pin is the float64 brute force in tests/pmdist_model.py.
* the reference draws from numpy's global random state.  Here every frame draws from a private device ``torch.Generator`` restarted from (seed, key of the
  frame) -- the convention of ``generator.Generator.reseed`` -- so a frame gets the same samples in whatever batch, on whatever rank, it is processed.
  The draws of one frame, in order: faces (inverse CDF of the fp64 areas), barycentric pairs, Gaussian noise, box points.
"""
from __future__ import annotations

import pickle

import numpy as np
import torch

from . import _lib as L
from . import ops

# left <-> right body parts (boundary_sampler.py:104-119)
FLIP_PAIRS = ((1, 6), (2, 7), (3, 8), (4, 9), (5, 10), (12, 13))
# the fixed sampling box, (min, max) per axis (boundary_sampler.py:216-217)
BOUNDS_MIN = (-3.0, -0.9, 0.2)
BOUNDS_MAX = (3.0, 1.80, 4.0)


def _mesh(mesh, name):
    """(verts (B,NV,3) float32 contiguous, faces as given, single) of a ``(verts, faces)`` pair"""
    try:
        verts, faces = mesh
    except (TypeError, ValueError):
        raise L.VtError(f"{name}: a (verts, faces) pair expected") from None
    if not torch.is_tensor(verts) or not verts.is_cuda:
        raise L.VtError(f"{name}: the vertices must be a device tensor; there is no CPU path")
    v, single = ops._frames(verts, name)
    return v, faces, single


class BoundarySampler:
    def __init__(self, part_labels="assets/smpl_parts_dense.pkl", seed=0):
        """``part_labels``: the (6890,) integer label of every SMPL vertex (``FitContext.labels``, ``synthetic.part_labels``), or the reference's asset
        (boundary_sampler.py:21-27): a path to, or the loaded dict of, a pickle {part name: vertex indices}, part n = the n-th key."""
        if isinstance(part_labels, (str, bytes)):
            with open(part_labels, "rb") as fh:
                part_labels = pickle.load(fh)
        if isinstance(part_labels, dict):
            labels = np.zeros((6890,), dtype="int32")
            for n, k in enumerate(part_labels):
                labels[np.asarray(part_labels[k])] = n
        else:
            labels = np.asarray(part_labels.cpu() if torch.is_tensor(part_labels) else part_labels).astype(np.int32).reshape(-1)
        self.part_labels = labels
        self.seed = int(seed)
        self._labels_d = {}          # device -> labels
        self._faces_ok = {}          # (id(faces), NV) -> validated int32 device faces

    # ---- helpers ------------------------------------------------------------------------------------------------------------------------------------------
    def _labels_on(self, device):
        if device not in self._labels_d:
            self._labels_d[device] = torch.as_tensor(self.part_labels, device=device)
        return self._labels_d[device]

    def _faces(self, faces, n_verts, device):
        """validated int32 faces on ``device``; the check reads the device once per (faces object, vertex count).  The cache goes by the OBJECT: a faces
        tensor changed in place after its first use is not looked at again (the kernel clamps indices, so memory stays safe, but the labels would be those of
        the clamped mesh) -- pass a new tensor for a new mesh."""
        key = (id(faces), n_verts, str(device))
        hit = self._faces_ok.get(key)
        if hit is None or hit[0] is not faces:
            if len(self._faces_ok) > 8:
                self._faces_ok.clear()
            hit = self._faces_ok[key] = (faces, ops.check_faces(faces, n_verts).to(device))
        return hit[1]

    def _base_seed(self, generator):
        """base seed of a call: ``generator`` is None (the sampler's seed), an int, or a torch.Generator, of which only ``initial_seed()`` is read.  The
        draws themselves come from a private device generator restarted per frame: the caller's object is never reseeded nor advanced, so passing the same
        Generator to several calls gives every call the same base."""
        if isinstance(generator, torch.Generator):
            return int(generator.initial_seed())
        return self.seed if generator is None else int(generator)

    @staticmethod
    def frame_seed(base, key):
        """seed of the frame with integer ``key`` (generator.Generator.reseed's mix)"""
        return (int(base) * 1000003 + int(key)) % (2 ** 63 - 1)

    @staticmethod
    def _surface_points(verts, faces, cdf, n, g):
        """n area-weighted uniform points on one frame's mesh: verts (NV,3), faces (NF,3) int64, cdf (NF,) fp64 running sum of the areas"""
        r = torch.rand(n, generator=g, device=verts.device, dtype=torch.float64) * cdf[-1]
        fi = torch.searchsorted(cdf, r, right=True).clamp_(max=faces.shape[0] - 1)
        u = torch.rand(n, 2, generator=g, device=verts.device)
        over = u.sum(1, keepdim=True) > 1
        u = torch.where(over, 1 - u, u)
        c = verts[faces[fi]]                                                     # (n,3,3)
        return c[:, 0] + u[:, :1] * (c[:, 1] - c[:, 0]) + u[:, 1:] * (c[:, 2] - c[:, 0])

    @staticmethod
    def _area_cdf(verts, faces):
        """(B,NF) fp64 running sum of the triangle areas, component-wise arithmetic only (a frame's values do not depend on the batch around it)"""
        c = verts.double()[:, faces]                                             # (B,NF,3,3)
        e1, e2 = c[:, :, 1] - c[:, :, 0], c[:, :, 2] - c[:, :, 0]
        nx = e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1]
        ny = e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2]
        nz = e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]
        area = 0.5 * torch.sqrt(nx * nx + ny * ny + nz * nz)
        return torch.stack([torch.cumsum(a, 0) for a in area])                   # one 1-D scan per frame: the same reduction whatever B

    # ---- the reference's interface ------------------------------------------------------------------------------------------------------------------------
    def boundary_sampling(self, smpl, obj, sigma=0.05, sample_num=100000, grid_ratio=0.01, equal_sample=False, generator=None, keys=None):
        """Sample boundary points on a pair of interacting SMPL and object meshes and label them (boundary_sampler.py:29-73).

        ``sample_num`` surface points -- area-weighted over the concatenation of both meshes, or exactly ``sample_num // 2`` on each with ``equal_sample``
        (body first) -- perturbed by ``sigma`` N(0,1), followed by ``int(grid_ratio * sample_num)`` uniform points of ``get_bounds()``.
        ``generator``: None, an int seed or a torch.Generator (see ``_base_seed``: read, never reseeded); ``keys``: one integer per frame (default 0 .. B-1): frame b
        draws from the stream seeded with ``frame_seed(base, keys[b])``.
        Returns (samples (B,N,3), d_h (B,N), d_o (B,N), parts (B,N) int32, neighbours_h (B,N,3), neighbours_o (B,N,3)) device tensors."""
        sv, sf_in, single = _mesh(smpl, "smpl")
        ov, of_in, osingle = _mesh(obj, "obj")
        if single != osingle or sv.shape[0] != ov.shape[0] or sv.device != ov.device:
            raise L.VtError(f"boundary_sampling: smpl {tuple(sv.shape)} and obj {tuple(ov.shape)} must share the frame axis and the device")
        B, dev = sv.shape[0], sv.device
        sf = self._faces(sf_in, sv.shape[1], dev).long(); of = self._faces(of_in, ov.shape[1], dev).long()
        keys = list(range(B)) if keys is None else [int(k) for k in keys]
        if len(keys) != B:
            raise L.VtError(f"boundary_sampling: {len(keys)} keys for {B} frames")
        n_grid = int(grid_ratio * sample_num)
        n_surf = 2 * (int(sample_num) // 2) if equal_sample else int(sample_num)      # the reference returns 2 (sample_num // 2) surface points there
        g, base = torch.Generator(device=dev), self._base_seed(generator)
        with torch.cuda.device(dev):
            if equal_sample:
                cdf_h, cdf_o = self._area_cdf(sv, sf), self._area_cdf(ov, of)
            else:
                cv = torch.cat([sv, ov], 1); cf = torch.cat([sf, of + sv.shape[1]], 0)
                cdf_c = self._area_cdf(cv, cf)
            pmin, pmax = self.get_bounds()
            out = torch.empty(B, n_surf + n_grid, 3, device=dev)
            for b in range(B):
                g.manual_seed(self.frame_seed(base, keys[b]))
                if equal_sample:
                    n = n_surf // 2
                    pts = torch.cat([self._surface_points(sv[b], sf, cdf_h[b], n, g), self._surface_points(ov[b], of, cdf_o[b], n, g)], 0)
                else:
                    pts = self._surface_points(cv[b], cf, cdf_c[b], n_surf, g)
                pts = pts + float(sigma) * torch.randn(pts.shape, generator=g, device=dev)
                out[b, :n_surf] = pts
                out[b, n_surf:] = self.get_grid_samples(pmin, pmax, n_grid, generator=g, device=dev)
            samples = out
            d_h, d_o, n_h, n_o, parts = self.compute_labels((ov, of_in), samples, (sv, sf_in))
        res = (samples, d_h, d_o, parts, n_h, n_o)
        return tuple(t[0] for t in res) if single else res

    def compute_labels(self, obj, samples_all, smpl):
        """Labels of the samples (boundary_sampler.py:75-100): returns (d_h, d_o, neighbours_h, neighbours_o, parts) -- unsigned distance to the human and
        to the object surface, the closest surface points, and the body part of the nearest SMPL vertex.  Device tensors; the frame axis follows the
        meshes'."""
        sv, sf_in, single = _mesh(smpl, "smpl")
        ov, of_in, _ = _mesh(obj, "obj")
        pts, psingle = ops._frames(samples_all, "samples_all")
        if psingle != single:
            raise L.VtError("compute_labels: the samples carry a frame axis exactly when the meshes do")
        dev = sv.device
        if sv.shape[1] != self.part_labels.shape[0]:
            raise L.VtError(f"compute_labels: {sv.shape[1]} SMPL vertices but {self.part_labels.shape[0]} part labels")
        with torch.cuda.device(dev):
            d_h, n_h, _ = ops.point_mesh_distance(pts, sv, self._faces(sf_in, sv.shape[1], dev), want_face=False, validate=False)
            d_o, n_o, _ = ops.point_mesh_distance(pts, ov, self._faces(of_in, ov.shape[1], dev), want_face=False, validate=False)
            vid, _ = ops.nearest_vertex(pts, sv, want_dist=False)
            parts = self._labels_on(dev)[vid.long()]
        res = (d_h, d_o, n_h, n_o, parts)
        return tuple(t[0] for t in res) if single else res

    def flip_part_labels(self, parts):
        """left <-> right (boundary_sampler.py:102-124); numpy array or tensor in, the same kind out"""
        new = parts.clone() if torch.is_tensor(parts) else np.array(parts, copy=True)
        for a, b in FLIP_PAIRS:
            new[parts == a] = b
            new[parts == b] = a
        return new

    def get_sample_num(self, ratio, total_sample, thres=10000):
        """int(ratio * total_sample), but no fewer than ``thres`` (boundary_sampler.py:126-130)"""
        n = int(ratio * total_sample)
        return thres if n < thres else n

    def boundary_sample_all(self, landmark, smpl_mesh, obj_mesh, sigmas, ratios, sample_num, grid_ratio=1 / 16., flip=False, add_neighbours=False,
                            equal_sample=False, generator=None, keys=None):
        """Boundary sampling for a set of sigmas (boundary_sampler.py:132-192), host numpy arrays out with the reference's keys and dtypes:
        'points', 'dist_h', 'dist_o', 'parts' -> {'sigma{s}': float32 / float32 / float32 / uint8}, 'pca_axis' (3,3), 'smpl_center' (3,), 'body_kpts' (25,3),
        'obj_center' (3,) float32, and 'neighbours_h', 'neighbours_o' with ``add_neighbours``; every array gains a leading frame axis when the meshes have one.
        ``landmark``: an ``ops.LandmarkHandle`` of the body-25 regressor, or an object with ``get_body_kpts(verts (B,6890,3)) -> (B,25,3)``; the SMPL centre is
        keypoint 8 (lib_smpl/body_landmark.py:52-56).  Each sigma draws from its own stream: frame key * 64 + position of the sigma."""
        sv, sf_in, single = _mesh(smpl_mesh, "smpl_mesh")
        ov, of_in, _ = _mesh(obj_mesh, "obj_mesh")
        B = sv.shape[0]
        keys = list(range(B)) if keys is None else [int(k) for k in keys]
        base = self._base_seed(generator)                 # read once: every sigma and every frame derives its stream from this one number
        if len(sigmas) > 64:
            raise L.VtError("boundary_sample_all: at most 64 sigmas")
        names = ("points", "dist_h", "dist_o", "parts", "neighbours_h", "neighbours_o")
        all_ = {n: {} for n in names}

        def host(t, dtype):
            a = t.cpu().numpy().astype(dtype)
            return a[0] if single else a

        for i, (s, r) in enumerate(zip(sigmas, ratios)):
            n_s = self.get_sample_num(r, sample_num, thres=sample_num // 2)
            pts, d_h, d_o, parts, n_h, n_o = self.boundary_sampling((sv, sf_in), (ov, of_in), s, n_s, grid_ratio=grid_ratio, equal_sample=equal_sample,
                                                                    generator=base, keys=[k * 64 + i for k in keys])
            if flip:
                parts = self.flip_part_labels(parts)
            name = "sigma{}".format(s)
            for n, t, dt in zip(names, (pts, d_h, d_o, parts, n_h, n_o), (np.float32, np.float32, np.float32, np.uint8, np.float32, np.float32)):
                all_[n][name] = host(t, dt)
        with torch.cuda.device(sv.device):
            kpts = ops.landmarks(landmark, sv) if isinstance(landmark, ops.LandmarkHandle) else torch.as_tensor(landmark.get_body_kpts(sv))
        data = {
            "points": all_["points"], "dist_h": all_["dist_h"], "dist_o": all_["dist_o"], "parts": all_["parts"],
            "pca_axis": self.compute_pca((ov[0] if single else ov, of_in)).astype(np.float32),
            "smpl_center": host(kpts[:, 8], np.float32),
            "body_kpts": host(kpts, np.float32),
            "obj_center": host(ov.mean(1), np.float32),
        }
        if add_neighbours:
            data["neighbours_h"] = all_["neighbours_h"]; data["neighbours_o"] = all_["neighbours_o"]
        return data

    @staticmethod
    def compute_pca(obj):
        """PCA axes of the object's vertices (boundary_sampler.py:194-200: sklearn PCA(n_components=3).fit(v).components_), on the host in float64:
        the rows are the right singular vectors of the centred vertices, by descending variance.  SIGN CONVENTION (sklearn 1.7's
        ``svd_flip(u, vt, u_based_decision=False)``, pinned by tests/test_host_boundary.py against the installed sklearn): each row is oriented so that its
        entry of largest magnitude is positive.  (sklearn < 1.5 decided on the columns of U instead; the two differ by the sign of whole rows.)
        ``obj``: (verts, faces) or the vertices alone, (NV,3) -> (3,3), (B,NV,3) -> (B,3,3); tensors or arrays."""
        v = obj[0] if isinstance(obj, (tuple, list)) else obj
        v = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64)
        single = v.ndim == 2
        out = []
        for x in (v[None] if single else v):
            _, _, vt = np.linalg.svd(x - x.mean(0), full_matrices=False)
            sign = np.sign(vt[np.arange(3), np.abs(vt).argmax(1)])
            sign[sign == 0] = 1
            out.append(vt * sign[:, None])
        return out[0] if single else np.stack(out)

    @staticmethod
    def get_grid_samples(pmin, pmax, sample_num, generator=None, device=None):
        """``sample_num`` uniform points of the box [pmin, pmax) (boundary_sampler.py:202-209): a (sample_num,3) float32 tensor on ``device`` (default: the
        generator's device, else the current GPU) drawn from ``generator``"""
        if device is None:
            device = generator.device if generator is not None else torch.device("cuda", torch.cuda.current_device())
        lo = torch.as_tensor(np.asarray(pmin, dtype=np.float32), device=device); hi = torch.as_tensor(np.asarray(pmax, dtype=np.float32), device=device)
        return torch.rand(int(sample_num), 3, generator=generator, device=device) * (hi - lo) + lo

    @staticmethod
    def get_bounds():
        """the fixed sampling box (boundary_sampler.py:211-218): (bmin, bmax) float64 arrays"""
        return np.array(BOUNDS_MIN), np.array(BOUNDS_MAX)
