"""A labelled training batch of SIF-Net assembled on the device, and the validation errors of a checkpoint on it.

``make_training_batch`` mirrors ``BehaveDatasetOnline.boundary_sampling`` and ``get_item`` (data/traindata_online.py:83-201) for B frames at once;
``validate`` is one batch of the reference's ``compute_val_loss`` (trainer/trainer.py:321-346: query, then ``get_errors``, no gradient) with no host labelling.

Out of scope here: file and ``KinectTransform`` IO (the meshes arrive in camera-local coordinates), image loading (``SequenceLoader(device_prep=True)``
builds the network inputs), ``smpl_vect`` (``load_neighbour_h``), the feature-map and encoder gradients, learning-rate schedules, checkpoint directories.

``DecoderTrainer`` is the reference's ``Trainer.train_step`` (trainer/trainer.py:97-106) for the decoder parameter group: the five point decoders of a checkpoint
are fine-tuned on labelled batches with the encoder, and so the feature maps, frozen.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as L
from . import ops
from .boundary_sampler import BoundarySampler, _mesh


def sample_counts(ratios, total_sample_num, grid_ratio=0.01):
    """(grid points, surface samples per sigma) of a frame (traindata_online.py:56-59), raising unless they add up to ``total_sample_num`` as
    ``check_sample_num`` asserts (:79-81)"""
    total = int(total_sample_num)
    n_grid = int(total * grid_ratio)
    nums = [int((total - n_grid) * r) for r in ratios]
    if n_grid + sum(nums) != total:
        raise L.VtError(f"make_training_batch: {n_grid} + {sum(nums)} != {total}")
    return n_grid, nums


def make_training_batch(sampler: BoundarySampler, smpl, obj, body_center, visibility, sigmas, ratios, total_sample_num, grid_ratio=0.01, depth=None, keys=None,
                        generator=None):
    """``smpl`` / ``obj``: (verts (B,NV,3) device tensor in camera-local coordinates, faces (NF,3)); ``body_center`` (B,3) the SMPL centre of every frame
    (``landmark.center_from_verts``); ``visibility`` (B,) the object's visibility ratio.  ``depth``: None, or the depth the body is brought to: both meshes and
    the centre are scaled by depth / body_center[:, 2] (:147-151).  Frame b draws, from its private generator restarted with
    ``sampler.frame_seed(base, keys[b])`` (``keys`` default 0 .. B-1; ``generator`` as in ``BoundarySampler.boundary_sampling``): the grid points of
    ``get_bounds()``, then for every sigma its surface samples on the concatenated mesh (faces, barycentric pairs, noise), then one random permutation the
    points are scattered by (:158-169) -- so a frame's entries do not depend on the batch around it.
    -> the reference's keys: points (B,N,3), df_h, df_o (B,N), labels (B,N) int32, and the per-frame labels in their compact form pca_axis (B,3,3), body_center
    (B,3), obj_center (B,3) = mean of the object's vertices - body_center, visibility (B,); device tensors, float32 unless noted."""
    sv, sf_in, single = _mesh(smpl, "smpl")
    ov, of_in, osingle = _mesh(obj, "obj")
    if single or osingle or sv.shape[0] != ov.shape[0] or sv.device != ov.device:
        raise L.VtError(f"make_training_batch: smpl {tuple(sv.shape)} and obj {tuple(ov.shape)} must carry the same frame axis on one device")
    B, dev = sv.shape[0], sv.device
    for t, name, shape in ((body_center, "body_center", (B, 3)), (visibility, "visibility", (B,))):
        if not torch.is_tensor(t) or t.device != dev or tuple(t.shape) != shape:
            raise L.VtError(f"make_training_batch: {name} is a {shape} tensor on {dev}")
    if len(sigmas) != len(ratios):
        raise L.VtError(f"make_training_batch: {len(sigmas)} sigmas for {len(ratios)} ratios")
    keys = list(range(B)) if keys is None else [int(k) for k in keys]
    if len(keys) != B:
        raise L.VtError(f"make_training_batch: {len(keys)} keys for {B} frames")
    n_grid, nums = sample_counts(ratios, total_sample_num, grid_ratio)
    total = n_grid + sum(nums)
    bc = ops._f32(body_center)
    with torch.cuda.device(dev):
        if depth is not None:
            scale = (float(depth) / bc[:, 2]).reshape(B, 1, 1)
            sv, ov, bc = sv * scale, ov * scale, bc * scale[:, 0]
        sf = sampler._faces(sf_in, sv.shape[1], dev).long(); of = sampler._faces(of_in, ov.shape[1], dev).long()
        cv = torch.cat([sv, ov], 1); cf = torch.cat([sf, of + sv.shape[1]], 0)
        cdf = sampler._area_cdf(cv, cf)
        pmin, pmax = sampler.get_bounds()
        g, base = torch.Generator(device=dev), sampler._base_seed(generator)
        points = torch.empty(B, total, 3, device=dev)
        for b in range(B):
            g.manual_seed(sampler.frame_seed(base, keys[b]))
            parts = [sampler.get_grid_samples(pmin, pmax, n_grid, generator=g, device=dev)]
            for sigma, num in zip(sigmas, nums):
                s = sampler._surface_points(cv[b], cf, cdf[b], num, g)
                parts.append(s + float(sigma) * torch.randn(s.shape, generator=g, device=dev))
            choice = torch.randperm(total, generator=g, device=dev)
            points[b, choice] = torch.cat(parts, 0)
        d_h, d_o, _, _, labels = sampler.compute_labels((ov, of_in), points, (sv, sf_in))
        pca = torch.as_tensor(np.ascontiguousarray(sampler.compute_pca(ov), dtype=np.float32), device=dev)
        return {"points": points, "df_h": d_h, "df_o": d_o, "labels": labels, "pca_axis": pca, "body_center": bc,
                "obj_center": torch.stack([v.mean(0) for v in ov]) - bc,          # one reduction per frame: the same whatever B
                "visibility": ops._f32(visibility)}


def validate(net, batch, crop_center, max_dist=5.0):
    """The validation errors of ``net`` (a ``SIFNetQuery`` whose feature maps are set) on a labelled batch: ``net.query`` at ``batch["points"]``, then
    ``net.get_errors``, without gradients.  -> {name: float} for df_h, df_o, parts, pca, vis, obj_center (weighted, the reference's ``sep_errors``) and
    ``total``.  One synchronisation: the seven numbers come back in one copy."""
    with torch.no_grad():
        net.query(batch["points"], crop_center=crop_center, body_center=batch["body_center"])
        error, losses_all = net.get_errors(batch["df_h"], batch["df_o"], batch["labels"], batch["pca_axis"], max_dist, batch["body_center"], batch["obj_center"],
                                           visibility=batch["visibility"])
        out = torch.cat([losses_all, error.reshape(1)]).cpu().tolist()
    return dict(zip(ops.LOSS_SLOTS + ("total",), out))


class DecoderTrainer:
    """``Trainer.train_step`` (trainer/trainer.py:97-106) with ``optim.Adam(param_groups, lr=1e-3)`` (trainer.py:31-44) for the decoders of ``net`` (a
    ``SIFNetQuery``): the parameters are copied from ``net.decoders`` into one flat device tensor (``ops.DecoderParams``) that ``ops.FusedAdam`` updates with one
    launch a step; ``net`` itself serves the maps, the loss weights and ``get_errors``, its packed handle is left alone.  ``export()`` hands the trained decoders
    back as a new ``SIFNetQuery``."""

    def __init__(self, net, lr=1e-3, max_dist=5.0):
        self.net, self.max_dist = net, float(max_dist)
        self.params = ops.DecoderParams.from_decoders(net.decoders, cam=net.camera.as_cam5(), device=net.device)
        self.optimizer = ops.FusedAdam([self.params.flat], lr=lr)

    def train_step(self, batch, crop_center, maps=None, train_decoders=True):
        """one step on a batch of ``make_training_batch``: zero_grad, query, get_errors, backward, Adam.  ``maps``: a ``FeatureMaps`` or a list of S, one per
        stack (default: the maps set on ``net``).  Map tensors that require grad receive (accumulate, as any leaf) their ``.grad`` from the same backward; what
        steps them -- an encoder's backward, an optimiser of the caller's -- is the caller's.  ``train_decoders=False``: the decoders are data, only the maps
        get a gradient and there is no Adam step.  -> (error (), losses_all (6,)): float64 device tensors of the step's objective BEFORE the update; nothing
        here synchronises."""
        if train_decoders:
            self.optimizer.zero_grad()
        self.net.query_train(self.params, batch["points"], crop_center=crop_center, body_center=batch["body_center"], maps=maps, train_decoders=train_decoders)
        error, losses_all = self.net.get_errors(batch["df_h"], batch["df_o"], batch["labels"], batch["pca_axis"], self.max_dist, batch["body_center"],
                                                batch["obj_center"], visibility=batch["visibility"])
        error.backward()
        if train_decoders:
            self.optimizer.step()
        return error.detach(), losses_all

    def state_dict(self, prefix=""):
        """the decoders under the reference's checkpoint keys (``df.0.weight`` (128, 611, 1), ...)"""
        return self.params.state_dict(prefix)

    def export(self):
        """-> a new ``SIFNetQuery`` holding the trained decoders (packed by ``vt_sifnet_create`` as any checkpoint's), with this network's camera, encoder, maps
        and loss settings: it goes straight into ``validate``, the fit loops and the generator.  Reads the parameters back to the host once."""
        from .sifnet import SIFNetQuery
        out = SIFNetQuery(self.params.to_decoders(), camera=self.net.camera, device=self.net.device)
        out.maps, out.encoder = self.net.maps, self.net.encoder
        out.loss_weights, out.vis_loss_name = list(self.net.loss_weights), self.net.vis_loss_name
        return out
