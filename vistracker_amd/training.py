"""A labelled training batch of SIF-Net assembled on the device, and the validation errors of a checkpoint on it.

``make_training_batch`` mirrors ``BehaveDatasetOnline.boundary_sampling`` and ``get_item`` (data/traindata_online.py:83-201) for B frames at once;
``validate`` is one batch of the reference's ``compute_val_loss`` (trainer/trainer.py:321-346: query, then ``get_errors``, no gradient) with no host labelling.

Out of scope here: file and ``KinectTransform`` IO (the meshes arrive in camera-local coordinates), image loading (``SequenceLoader(device_prep=True)``
builds the network inputs), ``smpl_vect`` (``load_neighbour_h``), data loaders over the sampled files, checkpoint directories.

``DecoderTrainer`` is the reference's ``Trainer.train_step`` (trainer/trainer.py:97-106) for the decoder parameter group: the five point decoders of a checkpoint
are fine-tuned on labelled batches with the encoder, and so the feature maps, frozen.

``SIFNetTrainer`` is the same ``train_step`` for the whole network (model/chore_triplane.py:60-164, model/chore_tri_vis.py): the image encoder and the shared
triplane encoder (``encoder.TrainableHGFilter``) and the five decoders (``ops.DecoderParams``) step together from one ``error.backward()``, with the reference's
``MultiStepLR`` as the host function ``multistep_lr``.  It adds no kernel: it is the host layer that joins the merged blocks.
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


def slice_batch(batch, sl):
    """the frames ``sl`` (a slice, or an index tensor / list) of a labelled batch: every entry of ``make_training_batch``'s dict carries the frame axis first"""
    return {k: v[sl] for k, v in batch.items()}


def distributed_indices(num_items, world, rank, epoch, seed=0, shuffle=True, drop_last=True):
    """this rank's item indices for an epoch: ``list(torch.utils.data.distributed.DistributedSampler(range(num_items), num_replicas=world, rank=rank,
    shuffle=shuffle, seed=seed, drop_last=drop_last))`` after ``set_epoch(epoch)``, index for index -- the permutation of ``torch.randperm`` under
    ``manual_seed(seed + epoch)``, cut to (``drop_last``, as data/base_data.py ``get_loader`` sets it) or padded by repetition to a multiple of ``world``, then
    every ``world``-th item from ``rank`` on.  A host function, as ``multistep_lr``."""
    num_items, world, rank = int(num_items), int(world), int(rank)
    if world < 1 or not 0 <= rank < world:
        raise L.VtError(f"distributed_indices: rank {rank} of {world}")
    if shuffle:
        g = torch.Generator()
        g.manual_seed(int(seed) + int(epoch))
        idx = torch.randperm(num_items, generator=g).tolist()
    else:
        idx = list(range(num_items))
    if drop_last and num_items % world != 0:
        per_rank = -(-(num_items - world) // world)
    else:
        per_rank = -(-num_items // world)
    total = per_rank * world
    if drop_last:
        idx = idx[:total]
    elif total > len(idx):
        pad = total - len(idx)
        idx = idx + (idx[:pad] if pad <= len(idx) else (idx * -(-pad // len(idx)))[:pad])
    return idx[rank:total:world]


def multistep_lr(lr0, milestones, gamma, epoch):
    """``torch.optim.lr_scheduler.MultiStepLR(milestones, gamma)`` as a function of the epoch counter: lr0 . gamma^(number of milestones <= epoch), multiplied up
    milestone by milestone as the scheduler does, so the value is the scheduler's to the last bit (a milestone listed k times counts k times)."""
    lr = float(lr0)
    for m in sorted(set(milestones)):
        if m <= epoch:
            lr *= float(gamma) ** list(milestones).count(m)
    return lr


IMAGE_PREFIX, TRIPLANE_PREFIX = "image_filter.", "triplane_encoder."


def network_state_dict(image, tri, params):
    """the whole network under the reference's checkpoint keys: ``image_filter.*`` and ``triplane_encoder.*`` from the two ``TrainableHGFilter``s, ``df.0.weight``
    ... from the ``ops.DecoderParams``; copies"""
    out = {IMAGE_PREFIX + k: v for k, v in image.state_dict().items()}
    out.update({TRIPLANE_PREFIX + k: v for k, v in tri.state_dict().items()})
    out.update(params.state_dict())
    return out


class SIFNetTrainer:
    """``Trainer.train_step`` (trainer/trainer.py:97-106) for the whole ``CHORETriplaneVisibility``: the image encoder (``.image``, Cin 5) and the shared triplane
    encoder (``.tri``, Cin 1, applied once to the 3B single-channel renders as ``SIFNetEncoder._chunk_eager`` batches them) are ``TrainableHGFilter``s, the five
    decoders an ``ops.DecoderParams`` (``.params``).  One ``EncoderAdam`` per encoder and one ``ops.FusedAdam`` over the decoders' flat buffer step at the same
    learning rate; they are built here, before any forward (``EncoderAdam`` re-homes every leaf's ``.data``).

        tr = SIFNetTrainer(torch.load(ckpt)["model_state_dict"], camera)
        for epoch in range(epochs):
            tr.set_step(epoch)                      # MultiStepLR(milestones, gamma); advancing the epoch is the caller's
            for batch, images, cc in loader:
                error, losses_all = tr.train_step(batch, images, cc)
        net = tr.export(images)                     # a SIFNetQuery with the trained decoders and a SIFNetEncoder of the trained encoders, maps of `images` set

    ``guard=True`` puts an ``ops.StepGuard`` (``.guard``) between the gradient mean and the optimiser steps: a step whose gradients or objective hold a NaN or Inf
    is skipped on the device, on every rank alike, and ``guard.read()`` (for epoch boundaries, as ``in_sync()``) tells which tensor blew up and what the norms
    were; ``clip_norm`` clips the global gradient norm as ``clip_grad_norm_`` does; ``record`` = K keeps the last K steps.  Without it every method does what
    it did before, launch for launch.

    ``sd`` carries the reference's keys (a leading ``module.`` is stripped).  Only the shared triplane encoder is served: per-view encoders
    (``triplane_encoder_0.`` ...) raise.  The query needs as many triplane stacks as image stacks (chore_triplane.py:146-147 indexes both with one counter)."""

    def __init__(self, sd, camera=None, num_stack=3, num_hourglass=2, triplane_stack=3, lr=1e-3, milestones=(), gamma=0.3, max_dist=5.0,
                 loss_weights=ops.LOSS_WEIGHTS, device="cuda:0", group=None, guard=False, clip_norm=None, record=0):
        from .encoder import EncoderAdam, TrainableHGFilter, state_dict_under
        from .sifnet import SIFNetQuery
        sd = state_dict_under(sd, "")
        if not guard and (clip_norm is not None or record):
            raise L.VtError("SIFNetTrainer: clip_norm and record belong to the step guard; pass guard=True with them")
        if any(k.startswith("triplane_encoder_") for k in sd):
            raise L.VtError("SIFNetTrainer: this checkpoint holds per-view triplane encoders (triplane_encoder_0. ...); only the shared form "
                            "(triplane_encoder.) is trained here")
        if int(num_stack) != int(triplane_stack):
            raise L.VtError(f"SIFNetTrainer: {num_stack} image stacks and {triplane_stack} triplane stacks; the training query pairs them one to one")
        self.device, self.max_dist = device, float(max_dist)
        self.num_stack, self.num_hourglass = int(num_stack), int(num_hourglass)
        self.lr0, self.milestones, self.gamma, self.epoch = float(lr), tuple(milestones), float(gamma), 0
        self.image = TrainableHGFilter.from_state_dict(sd, IMAGE_PREFIX, num_stack=num_stack, num_hourglass=num_hourglass, device=device)
        self.tri = TrainableHGFilter.from_state_dict(sd, TRIPLANE_PREFIX, num_stack=triplane_stack, num_hourglass=num_hourglass, device=device)
        self.net = SIFNetQuery(SIFNetQuery.decoders_from_state_dict(sd), camera=camera, device=device)          # serves query_train and get_errors
        self.net.loss_weights = list(loss_weights)
        self.camera = self.net.camera
        self.params = ops.DecoderParams.from_decoders(self.net.decoders, cam=self.camera.as_cam5(), device=device)
        self.image_optimizer, self.tri_optimizer = EncoderAdam(self.image, lr=lr), EncoderAdam(self.tri, lr=lr)
        self.optimizer = ops.FusedAdam([self.params.flat], lr=lr)
        self.set_step(0)
        # the three flat gradient buffers of the network (the decoders' is the one autograd makes anew every step: handed to the reducer per call)
        self.reducer = ops.RankMean([self.image_optimizer.grad, self.tri_optimizer.grad, self.params.flat.detach()], group)
        self.group = self.reducer.group
        self.guard = self._make_guard(clip_norm, record) if guard else None
        if self.group is not None and not self.in_sync():
            raise L.VtError(f"SIFNetTrainer: rank {self.reducer.rank} of {self.reducer.world} was built from weights that differ from another rank's; "
                            "data-parallel steps need the same parameters and moments on every rank")

    @property
    def lr(self):
        """the learning rate of the next step"""
        return self.image_optimizer.lr

    def set_step(self, k):
        """the epoch counter of the reference's ``MultiStepLR``: the three optimisers step at ``multistep_lr(lr0, milestones, gamma, k)`` from now on"""
        self.epoch = int(k)
        lr = multistep_lr(self.lr0, self.milestones, self.gamma, self.epoch)
        self.image_optimizer.lr = self.tri_optimizer.lr = lr
        self.optimizer.lrs = [lr] * len(self.optimizer.params)
        return lr

    def forward(self, images):
        """``CHORETriplane.filter`` in train mode on (B,8,H,W) inputs -> a list of S ``ops.FeatureMaps``, one per stack.  The NHWC tensors are permuted views of the
        encoders' channels-last outputs (no copy) and carry autograd; the three views of the triplane encoder are batch slices of one output; the stacks share
        ``tmpx`` / ``tri_tmpx{v}``, detached as the reference detaches them (HGFilters.py:203)."""
        assert images.dim() == 4 and images.shape[1] == 8, f"given image shape invalid: {tuple(images.shape)}"
        x = images.to(self.device).float()
        B = x.shape[0]
        feats, tmpx, _ = self.image(x[:, :5])
        tfeats, ttmpx, _ = self.tri(x[:, 5:8].transpose(0, 1).reshape(3 * B, 1, *x.shape[2:]))
        shared = {"tmpx": tmpx.permute(0, 2, 3, 1)}
        for v in range(3):
            shared[f"tri_tmpx{v}"] = ttmpx[v * B:(v + 1) * B].permute(0, 2, 3, 1)
        maps = []
        for s in range(self.num_stack):
            d = dict(shared)
            d["im_feat"] = feats[s].permute(0, 2, 3, 1)
            for v in range(3):
                d[f"tri_feat{v}"] = tfeats[s][v * B:(v + 1) * B].permute(0, 2, 3, 1)
            maps.append(ops.FeatureMaps(d))
        return maps

    def backward(self, batch, images, crop_center):
        """the gradient half of a step on a batch of ``make_training_batch`` and its (B,8,H,W) network input: zero_grad, both encoder forwards, the S per-stack
        ``FeatureMaps``, ``query_train`` over all stacks, ``get_errors``, one ``error.backward()`` (decoders, then both encoders, through the maps).
        -> (error (), losses_all (6,)): float64 device tensors of the objective; the gradients lie in ``flat_grads()``; nothing here waits on the host."""
        self.image_optimizer.zero_grad(); self.tri_optimizer.zero_grad(); self.optimizer.zero_grad()
        maps = self.forward(images)
        self.net.query_train(self.params, batch["points"], crop_center=crop_center, body_center=batch["body_center"], maps=maps)
        error, losses_all = self.net.get_errors(batch["df_h"], batch["df_o"], batch["labels"], batch["pca_axis"], self.max_dist, batch["body_center"],
                                                batch["obj_center"], visibility=batch["visibility"])
        error.backward()
        return error.detach(), losses_all

    def _make_guard(self, clip_norm, record):
        """the ``ops.StepGuard`` over the three flat gradient buffers: every stepped leaf of the two encoders at its ``EncoderAdam`` offset (the 64-float padding
        belongs to no segment), the decoders' 40 tensors at their ``vt_decoder_param_offset`` offsets, named by the reference's checkpoint keys in the order of
        ``state_dict()``"""
        segments, names = [], []
        for prefix, enc, opt in ((IMAGE_PREFIX, self.image, self.image_optimizer), (TRIPLANE_PREFIX, self.tri, self.tri_optimizer)):
            key = {id(p): k for k, p in reversed(enc.named_parameters())}
            segments.append([(o, p.numel()) for p, o in zip(opt.params, opt._offs)])
            names.append([prefix + key[id(p)] for p in opt.params])
        lib, segs, ns = L.lib(), [], []
        for h, head in enumerate(ops.HEADS):
            for l, i in enumerate(ops.STATE_DICT_LAYERS):
                for is_bias, kind in enumerate(("weight", "bias")):
                    segs.append((int(lib.vt_decoder_param_offset(h, l, is_bias)), self.params.views[(head, l, kind)].numel()))
                    ns.append(f"{ops.STATE_DICT_MODULES[head]}.{i}.{kind}")
        return ops.StepGuard([self.image_optimizer.grad, self.tri_optimizer.grad, self.params.flat.detach()], segments + [segs], names + [ns],
                             max_norm=clip_norm, record=record)

    def _guard_error(self, error):
        """the objective the guard looks at.  Every rank must take the same decision or the ranks part for good, and the objective is the one input of the
        decision that differs between them: with a group and the guard on, the ranks' values are gathered (8 bytes each) and added in rank order, which is also
        the sum a single rank forms over as many micro-batches.  Without a guard or a group: ``error`` as it is, no collective."""
        if self.guard is None or self.group is None:
            return error
        return self.reducer.gather(error.detach().reshape(1)).sum()

    def apply(self, error=None):
        """the three optimiser steps on whatever the gradient buffers hold.  With the guard on, ``guard.close`` first measures the three buffers, decides on the
        device whether the step is skipped (a NaN or Inf in a gradient, or in ``error``, the step's objective as a float64 device scalar) and clips them to
        ``clip_norm``; the three steps then take that decision as their stop flag.  A skipped step leaves every parameter and moment untouched; the optimisers'
        ``t`` advances all the same."""
        if self.guard is None:
            self.image_optimizer.step(); self.tri_optimizer.step(); self.optimizer.step()
            return
        skip = self.guard.close(self.flat_grads(), error)
        self.image_optimizer.step(skip=skip); self.tri_optimizer.step(skip=skip); self.optimizer.step(skip=skip)

    def flat_grads(self):
        """the three flat gradient buffers after a ``backward``: image encoder, triplane encoder, decoders.  An encoder leaf whose ``.grad`` autograd replaced is
        copied into its flat buffer first (``EncoderAdam.step`` does the same); a leaf without a gradient holds zeros there and is skipped by ``step`` as before."""
        self.image_optimizer._bind_grads(copy=True); self.tri_optimizer._bind_grads(copy=True)
        return [self.image_optimizer.grad, self.tri_optimizer.grad, self.params.flat.grad]

    def train_step(self, batch, images, crop_center):
        """one step on a batch of ``make_training_batch`` and its (B,8,H,W) network input: ``backward`` then ``apply``.  With a process group (``group=`` of the
        constructor) every rank calls it on ITS frames and the three flat gradient buffers become the mean over the ranks in between (``ops.RankMean.reduce``:
        gather, then a rank-ordered fp64 sum), as ``DistributedDataParallel`` leaves every leaf's ``.grad``, but with the same bits on every rank.
        -> (error (), losses_all (6,)): float64 device tensors of THIS rank's objective BEFORE the update; nothing here waits on the host (over RCCL; a gloo
        group, the single-GPU dry run of the tests, goes through host copies)."""
        error, losses_all = self.backward(batch, images, crop_center)
        if self.group is not None:
            self.reducer.reduce(self.flat_grads())
        self.apply(self._guard_error(error))
        return error, losses_all

    def train_step_micro(self, micro_batches):
        """one step whose gradient is the mean over micro-batches: a list of ``(batch, images, crop_center)`` with the same number of frames each (a B = 16 step
        taken as 2 x 8 when the activations of 16 frames do not fit).  Every micro-batch runs ``backward``; its three flat gradients are copied into row k of a
        workspace; ``vt_grad_rank_mean`` averages the rows in order into the flat gradients; with a group the result is then averaged over the ranks; one ``apply``.
        M micro-batches on one rank give the bits of M ranks with one of them each.  -> (errors (M,), losses_all (M, 6)); no host wait."""
        micro_batches = list(micro_batches)
        if not micro_batches:
            raise L.VtError("train_step_micro: no micro-batch")
        frames = [int(images.shape[0]) for _, images, _ in micro_batches]
        if len(set(frames)) != 1:
            raise L.VtError(f"train_step_micro: micro-batches of {frames} frames; the mean of their gradients is the gradient of the whole only for equal sizes")
        rows = self.reducer.rows(len(micro_batches))
        errors, losses = [], []
        for k, (batch, images, crop_center) in enumerate(micro_batches):
            error, losses_all = self.backward(batch, images, crop_center)
            for ws, g in zip(rows, self.flat_grads()):
                ws[k].copy_(g)
            errors.append(error); losses.append(losses_all)
        grads = self.reducer.reduce_local(rows, self.flat_grads())
        if self.group is not None:
            self.reducer.reduce(grads)
        self.apply(self._guard_error(torch.stack(errors).sum()) if self.guard is not None else None)          # the sum of the micro errors: for finiteness and the record only
        return torch.stack(errors), torch.stack(losses)

    def in_sync(self):
        """whether every rank of the group holds the same parameters and Adam moments: the three parameter buffers and the six moment buffers are each reduced to
        one integer on the device (the int32 view summed in int64), the nine numbers are gathered over the group and compared.  One small collective and ONE
        read-back: for epoch boundaries and tests, never inside ``train_step``.  Without a group: True."""
        if self.group is None:
            return True
        bufs = []
        for o in (self.image_optimizer, self.tri_optimizer):
            bufs += [o.flat, o.m, o.v]
        bufs += [self.params.flat.detach(), self.optimizer.m[0], self.optimizer.v[0]]
        with torch.cuda.device(self.reducer.device):
            sums = torch.stack([b.view(torch.int32).sum(dtype=torch.int64) for b in bufs])
            rows = self.reducer.gather(sums)
            return bool((rows == rows[0:1]).all().item())

    def state_dict(self):
        """the whole network under the reference's checkpoint keys (``image_filter.*``, ``triplane_encoder.*``, ``df.0.weight`` ...); device copies.  It loads
        back into a new ``SIFNetTrainer``."""
        return network_state_dict(self.image, self.tri, self.params)

    def export(self, images=None):
        """-> a new ``SIFNetQuery`` holding the trained decoders (packed by ``vt_sifnet_create`` as any checkpoint's) and, as ``.encoder``, a ``SIFNetEncoder`` built
        from the trained encoder weights, with this trainer's camera and loss settings.  ``images`` (B,8,H,W), when given, are encoded with the trained weights and set as its maps, so that it goes straight into
        ``validate``; without them the maps are None (the generator and the fit loops call ``filter`` themselves; the trainer keeps no input of a step alive).
        Host traffic: only the decoders are read back, once, as ``DecoderTrainer.export`` does.  The encoder weights are handed over as device tensors and the
        ``SIFNetEncoder`` packs its convolutions from them on the device at their first use: here when ``images`` are given, at the first ``filter`` otherwise."""
        from .encoder import SIFNetEncoder
        from .sifnet import SIFNetQuery
        out = SIFNetQuery(self.params.to_decoders(), camera=self.camera, device=self.device)
        enc_sd = {k: v for k, v in self.state_dict().items() if k.startswith((IMAGE_PREFIX, TRIPLANE_PREFIX))}
        out.encoder = SIFNetEncoder(enc_sd, num_stack=self.num_stack, num_hourglass=self.num_hourglass, triplane_stack=self.num_stack, shared_encoder=True,
                                    device=self.device)
        out.loss_weights, out.vis_loss_name = list(self.net.loss_weights), self.net.vis_loss_name
        if images is not None:
            out.filter(images)
        return out
