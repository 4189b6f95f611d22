"""Fused fit loops of the hot path: every Adam step is a fixed sequence of C-ABI launches on the current HIP stream --
no autograd tape, no host synchronisation inside the 10-step inner loop, early stop decided on the device.

Mirrors, with the reference's schedules / weights / stop rules:
  * ``ReconFitterBehave.optimize_smpl`` + ``forward_smpl``        (recon/recon_fit_behave.py:393-513)
  * ``ReconFitterTriVisFull.optimize_smpl_object`` + ``forward_step`` (recon/recon_fit_trivis_full.py:193-377)
  * ``BaseFitter.fit_one_batch`` + ``SMPLHFitter30fps.compute_loss``   (preprocess/fit_SMPLH_kpts.py:114-180,
    preprocess/fit_SMPLH_30fps.py:153-200)
Work the reference does but whose result is never used is skipped: the SMPL forward of the frozen body in
the object stage, the unused decoder heads, the object query in phase 'sil', the weight-0 'ocent' term, the constant hand
prior gradient.  Loss VALUES keep every term the reference sums (the early-stop rule depends on them).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os
import threading
import time
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib as L
from . import ops

# c * cst / (1 + decay) -- ReconFitterTriVisFull.get_loss_weights (recon_fit_trivis_full.py:124-153)
FIT_WEIGHTS = {"pose": 1e-5, "hand": 1e-5, "j2d": 0.09, "object": 900.0, "part": 0.0025, "contact": 900.0, "scale": 100.0,
               "df_h": 100.0, "mask": 0.0009, "ocent": 0.0, "pinit": 25.0, "rot": 100.0, "trans": 100.0,
               "stemp": 10000.0, "otemp": 225.0, "ovtemp": 2500.0, "collide": 9.0}
# SMPLHFitter30fps.get_loss_weights (fit_SMPLH_30fps.py:55-66); BaseFitter uses pinit 100 (fit_SMPLH_kpts.py:57-65)
SMPLT_WEIGHTS = {"pose": 1e-5, "hand": 1e-5, "kpts": 0.09, "temp": 900.0, "ptemp": 25.0, "pinit": 900.0}
# joint_weights of compute_Jaccel_loss (fit_SMPLH_30fps.py:26-51)
JOINT_WEIGHTS_66 = np.repeat(np.array([1, 10, 10, 10, 5, 5, 10, 1, 1, 10, 1, 1, 5, 5, 5, 5, 5, 5, 1, 1, 1, 1], np.float32), 3)
JOINT_WEIGHTS_66[37:39] = 10.0


def _lib():
    return L.lib()


def _chk(rc):
    L.check(rc)


def _ev_begin(prof):
    """HIP event before a kernel of interest (bench.py roofline); launches go to torch's current stream, so torch events see them."""
    if prof is None:
        return None
    e = torch.cuda.Event(enable_timing=True); e.record()
    return e


def _flush_events(prof, local, executed):
    """append a fit's per-launch events to the caller's lists; ``executed`` = the number of Adam steps that ran before the device-side stop: the launches
    of the steps queued behind it returned at their first instruction and are not query work.  Every event carries the index of the step that launched
    it (the object stage records no query event in its 'sil' steps, so a count of events says nothing about steps)."""
    if prof is None:
        return
    for k, v in local.items():
        # list.extend is atomic under the GIL (two fits in flight share ``prof``)
        prof[k].extend((a, b, n) for a, b, n, step in v if executed is None or step < executed)


def _ev_end(prof, key, e0, frames, step):
    if prof is None:
        return
    e1 = torch.cuda.Event(enable_timing=True); e1.record()
    prof[key].append((e0, e1, frames, step))      # frames of the launch (the tail batch of a sequence is smaller), Adam step of the fit that launched it


class Terms:
    """fp64 loss-term accumulators on the device, addressed by name."""

    def __init__(self, names, device):
        self.names = list(names)
        self.buf = torch.zeros(len(self.names), dtype=torch.float64, device=device)
        self.idx = {n: i for i, n in enumerate(self.names)}

    def ptr(self, name):
        return self.buf.data_ptr() + 8 * self.idx[name]

    def zero(self, first=0, count=None):
        count = len(self.names) - first if count is None else count
        _chk(_lib().vt_fill_f64(self.buf.data_ptr() + 8 * first, count, 0.0, L.stream_ptr()))

    def weights(self, table, decay, extra=None):
        w = np.zeros(16, np.float32)
        for n, i in self.idx.items():
            w[i] = table[n] / (1.0 + decay) * (1.0 if extra is None else extra.get(n, 1.0))
        return w


class AdamState:
    """torch.optim.Adam over column slices of parameter tensors: one launch per slice (``step``), or the groups handed to the tail of a fused step
    (``tick`` + ``smpl_tail_groups`` / ``object_tail_groups``)."""

    def __init__(self, slices, stop_flag):
        # slices: list of (tensor (B, C) contiguous, ncols, grad tensor (B, Cg) contiguous, lr)
        self.slices = slices
        self.m = [torch.zeros(p.shape[0], n, device=p.device) for p, n, g, lr in slices]
        self.v = [torch.zeros(p.shape[0], n, device=p.device) for p, n, g, lr in slices]
        self.t = 0
        self.stop_flag = stop_flag

    def tick(self):
        """the step counter of the next Adam step"""
        self.t += 1
        return self.t

    def step(self):
        t = self.tick()
        for (p, n, g, lr), m, v in zip(self.slices, self.m, self.v):
            _chk(_lib().vt_adam_step_2d(p.data_ptr(), p.shape[1], g.data_ptr(), g.shape[1], m.data_ptr(), v.data_ptr(), p.shape[0], n,
                                        t, lr, 0.9, 0.999, 1e-8, self.stop_flag.data_ptr(), L.stream_ptr()))

    # the pointers of the groups never change: the fused tails' argument lists are packed once per AdamState
    @functools.cached_property
    def smpl_tail_groups(self):
        """vt_smplstep_tail's three groups (param, stride, grad, stride, m, v, ncols, lr); unused ones NULL"""
        out = ()
        for (p, n, g, lr), m, v in zip(self.slices, self.m, self.v):
            out += (p.data_ptr(), p.shape[1], g.data_ptr(), g.shape[1], m.data_ptr(), v.data_ptr(), n, lr)
        return out + (None, 0, None, 0, None, None, 0, 0.0) * (3 - len(self.slices))

    @functools.cached_property
    def object_tail_groups(self):
        """vt_objstep_tail's (param, m, v, lr) of the rotation group (9 columns), then of the translation group; a group not optimised is NULL"""
        rot = trans = (None, None, None, 0.0)
        for (p, n, g, lr), m, v in zip(self.slices, self.m, self.v):
            if n == 9:
                rot = (p.data_ptr(), m.data_ptr(), v.data_ptr(), lr)
            else:
                trans = (p.data_ptr(), m.data_ptr(), v.data_ptr(), lr)
        return rot + trans


def _check_finite(res, what):
    """A non-finite loss among the executed steps means a non-finite intermediate somewhere in the step -- e.g. a decoder activation
    beyond the range of the split-f16 operands (|x| >= 1023) or NaN inputs.  The reference would carry the NaN
    silently into the saved parameters; here the fit fails loudly."""
    executed = res.losses[:res.steps]      # after an early stop res.steps already counts the finite prefix only (unwritten slots are NaN)
    if executed.size and not np.isfinite(executed).all():
        bad = int(np.flatnonzero(~np.isfinite(executed))[0])
        raise FloatingPointError(f"{what}: non-finite loss at Adam step {bad} (non-finite input or decoder activation out of range)")


def _as_input(t, dev):
    """constant input of a fit loop -> contiguous float32 tensor on ``dev`` (no copy when it already is one)"""
    if t is None:
        return None
    return torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous()


def _require_params(*ts):
    """the optimised tensors are updated in place through raw pointers: they must already be contiguous float32 CUDA tensors"""
    for t in ts:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise L.VtError("fit loops update their parameters in place: pass contiguous float32 CUDA tensors "
                            f"(got {type(t).__name__} {getattr(t, 'dtype', None)} on {getattr(t, 'device', None)})")
        if t.device != ts[0].device:
            raise L.VtError("fit loops: all parameters must live on the same device")


@dataclass
class FitResult:
    steps: int = 0
    outer_iters: int = 0
    stopped_early: bool = False
    losses: np.ndarray = field(default_factory=lambda: np.zeros(0, np.float32))


def morton_order(points) -> np.ndarray:
    """indices that sort (N,3) points along a 30-bit Morton (Z-order) curve of their bounding box"""
    p = np.asarray(points, np.float64)
    q = ((p - p.min(0)) / (p.max(0) - p.min(0) + 1e-12) * 1023).astype(np.int64)

    def part(x):
        x = (x | (x << 16)) & 0x030000FF; x = (x | (x << 8)) & 0x0300F00F; x = (x | (x << 4)) & 0x030C30C3
        return (x | (x << 2)) & 0x09249249
    return np.argsort(part(q[:, 0]) | (part(q[:, 1]) << 1) | (part(q[:, 2]) << 2), kind="stable")


def morton_order_device(p: torch.Tensor) -> torch.Tensor:
    """``morton_order`` for (N,2) or (N,3) points that live on the device: int32 indices, no host synchronisation"""
    p = p.double()
    lo = p.min(0).values; hi = p.max(0).values
    q = ((p - lo) / (hi - lo + 1e-12) * 1023).long()

    def part(x):
        x = (x | (x << 16)) & 0x030000FF; x = (x | (x << 8)) & 0x0300F00F; x = (x | (x << 4)) & 0x030C30C3
        return (x | (x << 2)) & 0x09249249
    key = part(q[:, 0]) | (part(q[:, 1]) << 1)
    if p.shape[1] > 2:
        key = key | (part(q[:, 2]) << 2)
    return torch.argsort(key, stable=True).to(torch.int32)


class _StopWatch:
    """The device-side stop flag of one fit as the launching thread sees it, once per outer iteration.  With the look-ahead (``lookahead``: the fit has the
    device-side skip, see FitContext._skip_after_stop) ``check()`` queues an asynchronous copy of the flag to pinned memory and an event behind the iteration
    just queued and waits for the PREVIOUS iteration's event: one iteration of launches always stands between the host and the GPU, so the stream never runs
    dry while the launching thread wakes up, takes the GIL and queues the next launches; the iteration queued behind a stop costs ~100 launches that return
    at once.  ``final()`` after the loop answers for whatever has not been looked at.  Without it (a nested fit) ``check()`` is a stream synchronisation."""
    _tls = threading.local()

    def __init__(self, ctx, stop, lookahead):
        self.ctx, self.stop, self.look = ctx, stop, lookahead
        self.pending = None; self.n = 0
        if lookahead:
            pool = getattr(self._tls, "pool", None)        # pinned words + events are per launching thread, reused by its (sequential) fits
            if pool is None or pool[0] != stop.device:
                pool = (stop.device, torch.zeros(2, dtype=torch.int32).pin_memory(), [torch.cuda.Event(), torch.cuda.Event()])
                self._tls.pool = pool
            _, self.host, self.ev = pool

    def _wait(self, k):
        t0 = time.perf_counter()
        self.ev[k].synchronize()
        with self.ctx._counter_lock:
            self.ctx.host_wait_s += time.perf_counter() - t0
        return bool(int(self.host[k]))

    def check(self):
        if not self.look:
            return bool(self.ctx._read_stop(self.stop))
        k = self.n & 1; self.n += 1
        self.host[k:k + 1].copy_(self.stop, non_blocking=True); self.ev[k].record()
        prev, self.pending = self.pending, k
        return prev is not None and self._wait(prev)

    def final(self):
        if not self.look or self.pending is None:
            return False
        k, self.pending = self.pending, None
        return self._wait(k)


class _Fit:
    """Per-fit state: one object per call, never stored on the FitContext (one context serves several launching threads at once).  This base holds the
    loop's device state -- stop flag, (prev_loss, loss) pair of the stop rule, step ticket of the fused tails, loss history --, the loss terms, the
    current Adam groups and the fit's per-launch events (flushed to the caller's ``prof`` by FitContext._run_fit)."""

    def __init__(self, dev, names, nsteps, prev_loss, prof):
        self.terms = Terms(names, dev)
        self.stop = torch.zeros(1, dtype=torch.int32, device=dev)
        self.loss_state = torch.full((2,), prev_loss, device=dev)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.hist = torch.full((nsteps,), float("nan"), device=dev)
        self.lp = {"human": [], "object": []} if prof is not None else None
        self.adam = None


class _SmplFit(_Fit):
    """Per-fit state of the SMPL-T pre-fit and the SMPL stage: pose / betas / trans (updated in place), pose_init and the SMPL-H forward / backward
    buffers.  The fit adds its inputs: ``kpts``, ``temporal`` (SMPL-T); ``maps``, ``net_size``, ``crop_center``, ``body_center``, ``body_kpts``,
    ``vert_order`` (SMPL stage)."""

    def __init__(self, pose, betas, trans, names, nsteps, prev_loss, prof=None, smpl=None):
        dev = pose.device; B = self.B = pose.shape[0]
        super().__init__(dev, names, nsteps, prev_loss, prof)
        self.pose, self.betas, self.trans = pose, betas, trans
        self.verts = torch.empty(B, 6890, 3, device=dev); self.jtr = torch.empty(B, 52, 3, device=dev); self.vposed = torch.empty_like(self.verts)
        self.ws = torch.empty(_lib().vt_smplh_workspace_floats(B), device=dev); self.scratch = torch.empty(_lib().vt_smplh_bwd_scratch_floats(B), device=dev)
        self.dverts = torch.empty_like(self.verts); self.J = torch.empty(B, 25, 3, device=dev); self.dJ = torch.empty_like(self.J)
        self.dpose = torch.empty(B, 156, device=dev); self.dbetas = torch.empty(B, 10, device=dev); self.dtrans = torch.empty(B, 3, device=dev)
        self.vb = torch.empty(B, device=dev)
        self.pose_init = pose.clone()
        # The hand joints' share of the SMPL-H forward, computed once (``smpl``: the SmplhHandle; None = every step runs the full layer).  INVARIANT: nothing
        # inside a fit writes pose[:, 66:] -- no Adam group of fit_smplt / optimize_smpl reaches past column 66 (``n_free``), neither does the reference --,
        # so ``prefix`` and the hand rotations in ``ws`` stay valid until the fit returns; they are never kept beyond it.  The restricted backward leaves
        # dpose[:, 66:] alone: zeroed here once (the fused tail adds the pinit gradient, exactly 0 there, to columns 66..71).
        self.prefix, self.n_free = None, 156
        if smpl is not None:
            self.prefix = torch.empty(_lib().vt_smplh_prefix_floats(B), device=dev); self.n_free = 66
            _chk(_lib().vt_smplh_prefix(smpl.h, pose.data_ptr(), B, self.ws.data_ptr(), self.prefix.data_ptr(), L.stream_ptr()))
            self.dpose.zero_()

    @property
    def vert_order_ptr(self):
        return self.vert_order.data_ptr() if self.vert_order is not None else None


class _ObjectFit(_Fit):
    """Per-fit state of the object stage: obj_R / obj_t (updated in place), the step buffers, the (B, 22) workspace in which the head of a fused step
    leaves its SVD of M0 + noise for the tail of the same step, the silhouette buffers (with a SilSetup; ``img`` / ``per`` for the single-purpose step
    only), the collision buffers (allocated by the first step that needs them) and the contact set (computed by the first 'joint' step).  The fit adds
    its inputs: ``maps``, ``smpl_verts``, ``obj_s``, ``crop_center``, ``body_center``, ``occ``, ``noise``."""

    def __init__(self, ctx, obj_R, obj_t, sil, nsteps, prof):
        dev = obj_R.device; B = self.B = obj_R.shape[0]; N = self.N = ctx.obj_points.shape[0]; NV = self.NV = ctx.obj_verts.shape[0]
        super().__init__(dev, ["object", "otemp", "ovtemp", "mask", "trans", "contact", "collide", "scale"], nsteps, 300.0, prof)   # prev_loss = 300
        self.obj_R, self.obj_t, self.sil = obj_R, obj_t, sil
        self.R = torch.empty(B, 3, 3, device=dev); self.X = torch.empty(B, N, 3, device=dev); self.dX = torch.empty_like(self.X)
        self.svd_ws = torch.empty(B, 22, device=dev)
        self.dR = torch.empty(B, 3, 3, device=dev); self.dM = torch.empty(B, 3, 3, device=dev); self.dt = torch.empty(B, 3, device=dev)
        if sil is not None:
            self.Vt = torch.empty(B, NV, 3, device=dev); self.dVt = torch.empty_like(self.Vt)
            self.fidx = torch.empty(B, sil.size, sil.size, dtype=torch.int32, device=dev); self.dimg = torch.empty(B, sil.size, sil.size, device=dev)
            self.sws = torch.empty(_lib().vt_sil_workspace_floats(B, NV, ctx.obj_faces.shape[0], sil.size), device=dev)
            if not ctx.fused_steps:
                self.img = torch.empty_like(self.dimg); self.per = torch.empty(B, device=dev)
        self.trans_init = None          # phase 'sil'
        self.Vc = self.cws = None       # collision term
        self.contact = None             # 'Computing contacts once'


class FitContext:
    """Device-resident constants shared by all batches of a sequence: SMPL-H model, body25 regressor, priors,
    SIF-Net decoders, part labels, object template / surface samples."""
    # hoist the im_feat part of the decoders' first layer out of the Adam loops (ops.FeatureMaps.build_projection)
    use_projection = True
    sort_object_points = True
    sort_query_points = True
    # human / object interpenetration term of phase 'joint' (recon_fit_base.py:736-765).  The reference computes it only on two machines of its
    # authors' cluster (hostname test, recon_fit_base.py:106); off here too unless switched on.
    collision_loss = False
    # heads / tails of an Adam step as fused launches (vt_objstep_head / vt_temporal_loss2 / vt_objstep_tail / vt_smplstep_tail: 4 launches around the
    # query per object-stage step instead of ~11, one tail instead of 8 in the SMPL stage); False = the single-purpose launches (same arithmetic in
    # the same order: the trajectories are bit-identical, tests/test_gpu_fit.py)
    fused_steps = os.environ.get("VT_FUSED_STEPS", "1") != "0"
    # SMPL stage: keypoint chain as one launch + the query adding its gradient and the vertex acceleration stencil in its epilogue (vt_kpts_step /
    # vt_query_human_step: 8 launches per step instead of 11, bit-identical).  MEASURED SLOWER and therefore off: the twelve neighbour-frame loads per
    # point in the tail of the dominant kernel cost it 1 % (1.684 -> 1.700 ms), more than the three small launches it replaces were worth behind
    # the query (one stream 767.9 -> 777.8 ms per batch, two streams 690 -> 696; same box, two repetitions)
    fused_smpl_query = os.environ.get("VT_FUSED_SMPL_QUERY", "0") != "0"
    # the query / SMPL-H launches queued behind the step that stopped a fit return at their first instruction (vt_stream_set_skip_flag); it also lets the
    # host look at the stop flag one outer iteration late (_StopWatch) -- the bubble a slow or contended host (8 ranks x 2 launching threads on one node)
    # would otherwise pay once per outer iteration
    device_skip = os.environ.get("VT_DEVICE_SKIP", "1") != "0"
    # SMPL-T pre-fit and SMPL stage: the frozen hand joints' part of SMPL-H once per fit instead of once per step (_SmplFit.prefix: vt_smplh_prefix /
    # vt_smplh_forward_prefixed / vt_smplh_backward_free); False = the full layer at every step.  Bit-identical trajectories (tests/test_gpu_smplh_frozen.py)
    frozen_hands = True

    def __init__(self, smpl_model, regressors, priors, decoders=None, part_labels=None, obj_verts=None, obj_faces=None, obj_points=None,
                 cam=ops.DEFAULT_CAM, device="cuda:0"):
        self.device = torch.device(device)
        dev = self.device
        self.smpl = ops.SmplhHandle(smpl_model, dev)
        self.b25 = ops.LandmarkHandle(regressors["body25"], dev)
        # the SMPL-T pre-fit (fit_smplt) needs neither the SIF-Net nor an object: decoders / part_labels / obj_* may be None there
        self.net = ops.SifNetHandle(decoders, cam, dev) if decoders is not None else None
        self.cam = np.ascontiguousarray(cam, np.float32)
        t = lambda a, dt=torch.float32: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
        self.pri = {k: t(v) for k, v in priors.items()}
        self.labels = t(part_labels, torch.int32)
        # processing order of the SMPL vertices in the fused SMPL-stage query: Morton order of the template (results are written back at the
        # original vertex index; the order only decides which 64 vertices share a workgroup, i.e. how local its gathers are)
        self.vert_order = t(morton_order(np.asarray(smpl_model["v_template"])), torch.int32) if self.sort_query_points else None
        if obj_points is not None and self.sort_object_points:
            # the surface samples are an unordered set (trimesh.sample order, recon_fit_base.py:144) and every term that uses them is a sum
            # over points: put them in Morton order so that the 64 consecutive points of a query workgroup project to neighbouring texels
            # (L2 hits instead of HBM round trips in the gather: -6 % on the object-stage query kernel)
            obj_points = np.asarray(obj_points, np.float32)[morton_order(obj_points)]
        self.obj_verts = t(obj_verts); self.obj_faces = t(obj_faces, torch.int32); self.obj_points = t(obj_points)
        self.smpl_faces = t(np.asarray(smpl_model["f"]).astype(np.int32), torch.int32) if "f" in smpl_model else None
        self.jw66 = t(JOINT_WEIGHTS_66)

    # ---- shared pieces ----------------------------------------------------------------------------------
    range_retries = 0       # fits of this context repeated at a wider operand-range level of the split-f16 decoders
    fp32_fallbacks = 0      # fits of this context that had to be repeated on the strict-fp32 kernels
    _counter_lock = threading.Lock()
    host_wait_s = 0.0       # seconds the launching threads spent blocked on the stop flag (see _read_stop)

    def _with_range_fallback(self, maps, params, run):
        """Run a fit; if the split-f16 decoders produced a non-finite loss (an activation beyond the range of the split operands at the maps'
        level -- |x| >= 1023 at level 0; possible with a real checkpoint, the reference's fp32 Conv1d has no such limit) restore
        the parameters and repeat the fit at the next operand-range level (same kernels, operand scale / 16: one repeated fit, not a slower
        route), and only after the last level on the strict-fp32 kernels (query_f32.hip).  Level and route are properties of THIS batch's
        maps (vt_maps::act_level / force_fp32): nothing another fit running concurrently through the same network handle can observe.  The
        maps keep the level that worked (the same batch would overflow again); a loss that is non-finite on the fp32 route too still raises."""
        if self.net is None or maps is None or maps.force_fp32 or self.net.precision == "fp32":
            return run()
        saved = [p.clone() for p in params]
        while True:
            try:
                return run()
            except FloatingPointError as e:
                import warnings
                for p, s0 in zip(params, saved):
                    p.copy_(s0)
                if maps.act_level + 1 < maps.ACT_LEVELS:
                    maps.set_act_level(maps.act_level + 1)
                    warnings.warn(f"{e}; repeating the fit at operand-range level {maps.act_level} of the split-f16 decoders", RuntimeWarning)
                    with self._counter_lock:
                        self.range_retries += 1
                    continue
                if maps.force_fp32:
                    raise
                warnings.warn(f"{e}; repeating the fit on the strict-fp32 decoder kernels (5x slower)", RuntimeWarning)
                maps.set_force_fp32(True)
                with self._counter_lock:
                    self.fp32_fallbacks += 1
                return run()

    def smpl_forward(self, pose, betas, trans, verts, jtr, vposed, ws, prefix=None):
        """``prefix``: a fit's _SmplFit.prefix (built with the same ``ws``) or None for the full layer"""
        if prefix is not None:
            _chk(_lib().vt_smplh_forward_prefixed(self.smpl.h, pose.data_ptr(), betas.data_ptr(), trans.data_ptr(), pose.shape[0], prefix.data_ptr(),
                                                  verts.data_ptr(), jtr.data_ptr(), vposed.data_ptr(), ws.data_ptr(), L.stream_ptr()))
            return
        _chk(_lib().vt_smplh_forward(self.smpl.h, pose.data_ptr(), betas.data_ptr(), trans.data_ptr(), pose.shape[0], verts.data_ptr(),
                                     jtr.data_ptr(), vposed.data_ptr(), ws.data_ptr(), L.stream_ptr()))

    def smpl_backward(self, pose, betas, dverts, vposed, ws, scratch, dpose, dbetas, dtrans, n_free=156):
        """``n_free`` < 156: the gradient of the first n_free pose columns only (dpose[:, n_free:] is left as it is)"""
        if n_free < 156:
            _chk(_lib().vt_smplh_backward_free(self.smpl.h, pose.data_ptr(), pose.shape[0], dverts.data_ptr(), None, vposed.data_ptr(), ws.data_ptr(),
                                               scratch.data_ptr(), n_free, dpose.data_ptr(), dbetas.data_ptr(), dtrans.data_ptr(), L.stream_ptr()))
            return
        _chk(_lib().vt_smplh_backward(self.smpl.h, pose.data_ptr(), betas.data_ptr(), pose.shape[0], dverts.data_ptr(), None, vposed.data_ptr(),
                                      ws.data_ptr(), scratch.data_ptr(), dpose.data_ptr(), dbetas.data_ptr(), dtrans.data_ptr(), L.stream_ptr()))

    def hand_prior_value(self, pose, terms, name, scratch_b):
        """HandPrior value (constant: hand pose is never optimised).  Quirk kept: sum over frames and hands / 45
        (th_hand_prior.py:57-72 broadcasts to (1,2B,45) and torch.mean divides by 45)."""
        B = pose.shape[0]
        for off, m, p in ((66, "lhand_mean", "lhand_prec"), (111, "rhand_mean", "rhand_prec")):
            _chk(_lib().vt_mahalanobis(pose.data_ptr(), B, 156, off, 45, self.pri[m].data_ptr(), self.pri[p].data_ptr(), scratch_b.data_ptr(), None, 0.0, L.stream_ptr()))
            _chk(_lib().vt_sum_to_term(scratch_b.data_ptr(), B, 1.0 / 45.0, terms.ptr(name), L.stream_ptr()))

    def body_prior(self, pose, dpose, w, terms, name, scratch_b):
        B = pose.shape[0]
        _chk(_lib().vt_mahalanobis(pose.data_ptr(), B, 156, 3, 63, self.pri["body_mean"].data_ptr(), self.pri["body_prec"].data_ptr(),
                                   scratch_b.data_ptr(), dpose.data_ptr(), w / B, L.stream_ptr()))
        _chk(_lib().vt_sum_to_term(scratch_b.data_ptr(), B, 1.0 / B, terms.ptr(name), L.stream_ptr()))

    # ---- the fit loop shared by the three fits ------------------------------------------------------------
    def _run_fit(self, f, start, end, check_every, outer, prof=None):
        """Outer iterations ``start`` .. ``end`` of 10 Adam steps each: ``outer(it)`` sets up iteration ``it`` (phase, Adam groups, decayed weights) and
        returns (step, phase, w, armed); ``step(f, phase, k, w, armed)`` queues the launches of step k of the fit (its slot in the loss history; also
        the step index of its per-launch events).  The host looks at the device-side stop flag every ``check_every`` outer iterations; after an early
        stop the steps are recounted from the loss history (the steps queued behind the stop step wrote nothing)."""
        res = FitResult()
        with self._skip_after_stop(f.stop) as skipping:
            watch = _StopWatch(self, f.stop, skipping)
            for it in range(start, end):
                step, phase, w, armed = outer(it)
                for i in range(10):
                    step(f, phase, (it - start) * 10 + i, w, armed)
                res.steps += 10
                res.outer_iters += 1
                if (it - start) % check_every == check_every - 1 and watch.check():
                    res.stopped_early = True
                    break
            res.stopped_early = res.stopped_early or watch.final()
        res.losses = f.hist.cpu().numpy()
        if res.stopped_early:
            res.steps = int(np.isfinite(res.losses).sum())
            res.outer_iters = -(-res.steps // 10)          # (with the look-ahead one more iteration was queued; its launches returned at once)
        _flush_events(prof, f.lp, res.steps if (res.stopped_early and self.device_skip) else None)
        _check_finite(res, "fit")
        return res

    # ---- SMPL-T pre-fit (fit_SMPLH_kpts.py:114-180) ------------------------------------------------------
    def fit_smplt(self, pose, betas, trans, kpts, max_iter=100, iter_for_global=8, temporal=True, pinit_w=900.0,
                  lr_global=0.01, lr_all=0.001, it_range=None, check_every=1, weights=None, early_stop=True):
        """In-place Adam fit of pose (B,156), betas (B,10), trans (B,3) to 2D keypoints kpts (B,25,3).
        ``it_range`` = (start, end) restricts the outer iterations (used by the trajectory parity tests).
        ``weights``: the constants c of the fitter's ``get_loss_weights()`` table (w = c / (1 + decay)) for any of the terms
        kpts / temp / ptemp / pose / pinit / hand; missing terms keep the 30fps defaults (``pinit_w`` for 'pinit')."""
        with torch.cuda.device(pose.device):
            return self._fit_smplt(pose, betas, trans, kpts, max_iter, iter_for_global, temporal, pinit_w, lr_global, lr_all, it_range, check_every, weights, early_stop)

    def _fit_smplt(self, pose, betas, trans, kpts, max_iter, iter_for_global, temporal, pinit_w, lr_global, lr_all, it_range, check_every, weights, early_stop=True):
        _require_params(pose, betas, trans)
        table = dict(SMPLT_WEIGHTS); table["pinit"] = pinit_w
        if weights is not None:
            table.update({k: float(v) for k, v in weights.items() if k in table})
        start, end = it_range if it_range is not None else (0, max_iter)
        f = _SmplFit(pose, betas, trans, ["kpts", "temp", "ptemp", "pose", "pinit", "hand"], (end - start) * 10, 0.0,   # prev_loss = 0 (fit_SMPLH_kpts.py:136)
                     smpl=self.smpl if self.frozen_hands else None)
        f.kpts = _as_input(kpts, pose.device)
        f.temporal = temporal and f.B >= 3
        self.hand_prior_value(pose, f.terms, "hand", f.vb)

        def outer(it):
            if f.adam is None or it == iter_for_global:
                if it < iter_for_global:      # init_globalpose_optimizer: trans, global_pose, top_betas
                    f.adam = AdamState([(trans, 3, f.dtrans, lr_global), (pose, 3, f.dpose, lr_global), (betas, 2, f.dbetas, lr_global)], f.stop)
                else:                         # init_allpose_optimizer: trans, global, body, top_betas, other_betas
                    f.adam = AdamState([(trans, 3, f.dtrans, lr_all), (pose, 66, f.dpose, lr_all), (betas, 10, f.dbetas, lr_all)], f.stop)
            return self._smplt_step, None, f.terms.weights(table, it // 3), int(early_stop and it > 0.3 * max_iter)
        return self._run_fit(f, start, end, check_every, outer)

    # ---- fit, SMPL stage (recon_fit_behave.py:393-513) ----------------------------------------------------
    def optimize_smpl(self, maps, pose, betas, trans, crop_center, body_center, body_kpts, max_iter=100, iter_for_betas=1,
                      iter_for_pose=1, iter_for_kpts=1, it_range=None, net_size=512.0, check_every=1, prof=None, early_stop=True):
        """pose (B,156), betas (B,10), trans (B,3): float32 CUDA tensors updated in place.  The constant inputs (crop_center, body_center,
        body_kpts) are converted to contiguous float32 on the parameters' device if they are not already (a reference-style driver hands
        over float64 from the dataloader's default collate)."""
        with torch.cuda.device(pose.device):
            return self._with_range_fallback(maps, (pose, betas, trans), lambda: self._optimize_smpl(
                maps, pose, betas, trans, crop_center, body_center, body_kpts, max_iter, iter_for_betas, iter_for_pose, iter_for_kpts, it_range, net_size,
                check_every, prof, early_stop))

    def _optimize_smpl(self, maps, pose, betas, trans, crop_center, body_center, body_kpts, max_iter, iter_for_betas, iter_for_pose, iter_for_kpts,
                       it_range, net_size, check_every, prof, early_stop=True):
        dev = pose.device
        _require_params(pose, betas, trans)
        split_route = self.net.precision != "fp32" and not maps.force_fp32          # the step forms of the query exist on the split-f16 route only
        if self.use_projection and split_route:
            maps.build_projection(self.net)     # rebuilt at every call: 2.5 ms per 96-frame batch, never stale (and at the maps' range level)
        total = iter_for_betas + iter_for_kpts + iter_for_pose + max_iter
        start, end = it_range if it_range is not None else (0, total)
        f = _SmplFit(pose, betas, trans, ["df_h", "part", "pose", "pinit", "j2d", "stemp", "hand"], (end - start) * 10, 300.0, prof,  # prev_loss = 300 (recon_fit_behave.py:408)
                     smpl=self.smpl if self.frozen_hands else None)
        f.maps, f.net_size = maps, net_size
        f.crop_center, f.body_center, f.body_kpts = _as_input(crop_center, dev), _as_input(body_center, dev), _as_input(body_kpts, dev)
        f.vert_order = self.vert_order
        if self.sort_query_points:
            # processing order for this batch: Morton order of the IMAGE positions of the initial vertices of the middle frame (the body moves
            # little inside a batch and during the fit); a little better than the template's 3-D order because the perspective maps -- the
            # projection rows and tmpx, two thirds of the gathered bytes -- see exactly this neighbourhood structure.  Results do not depend on it.
            # Computed on the device (bit interleave + one argsort of 6890 keys): no host round trip inside the batch.
            self.smpl_forward(pose, betas, trans, f.verts, f.jtr, f.vposed, f.ws, f.prefix)
            v0 = f.verts[f.B // 2]
            f.vert_order = morton_order_device(torch.stack([v0[:, 0] / v0[:, 2], v0[:, 1] / v0[:, 2]], 1))
        self.hand_prior_value(pose, f.terms, "hand", f.vb)
        if not self.fused_steps:
            step = self._smpl_step
        elif split_route and self.fused_smpl_query:
            step = self._smpl_step_fused_query
        else:
            step = self._smpl_step_fused
        arm_after = 0.25 * max_iter + iter_for_betas + iter_for_pose

        def outer(it):
            if it < iter_for_betas:
                phase = "global"
                if f.adam is None:
                    f.adam = AdamState([(betas, 2, f.dbetas, 0.02), (trans, 3, f.dtrans, 0.02)], f.stop)
            else:
                phase = "kpts" if it >= iter_for_betas + iter_for_pose else "smpl all pose"
                if f.adam is None or it == iter_for_betas:
                    f.adam = AdamState([(trans, 3, f.dtrans, 0.006), (pose, 66, f.dpose, 0.006), (betas, 10, f.dbetas, 0.006)], f.stop)
            return step, phase, f.terms.weights(FIT_WEIGHTS, 1 if phase != "kpts" else it / 3), int(early_stop and it > arm_after)
        return self._run_fit(f, start, end, check_every, outer, prof)

    # ---- fit, object stage (recon_fit_trivis_full.py:283-377) ----------------------------------------------
    def optimize_smpl_object(self, maps, smpl_verts, obj_R, obj_t, obj_s, crop_center, body_center, occ, sil=None, noise=None,
                             iter_for_obj=15, iter_for_sil=30, joint_iter=10, max_iter=100, it_range=None, seed=0, check_every=1, prof=None, early_stop=True):
        """obj_R (B,3,3), obj_t (B,3): float32 CUDA tensors updated in place.  ``smpl_verts`` (B,6890,3): the frozen body (contacts).
        ``sil``: SilSetup (phase 'sil'); ``noise``: (steps,B,3,3) U[0,1) samples of decopose_axis or None (drawn from ``seed``).
        Constant inputs are converted to contiguous float32 on the parameters' device if needed."""
        with torch.cuda.device(obj_R.device):
            return self._with_range_fallback(maps, (obj_R, obj_t), lambda: self._optimize_smpl_object(
                maps, smpl_verts, obj_R, obj_t, obj_s, crop_center, body_center, occ, sil, noise, iter_for_obj, iter_for_sil, joint_iter, max_iter, it_range,
                seed, check_every, prof, early_stop))

    def _optimize_smpl_object(self, maps, smpl_verts, obj_R, obj_t, obj_s, crop_center, body_center, occ, sil, noise, iter_for_obj, iter_for_sil,
                              joint_iter, max_iter, it_range, seed, check_every, prof, early_stop=True):
        dev = obj_R.device; B = obj_R.shape[0]
        _require_params(obj_R, obj_t)
        if self.use_projection and self.net.precision != "fp32" and not maps.force_fp32:
            maps.build_projection(self.net, reuse=True)     # the SMPL stage of the batch left it on these maps (same net, level, storage): kept, else built
        total = joint_iter + iter_for_obj + max_iter + iter_for_sil
        start, end = it_range if it_range is not None else (0, total)
        f = _ObjectFit(self, obj_R, obj_t, sil, (end - start) * 10, prof)
        f.maps = maps
        f.smpl_verts, f.obj_s, f.crop_center, f.body_center, f.occ = (_as_input(x, dev) for x in (smpl_verts, obj_s, crop_center, body_center, occ))
        f.obj_s = f.obj_s.reshape(-1)
        if noise is not None:
            f.noise = _as_input(noise, dev)
        else:
            gen = torch.Generator(device=dev); gen.manual_seed(seed)
            f.noise = torch.rand((end - start) * 10, B, 3, 3, device=dev, generator=gen)
        # 'scale' = mean((obj_s - 1)^2) (recon_fit_trivis_full.py:161,227): obj_s is never optimised, so the term is a constant of the call
        # -- zero for the obj_s == 1 that fit_recon passes -- but it is part of the summed loss the stop rule looks at
        ones = torch.ones_like(f.obj_s)
        _chk(_lib().vt_sqdiff_loss(f.obj_s.data_ptr(), 1, ones.data_ptr(), 1, B, 1, float(B), 0.0, f.terms.ptr("scale"), None, L.stream_ptr()))
        Rv, dMv = obj_R.view(B, 9), f.dM.view(B, 9)

        def outer(it):
            if it < iter_for_obj:
                phase = "object only"
                if f.adam is None:
                    f.adam = AdamState([(Rv, 9, dMv, 0.002), (obj_t, 3, f.dt, 0.006)], f.stop)
            elif it < iter_for_obj + iter_for_sil:
                phase = "sil"
                if sil is None:
                    raise L.VtError("phase 'sil' needs a SilSetup")
                if f.adam is None or it == iter_for_obj:
                    f.adam = AdamState([(Rv, 9, dMv, 0.006), (obj_t, 3, f.dt, 0.006)], f.stop)
                    f.trans_init = obj_t.clone()
            else:
                phase = "joint"
                if f.adam is None or it == iter_for_obj + iter_for_sil:
                    f.adam = AdamState([(obj_t, 3, f.dt, 0.002)], f.stop)
            decay = 1 if phase == "object only" else (it - iter_for_obj + 1 if phase == "sil" else (it - iter_for_obj + 1) / 3)
            tw = 10.0 if phase == "joint" else 1.0
            w = f.terms.weights(FIT_WEIGHTS, decay, {"otemp": tw, "ovtemp": tw})
            # the fused step launches cover everything but the interpenetration term (it adds to dt between the rigid VJP and the SO(3) VJP)
            fused = self.fused_steps and not (phase == "joint" and self.collision_loss)
            return (self._object_step_fused if fused else self._object_step), phase, w, int(early_stop and phase == "joint" and it > 0.25 * max_iter)
        return self._run_fit(f, start, end, check_every, outer, prof)

    def _read_stop(self, stop):
        """the host's look at the device-side stop flag, once per outer iteration: a stream synchronisation.  ``host_wait_s`` accumulates the time the host
        spends blocked here -- the slack of the launching thread: close to the wall-clock of a fit when the GPU is the bottleneck, close to zero when the
        host cannot queue launches as fast as the GPU retires them"""
        t0 = time.perf_counter()
        v = int(stop.item())
        with self._counter_lock:
            self.host_wait_s += time.perf_counter() - t0
        return v

    @contextlib.contextmanager
    def _skip_after_stop(self, stop):
        """While the body runs, the query and SMPL-H kernels launched on the current stream return at once when ``stop`` is set
        (vt_stream_set_skip_flag): the steps queued behind the one whose stop rule fired -- up to nine, the host reads the flag once per outer
        iteration -- cost a launch each instead of a pass (results unchanged: Adam and the loss history ignore them already).  The callers drop the
        per-launch events of those no-op launches from a profiled run, so that bench.py prices executed launches only."""
        if not self.device_skip:
            yield False
            return
        sp = L.stream_ptr()
        rc = _lib().vt_stream_set_skip_flag(sp, stop.data_ptr())
        if rc == L.VT_ERR_BUSY:
            # this thread already has another fit's flag registered for the stream (nested fits): run without the device-side skip (and the look-ahead)
            yield False
            return
        L.check(rc)                 # anything else is an error, not a reason to silently lose the skip
        try:
            yield True
        finally:
            _lib().vt_stream_set_skip_flag(sp, None)

    # ---- Adam steps: step(f, phase, k, w, armed) queues step k of fit ``f`` (see _run_fit) -------------------
    def _smplt_step(self, f, phase, k, w, armed):
        """one Adam step of the SMPL-T pre-fit (SMPLHFitter30fps.compute_loss, fit_SMPLH_30fps.py:153-200)"""
        lib = _lib(); st = L.stream_ptr(); B = f.B; pose = f.pose
        f.terms.zero(0, 5)
        self.smpl_forward(pose, f.betas, f.trans, f.verts, f.jtr, f.vposed, f.ws, f.prefix)
        _chk(lib.vt_landmarks_forward(self.b25.h, f.verts.data_ptr(), B, f.J.data_ptr(), st))
        _chk(lib.vt_kpts_loss(f.J.data_ptr(), f.kpts.data_ptr(), None, B, 25, 0, self.cam.ctypes.data, 0.0, float(w[0]), f.terms.ptr("kpts"), f.dJ.data_ptr(), st))
        _chk(lib.vt_landmarks_backward(self.b25.h, f.dJ.data_ptr(), B, f.dverts.data_ptr(), 0, st))
        if f.temporal:
            _chk(lib.vt_accel_loss(f.verts.data_ptr(), B, 6890 * 3, None, float(w[1]), f.terms.ptr("temp"), f.dverts.data_ptr(), st))
        self.smpl_backward(pose, f.betas, f.dverts, f.vposed, f.ws, f.scratch, f.dpose, f.dbetas, f.dtrans, f.n_free)
        if f.temporal:
            _chk(lib.vt_accel_loss_strided(pose.data_ptr(), B, 66, 156, self.jw66.data_ptr(), float(w[2]), f.terms.ptr("ptemp"), f.dpose.data_ptr(), st))
        self.body_prior(pose, f.dpose, float(w[3]), f.terms, "pose", f.vb)
        _chk(lib.vt_sqdiff_loss(pose.data_ptr() + 12, 156, f.pose_init.data_ptr() + 12, 156, B, 63, float(B * 63), float(w[4]),
                                f.terms.ptr("pinit"), f.dpose.data_ptr() + 12, st))
        f.adam.step()
        _chk(lib.vt_loss_reduce_and_stop(f.terms.buf.data_ptr(), w.ctypes.data, len(f.terms.names), 1e-3, armed, f.loss_state.data_ptr(),
                                         f.stop.data_ptr(), f.hist.data_ptr(), k, st))

    def _human_query(self, f, k, w):
        """the SMPL stage's SIF-Net query: df_h / part terms, their gradient written to dverts"""
        ev = _ev_begin(f.lp)
        _chk(_lib().vt_query_human_loss(self.net.h, C.byref(f.maps.c), f.verts.data_ptr(), f.crop_center.data_ptr(), f.body_center.data_ptr(), f.B, 6890,
                                        self.labels.data_ptr(), f.vert_order_ptr, float(w[0]), float(w[1]), f.dverts.data_ptr(), f.terms.ptr("df_h"),
                                        L.stream_ptr()))
        _ev_end(f.lp, "human", ev, f.B, k)

    def _smpl_step(self, f, phase, k, w, armed):
        """one Adam step of the SMPL stage as single-purpose launches (forward_smpl + the loss of recon_fit_behave.py:452-513)"""
        lib = _lib(); st = L.stream_ptr(); B = f.B; pose = f.pose
        f.terms.zero(0, 6)
        self.smpl_forward(pose, f.betas, f.trans, f.verts, f.jtr, f.vposed, f.ws, f.prefix)
        self._human_query(f, k, w)
        if phase == "kpts":
            _chk(lib.vt_landmarks_forward(self.b25.h, f.verts.data_ptr(), B, f.J.data_ptr(), st))
            _chk(lib.vt_kpts_loss(f.J.data_ptr(), f.body_kpts.data_ptr(), f.crop_center.data_ptr(), B, 25, 1, self.cam.ctypes.data, f.net_size,
                                  float(w[4]), f.terms.ptr("j2d"), f.dJ.data_ptr(), st))
            _chk(lib.vt_landmarks_backward(self.b25.h, f.dJ.data_ptr(), B, f.dverts.data_ptr(), 1, st))
        if B >= 4:
            _chk(lib.vt_accel_loss(f.verts.data_ptr(), B, 6890 * 3, None, float(w[5]), f.terms.ptr("stemp"), f.dverts.data_ptr(), st))
        self.smpl_backward(pose, f.betas, f.dverts, f.vposed, f.ws, f.scratch, f.dpose, f.dbetas, f.dtrans, f.n_free)
        self.body_prior(pose, f.dpose, float(w[2]), f.terms, "pose", f.vb)
        # pinit = mean_B sum (pose[:, 3:72] - pose_init)^2
        _chk(lib.vt_sqdiff_loss(pose.data_ptr() + 12, 156, f.pose_init.data_ptr() + 12, 156, B, 69, float(B), float(w[3]),
                                f.terms.ptr("pinit"), f.dpose.data_ptr() + 12, st))
        f.adam.step()
        _chk(lib.vt_loss_reduce_and_stop(f.terms.buf.data_ptr(), w.ctypes.data, len(f.terms.names), 1e-3, armed, f.loss_state.data_ptr(),
                                         f.stop.data_ptr(), f.hist.data_ptr(), k, st))

    def _smpl_step_fused(self, f, phase, k, w, armed):
        """``_smpl_step`` with the keypoint chain as one launch behind the query and one tail (the tail of the previous step left the terms zeroed)"""
        lib = _lib(); st = L.stream_ptr(); B = f.B
        self.smpl_forward(f.pose, f.betas, f.trans, f.verts, f.jtr, f.vposed, f.ws, f.prefix)
        self._human_query(f, k, w)
        if phase == "kpts":
            # joints, 2-D keypoint term and its gradient ADDED to the query's (accumulate = 1: the float addition of vt_landmarks_backward) in one launch
            _chk(lib.vt_kpts_step(self.b25.h, f.verts.data_ptr(), f.body_kpts.data_ptr(), f.crop_center.data_ptr(), B, 1, self.cam.ctypes.data, f.net_size,
                                  float(w[4]), f.terms.ptr("j2d"), f.J.data_ptr(), f.dverts.data_ptr(), 1, st))
        if B >= 4:
            _chk(lib.vt_accel_loss(f.verts.data_ptr(), B, 6890 * 3, None, float(w[5]), f.terms.ptr("stemp"), f.dverts.data_ptr(), st))
        self.smpl_backward(f.pose, f.betas, f.dverts, f.vposed, f.ws, f.scratch, f.dpose, f.dbetas, f.dtrans, f.n_free)
        self._smpl_tail(f, k, w, armed)

    def _smpl_step_fused_query(self, f, phase, k, w, armed):
        """``_smpl_step_fused`` with the keypoint chain BEFORE the query and the query adding its gradient and the vertex acceleration stencil in its own
        epilogue (vt_query_human_step: 8 launches per step with the two forward and three backward SMPL-H kernels and the tail)"""
        lib = _lib(); st = L.stream_ptr(); B = f.B
        self.smpl_forward(f.pose, f.betas, f.trans, f.verts, f.jtr, f.vposed, f.ws, f.prefix)
        if phase == "kpts":
            _chk(lib.vt_kpts_step(self.b25.h, f.verts.data_ptr(), f.body_kpts.data_ptr(), f.crop_center.data_ptr(), B, 1, self.cam.ctypes.data, f.net_size,
                                  float(w[4]), f.terms.ptr("j2d"), f.J.data_ptr(), f.dverts.data_ptr(), 0, st))
        ev = _ev_begin(f.lp)
        _chk(lib.vt_query_human_step(self.net.h, C.byref(f.maps.c), f.verts.data_ptr(), f.crop_center.data_ptr(), f.body_center.data_ptr(), B, 6890,
                                     self.labels.data_ptr(), f.vert_order_ptr, float(w[0]), float(w[1]), int(phase == "kpts"), float(w[5]),
                                     f.terms.ptr("stemp") if B >= 4 else None, f.dverts.data_ptr(), f.terms.ptr("df_h"), st))
        _ev_end(f.lp, "human", ev, B, k)
        self.smpl_backward(f.pose, f.betas, f.dverts, f.vposed, f.ws, f.scratch, f.dpose, f.dbetas, f.dtrans, f.n_free)
        self._smpl_tail(f, k, w, armed)

    def _smpl_tail(self, f, k, w, armed):
        """body prior + pinit + Adam on every group + loss reduction / stop rule + term zeroing: one launch (vt_smplstep_tail)"""
        _chk(_lib().vt_smplstep_tail(f.pose.data_ptr(), f.pose_init.data_ptr(), f.dpose.data_ptr(), f.B, self.pri["body_mean"].data_ptr(),
                                     self.pri["body_prec"].data_ptr(), float(w[2]) / f.B, f.terms.ptr("pose"), float(w[3]), f.terms.ptr("pinit"),
                                     *f.adam.smpl_tail_groups, f.adam.tick(), 0.9, 0.999, 1e-8,
                                     f.terms.buf.data_ptr(), w.ctypes.data, len(f.terms.names), 1e-3, armed, f.loss_state.data_ptr(), f.stop.data_ptr(),
                                     f.hist.data_ptr(), k, f.ticket.data_ptr(), 6, L.stream_ptr()))

    def _object_query(self, f, k, w):
        """the object stage's SIF-Net query: 'object' term, its gradient written to dX"""
        ev = _ev_begin(f.lp)
        _chk(_lib().vt_query_object_loss(self.net.h, C.byref(f.maps.c), f.X.data_ptr(), f.crop_center.data_ptr(), f.body_center.data_ptr(), f.B, f.N,
                                         f.occ.data_ptr(), float(w[0]), f.dX.data_ptr(), f.terms.ptr("object"), L.stream_ptr()))
        _ev_end(f.lp, "object", ev, f.B, k)

    def _contacts(self, f, w):
        """the contact term of a 'joint' step; the first one computes the contact set"""
        if f.contact is None:
            f.contact = self._contacts_once(f.maps, f.smpl_verts, f.X, f.crop_center, f.body_center)
        if f.contact["P"] > 0:
            self._contact_term(f.contact, f.X, f.dX, float(w[5]), f.terms)

    def _object_step(self, f, phase, k, w, armed):
        """one Adam step of the object stage as single-purpose launches (forward_step + the loss of recon_fit_trivis_full.py:193-283): the reference of
        the fused step, and the step of phase 'joint' with the interpenetration term"""
        lib = _lib(); st = L.stream_ptr(); B, N, NV, nz = f.B, f.N, f.NV, f.noise[k]
        obj_R, obj_t, obj_s, X, dX, R, dR, dt = f.obj_R, f.obj_t, f.obj_s, f.X, f.dX, f.R, f.dR, f.dt
        nf = self.obj_faces.shape[0]
        f.terms.zero(0, 7)
        _chk(lib.vt_so3_project_forward(obj_R.data_ptr(), nz.data_ptr(), B, R.data_ptr(), st))
        _chk(lib.vt_rigid_forward(self.obj_points.data_ptr(), 1, R.data_ptr(), obj_t.data_ptr(), obj_s.data_ptr(), B, N, X.data_ptr(), st))
        if phase == "sil":
            _chk(lib.vt_fill(dX.data_ptr(), dX.numel(), 0.0, st))
        else:
            self._object_query(f, k, w)
        if B >= 4:
            _chk(lib.vt_accel_loss(X.data_ptr(), B, N * 3, None, float(w[1]), f.terms.ptr("otemp"), dX.data_ptr(), st))
            _chk(lib.vt_velocity_loss(X.data_ptr(), B, N * 3, float(w[2]), f.terms.ptr("ovtemp"), dX.data_ptr(), st))
        acc = 0
        if phase == "sil":
            sil = f.sil
            _chk(lib.vt_rigid_forward(self.obj_verts.data_ptr(), 1, R.data_ptr(), obj_t.data_ptr(), obj_s.data_ptr(), B, NV, f.Vt.data_ptr(), st))
            _chk(lib.vt_sil_forward(f.Vt.data_ptr(), B, NV, self.obj_faces.data_ptr(), nf, sil.K.data_ptr(), sil.size, f.img.data_ptr(), f.fidx.data_ptr(),
                                    f.sws.data_ptr(), st))
            _chk(lib.vt_sil_mask_loss(f.img.data_ptr(), sil.keep.data_ptr(), sil.ref.data_ptr(), f.occ.data_ptr(), B, sil.size, float(w[3]),
                                      f.terms.ptr("mask"), f.per.data_ptr(), f.dimg.data_ptr(), st))
            _chk(lib.vt_sil_backward(f.Vt.data_ptr(), B, NV, self.obj_faces.data_ptr(), nf, sil.K.data_ptr(), sil.size, f.fidx.data_ptr(), f.dimg.data_ptr(),
                                     1e-4, f.sws.data_ptr(), f.dVt.data_ptr(), st))
            _chk(lib.vt_rigid_backward(self.obj_verts.data_ptr(), 1, obj_s.data_ptr(), B, NV, f.dVt.data_ptr(), dR.data_ptr(), dt.data_ptr(), 0, st))
            _chk(lib.vt_sqdiff_loss(obj_t.data_ptr(), 3, f.trans_init.data_ptr(), 3, B, 3, float(B * 3), float(w[4]), f.terms.ptr("trans"), dt.data_ptr(), st))
            acc = 1
        if phase == "joint":
            self._contacts(f, w)
        _chk(lib.vt_rigid_backward(self.obj_points.data_ptr(), 1, obj_s.data_ptr(), B, N, dX.data_ptr(), dR.data_ptr(), dt.data_ptr(), acc, st))
        if phase == "joint" and self.collision_loss:
            # prevent interpenetration (recon_fit_trivis_full.py:260-264): SMPL mesh vs the transformed object template
            if f.cws is None:
                f.Vc = torch.empty(B, NV, 3, device=X.device)
                f.cws = torch.empty((lib.vt_collision_workspace_bytes(B, self.smpl_faces.shape[0]) + 7) // 8, dtype=torch.int64, device=X.device)
            _chk(lib.vt_rigid_forward(self.obj_verts.data_ptr(), 1, R.data_ptr(), obj_t.data_ptr(), obj_s.data_ptr(), B, NV, f.Vc.data_ptr(), st))
            _chk(lib.vt_collision_loss(f.smpl_verts.data_ptr(), f.smpl_verts.shape[1], self.smpl_faces.data_ptr(), self.smpl_faces.shape[0], f.Vc.data_ptr(), NV,
                                       self.obj_faces.data_ptr(), nf, B, 0.5, 8, float(w[6]), f.terms.ptr("collide"), dt.data_ptr(), None, f.cws.data_ptr(), st))
        _chk(lib.vt_so3_project_backward(obj_R.data_ptr(), nz.data_ptr(), B, dR.data_ptr(), f.dM.data_ptr(), st))
        f.adam.step()
        _chk(lib.vt_loss_reduce_and_stop(f.terms.buf.data_ptr(), w.ctypes.data, len(f.terms.names), 1e-4, armed, f.loss_state.data_ptr(), f.stop.data_ptr(),
                                         f.hist.data_ptr(), k, st))

    def _object_step_fused(self, f, phase, k, w, armed):
        """one Adam step of the object stage as head -> (query | silhouette) -> stencils -> (contacts) -> tail; the arithmetic of ``_object_step`` in
        the same order.  The head leaves its SVD of M0 + noise in ``f.svd_ws`` for the tail of the same step."""
        lib = _lib(); st = L.stream_ptr(); B, N, NV, nz = f.B, f.N, f.NV, f.noise[k]
        is_sil = phase == "sil"
        X, dX = f.X.data_ptr(), f.dX.data_ptr()
        obj_verts, Vt, dVt = (self.obj_verts.data_ptr(), f.Vt.data_ptr(), f.dVt.data_ptr()) if is_sil else (None, None, None)
        _chk(lib.vt_objstep_head(f.obj_R.data_ptr(), nz.data_ptr(), f.obj_t.data_ptr(), f.obj_s.data_ptr(), B, self.obj_points.data_ptr(), N, X,
                                 obj_verts, NV, Vt, f.R.data_ptr(), f.terms.buf.data_ptr(), 7, f.svd_ws.data_ptr(), st))
        if not is_sil:
            self._object_query(f, k, w)
        # phases 'object only' / 'sil': nothing adds to dX between the temporal stencils and the tail, so the tail evaluates them itself
        # (vt_objstep_tail_temporal); phase 'joint' keeps the stencil launch (the contact term's additions come after it)
        tail_temporal = B >= 4 and phase != "joint"
        if B >= 4 and phase == "joint":
            _chk(lib.vt_temporal_loss2(X, B, N * 3, float(w[1]), f.terms.ptr("otemp"), float(w[2]), f.terms.ptr("ovtemp"), dX, 0, st))
        elif is_sil and B < 4:
            _chk(lib.vt_fill(dX, f.dX.numel(), 0.0, st))
        if is_sil:
            # the silhouette term in 5 launches: vt_sil_forward + vt_sil_mask_loss + vt_sil_backward, bit-identical gradients
            sil = f.sil
            _chk(lib.vt_sil_step(Vt, B, NV, self.obj_faces.data_ptr(), self.obj_faces.shape[0], sil.K.data_ptr(), sil.size, sil.keep.data_ptr(),
                                 sil.ref.data_ptr(), f.occ.data_ptr(), float(w[3]), 1e-4, f.terms.ptr("mask"), f.fidx.data_ptr(), f.dimg.data_ptr(),
                                 f.sws.data_ptr(), dVt, st))
        if phase == "joint":
            self._contacts(f, w)
        tail, pre = lib.vt_objstep_tail, ()
        if tail_temporal:
            tail, pre = lib.vt_objstep_tail_temporal, (X, float(w[1]), f.terms.ptr("otemp"), float(w[2]), f.terms.ptr("ovtemp"), int(is_sil))
        _chk(tail(*pre, obj_verts, NV, dVt, self.obj_points.data_ptr(), N, dX, f.obj_s.data_ptr(), B, f.obj_R.data_ptr(), nz.data_ptr(), f.obj_t.data_ptr(),
                  f.trans_init.data_ptr() if is_sil else None, float(w[4]), f.terms.ptr("trans"), f.dR.data_ptr(), f.dt.data_ptr(), f.dM.data_ptr(),
                  *f.adam.object_tail_groups, f.adam.tick(), 0.9, 0.999, 1e-8, f.terms.buf.data_ptr(), w.ctypes.data, len(f.terms.names), 1e-4, armed,
                  f.loss_state.data_ptr(), f.stop.data_ptr(), f.hist.data_ptr(), k, f.ticket.data_ptr(), 0, f.svd_ws.data_ptr(), st))

    def _contact_term(self, contact, X, dX, w, terms):
        """the contact Chamfer term of a 'joint' step (recon_fit_trivis_full.py:449-457): the object-side contact points are read out of X and their gradient
        added into dX through the index list inside the launch (vt_chamfer_ragged_idx: the additions of index_select -> Chamfer -> index_add_ in their
        order, without those three launches); the work-item plan of the -- per batch constant -- contact set is built by the first call only"""
        _chk(_lib().vt_chamfer_ragged_idx(contact["x"].data_ptr(), contact["offx"].data_ptr(), contact["x"].shape[0], X.data_ptr(), contact["idx_o32"].data_ptr(),
                                          contact["offy"].data_ptr(), contact["idx_o32"].shape[0], contact["P"], w, terms.ptr("contact"), dX.data_ptr(),
                                          contact["ws"].data_ptr(), int(not contact["planned"]), L.stream_ptr()))
        contact["planned"] = True

    def _contacts_once(self, maps, smpl_verts, X, crop_center, body_center, thres=0.08):
        """'Computing contacts once' (recon_fit_trivis_full.py:242-253) + the pairing of compute_contact_loss (:393-457):
        contact masks df < 0.08 on both sides, pairs (frame, part) present on both, ragged index lists on the device."""
        B, N = X.shape[:2]; V = smpl_verts.shape[1]; dev = X.device
        df_o, _, parts_o, _, _ = ops.sifnet_query(self.net, maps, X, crop_center, body_center, head_mask=0b00101)
        df_h, _, _, _, _ = ops.sifnet_query(self.net, maps, smpl_verts, crop_center, body_center, head_mask=0b00001)
        mask_o = df_o[:, 0] < thres                      # df_obj_h: human distance at the object points
        mask_h = df_h[:, 1] < thres                      # df_hum_o: object distance at the SMPL vertices
        lab_o = parts_o.argmax(1)                        # (B,N)
        lab_h = self.labels.long().unsqueeze(0).expand(B, V)
        oh = torch.zeros(B, 14, device=dev, dtype=torch.long); oo = torch.zeros_like(oh)
        oh.scatter_add_(1, lab_h, mask_h.long()); oo.scatter_add_(1, lab_o, mask_o.long())
        pair = (oh > 0) & (oo > 0)                       # (B,14)
        P = int(pair.sum().item())
        if P == 0:
            return {"P": 0}
        sel_h = mask_h & pair.gather(1, lab_h); sel_o = mask_o & pair.gather(1, lab_o)
        bh, vh = sel_h.nonzero(as_tuple=True); bo, no = sel_o.nonzero(as_tuple=True)
        cnt_h = (oh * pair).reshape(-1); cnt_o = (oo * pair).reshape(-1)
        keep = pair.reshape(-1)
        # the Chamfer kernel runs one workgroup per pair, brute force: the pairs are listed LARGEST FIRST (n_h x n_o evaluations each, 1 .. 5e5), so that the
        # dispatcher starts the long ones first and the small ones fill the tail (the term is a sum over pairs, the gradients are per point: the order of
        # the list is free); rank = position of a (frame, part) key in that list
        ch, co = cnt_h[keep], cnt_o[keep]
        perm = torch.argsort(ch * co, descending=True, stable=True)
        rank_of_key = torch.zeros(B * 14, dtype=torch.long, device=dev)
        rank_of_key[keep.nonzero(as_tuple=True)[0][perm]] = torch.arange(P, device=dev)
        kh = rank_of_key[bh * 14 + lab_h[bh, vh]]; ko = rank_of_key[bo * 14 + lab_o[bo, no]]
        oh_s = torch.sort(kh, stable=True); oo_s = torch.sort(ko, stable=True)
        idx_h = (bh * V + vh)[oh_s.indices]; idx_o = (bo * N + no)[oo_s.indices]
        offx = torch.zeros(P + 1, dtype=torch.int32, device=dev); offy = torch.zeros(P + 1, dtype=torch.int32, device=dev)
        offx[1:] = torch.cumsum(ch[perm], 0).int(); offy[1:] = torch.cumsum(co[perm], 0).int()
        x = smpl_verts.reshape(-1, 3).index_select(0, idx_h).contiguous()
        ws = torch.empty(int(_lib().vt_chamfer_ws_bytes(x.shape[0], idx_o.shape[0], P)), dtype=torch.uint8, device=dev)     # scratch of vt_chamfer_ragged_ws
        return {"P": P, "x": x, "offx": offx, "offy": offy, "idx_o": idx_o, "idx_o32": idx_o.int().contiguous(), "ws": ws, "planned": False}


class SilSetup:
    """Per-batch constants of SilLossROI (obj_pose_roi.py:39-75): ROI intrinsics K (B,9), keep mask and reference mask
    (B,size,size).  Built from already cropped masks by ``vistracker_amd.silhouette.SilLossROI`` or synthetically."""

    def __init__(self, K, keep, ref, size=256):
        self.K, self.keep, self.ref, self.size = K.contiguous(), keep.contiguous(), ref.contiguous(), size
