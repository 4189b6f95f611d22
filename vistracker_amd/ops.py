"""torch-facing operators over the C ABI: each op is a ``torch.autograd.Function`` whose forward and
backward are single calls into ``libvistracker_hip.so``.  PyTorch supplies device memory, the current
HIP stream and the autograd graph; all arithmetic happens in the HIP kernels.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import encoder_fwd as fwd


def _f32(t):
    return t.detach().contiguous().float()


def _np32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32)


# --------------------------------------------------------------------------------------------------
# SMPL-H
# --------------------------------------------------------------------------------------------------
class SmplhHandle:
    """Device-resident SMPL-H constants (smpl_layer.py:46-71)."""

    def __init__(self, model: dict, device="cuda:0"):
        self.device = torch.device(device)
        par = np.asarray(model["parents"]).astype(np.int64).copy()
        par[0] = 0
        par = np.ascontiguousarray(par, dtype=np.int32)
        arrs = [_np32(model[k]) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")]
        assert arrs[0].shape == (6890, 3) and arrs[1].shape == (6890, 3, 10) and arrs[2].shape == (6890, 3, 459)
        assert arrs[3].shape == (52, 6890) and arrs[4].shape == (6890, 52)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            L.check(L.lib().vt_smplh_create(C.byref(h), *[a.ctypes.data for a in arrs], par.ctypes.data, L.stream_ptr()))
        self.h = h
        self.faces = np.asarray(model["f"]).astype(np.int64) if "f" in model else None

    def __del__(self):
        try:
            if getattr(self, "h", None):
                L.lib().vt_smplh_destroy(self.h)
        except Exception:
            pass


class _SmplhFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, handle: SmplhHandle, pose, betas, trans):
        pose, betas, trans = _f32(pose), _f32(betas), _f32(trans)
        B = pose.shape[0]
        dev = pose.device
        verts = torch.empty(B, 6890, 3, device=dev); jtr = torch.empty(B, 52, 3, device=dev)
        vposed = torch.empty(B, 6890, 3, device=dev)
        ws = torch.empty(L.lib().vt_smplh_workspace_floats(B), device=dev)
        L.check(L.lib().vt_smplh_forward(handle.h, L.dptr(pose), L.dptr(betas), L.dptr(trans), B, L.dptr(verts), L.dptr(jtr),
                                         L.dptr(vposed), L.dptr(ws), L.stream_ptr()))
        ctx.handle = handle
        ctx.save_for_backward(pose, betas, vposed, ws)
        ctx.mark_non_differentiable(vposed)
        return verts, jtr, vposed

    @staticmethod
    def backward(ctx, dverts, djtr, _dvp):
        pose, betas, vposed, ws = ctx.saved_tensors
        B = pose.shape[0]
        dev = pose.device
        dverts = torch.zeros(B, 6890, 3, device=dev) if dverts is None else _f32(dverts)
        djtr = None if djtr is None else _f32(djtr)
        scratch = torch.empty(L.lib().vt_smplh_bwd_scratch_floats(B), device=dev)
        dpose = torch.empty(B, 156, device=dev); dbetas = torch.empty(B, 10, device=dev); dtrans = torch.empty(B, 3, device=dev)
        L.check(L.lib().vt_smplh_backward(ctx.handle.h, L.dptr(pose), L.dptr(betas), B, L.dptr(dverts), L.dptr(djtr), L.dptr(vposed),
                                          L.dptr(ws), L.dptr(scratch), L.dptr(dpose), L.dptr(dbetas), L.dptr(dtrans), L.stream_ptr()))
        return None, dpose, dbetas, dtrans


def smplh_forward(handle: SmplhHandle, pose, betas, trans):
    """-> verts (B,6890,3), jtr (B,52,3), v_posed (B,6890,3);  SMPL_Layer.forward (smpl_layer.py:73-176)."""
    return _SmplhFn.apply(handle, pose, betas, trans)


def rodrigues(aa):
    aa = _f32(aa).reshape(-1, 3)
    R = torch.empty(aa.shape[0], 9, device=aa.device)
    L.check(L.lib().vt_rodrigues_forward(L.dptr(aa), aa.shape[0], L.dptr(R), L.stream_ptr()))
    return R


def rodrigues_bwd(aa, dR):
    aa = _f32(aa).reshape(-1, 3); dR = _f32(dR).reshape(-1, 9)
    d = torch.empty_like(aa)
    L.check(L.lib().vt_rodrigues_backward(L.dptr(aa), aa.shape[0], L.dptr(dR), L.dptr(d), L.stream_ptr()))
    return d


# --------------------------------------------------------------------------------------------------
# landmark regressors
# --------------------------------------------------------------------------------------------------
class LandmarkHandle:
    def __init__(self, csr: dict, device="cuda:0"):
        self.K, self.V = csr["shape"]
        ip = np.ascontiguousarray(csr["indptr"], np.int32); ix = np.ascontiguousarray(csr["indices"], np.int32)
        da = _np32(csr["data"])
        h = C.c_void_p()
        with torch.cuda.device(torch.device(device)):
            L.check(L.lib().vt_landmarks_create(C.byref(h), ip.ctypes.data, ix.ctypes.data, da.ctypes.data, self.K, self.V, L.stream_ptr()))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                L.lib().vt_landmarks_destroy(self.h)
        except Exception:
            pass


class _LandmarkFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, handle, verts):
        verts = _f32(verts); B = verts.shape[0]
        out = torch.empty(B, handle.K, 3, device=verts.device)
        L.check(L.lib().vt_landmarks_forward(handle.h, L.dptr(verts), B, L.dptr(out), L.stream_ptr()))
        ctx.handle = handle; ctx.B = B
        return out

    @staticmethod
    def backward(ctx, dout):
        dout = _f32(dout)
        dverts = torch.empty(ctx.B, ctx.handle.V, 3, device=dout.device)
        L.check(L.lib().vt_landmarks_backward(ctx.handle.h, L.dptr(dout), ctx.B, L.dptr(dverts), 0, L.stream_ptr()))
        return None, dverts


def landmarks(handle: LandmarkHandle, verts):
    """batch_sparse_dense_matmul(regressor, verts) (torch_functions.py:52-76)."""
    return _LandmarkFn.apply(handle, verts)


# --------------------------------------------------------------------------------------------------
# priors
# --------------------------------------------------------------------------------------------------
class _MahalanobisFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, off, mean, prec):
        x = _f32(x); B, stride = x.shape; n = mean.shape[0]
        val = torch.empty(B, device=x.device)
        L.check(L.lib().vt_mahalanobis(L.dptr(x), B, stride, off, n, L.dptr(mean), L.dptr(prec), L.dptr(val), None, 0.0, L.stream_ptr()))
        ctx.save_for_backward(x, mean, prec); ctx.off = off
        return val

    @staticmethod
    def backward(ctx, dval):
        x, mean, prec = ctx.saved_tensors
        B, stride = x.shape; n = mean.shape[0]
        # d value[b]/dx scaled per row: run with gscale 1 and scale rows afterwards
        dx = torch.zeros_like(x); val = torch.empty(B, device=x.device)
        L.check(L.lib().vt_mahalanobis(L.dptr(x), B, stride, ctx.off, n, L.dptr(mean), L.dptr(prec), L.dptr(val), L.dptr(dx), 1.0, L.stream_ptr()))
        return dx * dval.reshape(B, 1), None, None, None


def mahalanobis(x, off, mean, prec):
    """th_Mahalanobis / HandPrior core (th_smpl_prior.py:30-38): |(x[:, off:off+n]-mean) @ prec|^2 per row."""
    return _MahalanobisFn.apply(x, off, mean, prec)


# --------------------------------------------------------------------------------------------------
# SIF-Net query
# --------------------------------------------------------------------------------------------------
HEADS = ("df", "pca", "parts", "centers", "vis")
HEAD_DIMS = (2, 9, 14, 3, 1)
MAP_ORDER = ("im_feat", "tmpx", "tri_tmpx0", "tri_tmpx1", "tri_tmpx2", "tri_feat0", "tri_feat1", "tri_feat2")
MAP_CHANNELS = (256, 64, 32, 32, 32, 64, 64, 64)
DEFAULT_CAM = (979.7844, 979.840, 1018.952, 779.486, 1200.0)   # camera.py:26-41, config/tri-vis-l2.json:40


class SifNetHandle:
    """The five point decoders (chore.py:113-126, chore_tri_vis.py:17-28) + camera, resident on the device."""

    def __init__(self, decoders: dict, cam=DEFAULT_CAM, device="cuda:0"):
        ws, bs = [], []
        for name, k in zip(HEADS, HEAD_DIMS):
            layers = decoders[name]
            assert len(layers) == 4 and tuple(layers[0][0].shape) == (128, 611) and tuple(layers[3][0].shape) == (k, 128)
            for (w, b) in layers:
                ws.append(_np32(w)); bs.append(_np32(b))
        wp = (C.c_void_p * 20)(*[w.ctypes.data for w in ws]); bp = (C.c_void_p * 20)(*[b.ctypes.data for b in bs])
        cam = _np32(cam)
        h = C.c_void_p()
        with torch.cuda.device(torch.device(device)):
            L.check(L.lib().vt_sifnet_create(C.byref(h), wp, bp, cam.ctypes.data, L.stream_ptr()))
        self.h = h; self.cam = cam

    PRECISIONS = {"split-f16": 0, "fp32": 1}

    def set_precision(self, mode: str):
        """'split-f16' (default: 22-bit split operands on the f16 MFMA) or 'fp32' (exact fp32 products on the f32-input MFMA, any activation
        magnitude, ~1/5 of the speed) for every query call through this handle (vt_sifnet_set_precision)"""
        L.check(L.lib().vt_sifnet_set_precision(self.h, self.PRECISIONS[mode]))
        return self

    @property
    def precision(self) -> str:
        return {v: k for k, v in self.PRECISIONS.items()}[L.lib().vt_sifnet_get_precision(self.h)]

    def __del__(self):
        try:
            if getattr(self, "h", None):
                L.lib().vt_sifnet_destroy(self.h)
        except Exception:
            pass


class FeatureMaps:
    """The eight feature maps of one batch, channel-last on the device (B,H,W,C)."""

    def __init__(self, nhwc: dict):
        self.t = [nhwc[k] for k in MAP_ORDER]
        for t, c in zip(self.t, MAP_CHANNELS):
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.shape[-1] == c and t.shape[1] == t.shape[2]
        self.B = self.t[0].shape[0]
        self.proj = None; self._proj_key = None
        self.c = L.VtMaps()
        for i, t in enumerate(self.t):
            self.c.maps[i] = t.data_ptr(); self.c.res[i] = t.shape[1]

    ACT_LEVELS = 3      # operand-range levels of the split-f16 decoders (vt_maps::act_level): |activation| < 1023 * 16^level

    @property
    def act_level(self) -> int:
        return int(self.c.act_level)

    def set_act_level(self, level: int):
        """operand-range level of the split-f16 decoders for every query call with THESE maps (per batch: concurrent fits through one network
        handle do not share it).  A hoisted projection built for another level is ignored by the kernels until it is rebuilt."""
        assert 0 <= level < self.ACT_LEVELS
        self.c.act_level = level
        return self

    @property
    def force_fp32(self) -> bool:
        return bool(self.c.force_fp32)

    def set_force_fp32(self, on: bool = True):
        """route the query calls with THESE maps to the strict-fp32 kernels (any activation magnitude, ~1/5 of the speed)"""
        self.c.force_fp32 = 1 if on else 0
        return self

    def slice(self, start, end):
        """frames [start, end) as a FeatureMaps of views (no copy; the projection, if any, is not carried over)"""
        fm = FeatureMaps({k: t[start:end] for k, t in zip(MAP_ORDER, self.t)})
        fm.c.act_level = self.c.act_level; fm.c.force_fp32 = self.c.force_fp32
        return fm

    def select(self, idx):
        """the frames ``idx`` (1-D index tensor) as a new FeatureMaps (copies: 71 MB per frame + the hoisted projection, 17 MB per frame, if there is
        one) -- for passes that continue with a subset of a batch"""
        fm = FeatureMaps({k: t.index_select(0, idx).contiguous() for k, t in zip(MAP_ORDER, self.t)})
        fm.c.act_level = self.c.act_level; fm.c.force_fp32 = self.c.force_fp32
        if self.proj is not None:
            fm.proj = self.proj.view(self.B, -1).index_select(0, idx).reshape(-1).contiguous()
            fm.c.proj = fm.proj.data_ptr(); fm.c.proj_cols = self.c.proj_cols; fm.c.proj_level = self.c.proj_level
        return fm

    def build_projection(self, net, reuse=False):
        """Hoist the im_feat part of the decoders' first layer out of the optimisation loop (vt_query_build_projection): one fp32 GEMM over
        all im_feat texels of the batch -> (B, res, res, 256) array the fused objective kernels blend instead of gathering 256 channels and
        multiplying by W1 at every step.  Valid for these maps and the network ``net`` only.  The SMPL stage, the first of a batch, builds it;
        the object stage gets the same maps and asks with ``reuse``: a projection built for the same network handle, range level, map storage
        and stream is kept and the call returns without a launch.  The key cannot see a write INTO the maps' storage (or new weights behind the
        same handle) between the two calls: whoever does that calls ``drop_projection()``."""
        h = net.h if hasattr(net, "h") else net.handle.h
        key = (h.value if hasattr(h, "value") else int(h), int(self.c.act_level), tuple(t.data_ptr() for t in self.t),
               torch.cuda.current_stream(self.t[0].device).cuda_stream)
        if reuse and self.proj is not None and self.c.proj and self._proj_key == key:
            return self
        self._proj_key = None
        n = L.lib().vt_query_projection_floats(C.byref(self.c), self.B)
        self.proj = torch.empty(n, device=self.t[0].device)
        self.c.proj = None; self.c.proj_cols = 0
        L.check(L.lib().vt_query_build_projection(h, C.byref(self.c), self.B, self.proj.data_ptr(), L.stream_ptr()))
        self.c.proj = self.proj.data_ptr(); self.c.proj_cols = n // (self.B * self.t[0].shape[1] * self.t[0].shape[2])
        self.c.proj_level = self.c.act_level
        self._proj_key = key
        return self

    def drop_projection(self):
        """forget the hoisted projection (also the explicit invalidation after the maps' contents or the network's weights were changed in place)"""
        self.proj = None; self.c.proj = None; self.c.proj_cols = 0; self._proj_key = None
        return self

    @staticmethod
    def from_nchw(maps: dict, device="cuda:0"):
        """NCHW (reference layout, numpy or torch) -> NHWC with the HIP transpose kernel."""
        out = {}
        for k in MAP_ORDER:
            src = maps[k]
            src = torch.as_tensor(src, dtype=torch.float32).to(device).contiguous()
            B, Cc, H, W = src.shape
            dst = torch.empty(B, H, W, Cc, device=src.device)
            L.check(L.lib().vt_nchw_to_nhwc(L.dptr(src), B, Cc, H, W, L.dptr(dst), L.stream_ptr()))
            out[k] = dst
        return FeatureMaps(out)


class _QueryFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net: SifNetHandle, maps: FeatureMaps, pts, cc, bc, head_mask):
        pts, cc, bc = _f32(pts), _f32(cc), _f32(bc)
        B, N = pts.shape[:2]
        outs = [torch.empty(B, k, N, device=pts.device) if (head_mask >> i) & 1 else None for i, k in enumerate(HEAD_DIMS)]
        L.check(L.lib().vt_query_forward(net.h, C.byref(maps.c), L.dptr(pts), L.dptr(cc), L.dptr(bc), B, N,
                                         *[L.dptr(o) for o in outs], L.stream_ptr()))
        ctx.net, ctx.maps, ctx.mask = net, maps, head_mask
        ctx.save_for_backward(pts, cc, bc)
        return tuple(o if o is not None else pts.new_zeros(0) for o in outs)

    @staticmethod
    def backward(ctx, *gs):
        pts, cc, bc = ctx.saved_tensors
        B, N = pts.shape[:2]
        live = [(i, _f32(g)) for i, g in enumerate(gs) if g is not None and (ctx.mask >> i) & 1 and g.numel() > 0]
        total = None
        for s in range(0, len(live), 2):
            args = [None] * 5
            for i, g in live[s:s + 2]:
                args[i] = g
            dpts = torch.empty(B, N, 3, device=pts.device)
            L.check(L.lib().vt_query_backward(ctx.net.h, C.byref(ctx.maps.c), L.dptr(pts), L.dptr(cc), L.dptr(bc), B, N,
                                              *[L.dptr(a) for a in args], L.dptr(dpts), L.stream_ptr()))
            total = dpts if total is None else total + dpts
        if total is None:
            total = torch.zeros(B, N, 3, device=pts.device)
        return None, None, total, None, None, None


def sifnet_query(net, maps, pts, crop_center, body_center, head_mask=31):
    """-> (df (B,2,N), pca (B,9,N), parts (B,14,N), centers (B,3,N), vis (B,1,N)); skipped heads are empty tensors."""
    return _QueryFn.apply(net, maps, pts, crop_center, body_center, head_mask)


def sifnet_project_step(net, maps, pts, crop_center, body_center, df_idx, threshold=1.0, out=None, want_target=True):
    """One fused projection step of Generator.approx_surface (recon/gen/generator.py:72-103): returns (new points, clamped
    distance at the input points).  ``out`` may be ``pts`` itself (in place).  No autograd: the reference detaches here too."""
    pts = _f32(pts.detach()); B, N = pts.shape[:2]
    cc = _f32(crop_center); bc = _f32(body_center)
    out = torch.empty_like(pts) if out is None else out
    dft = torch.empty(B, N, device=pts.device) if want_target else None
    L.check(L.lib().vt_query_project_step(net.h, C.byref(maps.c), L.dptr(pts), L.dptr(cc), L.dptr(bc), B, N, int(df_idx), float(threshold),
                                          L.dptr(out), L.dptr(dft), L.stream_ptr()))
    return out, dft


# --------------------------------------------------------------------------------------------------
# SO(3) projection, rigid transform
# --------------------------------------------------------------------------------------------------
class _So3Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, M, noise):
        M = _f32(M); B = M.shape[0]
        noise = None if noise is None else _f32(noise)
        R = torch.empty(B, 3, 3, device=M.device)
        L.check(L.lib().vt_so3_project_forward(L.dptr(M), L.dptr(noise), B, L.dptr(R), L.stream_ptr()))
        ctx.save_for_backward(M, noise if noise is not None else M.new_zeros(0)); ctx.has_noise = noise is not None
        return R

    @staticmethod
    def backward(ctx, dR):
        M, noise = ctx.saved_tensors
        dR = _f32(dR); dM = torch.empty_like(M)
        L.check(L.lib().vt_so3_project_backward(L.dptr(M), L.dptr(noise) if ctx.has_noise else None, M.shape[0], L.dptr(dR), L.dptr(dM), L.stream_ptr()))
        return dM, None


def so3_project(M, noise=None):
    """project_so3(M + 1e-4*noise) (recon_fit_base.py:179-199,462-469); ``noise`` is the U[0,1) sample or None."""
    return _So3Fn.apply(M, noise)


class _RigidFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X0, R, t, s):
        X0, R, t, s = _f32(X0), _f32(R), _f32(t), _f32(s)
        B = R.shape[0]; shared = int(X0.dim() == 2); N = X0.shape[-2]
        X = torch.empty(B, N, 3, device=R.device)
        L.check(L.lib().vt_rigid_forward(L.dptr(X0), shared, L.dptr(R), L.dptr(t), L.dptr(s), B, N, L.dptr(X), L.stream_ptr()))
        ctx.save_for_backward(X0, s); ctx.shared = shared
        return X

    @staticmethod
    def backward(ctx, dX):
        X0, s = ctx.saved_tensors
        dX = _f32(dX); B, N = dX.shape[:2]
        dR = torch.empty(B, 3, 3, device=dX.device); dt = torch.empty(B, 3, device=dX.device)
        L.check(L.lib().vt_rigid_backward(L.dptr(X0), ctx.shared, L.dptr(s), B, N, L.dptr(dX), L.dptr(dR), L.dptr(dt), 0, L.stream_ptr()))
        return None, dR, dt, None


def rigid_transform(X0, R, t, s):
    """transform_obj_verts (recon_fit_base.py:455-459): (X0 @ R + t) * s; gradients to R and t."""
    return _RigidFn.apply(X0, R, t, s)


# --------------------------------------------------------------------------------------------------
# temporal stencils
# --------------------------------------------------------------------------------------------------
class _StencilFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, kind, elem_w):
        v2 = _f32(v).reshape(v.shape[0], -1)
        B, D = v2.shape
        term = torch.zeros(1, dtype=torch.float64, device=v.device)
        if kind == "accel":
            L.check(L.lib().vt_accel_loss(L.dptr(v2), B, D, L.dptr(elem_w), 0.0, L.dptr(term), None, L.stream_ptr()))
        else:
            L.check(L.lib().vt_velocity_loss(L.dptr(v2), B, D, 0.0, L.dptr(term), None, L.stream_ptr()))
        ctx.save_for_backward(v2, elem_w if elem_w is not None else v2.new_zeros(0))
        ctx.kind, ctx.shape, ctx.has_w = kind, v.shape, elem_w is not None
        return term.float().reshape(())

    @staticmethod
    def backward(ctx, g):
        v2, w = ctx.saved_tensors
        B, D = v2.shape
        dv = torch.zeros_like(v2)
        if ctx.kind == "accel":
            L.check(L.lib().vt_accel_loss(L.dptr(v2), B, D, L.dptr(w) if ctx.has_w else None, 1.0, None, L.dptr(dv), L.stream_ptr()))
        else:
            L.check(L.lib().vt_velocity_loss(L.dptr(v2), B, D, 1.0, None, L.dptr(dv), L.stream_ptr()))
        return (dv * g).reshape(ctx.shape), None, None


def accel_loss(v, elem_w=None):
    """mse(v[1:-1]-v[:-2], v[2:]-v[1:-1]) over the leading (frame) axis (recon_fit_trivis_full.py:170-177)."""
    return _StencilFn.apply(v, "accel", elem_w)


def velocity_loss(v):
    """mse(v[1:], v[:-1]) (recon_fit_trivis_full.py:391)."""
    return _StencilFn.apply(v, "velocity", None)


# --------------------------------------------------------------------------------------------------
# ragged chamfer
# --------------------------------------------------------------------------------------------------
class _ChamferFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, offx, offy):
        x, y = _f32(x), _f32(y); P = offx.numel() - 1
        term = torch.zeros(1, dtype=torch.float64, device=x.device)
        L.check(L.lib().vt_chamfer_ragged(L.dptr(x), L.dptr(offx), L.dptr(y), L.dptr(offy), P, 0.0, L.dptr(term), None, None, L.stream_ptr()))
        ctx.save_for_backward(x, y, offx, offy)
        return term.float().reshape(())

    @staticmethod
    def backward(ctx, g):
        x, y, offx, offy = ctx.saved_tensors
        dx = torch.zeros_like(x); dy = torch.zeros_like(y)
        L.check(L.lib().vt_chamfer_ragged(L.dptr(x), L.dptr(offx), L.dptr(y), L.dptr(offy), offx.numel() - 1, 1.0, None, L.dptr(dx), L.dptr(dy), L.stream_ptr()))
        return dx * g, dy * g, None, None


def chamfer_ragged(x, y, offx, offy):
    return _ChamferFn.apply(x, y, offx, offy)


# --------------------------------------------------------------------------------------------------
# human / object interpenetration (host-gated off in the reference; PARITY UNPINNED: mesh_intersection)
# --------------------------------------------------------------------------------------------------
def collision_loss(smpl_verts, smpl_faces, obj_verts, obj_faces, sigma=0.5, max_collisions=8, gscale=0.0, want_pairs=False):
    """RegistrationBase.smpl_obj_collision (recon_fit_base.py:736-765) on transformed object vertices: returns (value, d value / d obj_t * gscale (B,3))
    [+ colliding pairs per frame].  No autograd graph: the gradient w.r.t. the object translation is what phase 'joint' needs."""
    sv, ov = _f32(smpl_verts), _f32(obj_verts)
    sf = smpl_faces.to(torch.int32).contiguous(); of = obj_faces.to(torch.int32).contiguous()
    B = sv.shape[0]; dev = sv.device
    ws = torch.empty((L.lib().vt_collision_workspace_bytes(B, sf.shape[0]) + 7) // 8, dtype=torch.int64, device=dev)
    term = torch.zeros(1, dtype=torch.float64, device=dev); dt = torch.zeros(B, 3, device=dev)
    npairs = torch.zeros(B, dtype=torch.int32, device=dev) if want_pairs else None
    L.check(L.lib().vt_collision_loss(L.dptr(sv), sv.shape[1], L.dptr(sf), sf.shape[0], L.dptr(ov), ov.shape[1], L.dptr(of), of.shape[0], B, float(sigma),
                                      int(max_collisions), float(gscale), L.dptr(term), L.dptr(dt), L.dptr(npairs), L.dptr(ws), L.stream_ptr()))
    return (term.float().reshape(()), dt, npairs) if want_pairs else (term.float().reshape(()), dt)


# --------------------------------------------------------------------------------------------------
# exact point-to-mesh distance / nearest vertex (csrc/pmdist.hip; PARITY UNPINNED: igl, trimesh)
# --------------------------------------------------------------------------------------------------
def _frames(t, name):
    """(B,K,3) float32 contiguous view of a (K,3) or (B,K,3) tensor, and whether a frame axis was added"""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise L.VtError(f"{name}: a device tensor expected; there is no CPU path")
    t = _f32(t)
    single = t.dim() == 2
    if single:
        t = t[None]
    if t.dim() != 3 or t.shape[-1] != 3 or t.shape[1] == 0:
        raise L.VtError(f"{name}: (B,K,3) or (K,3) with K > 0 expected, got {tuple(t.shape)}")
    return t.contiguous(), single


def check_faces(faces, n_verts):
    """(NF,3) int32 contiguous device tensor of ``faces``; raises unless every index is in [0, n_verts).  Reads two scalars back from the device: callers
    that reuse a mesh (BoundarySampler) call it once and pass ``validate=False`` to point_mesh_distance afterwards."""
    f = torch.as_tensor(faces)
    if f.dim() != 2 or f.shape[1] != 3 or f.shape[0] == 0 or f.dtype.is_floating_point:
        raise L.VtError(f"faces: (NF,3) integers with NF > 0 expected, got {tuple(f.shape)} {f.dtype}")
    lo, hi = int(f.min()), int(f.max())
    if lo < 0 or hi >= n_verts:
        raise L.VtError(f"faces: vertex indices span [{lo}, {hi}] but the mesh has {n_verts} vertices")
    return f.to(torch.int32).contiguous()


def point_mesh_distance(points, verts, faces, want_closest=True, want_face=True, validate=True, culling=True, n_tests=None):
    """vt_point_mesh_distance (igl.signed_distance's |distance| and closest point, boundary_sampler.py:75-100): points (B,N,3), verts (B,NV,3) one mesh
    pose per frame, faces (NF,3) shared -> (dist (B,N), closest (B,N,3), face_id (B,N) int32) device tensors; a single frame may come as (N,3) / (NV,3)
    and is answered without the frame axis.  ``want_closest`` / ``want_face`` False returns None in that place (the kernel then skips the stores).
    ``culling`` False and ``n_tests`` (a zeroed (1,) int64 device tensor the call adds its executed point-triangle tests to) go through
    vt_point_mesh_distance_ex: measurement and tests only, the results are bit-identical."""
    p, single = _frames(points, "points")
    v, vsingle = _frames(verts, "verts")
    if single != vsingle or p.shape[0] != v.shape[0] or p.device != v.device:
        raise L.VtError(f"point_mesh_distance: points {tuple(p.shape)} and verts {tuple(v.shape)} must share the frame axis and the device")
    B, N = p.shape[:2]; NV = v.shape[1]
    f = check_faces(faces, NV) if validate else faces
    if f.dtype != torch.int32 or f.device != p.device:
        f = f.to(device=p.device, dtype=torch.int32)
    f = f.contiguous(); NF = f.shape[0]
    dev = p.device
    with torch.cuda.device(dev):
        ws = torch.empty((L.lib().vt_point_mesh_workspace_bytes(B, NF) + 15) // 16, 2, dtype=torch.int64, device=dev)
        dist = torch.empty(B, N, device=dev)
        closest = torch.empty(B, N, 3, device=dev) if want_closest else None
        face_id = torch.empty(B, N, dtype=torch.int32, device=dev) if want_face else None
        if culling and n_tests is None:
            L.check(L.lib().vt_point_mesh_distance(L.dptr(p), N, L.dptr(v), NV, L.dptr(f), NF, B, L.dptr(dist), L.dptr(closest), L.dptr(face_id), L.dptr(ws),
                                                   L.stream_ptr()))
        else:
            if n_tests is not None and (n_tests.dtype != torch.int64 or n_tests.numel() != 1):
                raise L.VtError("point_mesh_distance: n_tests is a (1,) int64 device tensor")
            L.check(L.lib().vt_point_mesh_distance_ex(L.dptr(p), N, L.dptr(v), NV, L.dptr(f), NF, B, L.dptr(dist), L.dptr(closest), L.dptr(face_id), L.dptr(ws),
                                                      0 if culling else 1, L.dptr(n_tests), L.stream_ptr()))
    if single:
        dist, closest, face_id = dist[0], (closest[0] if want_closest else None), (face_id[0] if want_face else None)
    return dist, closest, face_id


def nearest_vertex(points, verts, want_dist=True):
    """vt_nearest_vertex (trimesh.proximity.ProximityQuery.vertex, boundary_sampler.py:87,97): points (B,N,3), verts (B,NV,3) -> (vert_id (B,N) int32,
    vert_dist (B,N) or None); exact ties go to the smaller index.  (N,3) / (NV,3) for a single frame."""
    p, single = _frames(points, "points")
    v, vsingle = _frames(verts, "verts")
    if single != vsingle or p.shape[0] != v.shape[0] or p.device != v.device:
        raise L.VtError(f"nearest_vertex: points {tuple(p.shape)} and verts {tuple(v.shape)} must share the frame axis and the device")
    B, N = p.shape[:2]; dev = p.device
    with torch.cuda.device(dev):
        vid = torch.empty(B, N, dtype=torch.int32, device=dev)
        vd = torch.empty(B, N, device=dev) if want_dist else None
        L.check(L.lib().vt_nearest_vertex(L.dptr(p), N, L.dptr(v), v.shape[1], B, L.dptr(vid), L.dptr(vd), L.stream_ptr()))
    return (vid[0], vd[0] if want_dist else None) if single else (vid, vd)


# --------------------------------------------------------------------------------------------------
# SIF-Net's training objective at labelled points (csrc/losshead.hip)
# --------------------------------------------------------------------------------------------------
LOSS_WEIGHTS = (1.0, 1.0, 0.006, 500.0, 1000.0, 1000.0)        # dfh, dfo, parts, pca, obj_center, vis (chore.py:86, config/tri-vis-l2.json:75)
LOSS_SLOTS = ("df_h", "df_o", "parts", "pca", "vis", "obj_center")      # the reference's losses_all; the vis term sits in its loss_smpl_center slot
LOSS_SLOT_WEIGHT = (0, 1, 2, 3, 5, 4)                          # slot -> index into loss_weights (chore_tri_vis.py:66-85)
VIS_LOSSES = {"l1": 0, "l2": 1}
_LOSS_WK = {}


def _loss_dev(t, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise L.VtError(f"sifnet_loss_head: {name} must be a device tensor; there is no CPU path")
    return t


def _loss_preds(preds):
    """five stacked (S,B,C,N) float32 contiguous tensors from five stacked tensors ((S,B,C,N), or (B,C,N) for one stack) or from a list of S five-tuples;
    pca may come as (.., 3, 3, N).  One stack is a view; several tuples are stacked (a copy autograd sees through)."""
    if len(preds) == 0:
        raise L.VtError("sifnet_loss_head: no predictions")
    if not torch.is_tensor(preds[0]):
        stacks = [tuple(p) for p in preds]
        if any(len(p) != 5 for p in stacks):
            raise L.VtError("sifnet_loss_head: every stack is a (df, pca, parts, centers, vis) tuple")
        for p in stacks:
            for t, name in zip(p, HEADS):
                _loss_dev(t, name)
        B, N = stacks[0][0].shape[0], stacks[0][0].shape[-1]
        heads = [torch.stack([p[i].reshape(B, k, N) for p in stacks]) if len(stacks) > 1 else stacks[0][i].reshape(1, B, k, N) for i, k in enumerate(HEAD_DIMS)]
    else:
        if len(preds) != 5:
            raise L.VtError("sifnet_loss_head: five prediction tensors (df, pca, parts, centers, vis) expected")
        for t, name in zip(preds, HEADS):
            _loss_dev(t, name)
        N = preds[0].shape[-1]
        if preds[0].dim() not in (3, 4):
            raise L.VtError(f"sifnet_loss_head: df is (S,B,2,N) or (B,2,N), got {tuple(preds[0].shape)}")
        S, B = (1, preds[0].shape[0]) if preds[0].dim() == 3 else tuple(preds[0].shape[:2])
        heads = [t.reshape(S, B, k, N) for t, k in zip(preds, HEAD_DIMS)]
    S, B, _, N = heads[0].shape
    if B == 0 or N == 0:
        raise L.VtError(f"sifnet_loss_head: B = {B}, N = {N}")
    for t, k, name in zip(heads, HEAD_DIMS, HEADS):
        if tuple(t.shape) != (S, B, k, N) or t.dtype != torch.float32:
            raise L.VtError(f"sifnet_loss_head: {name} is float32 ({S},{B},{k},{N}), got {t.dtype} {tuple(t.shape)}")
    return [t.contiguous() for t in heads]


class _LossHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, df, pca, parts, centers, vis, labels, per_frame, max_dist, weights, vis_loss):
        heads = (df, pca, parts, centers, vis)
        S, B, _, N = df.shape
        dev = df.device
        want = any(ctx.needs_input_grad[:5])
        with torch.cuda.device(dev):
            grads = [torch.empty_like(t) if want and ctx.needs_input_grad[i] else None for i, t in enumerate(heads)]
            terms = torch.empty(6, dtype=torch.float64, device=dev)
            ws = torch.empty(L.lib().vt_sifnet_loss_head_ws_bytes(B, N) // 8, dtype=torch.float64, device=dev)
            w = (C.c_double * 6)(*weights)
            L.check(L.lib().vt_sifnet_loss_head(*[L.dptr(t) for t in heads], S, B, N, *[L.dptr(t) for t in labels], int(per_frame), float(max_dist), w,
                                                int(vis_loss), 1.0, L.dptr(terms), *[L.dptr(g) for g in grads], L.dptr(ws), L.stream_ptr()))
        ctx.grads = grads
        key = (dev.index, weights)
        if key not in _LOSS_WK:                                # the slot weights on the device, uploaded once per (device, weights)
            if len(_LOSS_WK) > 16:
                _LOSS_WK.clear()
            _LOSS_WK[key] = torch.tensor([float(weights[i]) for i in LOSS_SLOT_WEIGHT], dtype=torch.float64, device=dev)
        wk = _LOSS_WK[key]
        losses_all = terms * wk
        ctx.mark_non_differentiable(terms, losses_all)
        return losses_all.sum(), losses_all, terms

    @staticmethod
    def backward(ctx, g, _gl, _gt):
        g = g.to(torch.float32)
        return tuple(None if d is None else d * g for d in ctx.grads) + (None,) * 5


def sifnet_loss_head(preds, df_h, df_o, parts_gt, pca_gt, obj_center, visibility, max_dist=5.0, weights=LOSS_WEIGHTS, vis_loss="l2", validate=False,
                     want_terms=False):
    """vt_sifnet_loss_head: the six losses of CHORETriplaneVisibility.get_errors (chore_tri_vis.py:52-99) and, through autograd, their gradient to the
    predictions.  ``preds``: a list of S (df (B,2,N), pca (B,9,N) or (B,3,3,N), parts (B,14,N), centers (B,3,N), vis (B,1,N)) tuples -- one per hourglass stack,
    ``SIFNetQuery.intermediate_preds_list`` -- or the five tensors already stacked to (S,B,C,N).  Labels: df_h, df_o (B,N); parts_gt (B,N) integers (or floats
    holding integers, as the reference's loader delivers them); pca_gt (B,9,N) / (B,3,3,N), obj_center (B,3,N), visibility (B,N) per point, or (B,9) / (B,3,3),
    (B,3), (B) per frame (the compact form: the same bits); mixed forms are expanded to per point.  Device tensors only.  ``validate`` checks that every part
    label is in [0,14) -- it reads the device, so it is off by default; the kernel clamps.
    -> (error, losses_all): float64 device tensors, () and (6,); losses_all is weighted and in the reference's slot order (LOSS_SLOTS); with ``want_terms`` also
    the unweighted terms.  The gradients are computed by the same launch as the values, and only for the predictions that require grad."""
    heads = _loss_preds(preds)
    S, B, _, N = heads[0].shape
    dev = heads[0].device
    if vis_loss not in VIS_LOSSES:
        raise L.VtError(f"sifnet_loss_head: unknown vis_loss {vis_loss!r} (l1 or l2)")
    if len(weights) != 6:
        raise L.VtError("sifnet_loss_head: six loss weights expected")
    for t, name in ((df_h, "df_h"), (df_o, "df_o"), (parts_gt, "parts_gt"), (pca_gt, "pca_gt"), (obj_center, "obj_center"), (visibility, "visibility")):
        if _loss_dev(t, name).device != dev:
            raise L.VtError(f"sifnet_loss_head: {name} on {t.device}, the predictions on {dev}")
    if tuple(df_h.shape) != (B, N) or tuple(df_o.shape) != (B, N) or tuple(parts_gt.shape) != (B, N):
        raise L.VtError(f"sifnet_loss_head: df_h, df_o, parts_gt are ({B},{N}), got {tuple(df_h.shape)}, {tuple(df_o.shape)}, {tuple(parts_gt.shape)}")
    if validate:
        lo, hi = float(parts_gt.min()), float(parts_gt.max())
        if lo < 0 or hi > HEAD_DIMS[2] - 1:
            raise L.VtError(f"sifnet_loss_head: part labels span [{lo:g}, {hi:g}], outside [0, {HEAD_DIMS[2]})")
    frame = {"pca_gt": (pca_gt, 9), "obj_center": (obj_center, 3), "visibility": (visibility, 1)}
    kinds = {}
    for name, (t, k) in frame.items():
        if t.numel() == B * k * N and (N > 1 or t.dim() > (1 if k == 1 else 2)):
            kinds[name] = False
        elif t.numel() == B * k:
            kinds[name] = True
        else:
            raise L.VtError(f"sifnet_loss_head: {name} holds {B} x {k} x {N} values per point or {B} x {k} per frame, got {tuple(t.shape)}")
    per_frame = all(kinds.values())
    lab = []
    for name, (t, k) in frame.items():
        t = _f32(t)
        if kinds[name] and not per_frame:
            t = t.reshape(B, k, 1).expand(B, k, N)
        lab.append(t.reshape(B, k) if per_frame else t.reshape(B, k, N).contiguous())
    labels = (_f32(df_h), _f32(df_o), parts_gt.detach().to(torch.int32).contiguous(), *lab)
    error, losses_all, terms = _LossHeadFn.apply(*heads, labels, per_frame, max_dist, tuple(float(w) for w in weights), VIS_LOSSES[vis_loss])
    return (error, losses_all, terms) if want_terms else (error, losses_all)


# --------------------------------------------------------------------------------------------------
# training the point decoders, with or without the gradient to the feature maps (csrc/dectrain.hip)
# --------------------------------------------------------------------------------------------------
STATE_DICT_MODULES = {"df": "df", "pca": "pca_predictor", "parts": "part_predictor", "centers": "center_predictor", "vis": "visib_predictor"}
STATE_DICT_LAYERS = (0, 2, 4, 6)                               # the Conv1d entries of make_decoder's Sequential (chore.py:113-126)


class DecoderParams:
    """The weights and biases of the five decoders as ONE flat float32 tensor (``flat``, the leaf that requires grad: one Adam launch a step) in the layout of
    ``vt_decoder_param_offset``, plus the 40 named views into it: ``views[(head, layer, "weight" | "bias")]``, (out, in) and (out,).  The offsets come from
    the library; nothing here restates the table.  A container: it lives on any device, the kernels take it on the GPU only."""

    def __init__(self, flat, cam=DEFAULT_CAM):
        lib = L.lib()
        n = int(lib.vt_decoder_param_floats())
        if not torch.is_tensor(flat) or flat.dtype != torch.float32 or tuple(flat.shape) != (n,):
            raise L.VtError(f"DecoderParams: a float32 tensor of {n} values expected")
        self.flat = flat.detach().contiguous().requires_grad_(True)
        self.cam = _np32(cam)
        self.views, data = {}, self.flat.detach()
        for h, (name, k) in enumerate(zip(HEADS, HEAD_DIMS)):
            for l in range(4):
                shape = (k if l == 3 else 128, MAP_CHANNELS_TOTAL if l == 0 else 128)
                ow, ob = int(lib.vt_decoder_param_offset(h, l, 0)), int(lib.vt_decoder_param_offset(h, l, 1))
                self.views[(name, l, "weight")] = data[ow:ow + shape[0] * shape[1]].view(shape)
                self.views[(name, l, "bias")] = data[ob:ob + shape[0]]
        if sum(v.numel() for v in self.views.values()) != n:
            raise L.VtError("DecoderParams: the library's offsets do not tile the parameter buffer")

    @classmethod
    def from_decoders(cls, decoders: dict, cam=DEFAULT_CAM, device="cuda:0"):
        """from the host form ``SIFNetQuery.decoders_from_state_dict`` produces: name -> four (weight (out,in), bias (out,)) pairs"""
        p = cls(torch.zeros(int(L.lib().vt_decoder_param_floats())), cam)
        for name in HEADS:
            if len(decoders[name]) != 4:
                raise L.VtError(f"DecoderParams: {name} has {len(decoders[name])} layers, 4 expected")
            for l, (w, b) in enumerate(decoders[name]):
                for kind, a in (("weight", w), ("bias", b)):
                    v = p.views[(name, l, kind)]
                    a = torch.as_tensor(_np32(a))
                    if tuple(a.shape) != tuple(v.shape):
                        raise L.VtError(f"DecoderParams: {name} layer {l} {kind} is {tuple(v.shape)}, got {tuple(a.shape)}")
                    v.copy_(a)
        return cls(p.flat.detach().to(device), cam)

    def to_decoders(self) -> dict:
        """-> the host form (numpy), what ``SIFNetQuery`` and ``SifNetHandle`` take"""
        host = DecoderParams(self.flat.detach().cpu(), self.cam)
        return {name: [(host.views[(name, l, "weight")].numpy().copy(), host.views[(name, l, "bias")].numpy().copy()) for l in range(4)] for name in HEADS}

    def state_dict(self, prefix: str = "") -> dict:
        """the reference's keys and Conv1d shapes: ``df.0.weight`` (128, 611, 1), ``df.0.bias`` (128,), ... ``visib_predictor.6.bias`` (1,); copies"""
        out = {}
        for name in HEADS:
            for l, i in enumerate(STATE_DICT_LAYERS):
                out[f"{prefix}{STATE_DICT_MODULES[name]}.{i}.weight"] = self.views[(name, l, "weight")].clone().unsqueeze(-1)
                out[f"{prefix}{STATE_DICT_MODULES[name]}.{i}.bias"] = self.views[(name, l, "bias")].clone()
        return out

    def load_state_dict(self, sd: dict):
        """in place, from the reference's keys with or without the ``module.`` prefix (other keys, the encoder's, are ignored); a missing key raises"""
        with torch.no_grad():
            for name in HEADS:
                for l, i in enumerate(STATE_DICT_LAYERS):
                    for kind in ("weight", "bias"):
                        key = f"{STATE_DICT_MODULES[name]}.{i}.{kind}"
                        t = sd.get(key, sd.get("module." + key))
                        if t is None:
                            raise KeyError(key)
                        v = self.views[(name, l, kind)]
                        t = torch.as_tensor(t, dtype=torch.float32)
                        if t.numel() != v.numel():
                            raise L.VtError(f"DecoderParams.load_state_dict: {key} holds {v.numel()} values, got {tuple(t.shape)}")
                        v.copy_(t.reshape(v.shape))
        return self


MAP_CHANNELS_TOTAL = sum(MAP_CHANNELS) + 3                     # 611: the eight maps and z_feat


def _train_maps(maps):
    maps = [maps] if isinstance(maps, FeatureMaps) else list(maps)
    if not maps or not all(isinstance(m, FeatureMaps) for m in maps):
        raise L.VtError("sifnet_query_train: maps is a FeatureMaps or a list of them, one per stack")
    return maps


class _QueryTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flat, cam, maps, pts, cc, bc, chunk_points, *map_tensors):
        # map_tensors: the 8 S tensors of ``maps`` in stack order, here only so that autograd sees them as inputs; the kernels read them through maps[s].c
        B, N = pts.shape[:2]
        outs = []
        with torch.cuda.device(flat.device):
            for m in maps:
                o = [torch.empty(B, k, N, device=flat.device) for k in HEAD_DIMS]
                L.check(L.lib().vt_decoder_train_forward(L.dptr(flat), cam.ctypes.data, C.byref(m.c), L.dptr(pts), L.dptr(cc), L.dptr(bc), B, N,
                                                         *[L.dptr(t) for t in o], L.stream_ptr()))
                outs += o
        ctx.cam, ctx.maps, ctx.chunk = cam, maps, chunk_points
        ctx.set_materialize_grads(False)                       # a prediction the objective does not use arrives as None -> NULL: its head costs nothing
        ctx.save_for_backward(flat, pts, cc, bc)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        flat, pts, cc, bc = ctx.saved_tensors
        B, N = pts.shape[:2]
        want_w, want_m = ctx.needs_input_grad[0], ctx.needs_input_grad[7:]
        lib = L.lib()
        with torch.cuda.device(flat.device):
            dflat = torch.empty_like(flat) if want_w else None
            dmaps = [None] * len(want_m)
            if not any(want_m):                                # the maps are data: the weight-gradient entry, as before
                ws = torch.empty(int(lib.vt_decoder_weight_grads_ws_bytes(B, N, ctx.chunk)) // 4 + 4, device=flat.device)
            else:
                ws = torch.empty(int(lib.vt_decoder_grads_ws_bytes(B, N, ctx.chunk, 1)) // 4 + 4, device=flat.device)
            for s, m in enumerate(ctx.maps):
                g = [None if t is None else _f32(t) for t in gs[5 * s:5 * s + 5]]
                if not any(want_m):
                    if want_w:
                        L.check(lib.vt_decoder_weight_grads(L.dptr(flat), ctx.cam.ctypes.data, C.byref(m.c), L.dptr(pts), L.dptr(cc), L.dptr(bc), B, N,
                                                            *[L.dptr(t) for t in g], L.dptr(dflat), 1 if s else 0, int(ctx.chunk), L.dptr(ws), L.stream_ptr()))
                    continue
                # weights and maps of the stack from ONE call: the tape is built once.  A tensor two stacks share gets one buffer per stack; autograd adds them.
                dm = L.VtMaps()
                for i, t in enumerate(m.t):
                    dm.res[i] = t.shape[1]
                    if want_m[8 * s + i]:
                        dmaps[8 * s + i] = torch.empty_like(t)
                        dm.maps[i] = dmaps[8 * s + i].data_ptr()
                if not want_w and not any(want_m[8 * s:8 * s + 8]):
                    continue
                L.check(lib.vt_decoder_grads(L.dptr(flat), ctx.cam.ctypes.data, C.byref(m.c), L.dptr(pts), L.dptr(cc), L.dptr(bc), B, N,
                                             *[L.dptr(t) for t in g], L.dptr(dflat), 1 if s else 0, C.byref(dm), 0, int(ctx.chunk), L.dptr(ws), L.stream_ptr()))
        return (dflat, None, None, None, None, None, None, *dmaps)


def sifnet_query_train(params: DecoderParams, maps, pts, crop_center, body_center, chunk_points=0, train_decoders=True):
    """The query of a training step (chore_triplane.py:97-164 in train mode) from the plain weights of ``params``: ``maps`` is one ``FeatureMaps`` or a list of
    S, one per hourglass stack (they share their tmpx tensors, chore_triplane.py:139-149).  -> a list of S (df (B,2,N), pca (B,3,3,N), parts (B,14,N), centers
    (B,3,N), vis (B,1,N)) tuples, the shape of ``intermediate_preds_list``.  Backward: one call per stack, into ONE flat gradient (``params.flat.grad``) and into
    ``t.grad`` of every map tensor that requires grad (NHWC, as the tensor; a tensor two stacks share receives the sum) -- the gradient an encoder's backward
    continues from.  With no map requiring grad the call is vt_decoder_weight_grads, otherwise vt_decoder_grads (weights and maps from one tape).
    ``train_decoders=False``: the decoders are data, only the maps receive a gradient.  The points are data here: one that requires grad raises."""
    maps = _train_maps(maps)
    if not isinstance(params, DecoderParams):
        raise L.VtError("sifnet_query_train: params is an ops.DecoderParams")
    for t, name in ((pts, "points"), (crop_center, "crop_center"), (body_center, "body_center")):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise L.VtError(f"sifnet_query_train: {name} must be a device tensor; there is no CPU path")
    if pts.requires_grad:
        raise L.VtError("sifnet_query_train: the points are data here (no gradient flows to them); detach them, or use sifnet_query for the gradient to the points")
    pts, cc, bc = _f32(pts), _f32(crop_center), _f32(body_center)
    B, N = pts.shape[:2]
    if pts.dim() != 3 or pts.shape[2] != 3 or tuple(cc.shape) != (B, 2) or tuple(bc.shape) != (B, 3) or any(m.B != B for m in maps):
        raise L.VtError(f"sifnet_query_train: points (B,N,3), crop_center (B,2), body_center (B,3), maps of B frames; got {tuple(pts.shape)}, {tuple(cc.shape)}, "
                        f"{tuple(bc.shape)}, {[m.B for m in maps]}")
    flat = params.flat if train_decoders else params.flat.detach()
    outs = _QueryTrainFn.apply(flat, params.cam, maps, pts, cc, bc, int(chunk_points), *[t for m in maps for t in m.t])
    return [(outs[5 * s], outs[5 * s + 1].view(B, 3, 3, N), outs[5 * s + 2], outs[5 * s + 3], outs[5 * s + 4]) for s in range(len(maps))]


# --------------------------------------------------------------------------------------------------
# a trainable ConvBlock of the encoders (model/net_util.py:346-396)
# --------------------------------------------------------------------------------------------------
CONV_BLOCK_PARAMS = ("w1", "w2", "w3", "gamma1", "gamma2", "gamma3", "beta1", "beta2", "beta3", "wproj", "gamma4", "beta4")
# flat argument order of vt_conv_block_backward (include/vistracker.h); tests/test_host_convblock.py holds it against _lib.SIGNATURES
CONV_BLOCK_BACKWARD_ARGS = (("dy", "x", "raw", "stats1", "stats2", "stats3") + CONV_BLOCK_PARAMS + ("B", "H", "W", "cin", "c1", "c2", "c3")
                            + ("d_x", "dW1", "dW2", "dW3", "dgamma1", "dbeta1", "dgamma2", "dbeta2", "dgamma3", "dbeta3", "dgamma4", "dbeta4", "dWproj")
                            + ("workspace", "accumulate", "stream"))


def conv_block_backward_raw(dy, x, raw, stats, params, want=None, out=None, accumulate=0, ws=None):
    """one vt_conv_block_backward call.  dy / x / raw: channels-last (B,C,H,W) device tensors; stats: the three {mean, rstd} workspaces; params: dict over
    CONV_BLOCK_PARAMS (wproj / gamma4 / beta4 None without a projection); ``want``: names of the outputs to compute (default: all that exist); ``out``: dict of
    preallocated outputs by name (accumulate != 0 adds onto the parameter gradients in them).  -> dict name -> tensor"""
    lib = L.lib()
    B, cin, H, W = x.shape
    c1, c2, c3 = (int(params[k].shape[0]) for k in ("w1", "w2", "w3"))
    proj = params.get("wproj") is not None
    names = ["d_x", "dW1", "dW2", "dW3", "dgamma1", "dbeta1", "dgamma2", "dbeta2", "dgamma3", "dbeta3"] + (["dgamma4", "dbeta4", "dWproj"] if proj else [])
    like = {"d_x": x, "dW1": params["w1"], "dW2": params["w2"], "dW3": params["w3"], "dWproj": params.get("wproj")}
    for i in "1234":
        like["dgamma" + i] = like["dbeta" + i] = params.get("gamma" + i)
    want = names if want is None else [n for n in names if n in want]
    res = dict(out or {})
    for n in want:
        if n not in res:
            res[n] = torch.empty_like(like[n], memory_format=torch.channels_last if n == "d_x" else torch.contiguous_format)
    if ws is None:
        nbytes = int(lib.vt_conv_block_backward_workspace(B, H, W, cin, c1, c2, c3))
        if nbytes < 0:
            raise L.VtError(f"conv_block_backward: unsupported block shape B={B} H={H} W={W} {cin}->({c1},{c2},{c3})")
        ws = torch.empty(nbytes // 4 + 4, device=x.device)
    ptr = lambda t: None if t is None else t.data_ptr()         # noqa: E731
    order = ("d_x", "dW1", "dW2", "dW3", "dgamma1", "dbeta1", "dgamma2", "dbeta2", "dgamma3", "dbeta3", "dgamma4", "dbeta4", "dWproj")
    with torch.cuda.device(x.device):
        L.check(lib.vt_conv_block_backward(dy.data_ptr(), x.data_ptr(), raw.data_ptr(), *[s.data_ptr() for s in stats], *[ptr(params.get(k)) for k in CONV_BLOCK_PARAMS],
                                           B, H, W, cin, c1, c2, c3, *[ptr(res.get(n)) if n in want else None for n in order],
                                           ws.data_ptr(), int(accumulate), L.stream_ptr()))
    return res


class _ConvBlockTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, blk, x, *tensors):
        # the fused block of encoder_fwd, keeping what the backward reads: x, raw = o1 | o2 and the three {mean, rstd} areas
        p = dict(zip(CONV_BLOCK_PARAMS, tensors))
        couts = [int(p[k].shape[0]) for k in ("w1", "w2", "w3")]
        with torch.cuda.device(x.device):
            h3, h1 = blk.handles(x.device)
            ws = fwd.input_stats(x, True)           # left behind by the producer of x (a previous block), else one pass
            res = x if h1 is None else fwd.conv1x1(h1, x, sum(couts), gn=(ws, p["gamma4"], p["beta4"]))[0]
            fin, raw, stats, ws_fin = fwd.conv_block(h3, [p[f"gamma{i}"] for i in (1, 2, 3)], [p[f"beta{i}"] for i in (1, 2, 3)], x, ws, res, couts, True)
        ctx.save_for_backward(x, raw, *stats, *[t for t in tensors if t is not None])
        ctx.present = [t is not None for t in tensors]
        ctx.mark_non_differentiable(ws_fin)
        return fin, ws_fin

    @staticmethod
    def backward(ctx, dy, _):
        sv = ctx.saved_tensors
        x, raw, stats = sv[0], sv[1], sv[2:5]
        it = iter(sv[5:])
        p = {k: (next(it) if have else None) for k, have in zip(CONV_BLOCK_PARAMS, ctx.present)}
        need = dict(zip(("d_x",) + CONV_BLOCK_PARAMS, ctx.needs_input_grad[1:]))
        gname = {"d_x": "d_x", "w1": "dW1", "w2": "dW2", "w3": "dW3", "wproj": "dWproj"}
        for i in "1234":
            gname["gamma" + i], gname["beta" + i] = "dgamma" + i, "dbeta" + i
        want = [gname[k] for k, n in need.items() if n and (k == "d_x" or p[k] is not None)]
        dy = dy.float().contiguous(memory_format=torch.channels_last)
        g = conv_block_backward_raw(dy, x, raw, stats, p, want=want)
        return (None, g.get("d_x"), *[g.get(gname[k]) if need[k] and p[k] is not None else None for k in CONV_BLOCK_PARAMS])


def conv_block_train(x, params):
    """A ConvBlock (model/net_util.py:346-396) that a torch graph can contain.  ``x``: (B,Cin,H,W) device tensor (kept channels-last); ``params``: an
    ``encoder.TrainableConvBlock`` (its leaves ``tensors()`` in CONV_BLOCK_PARAMS order and the packed forward handles ``handles(device)``).  Forward:
    exactly the fused inference forward (``encoder_fwd.conv_block``, the launches ``HGFilterEncoder._conv_block_fused`` issues); backward: one ``vt_conv_block_backward`` call, a gradient for
    every input that requires one.  The result carries the GroupNorm partial sums of itself for a block that reads it next, as the inference path does."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4):
        raise L.VtError("conv_block_train: x must be a (B,C,H,W) device tensor; there is no CPU path")
    B, Cin, H, W = x.shape
    tensors = params.tensors()
    couts = [int(tensors[i].shape[0]) for i in range(3)]
    if int(L.lib().vt_conv_block_backward_workspace(B, H, W, Cin, *couts)) < 0 or int(tensors[0].shape[1]) != Cin or (tensors[9] is None) != (Cin == sum(couts)):
        raise L.VtError(f"conv_block_train: block {Cin}->{couts} at {H}x{W} is not served (H % 8 == 0, W % 16 == 0, widths in {{32, 64, 128}}, Cin % 32 == 0 up to 256)")
    xc = x if x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last) else fwd.carry_stats(x, x.float().contiguous(memory_format=torch.channels_last))
    fin, ws_fin = _ConvBlockTrainFn.apply(params, xc, *tensors)
    return fwd.attach_stats(fin, ws_fin, int(L.lib().vt_conv3x3_tiles(H, W)))


# --------------------------------------------------------------------------------------------------
# the two operators that join the ConvBlocks of an hourglass (model/HGFilters.py:26-50), trainable
# --------------------------------------------------------------------------------------------------
def _resample_arg(what, t):
    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 4):
        raise L.VtError(f"{what}: needs a (B,C,H,W) device tensor; there is no CPU path")
    return t if t.dtype == torch.float32 and t.is_contiguous(memory_format=torch.channels_last) else t.float().contiguous(memory_format=torch.channels_last)


def avgpool2x2_backward(d_out):
    """one vt_avgpool2x2_backward call: d_out (B,C,H/2,W/2) channels-last -> d_x (B,C,H,W) = 0.25 d_out at [y/2, x/2] (F.avg_pool2d(x, 2, stride=2) backward)"""
    d = _resample_arg("avgpool2x2_backward", d_out)
    B, C, h, w = d.shape
    d_x = torch.empty(B, C, 2 * h, 2 * w, device=d.device, memory_format=torch.channels_last)
    with torch.cuda.device(d.device):
        L.check(L.lib().vt_avgpool2x2_backward(d.data_ptr(), B, 2 * h, 2 * w, C, d_x.data_ptr(), L.stream_ptr()))
    return d_x


def upsample2x_bicubic_backward(d_out):
    """one vt_upsample2x_bicubic_backward call: d_out (B,C,2h,2w) channels-last -> d_low (B,C,h,w), the transpose of the forward's bicubic x2 operator
    (F.interpolate(low, scale_factor=2, mode='bicubic', align_corners=True) backward)"""
    d = _resample_arg("upsample2x_bicubic_backward", d_out)
    B, C, H, W = d.shape
    if H % 2 or W % 2:
        raise L.VtError(f"upsample2x_bicubic_backward: d_out is {H}x{W}, not twice a size")
    d_low = torch.empty(B, C, H // 2, W // 2, device=d.device, memory_format=torch.channels_last)
    with torch.cuda.device(d.device):
        L.check(L.lib().vt_upsample2x_bicubic_backward(d.data_ptr(), B, H // 2, W // 2, C, d_low.data_ptr(), L.stream_ptr()))
    return d_low


class _AvgPoolTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        with torch.cuda.device(x.device):
            out = fwd.avgpool2x2_stats(x)
        ws, _ = fwd.partials_of(out)
        ctx.mark_non_differentiable(ws)
        return out, ws

    @staticmethod
    def backward(ctx, dy, _):
        return avgpool2x2_backward(dy)


class _UpsampleAddTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, low, skip):
        with torch.cuda.device(low.device):
            out = fwd.upsample2x_bicubic_add_stats(low, skip)
        ws, _ = fwd.partials_of(out)
        ctx.mark_non_differentiable(ws)
        return out, ws

    @staticmethod
    def backward(ctx, dy, _):
        # out = skip + U low: the gradient to skip is dy itself, to low U^T dy
        return (upsample2x_bicubic_backward(dy) if ctx.needs_input_grad[0] else None), (dy if ctx.needs_input_grad[1] else None)


def avgpool2x2_train(x):
    """``F.avg_pool2d(x, 2, stride=2)`` that a torch graph can contain.  Forward: the inference launch (``encoder_fwd.avgpool2x2_stats``) bit for
    bit, the result carrying the GroupNorm partial sums of itself for the block that reads it next; backward: one ``vt_avgpool2x2_backward`` call."""
    xc = _resample_arg("avgpool2x2_train", x)
    B, C, H, W = xc.shape
    if C % 32 or C > 1024 or H % 2 or W % 2 or H < 2 or W < 2:
        raise L.VtError(f"avgpool2x2_train: {C} channels at {H}x{W} is not served (C % 32 == 0 up to 1024, even H and W)")
    out, ws = _AvgPoolTrainFn.apply(xc)
    return fwd.attach_stats(out, ws, int(L.lib().vt_sweep_blocks((H // 2) * (W // 2))))


def upsample2x_bicubic_add_train(low, skip):
    """``skip + F.interpolate(low, scale_factor=2, mode='bicubic', align_corners=True)`` that a torch graph can contain.  Forward: the inference launch
    (``encoder_fwd.upsample2x_bicubic_add_stats``) bit for bit, with the GroupNorm partial sums of the result attached; backward: one
    ``vt_upsample2x_bicubic_backward`` call for ``low``, the upstream gradient itself for ``skip``."""
    lc, sc = _resample_arg("upsample2x_bicubic_add_train", low), _resample_arg("upsample2x_bicubic_add_train", skip)
    B, C, h, w = lc.shape
    if tuple(sc.shape) != (B, C, 2 * h, 2 * w) or sc.device != lc.device:
        raise L.VtError(f"upsample2x_bicubic_add_train: low {tuple(lc.shape)} and skip {tuple(sc.shape)} do not fit (skip is twice the size, same device)")
    if C % 32 or C > 1024:
        raise L.VtError(f"upsample2x_bicubic_add_train: {C} channels is not served (C % 32 == 0 up to 1024)")
    out, ws = _UpsampleAddTrainFn.apply(lc, sc)
    return fwd.attach_stats(out, ws, int(L.lib().vt_sweep_blocks(4 * h * w)))


# --------------------------------------------------------------------------------------------------
# the stem and the 1 x 1 tail of a stack (model/HGFilters.py:120-125, 167 and 191-201), trainable
# --------------------------------------------------------------------------------------------------
STEM_PARAMS = ("conv1.weight", "conv1.bias", "bn1.weight", "bn1.bias")
STACK_TAIL_PARAMS = ("conv_last.weight", "conv_last.bias", "bn_end.weight", "bn_end.bias", "l.weight", "l.bias", "bl.weight", "bl.bias", "al.weight", "al.bias")
# outputs of vt_stack_tail_backward in argument order, and the parameter each one is the gradient of
STACK_TAIL_GRADS = ("d_ll", "dWcl", "dbcl", "dgamma", "dbeta", "dWl", "dbl", "dWbl", "dbbl", "dWal", "dbal")
_TAIL_GRAD_OF = dict(zip(("conv_last.weight", "conv_last.bias", "bn_end.weight", "bn_end.bias", "l.weight", "l.bias", "bl.weight", "bl.bias", "al.weight", "al.bias"),
                         STACK_TAIL_GRADS[1:]))


def _ws(nbytes, device, what):
    if nbytes < 0:
        raise L.VtError(f"{what}: unsupported shape")
    return torch.empty(int(nbytes) // 4 + 4, device=device)


def bias_grad(d_out, C=None, coff=0, out=None, accumulate=0):
    """one vt_bias_grad call: db[c] = sum over (b, pixel) of channels [coff, coff + C) of the channels-last (B,Ct,H,W) tensor d_out"""
    d = _resample_arg("bias_grad", d_out)
    B, Ct, H, W = d.shape
    C = Ct - coff if C is None else int(C)
    db = torch.empty(C, device=d.device) if out is None else out
    with torch.cuda.device(d.device):
        ws = _ws(L.lib().vt_bias_grad_workspace_bytes(B, H * W, C), d.device, f"bias_grad: {C} channels at {H}x{W}")
        L.check(L.lib().vt_bias_grad(d.data_ptr(), Ct, int(coff), B, H * W, C, db.data_ptr(), int(accumulate), ws.data_ptr(), L.stream_ptr()))
    return db


def stem7x7_wgrad(d_y, x, out=None, accumulate=0):
    """one vt_stem7x7_wgrad call: d_y (B,Cout,H2,W2) and x (B,Cin,H,W) channels-last -> dW (Cout,Cin,7,7) of conv1 = Conv2d(Cin, Cout, 7, stride 2, padding 3)"""
    d, xc = _resample_arg("stem7x7_wgrad", d_y), _resample_arg("stem7x7_wgrad", x)
    B, cin, H, W = xc.shape
    cout = d.shape[1]
    if tuple(d.shape) != (B, cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1):
        raise L.VtError(f"stem7x7_wgrad: d_y {tuple(d.shape)} does not belong to an input {tuple(xc.shape)}")
    dW = torch.empty(cout, cin, 7, 7, device=d.device) if out is None else out
    with torch.cuda.device(d.device):
        ws = _ws(L.lib().vt_stem7x7_wgrad_workspace_bytes(B, H, W, cin, cout), d.device, f"stem7x7_wgrad: {cin}->{cout} at {H}x{W}")
        L.check(L.lib().vt_stem7x7_wgrad(d.data_ptr(), cout, 0, xc.data_ptr(), cin, 0, B, H, W, cin, cout, dW.data_ptr(), int(accumulate), ws.data_ptr(), L.stream_ptr()))
    return dW


def gn_relu_backward_y(g, x_in, y, stats, gamma, groups=32, want_dx=True, accumulate=0, dgamma=None, dbeta=None):
    """one vt_gn_relu_backward_y call: the backward of y = ReLU(GroupNorm(x_in)) with the mask read from the saved y.  g, x_in, y channels-last (B,C,H,W);
    stats the {mean, rstd} area the forward left.  -> (d_x or None, dgamma, dbeta)"""
    gc, xc, yc = (_resample_arg("gn_relu_backward_y", t) for t in (g, x_in, y))
    B, C, H, W = xc.shape
    d_x = torch.empty_like(xc, memory_format=torch.channels_last) if want_dx else None
    dgamma = torch.empty(C, device=xc.device) if dgamma is None else dgamma
    dbeta = torch.empty(C, device=xc.device) if dbeta is None else dbeta
    with torch.cuda.device(xc.device):
        ws = _ws(L.lib().vt_gn_relu_backward_workspace_bytes(B, H * W, C, groups), xc.device, f"gn_relu_backward_y: {C} channels in {groups} groups")
        L.check(L.lib().vt_gn_relu_backward_y(gc.data_ptr(), C, 0, xc.data_ptr(), C, 0, yc.data_ptr(), C, 0, stats.data_ptr(), gamma.data_ptr(), groups, B, H * W, C,
                                              None, 0, 0, d_x.data_ptr() if want_dx else None, C, 0, dgamma.data_ptr(), dbeta.data_ptr(), int(accumulate),
                                              ws.data_ptr(), L.stream_ptr()))
    return d_x, dgamma, dbeta


def stack_tail_backward_raw(d_out, d_prev, ll, raw, out, stats, params, want=None, res=None, accumulate=0):
    """one vt_stack_tail_backward call.  d_out (B,Co,H,W) / d_prev (B,C,H,W) or None; ll, raw, out the forward's tensors (channels-last); stats the {mean, rstd}
    area of bn_end; params: dict over STACK_TAIL_PARAMS (the bl / al entries None on the last stack); ``want``: names out of STACK_TAIL_GRADS (default: all that
    exist); ``res``: preallocated outputs by name (accumulate != 0 adds onto the parameter gradients in them).  -> dict name -> tensor"""
    lib = L.lib()
    B, C, H, W = ll.shape
    Co = int(params["l.weight"].shape[0])
    mid = d_prev is not None
    names = [n for n in STACK_TAIL_GRADS if mid or n not in ("dWbl", "dbbl", "dWal", "dbal")]
    want = names if want is None else [n for n in names if n in want]
    like = {"d_ll": ll}
    like.update({g: params.get(k) for k, g in _TAIL_GRAD_OF.items()})
    got = dict(res or {})
    for n in want:
        if n not in got:
            got[n] = torch.empty_like(like[n], memory_format=torch.channels_last if n == "d_ll" else torch.contiguous_format)
    ptr = lambda t: None if t is None else t.data_ptr()         # noqa: E731
    with torch.cuda.device(ll.device):
        ws = _ws(lib.vt_stack_tail_backward_workspace(B, H, W, C, Co), ll.device, f"stack_tail_backward: {C} / {Co} channels at {H}x{W}")
        L.check(lib.vt_stack_tail_backward(ptr(d_out), ptr(d_prev), ll.data_ptr(), raw.data_ptr(), ptr(out), stats.data_ptr(),
                                           *[ptr(params.get(k)) for k in ("conv_last.weight", "bn_end.weight", "bn_end.bias", "l.weight", "bl.weight", "al.weight")],
                                           B, H, W, C, Co, *[ptr(got.get(n)) if n in want else None for n in STACK_TAIL_GRADS], ws.data_ptr(), int(accumulate), L.stream_ptr()))
    return {n: got[n] for n in want}


class _StemTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, x, w, b, gamma, beta):
        # stem + GroupNorm / ReLU of encoder_fwd, keeping what the backward reads: x, conv1's output, tmpx, the {mean, rstd} area
        with torch.cuda.device(x.device):
            y1 = fwd.stem(mod.handles(x.device), x, int(w.shape[0]))
            y, ws = fwd.groupnorm_relu(y1, gamma, beta)
        ctx.save_for_backward(x, y1, y, ws, gamma)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y1, y, ws, gamma = ctx.saved_tensors
        need = ctx.needs_input_grad[2:]
        if not any(need):
            return (None,) * 6
        dy = dy.float().contiguous(memory_format=torch.channels_last)
        d_y1, dgamma, dbeta = gn_relu_backward_y(dy, y1, y, ws, gamma, 32, want_dx=need[0] or need[1])
        dW = stem7x7_wgrad(d_y1, x) if need[0] else None
        db = bias_grad(d_y1) if need[1] else None
        return None, None, dW, db, (dgamma if need[2] else None), (dbeta if need[3] else None)


def stem_train(x, module):
    """``F.relu(bn1(conv1(x)))`` (model/HGFilters.py:167) that a torch graph can contain.  ``x``: (B,Cin,H,W) device tensor; ``module``: an
    ``encoder.TrainableStem`` (its leaves ``tensors()`` in STEM_PARAMS order and the packed forward handle ``handles(device)``).  Forward: exactly the launches of
    the inference encoder (``encoder_fwd.stem`` + ``groupnorm_relu``); backward: vt_gn_relu_backward_y (mask from the saved output), vt_bias_grad and vt_stem7x7_wgrad.  The image
    receives no gradient."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4):
        raise L.VtError("stem_train: x must be a (B,C,H,W) device tensor; there is no CPU path")
    w, b, gamma, beta = module.tensors()
    cout, cin = int(w.shape[0]), int(w.shape[1])
    if cout not in (32, 64) or not 1 <= cin <= 8 or tuple(w.shape[2:]) != (7, 7) or x.shape[1] != cin:
        raise L.VtError(f"stem_train: a {tuple(w.shape)} stem on an input with {x.shape[1]} channels is not served (Cout in {{32, 64}}, Cin in 1..8, 7 x 7)")
    xc = x.detach().float().contiguous(memory_format=torch.channels_last)
    return _StemTrainFn.apply(module, xc, w, b, gamma, beta)


class _StackTailTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, last, ll, previous, *tensors):
        # the 1 x 1 tail of encoder_fwd (four launches, two on the last stack), keeping what the backward reads: ll, raw, out and bn_end's {mean, rstd} area
        p = dict(zip(STACK_TAIL_PARAMS, tensors))
        with torch.cuda.device(ll.device):
            raw, ws, out, prev2, ws2 = fwd.stack_tail(mod.handles(ll.device), p["bn_end.weight"], p["bn_end.bias"], ll, previous, int(p["l.weight"].shape[0]), last)
        ctx.set_materialize_grads(False)
        ctx.present = [t is not None for t in tensors]
        ctx.last = bool(last)
        ctx.save_for_backward(ll, raw, out, ws, *[t for t in tensors if t is not None])
        if last:
            return out
        ctx.mark_non_differentiable(ws2)
        return out, prev2, ws2

    @staticmethod
    def backward(ctx, *gs):
        sv = ctx.saved_tensors
        ll, raw, out, ws = sv[:4]
        it = iter(sv[4:])
        p = {k: (next(it) if have else None) for k, have in zip(STACK_TAIL_PARAMS, ctx.present)}
        d_out = gs[0]
        d_prev = None if ctx.last else gs[1]
        nothing = (None,) * (4 + len(STACK_TAIL_PARAMS))
        if d_out is None and d_prev is None:
            return nothing
        cl = lambda t: None if t is None else t.float().contiguous(memory_format=torch.channels_last)       # noqa: E731
        d_out, d_prev = cl(d_out), cl(d_prev)
        need = ctx.needs_input_grad
        want = (["d_ll"] if need[2] else []) + [_TAIL_GRAD_OF[k] for k, n in zip(STACK_TAIL_PARAMS, need[4:]) if n and p[k] is not None]
        g = stack_tail_backward_raw(d_out, d_prev, ll, raw, out, ws, p, want=want)
        # previous' = previous + ...: the gradient to `previous` is d_prev itself
        return (None, None, g.get("d_ll"), d_prev if (not ctx.last and need[3]) else None, *[g.get(_TAIL_GRAD_OF[k]) for k in STACK_TAIL_PARAMS])


def stack_tail_train(ll, previous, module, last):
    """The tail of one stack (model/HGFilters.py:191-201) that a torch graph can contain: ``ll`` (B,C,H,W) the output of top_m, ``previous`` the stack's input
    (ignored when ``last``), ``module`` an ``encoder.TrainableStackTail``.  -> ``out`` when ``last``, else ``(out, previous')`` with the GroupNorm statistics of
    previous' attached for the next stack's first block.  Forward: exactly the four (two) launches of the inference tail (``encoder_fwd.stack_tail``); backward: one
    ``vt_stack_tail_backward`` call, an absent upstream gradient passed as NULL."""
    if not (torch.is_tensor(ll) and ll.is_cuda and ll.dim() == 4):
        raise L.VtError("stack_tail_train: ll must be a (B,C,H,W) device tensor; there is no CPU path")
    tensors = module.tensors()
    B, C, H, W = ll.shape
    Co = int(tensors[4].shape[0])
    if int(L.lib().vt_stack_tail_backward_workspace(B, H, W, C, Co)) < 0 or tuple(tensors[0].shape[:2]) != (C, C) or (tensors[6] is None) != bool(last):
        raise L.VtError(f"stack_tail_train: a tail of {C} / {Co} channels at {H}x{W} (last={bool(last)}) is not served (H % 8 == 0, W % 16 == 0, channels in {{64, 128, 256}}, "
                        f"bl / al exactly on the stacks before the last)")
    llc = _resample_arg("stack_tail_train", ll)
    if last:
        return _StackTailTrainFn.apply(module, True, llc, None, *tensors)
    pc = _resample_arg("stack_tail_train", previous)
    if tuple(pc.shape) != (B, C, H, W):
        raise L.VtError(f"stack_tail_train: previous {tuple(pc.shape)} does not fit ll {tuple(llc.shape)}")
    out, prev2, ws2 = _StackTailTrainFn.apply(module, False, llc, pc, *tensors)
    return out, fwd.attach_stats(prev2, ws2, int(L.lib().vt_conv3x3_tiles(H, W)), finalized=True)


# --------------------------------------------------------------------------------------------------
# silhouette
# --------------------------------------------------------------------------------------------------
class _SilFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, faces, K, size, eps):
        verts, K = _f32(verts), _f32(K); B, NV = verts.shape[:2]; NF = faces.shape[0]
        img = torch.empty(B, size, size, device=verts.device)
        fidx = torch.empty(B, size, size, dtype=torch.int32, device=verts.device)
        ws = torch.empty(L.lib().vt_sil_workspace_floats(B, NV, NF, size), device=verts.device)
        L.check(L.lib().vt_sil_forward(L.dptr(verts), B, NV, L.dptr(faces), NF, L.dptr(K), size, L.dptr(img), L.dptr(fidx), L.dptr(ws), L.stream_ptr()))
        ctx.save_for_backward(verts, faces, K, fidx, ws); ctx.size, ctx.eps = size, eps
        return img

    @staticmethod
    def backward(ctx, dimg):
        verts, faces, K, fidx, ws = ctx.saved_tensors
        B, NV = verts.shape[:2]
        dimg = _f32(dimg)
        dverts = torch.empty_like(verts)
        L.check(L.lib().vt_sil_backward(L.dptr(verts), B, NV, L.dptr(faces), faces.shape[0], L.dptr(K), ctx.size, L.dptr(fidx),
                                        L.dptr(dimg), ctx.eps, L.dptr(ws), L.dptr(dverts), L.stream_ptr()))
        return dverts, None, None, None, None


def silhouette(verts, faces, K, size=256, eps=1e-4):
    """neural_renderer silhouettes with per-frame intrinsics K (obj_pose_roi.py:77-94,191-192)."""
    return _SilFn.apply(verts, faces, K, size, eps)


# --------------------------------------------------------------------------------------------------
# network inputs from decoded frames (csrc/inputs.hip)
# --------------------------------------------------------------------------------------------------
def div255_table():
    """host (256,) float32: float32(q / 255.0), the value the host loader stores for grey level q (uint8 / 255.0 in float64, narrowed by astype)"""
    return (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)


_DIV255 = {}          # device index -> the table on that device


def _u8(t, name):
    if t.dtype != torch.uint8:
        raise L.VtError(f"{name}: uint8 expected, got {t.dtype}")
    return t


def mask_bbox(pm, om, thres=127):
    """vt_mask_bbox: pm, om (B,H,W) uint8 device tensors -> (B,4) int32 device tensor xmin, ymin, xmax, ymax (inclusive) of the pixels with
    (uint8)(pm + om) > thres; (W, H, -1, -1) for a frame without one.  ``sequence_io.masks2bbox`` for a batch."""
    B, H, W = pm.shape
    if tuple(om.shape) != (B, H, W):
        raise L.VtError(f"mask_bbox: masks of {tuple(pm.shape)} and {tuple(om.shape)}")
    p, o = L.dptr(_u8(pm, "pm")), L.dptr(_u8(om, "om"))
    box = torch.empty(B, 4, dtype=torch.int32, device=pm.device)
    L.check(L.lib().vt_mask_bbox(p, o, B, H, W, int(thres), L.dptr(box), L.stream_ptr()))
    return box


def crop_resize_compose(rgb, pm, om, corners, crop_size, out_size, out=None):
    """vt_crop_resize_compose: rgb (B,H,W,3), pm, om (B,H,W) uint8 device tensors; ``corners`` (B,4) host integers tl.x, tl.y, br.x, br.y of each frame's
    crop as ``sequence_io.crop`` rounds them.  Writes channels 0..4 of ``out`` (B,C>=5,S,S) float32 (allocated as (B,5,S,S) when None) = RGB * (person |
    object), person mask, object mask at the network size, bit for bit what ``SequenceLoader.load_crop`` computes on the host; other channels are untouched."""
    B, H, W = pm.shape
    S, cs = int(out_size), int(crop_size)
    if tuple(rgb.shape) != (B, H, W, 3) or tuple(om.shape) != (B, H, W):
        raise L.VtError(f"crop_resize_compose: rgb {tuple(rgb.shape)}, masks {tuple(pm.shape)} and {tuple(om.shape)}")
    ptrs = [L.dptr(_u8(t, n)) for t, n in ((rgb, "rgb"), (pm, "pm"), (om, "om"))]
    c = np.ascontiguousarray(corners, dtype=np.int64).reshape(-1, 4)
    ext = np.stack([c[:, 2] - c[:, 0], c[:, 3] - c[:, 1]], 1)
    if c.shape[0] != B or (ext <= 0).any() or (np.abs(ext - cs) > 1).any() or np.abs(c).max(initial=0) >= 2 ** 29:
        raise ValueError(f"crop_resize_compose: corners {c.tolist()} are not {B} crops of size {cs}")
    if out is None:
        out = torch.empty(B, 5, S, S, device=rgb.device)
    elif out.dtype != torch.float32 or out.dim() != 4 or out.shape[0] != B or out.shape[1] < 5 or tuple(out.shape[2:]) != (S, S):
        raise L.VtError(f"crop_resize_compose: out {tuple(out.shape)} {out.dtype} for {B} crops of {S} x {S}")
    dev = rgb.device.index
    if dev not in _DIV255:
        _DIV255[dev] = torch.as_tensor(div255_table(), device=rgb.device)
    cd = torch.as_tensor(c.astype(np.int32), device=rgb.device)
    L.check(L.lib().vt_crop_resize_compose(*ptrs, B, H, W, L.dptr(cd), cs, S, L.dptr(_DIV255[dev]), L.dptr(out), out.stride(0), L.stream_ptr()))
    return out


def resize_panel_u8(src, frames, H, size, col0, pw, out, out_off, out_row_stride):
    """vt_resize_panel_u8: ``src`` a uint8 device tensor holding the staged images, ``frames`` (n,6) host integers (byte offset into ``src``, h, w, first staged
    column, staged width, row stride in bytes).  Writes rows [0, H) x columns [col0, col0 + pw) of every image's bilinear H x size resize into the uint8 device
    tensor ``out`` at the byte offsets ``out_off`` (n,) -- an int64 device tensor, or host integers, which cost a small upload -- with ``out_row_stride`` bytes per row: ``sequence_io.resize_bilinear_hw(img, H, size)[:, col0:col0 + pw]``."""
    d = np.ascontiguousarray(frames, dtype=np.int64).reshape(-1, 6)
    if src.dim() == 0 or src.stride(-1) != 1 or out.device != src.device:
        raise L.VtError("resize_panel_u8: src must have packed bytes and live on out's device")
    off = torch.as_tensor(np.ascontiguousarray(out_off, dtype=np.int64).reshape(-1), device=out.device) if not torch.is_tensor(out_off) else out_off
    if off.dtype != torch.int64 or off.numel() != d.shape[0]:
        raise L.VtError(f"resize_panel_u8: {off.numel()} {off.dtype} offsets for {d.shape[0]} frames")
    L.dptr(_u8(out, "out")); L.dptr(off)                               # device and contiguity checks; src may be a strided view
    if not src.is_cuda or src.device.index != torch.cuda.current_device():
        raise L.VtError("resize_panel_u8: src must be a tensor of the current device; there is no CPU route")
    span = 1 + sum((n - 1) * st for n, st in zip(src.shape, src.stride()))          # bytes from src's first to its last element
    L.check(L.lib().vt_resize_panel_u8(_u8(src, "src").data_ptr(), span, d.ctypes.data, d.shape[0], int(H), int(size), int(col0), int(pw), out.data_ptr(),
                                       off.data_ptr(), int(out_row_stride), L.stream_ptr()))
    return out


# --------------------------------------------------------------------------------------------------
# the fit on the camera image, and its score on the masks (csrc/overlay.hip)
# --------------------------------------------------------------------------------------------------
def _offsets(off, n, device, name):
    off = torch.as_tensor(np.ascontiguousarray(off, dtype=np.int64).reshape(-1), device=device) if not torch.is_tensor(off) else off
    if off.dtype != torch.int64 or off.numel() != n:
        raise L.VtError(f"{name}: {off.numel()} {off.dtype} offsets for {n} views")
    return off


def overlay_panel_u8(rgb, alpha, out, src_off, dst_off, row0, nrows, col0, ncols, out_row_stride, opacity):
    """vt_overlay_panel_u8: rgb (B,S,S,3), alpha (B,S,S) of a render without a static layer over background 0; view b's crop rows [row0, row0 + nrows) x columns
    [col0, col0 + ncols) is composited at ``opacity`` over the uint8 panel at byte offset ``src_off[b]`` of the device tensor ``out`` and written at ``dst_off[b]``
    (int64 device tensors, or host integers, which cost a small upload; equal offsets = in place), rows ``out_row_stride`` bytes apart."""
    B, S = rgb.shape[0], rgb.shape[1]
    if tuple(rgb.shape) != (B, S, S, 3) or tuple(alpha.shape) != (B, S, S) or rgb.dtype != torch.float32 or alpha.dtype != torch.float32:
        raise L.VtError(f"overlay_panel_u8: rgb {tuple(rgb.shape)} {rgb.dtype}, alpha {tuple(alpha.shape)} {alpha.dtype}")
    so, do = _offsets(src_off, B, rgb.device, "overlay_panel_u8"), _offsets(dst_off, B, rgb.device, "overlay_panel_u8")
    L.check(L.lib().vt_overlay_panel_u8(L.dptr(rgb), L.dptr(alpha), B, S, int(row0), int(nrows), int(col0), int(ncols), L.dptr(_u8(out, "out")), L.dptr(so),
                                        L.dptr(do), int(out_row_stride), float(opacity), L.stream_ptr()))
    return out


def _span(t):
    """bytes from a uint8 tensor's first to its last element"""
    return 1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride()))


def mask_score(fidx, rows, F, nf_body, nf_obj, pm, om, frames, thres=127, count=None):
    """vt_mask_score: fidx (B,is,is) int32 owner maps of a render without a static layer over ``F`` faces (the first ``nf_body`` body, the next ``nf_obj`` object);
    ``pm`` / ``om`` uint8 device tensors holding the person / object masks (may be the same tensor, may be strided views), ``frames`` (B,8) host integers per view:
    byte offset of the person mask in ``pm``, of the object mask in ``om``, h, w, pixel and row stride of the person mask, of the object mask.  Scores raster rows
    [0, rows).  -> count (B,2,4) int32 device tensor (written into ``count`` when given): per class (body against pm, object against om) inter, fit, mask, hidden."""
    B, s = fidx.shape[0], fidx.shape[1]
    d = np.ascontiguousarray(frames, dtype=np.int64).reshape(-1, 8)
    if fidx.dim() != 3 or fidx.shape[2] != s or fidx.dtype != torch.int32 or d.shape[0] != B:
        raise L.VtError(f"mask_score: fidx {tuple(fidx.shape)} {fidx.dtype} with {d.shape[0]} mask descriptors")
    for m, name in ((pm, "pm"), (om, "om")):
        if not m.is_cuda or m.device != fidx.device or m.device.index != torch.cuda.current_device() or m.numel() == 0:
            raise L.VtError(f"mask_score: {name} must be a non-empty tensor of fidx's (the current) device; there is no CPU route")
        _u8(m, name)
    if count is None:
        count = torch.empty(B, 2, 4, dtype=torch.int32, device=fidx.device)
    elif count.dtype != torch.int32 or tuple(count.shape) != (B, 2, 4):
        raise L.VtError(f"mask_score: count {tuple(count.shape)} {count.dtype} for {B} views")
    L.check(L.lib().vt_mask_score(L.dptr(fidx), B, s, int(rows), int(F), int(nf_body), int(nf_obj), pm.data_ptr(), _span(pm), om.data_ptr(), _span(om),
                                  d.ctypes.data, int(thres), L.dptr(count), L.stream_ptr()))
    return count


# --------------------------------------------------------------------------------------------------
# Adam
# --------------------------------------------------------------------------------------------------
class FusedAdam:
    """torch.optim.Adam semantics (defaults) with one HIP launch per parameter tensor and an optional
    device-side stop flag (no host synchronisation inside the fit loop)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, stop_flag=None):
        if isinstance(params[0], dict):
            self.params = [p["params"] for p in params]; self.lrs = [p.get("lr", lr) for p in params]
        else:
            self.params = list(params); self.lrs = [lr] * len(self.params)
        self.betas, self.eps, self.t = betas, eps, 0
        self.m = [torch.zeros_like(p) for p in self.params]; self.v = [torch.zeros_like(p) for p in self.params]
        self.stop_flag = stop_flag

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    def step(self, grads=None, skip=None):
        """``skip``: a device int32 tensor of one value (``StepGuard.close``) handed to the kernel as its stop flag for this step: when it is set, parameters and
        both moments are left untouched.  The host counter ``t`` advances all the same -- the host cannot know the outcome without waiting -- so a skipped step
        costs one step of bias correction and nothing else."""
        self.t += 1
        stop = self.stop_flag if skip is None else skip
        for i, p in enumerate(self.params):
            g = p.grad if grads is None else grads[i]
            if g is None:
                continue
            g = g.contiguous()
            L.check(L.lib().vt_adam_step(L.dptr(p.data), L.dptr(g), L.dptr(self.m[i]), L.dptr(self.v[i]), p.numel(), self.t, self.lrs[i],
                                         self.betas[0], self.betas[1], self.eps, L.dptr(stop), L.stream_ptr()))


# --------------------------------------------------------------------------------------------------
# Data-parallel training: the rank-ordered gradient mean
# --------------------------------------------------------------------------------------------------
def grad_rank_mean(parts, out=None):
    """``vt_grad_rank_mean``: ``parts`` (W, n) float32 on the device, row r = rank r's gradient; the rows may be ``stride`` >= n apart (a (W, n) view of a
    (W, stride) tensor: ``parts.stride(0)`` is passed on).  -> ``out`` (n,), default a new tensor: the rows added in rank order in fp64, divided by W once, rounded
    to fp32 once.  ``out`` may be one of the rows (in place).  The same bits on every call."""
    if not (torch.is_tensor(parts) and parts.is_cuda and parts.dtype == torch.float32 and parts.dim() == 2):
        raise L.VtError("grad_rank_mean: parts is a (W, n) float32 device tensor")
    W, n = parts.shape
    stride = parts.stride(0) if W > 1 else max(parts.stride(0), n)
    if n > 1 and parts.stride(1) != 1:
        raise L.VtError("grad_rank_mean: the rows of parts must be contiguous")
    with torch.cuda.device(parts.device):
        if out is None:
            out = torch.empty(n, device=parts.device)
        if not (torch.is_tensor(out) and out.device == parts.device and out.dtype == torch.float32 and out.numel() == n and out.is_contiguous()):
            raise L.VtError(f"grad_rank_mean: out is a contiguous float32 tensor of {n} values on {parts.device}")
        L.check(L.lib().vt_grad_rank_mean(parts.data_ptr() if n else None, W, n, stride, out.data_ptr() if n else None, L.stream_ptr()))
    return out


class RankMean:
    """The gradient average of a data-parallel step over flat gradient buffers, with the same bits on every rank: the ranks' buffers are GATHERED (a pure copy) into
    one (W, n_k) workspace per buffer, allocated once at the first use, and ``vt_grad_rank_mean`` adds the rows in rank order in fp64 into the buffer itself.

        rm = RankMean([enc_opt.grad, tri_opt.grad, params.flat], group)       # the tensors give sizes and device; reduce() may be handed others of the same sizes
        loss.backward(); rm.reduce(); optimiser steps

    ``group``: a ``torch.distributed`` process group, ``True`` for the default group, ``None`` for no group (a world of one).
    * RCCL ("nccl"): ``dist.all_gather_into_tensor`` on the current stream, no host wait.
    * gloo: the gather goes through host copies, as ``sharding.gather_params`` and ``reduce_rows_exact`` do.  TEST ONLY: it synchronises; it exists so that several
      ranks can share the one GPU of a test box.
    * a world of one: the gather is a copy (``VT_FORCE_DIST=1``: the collective runs all the same, as in ``sharding.gather_params``).
    ``reduce_local(parts)`` runs the same kernel over rows the caller filled itself (``rows(M)``: M rows per buffer, allocated once per M): micro-batches."""

    def __init__(self, buffers, group=None):
        import os
        buffers = list(buffers)
        if not buffers or any(not (torch.is_tensor(b) and b.is_cuda and b.dtype == torch.float32 and b.dim() == 1 and b.is_contiguous()) for b in buffers):
            raise L.VtError("RankMean: flat contiguous float32 device buffers expected")
        self.buffers, self.device = buffers, buffers[0].device
        self.sizes = [b.numel() for b in buffers]
        self.group, self.world, self.rank, self.backend = None, 1, 0, None
        if group is not None and group is not False:
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized()):
                raise L.VtError("RankMean: a process group was asked for, but torch.distributed is not initialised")
            self.group = dist.group.WORLD if group is True else group
            self.world, self.rank, self.backend = dist.get_world_size(self.group), dist.get_rank(self.group), dist.get_backend(self.group)
            if self.backend not in ("nccl", "gloo"):
                raise L.VtError(f"RankMean: backend {self.backend!r}; nccl (RCCL) or gloo expected")
        self.collective = self.group is not None and (self.world > 1 or os.environ.get("VT_FORCE_DIST") == "1")
        self._rows = {}

    @property
    def workspaces(self):
        """the (W, n_k) gather workspaces, allocated at the first ``reduce`` (a trainer without a group never pays for them)"""
        return self.rows(self.world)

    def rows(self, M):
        """one (M, n_k) float32 workspace per buffer, allocated at the first call for this M"""
        M = int(M)
        if M < 1:
            raise L.VtError("RankMean.rows: at least one row")
        if M not in self._rows:
            with torch.cuda.device(self.device):
                self._rows[M] = [torch.empty(M, n, device=self.device) for n in self.sizes]
        return self._rows[M]

    def gather(self, t, out=None):
        """``t`` (any shape and dtype, on the device, the same on every rank) from every rank of the group -> (W, *t.shape) in rank order"""
        t = t.contiguous()
        if out is None:
            out = torch.empty((self.world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        if not self.collective:
            out[0].copy_(t)
            return out
        import torch.distributed as dist
        if self.backend == "gloo":                                 # test only: no device collectives, host copies either side
            host = torch.empty(out.shape, dtype=t.dtype)
            dist.all_gather(list(host.unbind(0)), t.cpu(), group=self.group)
            out.copy_(host)
        else:
            dist.all_gather_into_tensor(out.view(-1), t.view(-1), group=self.group)
        return out

    def _check(self, buffers):
        buffers = self.buffers if buffers is None else list(buffers)
        if len(buffers) != len(self.sizes) or any(not torch.is_tensor(b) or b.numel() != n or b.device != self.device for b, n in zip(buffers, self.sizes)):
            raise L.VtError(f"RankMean: {len(self.sizes)} buffers of {self.sizes} values on {self.device} expected")
        return buffers

    def reduce(self, buffers=None):
        """every buffer (default: those of the constructor) becomes the mean over the group's ranks, in place; all ranks call it, with the same sizes"""
        buffers = self._check(buffers)
        for b, ws in zip(buffers, self.workspaces):
            self.gather(b, out=ws)
            grad_rank_mean(ws, out=b)
        return buffers

    def reduce_local(self, parts, buffers=None):
        """``parts``: one (M, n_k) tensor per buffer (``rows(M)``), filled by the caller; every buffer becomes the mean of its M rows, in row order"""
        buffers = self._check(buffers)
        parts = list(parts)
        if len(parts) != len(buffers) or any(p.dim() != 2 or p.shape[1] != n or p.shape[0] != parts[0].shape[0] for p, n in zip(parts, self.sizes)):
            raise L.VtError(f"RankMean.reduce_local: one (M, n) tensor per buffer expected, n = {self.sizes}")
        for b, p in zip(buffers, parts):
            grad_rank_mean(p, out=b)
        return buffers


# --------------------------------------------------------------------------------------------------
# The gradient record and the non-finite step guard
# --------------------------------------------------------------------------------------------------
GRAD_STATS_CHUNK = 4096                                        # VT_GRAD_STATS_CHUNK (include/vistracker.h)
_GUARD_HEAD, _GUARD_SLOT_HEAD, _GUARD_COEF, _GUARD_SKIP = 16, 32, 16, 20      # VT_GUARD_* (include/vistracker.h)


def _seg_table(seg_off, n, device, what):
    """(n_seg, 2) begin / end offsets, ascending and inside [0, n], as an int64 device tensor; a host list is checked, a device tensor is the caller's"""
    if torch.is_tensor(seg_off) and seg_off.is_cuda:
        if seg_off.dtype != torch.int64 or seg_off.dim() != 2 or seg_off.shape[1] != 2 or not seg_off.is_contiguous() or seg_off.device != device:
            raise L.VtError(f"{what}: seg_off is a contiguous (n_seg, 2) int64 tensor on {device}")
        return seg_off
    a = np.asarray(seg_off, dtype=np.int64).reshape(-1, 2)
    flat = a.reshape(-1)
    if flat.size and (flat[0] < 0 or flat[-1] > n or (np.diff(flat) < 0).any()):
        raise L.VtError(f"{what}: the segments' begin / end offsets must ascend inside [0, {n}]")
    return torch.as_tensor(a, device=device)


def grad_stats(g, seg_off, ws=None, out=None):
    """``vt_grad_stats``: ``g`` a flat float32 device tensor, ``seg_off`` (n_seg, 2) begin / end offsets into it (a list, or an int64 device tensor), ascending;
    what lies between two segments belongs to none.  -> (sumsq (n_seg,) float64, maxabs (n_seg,) float32, nonfinite (n_seg,) int32) on the device: per segment
    the fp64 sum of squares and the largest magnitude of the FINITE elements, and the number of NaN / Inf.  The same bits on every call.  ``ws`` (uint8,
    ``vt_grad_stats_workspace_bytes``) and ``out`` (the three tensors) may be handed in to save the allocations.  No host wait."""
    if not (torch.is_tensor(g) and g.is_cuda and g.dtype == torch.float32 and g.dim() == 1 and g.is_contiguous()):
        raise L.VtError("grad_stats: g is a flat contiguous float32 device tensor")
    n = g.numel()
    with torch.cuda.device(g.device):
        seg = _seg_table(seg_off, n, g.device, "grad_stats")
        n_seg = seg.shape[0]
        if out is None:
            out = (torch.zeros(n_seg, dtype=torch.float64, device=g.device), torch.zeros(n_seg, device=g.device),
                   torch.zeros(n_seg, dtype=torch.int32, device=g.device))
        need = int(L.lib().vt_grad_stats_workspace_bytes(n, n_seg))
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=g.device)
        if ws.numel() < need or ws.device != g.device:
            raise L.VtError(f"grad_stats: a workspace of {need} bytes on {g.device} expected")
        if n_seg:
            L.check(L.lib().vt_grad_stats(g.data_ptr(), n, seg.data_ptr(), n_seg, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), ws.data_ptr(),
                                          L.stream_ptr()))
    return out


def grad_scale(g, coef, skip=None):
    """``vt_grad_scale``: ``g[i] *= coef[0]`` in place (one fp32 multiplication per element) unless ``skip[0]`` is set; ``coef`` float32 and ``skip`` int32 device
    tensors of one value"""
    with torch.cuda.device(g.device):
        L.check(L.lib().vt_grad_scale(L.dptr(g), g.numel(), L.dptr(coef), L.dptr(skip), L.stream_ptr()))
    return g


class StepGuard:
    """The gradient record and the non-finite guard of a training step over up to three flat gradient buffers, decided on the device.

        guard = StepGuard([enc_opt.grad, tri_opt.grad, params.flat], segments, names, max_norm=1.0, record=8)
        loss.backward(); skip = guard.close(grads, loss); opt.step(skip=skip) ...
        guard.read()                                # epoch boundaries: the one method that waits on the host

    ``segments[k]``: the (offset, length) of every tensor in buffer k, ascending and disjoint (padding between them belongs to no segment); ``names[k]`` their
    names.  ``close`` measures every buffer (``vt_grad_stats``), closes the step (``vt_grad_guard_close``: the step is SKIPPED when any element of a segment or
    the error is NaN / Inf; ``max_norm``: torch's ``clip_grad_norm_`` coefficient from the global norm of the finite elements) and, with ``max_norm``, scales
    the buffers in place (``vt_grad_scale``; not on a skipped step).  -> the device int32 ``skip``, the ``stop_flag`` of the optimiser launches.  Offsets,
    workspaces, results and the record are allocated here once; ``record`` = K keeps the last K steps in a ring.  Computed from buffers that every rank holds
    identically (after ``RankMean.reduce``), the decision is the same on every rank with no collective."""

    def __init__(self, buffers, segments, names, max_norm=None, record=0):
        buffers, segments, names = list(buffers), [list(s) for s in segments], [list(n) for n in names]
        if not 1 <= len(buffers) <= 3 or len(segments) != len(buffers) or len(names) != len(buffers):
            raise L.VtError("StepGuard: one to three buffers, with one list of segments and one of names each")
        if any(not (torch.is_tensor(b) and b.is_cuda and b.dtype == torch.float32 and b.dim() == 1) for b in buffers):
            raise L.VtError("StepGuard: flat float32 device buffers expected")
        self.device, self.sizes = buffers[0].device, [b.numel() for b in buffers]
        self.max_norm = None if max_norm is None else float(max_norm)
        if self.max_norm is not None and not self.max_norm > 0:
            raise L.VtError(f"StepGuard: max_norm {max_norm}; a positive norm, or None for no clipping")
        self.ring = int(record)
        if self.ring < 0:
            raise L.VtError(f"StepGuard: record {record}; the number of steps kept, 0 for the last one only")
        self.names = [str(x) for ns in names for x in ns]
        if len(set(self.names)) != len(self.names):
            raise L.VtError("StepGuard: the names must differ")
        lib = L.lib()
        with torch.cuda.device(self.device):
            self._seg, self._out, self._ws = [], [], []
            for k, (n, segs, ns) in enumerate(zip(self.sizes, segments, names)):
                if len(segs) != len(ns):
                    raise L.VtError(f"StepGuard: buffer {k} has {len(segs)} segments and {len(ns)} names")
                table = [(int(o), int(o) + int(l)) for o, l in segs]
                if any(e < b for b, e in table):
                    raise L.VtError(f"StepGuard: buffer {k} has a segment of negative length")
                self._seg.append(_seg_table(table, n, self.device, f"StepGuard: buffer {k}"))
                self._out.append((torch.zeros(len(segs), dtype=torch.float64, device=self.device), torch.zeros(len(segs), device=self.device),
                                  torch.zeros(len(segs), dtype=torch.int32, device=self.device)))
                self._ws.append(torch.empty(int(lib.vt_grad_stats_workspace_bytes(n, len(segs))), dtype=torch.uint8, device=self.device))
            self.n_seg = len(self.names)
            self._slot = _GUARD_SLOT_HEAD + 16 * self.n_seg
            self.record = torch.zeros(int(lib.vt_grad_guard_record_bytes(self.n_seg, self.ring)) // 8, dtype=torch.int64, device=self.device)
            raw = self.record.view(torch.uint8)
            self.coef = raw[_GUARD_HEAD + _GUARD_COEF:_GUARD_HEAD + _GUARD_COEF + 4].view(torch.float32)
            self.skip = raw[_GUARD_HEAD + _GUARD_SKIP:_GUARD_HEAD + _GUARD_SKIP + 4].view(torch.int32)
        self.launches_per_close = 3 * len(buffers) + 1 + (len(buffers) if self.max_norm is not None else 0)

    def close(self, grads, error=None):
        """``grads``: one flat float32 tensor per buffer of the constructor, of its size; ``error``: the step's objective, a float64 device scalar, or None.
        -> ``skip``, a device int32 tensor of one value (the same tensor every call).  Nothing here waits on the host."""
        grads = list(grads)
        if len(grads) != len(self.sizes) or any(not torch.is_tensor(g) or g.numel() != n or g.device != self.device or g.dtype != torch.float32
                                                 for g, n in zip(grads, self.sizes)):
            raise L.VtError(f"StepGuard.close: {len(self.sizes)} float32 buffers of {self.sizes} values on {self.device} expected")
        if error is not None and not (torch.is_tensor(error) and error.device == self.device and error.dtype == torch.float64 and error.numel() == 1):
            raise L.VtError(f"StepGuard.close: error is a float64 scalar on {self.device}")
        lib = L.lib()
        with torch.cuda.device(self.device):
            grads = [g.detach().reshape(-1) for g in grads]
            stream, args = L.stream_ptr(), []
            for g, seg, out, ws in zip(grads, self._seg, self._out, self._ws):
                grad_stats(g, seg, ws=ws, out=out)
                args += [out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), seg.shape[0]]
            args += [None, None, None, 0] * (3 - len(grads))
            L.check(lib.vt_grad_guard_close(*args, L.dptr(error.detach().reshape(1)) if error is not None else None,
                                            self.max_norm if self.max_norm is not None else 0.0, self.record.data_ptr(), self.ring, stream))
            if self.max_norm is not None:
                for g in grads:
                    L.check(lib.vt_grad_scale(L.dptr(g), g.numel(), self.coef.data_ptr(), self.skip.data_ptr(), stream))
        return self.skip

    def _slot_dict(self, raw, at):
        S = self.n_seg
        head = raw[at:at + _GUARD_SLOT_HEAD]
        body = raw[at + _GUARD_SLOT_HEAD:at + self._slot]
        sumsq, maxabs, nonfinite = body[:8 * S].view(np.float64), body[8 * S:12 * S].view(np.float32), body[12 * S:16 * S].view(np.int32)
        return {"step": int(head[24:32].view(np.int64)[0]), "norm": float(head[0:8].view(np.float64)[0]), "error": float(head[8:16].view(np.float64)[0]),
                "coef": float(head[16:20].view(np.float32)[0]), "skip": bool(head[20:24].view(np.int32)[0]),
                "sumsq": {k: float(v) for k, v in zip(self.names, sumsq)}, "maxabs": {k: float(v) for k, v in zip(self.names, maxabs)},
                "nonfinite": {k: int(v) for k, v in zip(self.names, nonfinite)}}

    def read(self):
        """the record as a host dict, in ONE copy (it waits for the stream): ``steps`` and ``skipped`` (counters since the guard was built); of the last step
        ``step`` (its index), ``norm``, ``coef``, ``skip``, ``error`` and per name ``sumsq``, ``maxabs``, ``nonfinite``; ``ring``: the same dicts for the last
        ``record`` steps, oldest first.  Before the first ``close`` the last step is all zeros and the ring empty."""
        raw = self.record.cpu().numpy().view(np.uint8)
        steps, skipped = (int(x) for x in raw[:_GUARD_HEAD].view(np.int64))
        out = {"steps": steps, "skipped": skipped}
        out.update(self._slot_dict(raw, _GUARD_HEAD))
        out["ring"] = [self._slot_dict(raw, _GUARD_HEAD + (1 + t % self.ring) * self._slot) for t in range(max(0, steps - self.ring), steps)] if self.ring else []
        return out


# ---- HVOP-Net training (csrc/formertrain.hip): one pre-norm encoder layer and the final LayerNorm of a TransformerV2 as autograd Functions ----------------
FORMER_PARAM_KEYS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "linear1.weight", "linear1.bias",
                     "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")
FORMER_ACT = {"relu": 0, "gelu": 1, "leaky_relu": 2}


def _former_ptrs(ts):
    return (C.c_void_p * 12)(*[None if t is None else L.dptr(t) for t in ts])


def former_tape_views(tape, B, T, D, H, F):
    """the named tensors of a layer tape (layout: csrc/formertrain.hip): fp64 mean1, rstd1, mean2, rstd2 (B, T, 1); fp32 qkv (B, T, 3D), O, y1 (B, T, D), h (B, T, F),
    lse (B, H, T)"""
    M = B * T
    st = tape[:8 * M].view(torch.float64).view(2, M, 2)
    out = {"mean1": st[0, :, 0].reshape(B, T, 1), "rstd1": st[0, :, 1].reshape(B, T, 1), "mean2": st[1, :, 0].reshape(B, T, 1), "rstd2": st[1, :, 1].reshape(B, T, 1)}
    o = 8 * M
    for k, n, shape in (("qkv", 3 * M * D, (B, T, 3 * D)), ("O", M * D, (B, T, D)), ("y1", M * D, (B, T, D)), ("h", M * F, (B, T, F)), ("lse", B * H * T, (B, H, T))):
        out[k] = tape[o:o + n].view(shape); o += n
    return out


def _former_check(x, pos, key_padding_mask, params, H, activation, extra=()):
    """float32 contiguous device tensors of the shapes the kernels assume: they read raw pointers"""
    f32 = lambda t: torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32           # noqa: E731
    if not f32(x) or x.dim() != 3:
        raise L.VtError("former layer: x must be a float32 device tensor (B, T, D)")
    B, T, D = x.shape
    if activation not in FORMER_ACT:
        raise L.VtError(f"former layer: activation {activation!r}; one of {sorted(FORMER_ACT)}")
    if not f32(pos) or tuple(pos.shape) != (T, D):
        raise L.VtError(f"former layer: pos must be float32 ({T}, {D})")
    if len(params) != 12 or not all(f32(q) for q in params) or params[4].dim() != 2:
        raise L.VtError("former layer: twelve float32 device parameters in FORMER_PARAM_KEYS order expected")
    F = params[4].shape[0]
    shapes = ((3 * D, D), (3 * D,), (D, D), (D,), (F, D), (F,), (D, F), (D,), (D,), (D,), (D,), (D,))
    for k, q, s in zip(FORMER_PARAM_KEYS, params, shapes):
        if tuple(q.shape) != s:
            raise L.VtError(f"former layer: {k} has shape {tuple(q.shape)}, expected {s}")
    if key_padding_mask is not None and (not torch.is_tensor(key_padding_mask) or tuple(key_padding_mask.shape) != (B, T)
                                         or key_padding_mask.dtype not in (torch.bool, torch.uint8)):
        raise L.VtError(f"former layer: key_padding_mask must be bool / uint8 ({B}, {T})")
    for name, t, s in extra:
        if t is not None and (not f32(t) or tuple(t.shape) != tuple(s)):
            raise L.VtError(f"former layer: {name} must be float32 {tuple(s)}")
    return B, T, D, F


def former_layer_forward(x, pos, key_padding_mask, params, H, activation, p=0.0, seed=0, tape=True):
    """vt_former_layer_forward -> (y, tape or None).  ``params``: the twelve tensors in FORMER_PARAM_KEYS order; ``key_padding_mask`` (B, T) uint8 / bool or None."""
    B, T, D, F = _former_check(x, pos, key_padding_mask, params, H, activation)
    lib = L.lib()
    n = int(lib.vt_former_layer_tape_floats(B, T, D, H, F))
    if n < 0:
        raise L.VtError(f"former layer: unsupported shape B {B} T {T} D {D} H {H} F {F} (T <= 192, D % 16 == 0 <= 160, F % 16 == 0 <= 256, D / H in {{16, 32, 160}})")
    y = torch.empty_like(x)
    tp = torch.empty(n, dtype=torch.float32, device=x.device) if tape else None
    ws = None if tape else torch.empty(4 * B * T * D, dtype=torch.float32, device=x.device)
    m = None if key_padding_mask is None else key_padding_mask.to(torch.uint8).contiguous()
    L.check(lib.vt_former_layer_forward(L.dptr(x), L.dptr(pos), L.dptr(m), _former_ptrs(params), B, T, D, H, F, FORMER_ACT[activation], float(p), int(seed),
                                        L.dptr(y), L.dptr(tp), L.dptr(ws), L.stream_ptr()))
    return y, tp


def former_layer_backward(d_y, tape, x, pos, key_padding_mask, params, H, activation, p=0.0, seed=0, want_dx=True, want=None, out=None, accumulate=False):
    """vt_former_layer_backward -> (d_x or None, [twelve gradients or None]).  ``want``: twelve flags (default all); ``out``: (d_x, [twelve]) buffers to write / add into."""
    B, T, D, F = _former_check(x, pos, key_padding_mask, params, H, activation, extra=(("d_y", d_y, x.shape),))
    lib = L.lib()
    n = int(lib.vt_former_layer_workspace_floats(B, T, D, H, F))
    nt = int(lib.vt_former_layer_tape_floats(B, T, D, H, F))
    if n < 0 or nt < 0:
        raise L.VtError(f"former layer: unsupported shape B {B} T {T} D {D} H {H} F {F}")
    if not (torch.is_tensor(tape) and tape.is_cuda and tape.dtype == torch.float32 and tape.numel() == nt):
        raise L.VtError(f"former layer: the tape must be the float32 tensor of {nt} values a taped forward of this shape returned")
    if out is not None:
        _former_check(x, pos, key_padding_mask, params, H, activation, extra=[("d_x", out[0], x.shape)] + [(k, t, q.shape) for k, t, q in zip(FORMER_PARAM_KEYS, out[1], params)])
    ws = torch.empty(n, dtype=torch.float32, device=x.device)
    want = [True] * 12 if want is None else list(want)
    if out is not None:
        d_x, grads = out
    else:
        d_x = torch.empty_like(x) if want_dx else None
        grads = [torch.empty_like(q) if w else None for q, w in zip(params, want)]
    m = None if key_padding_mask is None else key_padding_mask.to(torch.uint8).contiguous()
    L.check(lib.vt_former_layer_backward(L.dptr(d_y), L.dptr(tape), L.dptr(x), L.dptr(pos), L.dptr(m), _former_ptrs(params), B, T, D, H, F, FORMER_ACT[activation],
                                         float(p), int(seed), L.dptr(d_x), _former_ptrs(grads), int(bool(accumulate)), L.dptr(ws), L.stream_ptr()))
    return d_x, grads


class _FormerLayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos, mask, H, activation, p, seed, *params):
        x = x.contiguous(); params = [q.contiguous() for q in params]
        y, tape = former_layer_forward(x, pos, mask, params, H, activation, p, seed)
        ctx.save_for_backward(x, pos, tape, *params)
        ctx.mask, ctx.cfg = mask, (H, activation, p, seed)
        return y

    @staticmethod
    def backward(ctx, d_y):
        x, pos, tape, *params = ctx.saved_tensors
        H, activation, p, seed = ctx.cfg
        want = list(ctx.needs_input_grad[7:])
        d_x, grads = former_layer_backward(d_y.contiguous(), tape, x, pos, ctx.mask, params, H, activation, p, seed, want_dx=ctx.needs_input_grad[0], want=want)
        return (d_x, None, None, None, None, None, None, *grads)


def former_layer_train(x, pos, key_padding_mask, params, H, activation, p=0.0, seed=0):
    """one pre-norm encoder layer (former_deci.py:77-93) under autograd: x (B, T, D) and the twelve ``params`` (FORMER_PARAM_KEYS order) receive gradients from the
    hand-written backward.  No host wait in either direction."""
    return _FormerLayerFn.apply(x, pos, key_padding_mask, H, activation, float(p), int(seed), *params)


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        D = x.shape[-1]
        if any(not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32) for t in (x, weight, bias)) or tuple(weight.shape) != (D,) or tuple(bias.shape) != (D,):
            raise L.VtError(f"layernorm_train: float32 device tensors expected, weight and bias of shape ({D},)")
        x = x.contiguous()
        M = x.numel() // D
        if L.lib().vt_layernorm_backward_workspace_floats(M, D) < 0:
            raise L.VtError(f"layernorm_train: unsupported M {M} D {D} (D % 16 == 0, 16 <= D <= 160)")
        y = torch.empty_like(x); stats = torch.empty(M, 2, dtype=torch.float64, device=x.device)
        L.check(L.lib().vt_layernorm_forward(L.dptr(x), L.dptr(weight.contiguous()), L.dptr(bias.contiguous()), M, D, L.dptr(y), L.dptr(stats), L.stream_ptr()))
        ctx.save_for_backward(x, weight, stats)
        return y

    @staticmethod
    def backward(ctx, d_y):
        x, weight, stats = ctx.saved_tensors
        D = x.shape[-1]; M = x.numel() // D
        lib = L.lib()
        ws = torch.empty(int(lib.vt_layernorm_backward_workspace_floats(M, D)), dtype=torch.float32, device=x.device)
        d_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(weight) if ctx.needs_input_grad[1] else None
        db = torch.empty_like(weight) if ctx.needs_input_grad[2] else None
        L.check(lib.vt_layernorm_backward(L.dptr(d_y.contiguous()), L.dptr(x), L.dptr(stats), L.dptr(weight.contiguous()), M, D, L.dptr(d_x), L.dptr(dw), L.dptr(db), 0,
                                          L.dptr(ws), L.stream_ptr()))
        return d_x, dw, db


def layernorm_train(x, weight, bias):
    """nn.LayerNorm over the last dimension (eps 1e-5) under autograd: vt_layernorm_forward / vt_layernorm_backward"""
    return _LayerNormFn.apply(x, weight, bias)


# ---- HVOP-Net training (csrc/infillhead.hip): the input projections, the predictor MLP and the motion objective -----------------------------------------
INFILL_HEAD_KEYS = ("predictor.0.weight", "predictor.0.bias", "predictor.2.weight", "predictor.2.bias")
_PROJ_RANGE = "1 .. 4 projections over the same rows, Kin in 1 .. 160, N % 16 == 0 in 16 .. 160"
_HEAD_RANGE = "T >= 3, D % 16 == 0 in 16 .. 160, hidden % 16 == 0 in 16 .. 64, out_dim in 1 .. 16"


def _ptr_array(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else L.dptr(t) for t in ts])


def _dense32(what, name, t, shape=None, device=None, optional=False):
    """a float32 contiguous device tensor of `shape`: the kernels read raw pointers"""
    if t is None and optional:
        return
    if not torch.is_tensor(t) or not t.is_cuda:
        raise L.VtError(f"{what}: {name} must be a device tensor; there is no CPU path")
    if t.dtype != torch.float32:
        raise L.VtError(f"{what}: {name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise L.VtError(f"{what}: {name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise L.VtError(f"{what}: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if device is not None and t.device != device:
        raise L.VtError(f"{what}: {name} on {t.device}, expected {device}")


def _proj_check(what, xs, weights, biases):
    """-> (M, kin, n) of a table of projections; every x is (..., Kin) over the same leading shape"""
    if not (isinstance(xs, (list, tuple)) and isinstance(weights, (list, tuple)) and isinstance(biases, (list, tuple))) or not 1 <= len(xs) <= 4 \
            or len(weights) != len(xs) or len(biases) != len(xs):
        raise L.VtError(f"{what}: lists of the same length expected ({_PROJ_RANGE})")
    for i, x in enumerate(xs):
        _dense32(what, f"xs[{i}]", x)
        if x.dim() < 2:
            raise L.VtError(f"{what}: xs[{i}] must be (..., Kin)")
    dev, lead = xs[0].device, tuple(xs[0].shape[:-1])
    kin, n = [], []
    for i, (x, w, b) in enumerate(zip(xs, weights, biases)):
        if tuple(x.shape[:-1]) != lead:
            raise L.VtError(f"{what}: xs[{i}] has leading shape {tuple(x.shape[:-1])}, xs[0] {lead}")
        _dense32(what, f"weights[{i}]", w, device=dev)
        if w.dim() != 2 or w.shape[1] != x.shape[-1]:
            raise L.VtError(f"{what}: weights[{i}] has shape {tuple(w.shape)}, expected (N, {x.shape[-1]})")
        _dense32(what, f"biases[{i}]", b, (w.shape[0],), dev)
        kin.append(int(w.shape[1])); n.append(int(w.shape[0]))
    M = xs[0].numel() // kin[0]
    ka, na = (C.c_int * len(kin))(*kin), (C.c_int * len(n))(*n)
    nws = int(L.lib().vt_infill_proj_workspace_floats(ka, na, len(kin), M))
    if nws < 0:
        raise L.VtError(f"{what}: unsupported shapes M {M} Kin {kin} N {n} ({_PROJ_RANGE})")
    return M, ka, na, nws


def infill_proj_forward(xs, weights, biases):
    """vt_infill_proj_forward: [x (..., Kin) W^T + b for each problem] in one launch"""
    M, ka, na, _ = _proj_check("infill_proj_forward", xs, weights, biases)
    ys = [torch.empty(x.shape[:-1] + (w.shape[0],), dtype=torch.float32, device=x.device) for x, w in zip(xs, weights)]
    with torch.cuda.device(xs[0].device):
        L.check(L.lib().vt_infill_proj_forward(_ptr_array(xs), _ptr_array(weights), _ptr_array(biases), ka, na, len(xs), M, _ptr_array(ys), L.stream_ptr()))
    return ys


def infill_proj_backward(d_ys, xs, weights, biases, want=None, out=None, accumulate=False):
    """vt_infill_proj_backward -> ([d_weight or None], [d_bias or None]).  ``weights`` / ``biases`` give the shapes only; ``want``: (flags of the weights, flags of
    the biases), default all; ``out``: ([d_weight], [d_bias]) buffers to write / add into (None entries are skipped)."""
    what = "infill_proj_backward"
    M, ka, na, nws = _proj_check(what, xs, weights, biases)
    if not isinstance(d_ys, (list, tuple)) or len(d_ys) != len(xs):
        raise L.VtError(f"{what}: one d_y per projection expected")
    dev = xs[0].device
    for i, (d, x, w) in enumerate(zip(d_ys, xs, weights)):
        _dense32(what, f"d_ys[{i}]", d, tuple(x.shape[:-1]) + (w.shape[0],), dev)
    if out is not None:
        dws, dbs = list(out[0]), list(out[1])
        for i, (w, b) in enumerate(zip(weights, biases)):
            _dense32(what, f"out d_weight[{i}]", dws[i], w.shape, dev, optional=True)
            _dense32(what, f"out d_bias[{i}]", dbs[i], b.shape, dev, optional=True)
    else:
        ww, wb = ([True] * len(xs), [True] * len(xs)) if want is None else want
        dws = [torch.empty_like(w) if f else None for w, f in zip(weights, ww)]
        dbs = [torch.empty_like(b) if f else None for b, f in zip(biases, wb)]
    ws = torch.empty(nws, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().vt_infill_proj_backward(_ptr_array(d_ys), _ptr_array(xs), ka, na, len(xs), M, _ptr_array(dws), _ptr_array(dbs), int(bool(accumulate)),
                                                L.dptr(ws), L.stream_ptr()))
    return dws, dbs


class _InfillProjFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, n, *args):
        xs, weights, biases = list(args[:n]), list(args[n:2 * n]), list(args[2 * n:])
        ctx.n = n
        ctx.save_for_backward(*xs, *weights, *biases)
        return tuple(infill_proj_forward(xs, weights, biases))

    @staticmethod
    def backward(ctx, *d_ys):
        n, t = ctx.n, ctx.saved_tensors
        xs, weights, biases = list(t[:n]), list(t[n:2 * n]), list(t[2 * n:])
        d_ys = [torch.zeros(x.shape[:-1] + (w.shape[0],), dtype=torch.float32, device=x.device) if d is None else d.contiguous() for d, x, w in zip(d_ys, xs, weights)]
        need = ctx.needs_input_grad
        dws, dbs = infill_proj_backward(d_ys, xs, weights, biases, want=(need[1 + n:1 + 2 * n], need[1 + 2 * n:]))
        return (None,) + (None,) * n + tuple(dws) + tuple(dbs)


def infill_proj_train(xs, weights, biases):
    """the input projections of ConditionalMInfiller.forward (mfiller_cond.py:82-96) under autograd, all of them in one forward launch and three backward
    launches: [x W^T + b]; gradients go to the weights and biases only (the inputs are data).  xs float32 contiguous device tensors (..., Kin) over the same rows.
    No host wait in either direction."""
    xs, weights, biases = list(xs), list(weights), list(biases)
    _proj_check("infill_proj_train", xs, weights, biases)
    return list(_InfillProjFn.apply(len(xs), *[x.detach() for x in xs], *weights, *biases))


def _head_check(what, f, params, gt=None, need_gt=False):
    _dense32(what, "f", f)
    if f.dim() != 3:
        raise L.VtError(f"{what}: f must be (B, T, D)")
    B, T, D = (int(s) for s in f.shape)
    if not isinstance(params, (list, tuple)) or len(params) != 4:
        raise L.VtError(f"{what}: four parameters expected, in the order {INFILL_HEAD_KEYS}")
    for k, q in zip(INFILL_HEAD_KEYS, params):
        _dense32(what, k, q, device=f.device)
    if params[0].dim() != 2 or params[2].dim() != 2:
        raise L.VtError(f"{what}: the two weights must be matrices")
    Hd, C_ = int(params[0].shape[0]), int(params[2].shape[0])
    for k, q, s in zip(INFILL_HEAD_KEYS, params, ((Hd, D), (Hd,), (C_, Hd), (C_,))):
        if tuple(q.shape) != s:
            raise L.VtError(f"{what}: {k} has shape {tuple(q.shape)}, expected {s}")
    nws = int(L.lib().vt_infill_head_workspace_floats(B, T, D, Hd, C_))
    if nws < 0:
        raise L.VtError(f"{what}: unsupported shape B {B} T {T} D {D} hidden {Hd} out_dim {C_} ({_HEAD_RANGE})")
    if gt is not None or need_gt:
        _dense32(what, "gt", gt, (B, T, C_), f.device)
    return B, T, D, Hd, C_, nws


def infill_head_forward(f, params, gt=None, lw_pose=1.0, lw_accel=0.1, save_h=True):
    """vt_infill_head_forward -> (pred (B, T, out_dim), h (B, T, hidden) or None, terms or None).  With ``gt`` the two fp64 terms [loss_pos, loss_accel] of
    trainer_infiller.py:33-47 are formed too; ``save_h=False`` is the forward-only mode of a validation."""
    B, T, D, Hd, C_, nws = _head_check("infill_head_forward", f, params, gt)
    dev = f.device
    pred = torch.empty(B, T, C_, dtype=torch.float32, device=dev)
    h = torch.empty(B, T, Hd, dtype=torch.float32, device=dev) if save_h else None
    terms = torch.empty(2, dtype=torch.float64, device=dev) if gt is not None else None
    ws = torch.empty(nws, dtype=torch.float32, device=dev) if gt is not None else None
    with torch.cuda.device(dev):
        L.check(L.lib().vt_infill_head_forward(L.dptr(f), _ptr_array(params), L.dptr(gt), B, T, D, Hd, C_, float(lw_pose), float(lw_accel), L.dptr(pred), L.dptr(h),
                                               L.dptr(terms), L.dptr(ws), L.stream_ptr()))
    return pred, h, terms


def infill_head_backward(f, h, params, d_pred=None, gt=None, pred=None, lw_pose=1.0, lw_accel=0.1, upstream=1.0, want_terms=False, want_df=True, want=None, out=None,
                         accumulate=False):
    """vt_infill_head_backward -> (d_pred, d_f or None, [four gradients or None], terms or None).  With ``d_pred`` given it is the gradient to the prediction;
    without, ``gt`` and ``pred`` are needed and d_pred is ``upstream`` times the gradient of loss_pos + loss_accel (``want_terms``: the two fp64 terms too).
    ``want``: four flags (default all); ``out``: (d_f, [four]) buffers to write / add into."""
    what = "infill_head_backward"
    B, T, D, Hd, C_, nws = _head_check(what, f, params, gt, need_gt=d_pred is None)
    dev = f.device
    _dense32(what, "h", h, (B, T, Hd), dev)
    if d_pred is None:
        _dense32(what, "pred", pred, (B, T, C_), dev)
        dp_out = torch.empty(B, T, C_, dtype=torch.float32, device=dev)
    else:
        _dense32(what, "d_pred", d_pred, (B, T, C_), dev)
        if want_terms:
            raise L.VtError(f"{what}: the objective's terms are not formed when d_pred is given")
        dp_out = None
    if out is not None:
        d_f, grads = out[0], list(out[1])
        _dense32(what, "out d_f", d_f, f.shape, dev, optional=True)
        for k, g, q in zip(INFILL_HEAD_KEYS, grads, params):
            _dense32(what, "out " + k, g, q.shape, dev, optional=True)
    else:
        want = [True] * 4 if want is None else list(want)
        d_f = torch.empty_like(f) if want_df else None
        grads = [torch.empty_like(q) if w else None for q, w in zip(params, want)]
    terms = torch.empty(2, dtype=torch.float64, device=dev) if want_terms else None
    ws = torch.empty(nws, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().vt_infill_head_backward(L.dptr(d_pred), L.dptr(gt), L.dptr(pred), L.dptr(h), L.dptr(f), _ptr_array(params), B, T, D, Hd, C_, float(lw_pose),
                                                float(lw_accel), float(upstream), L.dptr(terms), L.dptr(dp_out), L.dptr(d_f), _ptr_array(grads),
                                                int(bool(accumulate)), L.dptr(ws), L.stream_ptr()))
    return (d_pred if dp_out is None else dp_out), d_f, grads, terms


class _InfillHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, gt, lw_pose, lw_accel, *params):
        f = f.contiguous(); params = [q.contiguous() for q in params]
        need = ctx.needs_input_grad
        if need[0] or any(need[4:]):
            pred, h, _ = infill_head_forward(f, params)
            _, d_f, grads, terms = infill_head_backward(f, h, params, gt=gt, pred=pred, lw_pose=lw_pose, lw_accel=lw_accel, want_terms=True, want_df=need[0],
                                                        want=need[4:])
            ctx.grads = [d_f] + grads
        else:
            pred, _, terms = infill_head_forward(f, params, gt, lw_pose, lw_accel, save_h=False)
            ctx.grads = [None] * 5
        ctx.mark_non_differentiable(terms, pred)
        return terms.sum(), terms, pred

    @staticmethod
    def backward(ctx, g, _gt, _gp):
        g = g.to(torch.float32)
        d = [None if t is None else t * g for t in ctx.grads]
        return (d[0], None, None, None, *d[1:])


def infill_head_train(f, gt, params, lw_pose=1.0, lw_accel=0.1):
    """the predictor MLP (mfiller_cond.py:97-104) and motion_losses (trainer_infiller.py:33-47) under autograd -> (loss, loss_pos, loss_accel, pred): float64
    device scalars (loss = loss_pos + loss_accel carries the graph, the two terms and pred (B, T, out_dim) float32 are not differentiable).  f (B, T, D) and the
    four ``params`` (INFILL_HEAD_KEYS order) receive gradients; they are computed with the values for an upstream gradient of 1 and multiplied by the upstream
    scalar in the backward.  Without a gradient to form (``torch.no_grad()``) only the values are computed and h is not saved.  No host wait."""
    what = "infill_head_train"
    if not (torch.is_tensor(f) and f.is_cuda):
        raise L.VtError(f"{what}: f must be a device tensor; there is no CPU path")
    f, params = f.contiguous(), list(params)
    _head_check(what, f, params, gt, need_gt=True)
    loss, terms, pred = _InfillHeadFn.apply(f, gt, float(lw_pose), float(lw_accel), *params)
    return loss, terms[0], terms[1], pred


# --------------------------------------------------------------------------------------------------
# HVOP-Net training: the clip data set (csrc/clipdata.hip)
# --------------------------------------------------------------------------------------------------
CLIP_DECISIONS = ("kid", "drop_len", "start_fr", "aug_start")
CLIP_TABLES = (("poses", 72), ("trans", 3), ("roots", 3), ("obj_angles", 3), ("obj_trans", 3))


def _clip_arg(what, t, dtype, shape, device=None):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise L.VtError(f"{what}: a device tensor is expected")
    if device is not None and t.device != device:
        raise L.VtError(f"{what}: on {t.device}, the other tensors are on {device}")
    if t.dtype != dtype:
        raise L.VtError(f"{what}: dtype {t.dtype}, {dtype} expected")
    if tuple(t.shape) != tuple(shape):
        raise L.VtError(f"{what}: shape {tuple(t.shape)}, {tuple(shape)} expected")
    if not t.is_contiguous():
        raise L.VtError(f"{what}: not contiguous")
    return t


def clip_draw(clip_index, seed, epoch, T, multi_kinects, min_drop_len, max_drop_len, start_fr_min, start_fr_max, aug_num):
    """``vt_clip_draw``: the random decisions of TrainDataCMotionFiller.get_item / gen_masks for the clips ``clip_index`` (B,) int32 on the device (their GLOBAL
    indices).  -> dict of int32 device tensors kid, drop_len, start_fr (B,), aug_start (B, aug_num): functions of (seed, epoch, clip index, draw number) alone.  A
    range that can be empty raises; nothing is clamped."""
    if not torch.is_tensor(clip_index) or clip_index.dim() != 1 or clip_index.numel() < 1:
        raise L.VtError("clip_draw: clip_index is a (B,) int32 device tensor, B >= 1")
    B, T, aug_num = clip_index.numel(), int(T), int(aug_num)
    _clip_arg("clip_draw: clip_index", clip_index, torch.int32, (B,))
    seed, epoch = int(seed), int(epoch)
    if not (0 <= seed < 1 << 64 and 0 <= epoch < 1 << 32):
        raise L.VtError(f"clip_draw: seed {seed} is a 64-bit, epoch {epoch} a 32-bit unsigned integer")
    min_drop_len, max_drop_len, start_fr_min, start_fr_max = int(min_drop_len), int(max_drop_len), int(start_fr_min), int(start_fr_max)
    if T < 1 or min_drop_len < 0 or max_drop_len < min_drop_len:
        raise L.VtError(f"clip_draw: T = {T}, drop lengths [{min_drop_len}, {max_drop_len}]")
    if start_fr_min < 0 or min(T - max_drop_len, start_fr_max) <= start_fr_min:
        raise L.VtError(f"clip_draw: the start-frame range [{start_fr_min}, min({T} - {max_drop_len}, {start_fr_max})) is empty")
    if not 0 <= aug_num <= 64 or (aug_num > 0 and T - aug_num <= 0):
        raise L.VtError(f"clip_draw: aug_num = {aug_num} with T = {T}: the window-start range [0, T - aug_num) is empty, or aug_num is not in 0..64")
    with torch.cuda.device(clip_index.device):
        o = {k: torch.empty(B, dtype=torch.int32, device=clip_index.device) for k in CLIP_DECISIONS[:3]}
        o["aug_start"] = torch.empty((B, aug_num), dtype=torch.int32, device=clip_index.device)
        L.check(L.lib().vt_clip_draw(clip_index.data_ptr(), B, seed, epoch, T, 1 if multi_kinects else 0, min_drop_len, max_drop_len, start_fr_min, start_fr_max,
                                     aug_num, o["kid"].data_ptr(), o["drop_len"].data_ptr(), o["start_fr"].data_ptr(),
                                     o["aug_start"].data_ptr() if aug_num else None, L.stream_ptr()))
    return o


def clip_build(tables, w2c_R, w2c_t, start, date, decisions, T, obj_dim, noise=None, clip_index=None, seed=0, epoch=0):
    """``vt_clip_build``: the batch of TrainDataCMotionFiller.get_item for B clips.  ``tables``: dict of float32 device tensors poses (N, 72), trans, roots,
    obj_angles, obj_trans (N, 3); w2c_R (n_dates, 4, 3, 3), w2c_t (n_dates, 4, 3); start, date (B,) int32: clip b is frames [start[b], start[b] + T) of date
    date[b]; ``decisions``: the dict of ``clip_draw`` (or explicit ones).  The noise of the augmentation is hashed from (seed, epoch, clip_index) unless ``noise``
    (B, aug_num^2, 3) float32 is given (tests).  -> data_smpl, gt_smpl (B, T, 147), data_obj, gt_obj (B, T, obj_dim) float32, mask_obj, mask_smpl (B, T) bool."""
    T, obj_dim = int(T), int(obj_dim)
    if obj_dim not in (6, 9):
        raise L.VtError(f"clip_build: obj_dim = {obj_dim}; 6 ('6d') or 9 ('9d')")
    if not torch.is_tensor(tables.get("poses")) or tables["poses"].dim() != 2:
        raise L.VtError("clip_build: tables['poses'] is an (N, 72) float32 device tensor")
    dev, N = tables["poses"].device, tables["poses"].shape[0]
    for k, w in CLIP_TABLES:
        _clip_arg(f"clip_build: tables[{k!r}]", tables.get(k), torch.float32, (N, w), dev)
    if T < 1 or N < T:
        raise L.VtError(f"clip_build: T = {T} with {N} frames")
    if not torch.is_tensor(w2c_R) or w2c_R.dim() != 4 or w2c_R.shape[0] < 1:
        raise L.VtError("clip_build: w2c_R is an (n_dates, 4, 3, 3) float32 device tensor, n_dates >= 1")
    nd = w2c_R.shape[0]
    _clip_arg("clip_build: w2c_R", w2c_R, torch.float32, (nd, 4, 3, 3), dev)
    _clip_arg("clip_build: w2c_t", w2c_t, torch.float32, (nd, 4, 3), dev)
    if not torch.is_tensor(start) or start.dim() != 1 or start.numel() < 1:
        raise L.VtError("clip_build: start is a (B,) int32 device tensor, B >= 1")
    B = start.numel()
    _clip_arg("clip_build: start", start, torch.int32, (B,), dev)
    _clip_arg("clip_build: date", date, torch.int32, (B,), dev)
    for k in CLIP_DECISIONS[:3]:
        _clip_arg(f"clip_build: decisions[{k!r}]", decisions.get(k), torch.int32, (B,), dev)
    au = decisions.get("aug_start")
    aug_num = 0 if au is None else (au.shape[1] if torch.is_tensor(au) and au.dim() == 2 else -1)
    if not 0 <= aug_num <= 64:
        raise L.VtError("clip_build: decisions['aug_start'] is a (B, aug_num) int32 device tensor, aug_num <= 64")
    if aug_num:
        _clip_arg("clip_build: decisions['aug_start']", au, torch.int32, (B, aug_num), dev)
        if noise is not None:
            _clip_arg("clip_build: noise", noise, torch.float32, (B, aug_num * aug_num, 3), dev)
        else:
            _clip_arg("clip_build: clip_index", clip_index, torch.int32, (B,), dev)
    seed, epoch = int(seed), int(epoch)
    if not (0 <= seed < 1 << 64 and 0 <= epoch < 1 << 32):
        raise L.VtError(f"clip_build: seed {seed} is a 64-bit, epoch {epoch} a 32-bit unsigned integer")
    with torch.cuda.device(dev):
        o = {"data_smpl": torch.empty((B, T, 147), device=dev), "data_obj": torch.empty((B, T, obj_dim), device=dev),
             "gt_smpl": torch.empty((B, T, 147), device=dev), "gt_obj": torch.empty((B, T, obj_dim), device=dev),
             "mask_obj": torch.empty((B, T), dtype=torch.bool, device=dev), "mask_smpl": torch.empty((B, T), dtype=torch.bool, device=dev)}
        ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
        L.check(L.lib().vt_clip_build(*[tables[k].data_ptr() for k, _ in CLIP_TABLES], N, w2c_R.data_ptr(), w2c_t.data_ptr(), nd, start.data_ptr(), date.data_ptr(),
                                      decisions["kid"].data_ptr(), decisions["drop_len"].data_ptr(), decisions["start_fr"].data_ptr(), ptr(au if aug_num else None),
                                      B, T, obj_dim, aug_num, ptr(noise if aug_num else None), ptr(clip_index if aug_num and noise is None else None), seed, epoch,
                                      o["data_smpl"].data_ptr(), o["data_obj"].data_ptr(), o["gt_smpl"].data_ptr(), o["gt_obj"].data_ptr(),
                                      o["mask_obj"].data_ptr(), o["mask_smpl"].data_ptr(), L.stream_ptr()))
    return o
