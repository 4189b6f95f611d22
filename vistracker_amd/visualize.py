"""Step 7 of the demo (scripts/demo.sh: render/render_side_comp.py): the fitted SMPL-H body and object, shaded, on a checkerboard ground, seen from
two Kinect cameras next to the input image.

Drop-ins for the reference's callables (render/nr_utils.py, render/checkerboard.py, render/render_recon.py, render/render_side_comp.py,
behave/kinect_transform.py, behave/utils.py:41-70) with their signatures.  neural_renderer is replaced by the HIP rasteriser of
``csrc/render.hip`` (``vt_render_rgb``; its rule is written down in that file's header): ``setup_renderer`` returns a parameter object in place of
an ``nr.Renderer``.  The ground is rendered as a *static layer*: set up, binned and resolved once per camera, then the seed of every view's
resolve (bit-identical to rendering the concatenated scene).  The video is ``video.write_video`` (Motion-JPEG AVI, GPU JPEG encoder; frames from
``render_frames(..., on_device=True)`` never leave the device).  Contacts (``viz_contact``: one sphere per touching body part, or the touched object
faces recoloured) come from ``csrc/contact.hip`` through ``ContactVisualizer``; the ``-add_top`` view is the same rasteriser behind a look-at
transform, over the ``xy`` ground.  ``overlay`` draws the fit on the camera image and ``mask_scores`` counts its overlap with the input masks
(``csrc/overlay.hip``).  Not here: ``cv2.putText`` labels (no cv2), ``-w`` Procrustes alignment, PHOSA, lens distortion.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import os.path as osp
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib as L
from . import ops
from .sequence_io import device_mask_scores, device_panels, mask_sources, panel_sources, resize_bilinear_hw

# render/nr_utils.py:282-296
SMPL_OBJ_COLOR_LIST = [
    [0.65098039, 0.74117647, 0.85882353],  # SMPL
    [251 / 255.0, 128 / 255.0, 114 / 255.0],  # object
]
COLOR_LIST3 = [
    [0.65098039, 0.74117647, 0.85882353],  # SMPL
    [251 / 255.0, 128 / 255.0, 114 / 255.0],  # object
    [23 / 255., 190 / 255., 207 / 255.],  # 3rd color
]
KINECT_SIZE = 2048.
NEAR, FAR = 0.1, 100.0          # neural_renderer defaults; the kernel's clipping planes


class Mesh:
    """the part of psbody.mesh.Mesh step 7 uses: vertices ``v``, faces ``f``, face colours ``fc``"""

    def __init__(self, v=None, f=None, fc=None):
        self.v = None if v is None else np.asarray(v)
        if f is not None:
            self.f = np.asarray(f)
        if fc is not None:
            self.fc = np.asarray(fc)


# ---- render/checkerboard.py ------------------------------------------------------------------------------------------------------------------
class CheckerBoard:
    def __init__(self, white=(247, 246, 244), black=(146, 163, 171)):
        self.white = np.array(white) / 255.
        self.black = np.array(black) / 255.
        self.verts, self.faces, self.texts = None, None, None
        self.offset = None
        self.checker_mesh = None

    def init_checker(self, offset, plane='xz', xlength=50, ylength=50, square_size=0.5):
        """checkerboard.py:21-44: the xy board, rotated about x by 90 degrees for 'xz', then offset"""
        checker = self.gen_checker_xy_no_repeat(self.black, self.white, square_size, xlength, ylength)
        rot = np.eye(3)
        if plane == 'xz':
            rot[1, 1] = rot[2, 2] = 0
            rot[1, 2] = -1
            rot[2, 1] = 1
        elif plane != 'xy':
            raise NotImplementedError(plane)
        checker.v = np.matmul(checker.v, rot.T)
        self.checker_mesh = checker
        checker.v += offset
        self.offset = offset
        self.verts, self.faces, self.texts = self.prep_checker_rend(checker)

    def get_rends(self):
        return self.verts, self.faces, self.texts

    def append_checker(self, checker):
        v, f, t = checker.get_rends()
        nv = self.verts.shape[1]
        self.verts = torch.cat([self.verts, v], 1)
        self.faces = torch.cat([self.faces, f + nv], 1)
        self.texts = torch.cat([self.texts, t], 1)

    @staticmethod
    def prep_checker_rend(checker: Mesh):
        """(1,NV,3) float32, (1,NF,3) int64, (1,NF,1,1,1,3) float32 -- host tensors (the renderer uploads them once, as a static layer)"""
        verts = torch.from_numpy(checker.v.astype(np.float32)).unsqueeze(0)
        faces = torch.from_numpy(checker.f.astype(np.int64)).unsqueeze(0)
        texts = torch.from_numpy(np.asarray(checker.fc, np.float32)).reshape(1, -1, 1, 1, 1, 3)
        return verts, faces, texts

    @staticmethod
    def gen_checker_xy_no_repeat(black, white, square_size=0.5, xlength=5.0, ylength=5.0, vc=False):
        """checkerboard.py:83-145: an xy board, normal +z, no repeated vertices; faces in the order of the reference's i (x) outer, j (y) inner
        loops, two per square, squares with (i + j) even black"""
        xsquares = int(xlength / square_size)
        ysquares = int(ylength / square_size)
        verts_count = (xsquares + 1) * (ysquares + 1)
        x, y = np.arange(0, (xsquares + 1) * square_size, square_size), np.arange(0, (ysquares + 1) * square_size, square_size)
        x, y = x[:xsquares + 1], y[:ysquares + 1]
        xv, yv = np.meshgrid(x, y)
        verts_all = np.stack((xv, yv, np.zeros_like(xv)), -1).reshape((verts_count, 3))
        i, j = np.meshgrid(np.arange(xsquares), np.arange(ysquares), indexing="ij")
        i, j = i.reshape(-1), j.reshape(-1)
        w = xsquares + 1
        f1 = np.stack([j * w + i, (j + 1) * w + i + 1, (j + 1) * w + i], -1)
        f2 = np.stack([j * w + i, j * w + i + 1, (j + 1) * w + i + 1], -1)
        faces = np.stack([f1, f2], 1).reshape(-1, 3)
        col = np.where(((i + j) % 2 == 0)[:, None], np.asarray(black, np.float64)[None], np.asarray(white, np.float64)[None])
        return Mesh(v=verts_all, f=faces, fc=np.repeat(col, 2, 0))


# ---- render/nr_utils.py: cameras, scene layout -------------------------------------------------------------------------------------------------
def get_intercap_K(image_size=1920, kid=0):
    """nr_utils.py:480-497"""
    ICAP_SIZE = 1920
    assert kid in [0, 1, 2, 3, 4, 5], f'invalid kinect index {kid}!'
    focals = np.array([[918.457763671875, 918.4373779296875], [915.29962158203125, 915.1966552734375],
                       [912.8626708984375, 912.67633056640625], [909.82025146484375, 909.62469482421875],
                       [920.533447265625, 920.09722900390625], [909.17633056640625, 909.23529052734375]])
    centers = np.array([[956.9661865234375, 555.944580078125], [956.664306640625, 551.6165771484375],
                        [956.72003173828125, 554.2166748046875], [957.6181640625, 554.60296630859375],
                        [958.4615478515625, 550.42987060546875], [956.14801025390625, 555.01593017578125]])
    fx, fy = focals[kid]
    cx, cy = centers[kid]
    ratio = image_size / ICAP_SIZE
    return torch.tensor([[[fx * ratio, 0, cx * ratio], [0, fy * ratio, cy * ratio], [0, 0, 1]]], dtype=torch.float32), ratio


def get_kinect_K(image_size=2048, kid=1):
    """nr_utils.py:499-525"""
    assert kid in [0, 1, 2, 3], f'invalid kinect index {kid}!'
    fx, fy, cx, cy = {0: (976.212, 976.047, 1017.958, 787.313), 1: (979.784, 979.840, 1018.952, 779.486),
                      2: (974.899, 974.337, 1018.747, 786.176), 3: (972.873, 972.790, 1022.0565, 770.397)}[kid]
    ratio = image_size / KINECT_SIZE
    return torch.tensor([[[fx * ratio, 0, cx * ratio], [0, fy * ratio, cy * ratio], [0, 0, 1]]], dtype=torch.float32), ratio


class RenderParams(SimpleNamespace):
    """what nr.Renderer(image_size, K, R, t, orig_size) holds after setup_renderer (nr_utils.py:567-577) plus neural_renderer's defaults"""

    def light(self) -> np.ndarray:
        return np.array([self.light_intensity_ambient, self.light_intensity_direction, *self.light_color_ambient, *self.light_color_directional,
                         *self.light_direction], np.float32)

    def key(self):
        return (self.image_size, bool(self.anti_aliasing), float(self.orig_size), self.K.numpy().tobytes(), self.R.numpy().tobytes(),
                self.t.numpy().tobytes(), self.light().tobytes())


def setup_renderer(view='front', rotate=False, image_size=2048, kid=1, distort=False, dataset_name='behave', R=None, T=None):
    """nr_utils.py:534-577 -> RenderParams (light [1, 0.5, 1], directional 0.3, ambient 0.4, white background, anti-aliasing, fill_back)"""
    assert dataset_name in ['behave', 'InterCap']
    if distort:
        raise NotImplementedError("lens distortion is not part of step 7 (every call of the demo passes distort=False)")
    w, func = (2048, get_kinect_K) if dataset_name == 'behave' else (1920, get_intercap_K)
    K, ratio = func(image_size, kid)
    if R is None:
        if view == 'front':
            R = torch.tensor([[[-1., 0, 0], [0, -1, 0], [0, 0, 1]]] if rotate else [[[1., 0, 0], [0, 1, 0], [0, 0, 1]]])
            t = torch.zeros(1, 3)
        elif view == 'top':
            theta, d = 1.3, 1.3
            x, y = np.cos(theta), np.sin(theta)
            R = torch.tensor([[[1, 0, 0], [0, x, -y], [0, y, x]]], dtype=torch.float32)
            t = torch.tensor([0., 0. + d, 2.5])
        else:
            raise NotImplementedError(view)
    else:
        t = T
    return RenderParams(image_size=image_size, K=K, R=torch.as_tensor(R, dtype=torch.float32).reshape(1, 3, 3).cpu(),
                        t=torch.as_tensor(t, dtype=torch.float32).reshape(1, 3).cpu(), orig_size=w * ratio,
                        light_direction=[1, 0.5, 1], light_intensity_direction=0.3, light_intensity_ambient=0.4,
                        light_color_ambient=[1, 1, 1], light_color_directional=[1, 1, 1], background_color=[1, 1, 1],
                        anti_aliasing=True, fill_back=True, near=NEAR, far=FAR)


def get_faces_and_textures(verts_list, faces_list, colors_list=SMPL_OBJ_COLOR_LIST):
    """nr_utils.py:381-415: faces (1,F,3) with per-mesh vertex offsets, one colour per face (1,F,1,1,1,3)"""
    all_faces, all_tex = [], []
    o = 0
    for verts, faces, colors in zip(verts_list, faces_list, colors_list):
        B = len(verts)
        index_offset = torch.arange(B).to(verts.device) * verts.shape[1] + o
        o += verts.shape[1] * B
        faces_repeat = faces.clone().repeat(B, 1, 1)
        faces_repeat += index_offset.view(-1, 1, 1)
        faces_repeat = faces_repeat.reshape(-1, 3)
        all_faces.append(faces_repeat)
        all_tex.append(torch.tensor(colors, dtype=torch.float32, device=verts.device).repeat(faces_repeat.shape[0], 1, 1, 1, 1))
    return torch.cat(all_faces).unsqueeze(0), torch.cat(all_tex).unsqueeze(0)


# ---- the rasteriser ------------------------------------------------------------------------------------------------------------------------
class StaticLayer:
    """vt_render_static_create: a part of the scene shared by every view of one camera (verts already in its coordinates)"""

    def __init__(self, verts, faces, colors, params: RenderParams, device="cuda:0"):
        dev = torch.device(device)
        self.params_key, self.NS = params.key(), int(faces.shape[0])
        v = torch.as_tensor(verts, dtype=torch.float32).reshape(-1, 3).to(dev)
        v = (v @ params.R[0].to(dev).T + params.t[0].to(dev)).contiguous()
        f = torch.as_tensor(np.asarray(faces), dtype=torch.int32).reshape(-1, 3).to(dev).contiguous()
        c = torch.as_tensor(np.asarray(colors), dtype=torch.float32).reshape(-1, 3).to(dev).contiguous()
        K = params.K.reshape(9).to(dev).contiguous()
        light = params.light()
        h = C.c_void_p()
        with torch.cuda.device(dev):
            L.check(L.lib().vt_render_static_create(C.byref(h), L.dptr(v), v.shape[0], L.dptr(f), self.NS, L.dptr(c), L.dptr(K), float(params.orig_size),
                                                    light.ctypes.data_as(C.POINTER(C.c_float)), int(params.image_size), int(bool(params.anti_aliasing)),
                                                    L.stream_ptr()))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                L.lib().vt_render_static_destroy(self.h)
        except Exception:
            pass


class ShadedRasterizer:
    """vt_render_rgb with a cached workspace that grows to the largest tile list seen"""

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        self.ws = None
        self.entries = 0
        self.last_entries = 0

    def render(self, verts, faces, colors, params: RenderParams, static: StaticLayer | None = None, K=None, want_depth=False, want_index=False):
        """verts (B,NV,3) world-of-the-renderer coordinates (R, t of ``params`` are applied here), faces (NF,3), colors (NF,3) or one table per
        view (B,NF,3) (vt_render_rgb_pv) -> dict of rgb (B,S,S,3), alpha (B,S,S), depth, face_index (device tensors)"""
        if not params.fill_back or params.near != NEAR or params.far != FAR:
            raise NotImplementedError("the rasteriser implements neural_renderer's defaults: fill_back, near 0.1, far 100")
        dev = self.device
        v = torch.as_tensor(verts, dtype=torch.float32, device=dev)
        if not (torch.equal(params.R[0], torch.eye(3)) and not params.t.any()):
            v = v @ params.R[0].to(dev).T + params.t[0].to(dev)
        v = v.contiguous()
        B, NV = v.shape[0], v.shape[1]
        f = torch.as_tensor(faces, dtype=torch.int32, device=dev).reshape(-1, 3).contiguous()
        NF = f.shape[0]
        c = torch.as_tensor(colors, dtype=torch.float32, device=dev)
        cpv = int(c.dim() == 3)
        if cpv and c.shape[0] != B:
            raise ValueError(f"per-view colours: {c.shape[0]} tables for {B} views")
        c = c.reshape(-1, 3).contiguous()
        if c.shape[0] != (B if cpv else 1) * NF:
            raise ValueError(f"{c.shape[0]} face colours for {NF} faces")
        size, aa = int(params.image_size), int(bool(params.anti_aliasing))
        if static is not None and static.params_key != params.key():
            raise ValueError("static layer was built for another camera / size / light")
        if K is None:
            Kd, kpv = params.K.reshape(9).to(dev).contiguous(), 0
        else:
            Kd, kpv = torch.as_tensor(K, dtype=torch.float32, device=dev).reshape(B, 9).contiguous(), 1
        rs = size * (2 if aa else 1)
        rgb = torch.empty(B, size, size, 3, device=dev); alpha = torch.empty(B, size, size, device=dev)
        depth = torch.empty(B, size, size, device=dev) if want_depth else None
        fidx = torch.empty(B, rs, rs, dtype=torch.int32, device=dev) if want_index else None
        light = params.light(); bg = np.asarray(params.background_color, np.float32)
        need = C.c_long(0)
        want = max(self.entries, 2 * B * NF + B * (rs // 16) ** 2)
        for _ in range(2):
            nbytes = L.lib().vt_render_workspace_bytes(B, NF, size, aa, want)
            if self.ws is None or self.ws.numel() < nbytes:
                self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            args = (L.dptr(Kd), kpv, float(params.orig_size), light.ctypes.data_as(C.POINTER(C.c_float)), bg.ctypes.data_as(C.POINTER(C.c_float)),
                    static.h if static is not None else None, size, aa, L.dptr(rgb), L.dptr(alpha), L.dptr(depth), L.dptr(fidx),
                    L.dptr(self.ws), self.ws.numel(), C.byref(need), L.stream_ptr())
            if cpv:
                rc = L.lib().vt_render_rgb_pv(L.dptr(v), B, NV, L.dptr(f), NF, L.dptr(c), 1, *args)
            else:
                rc = L.lib().vt_render_rgb(L.dptr(v), B, NV, L.dptr(f), NF, L.dptr(c), *args)
            if rc == 0 or need.value <= want:
                break
            want = int(need.value * 1.25) + 1024                            # the list did not fit: grow to it and render again
        L.check(rc)
        self.last_entries = need.value
        self.entries = max(self.entries, want)
        return {"rgb": rgb, "alpha": alpha, "depth": depth, "face_index": fidx}


def panels_u8(rgb, out, view_off, row0, nrows, col0, ncols, row_stride):
    """vt_render_panel_u8: (clip(rgb, 0, 1) * 255).astype(uint8) crops of (B,S,S,3) renders into the uint8 tensor ``out`` at byte offsets view_off (B,)"""
    B, S = rgb.shape[0], rgb.shape[1]
    off = torch.as_tensor(view_off, dtype=torch.int64, device=rgb.device).contiguous()
    L.check(L.lib().vt_render_panel_u8(L.dptr(rgb.contiguous()), B, S, row0, nrows, col0, ncols, out.data_ptr(), L.dptr(off), row_stride, L.stream_ptr()))


class NrWrapper:
    """nr_utils.py:663-808 (the camera-view path).  ``part_labels`` (6890,) body part of every SMPL vertex (paths.load_part_labels,
    synthetic.part_labels): needed for ``viz_contact`` only."""

    def __init__(self, device='cuda:0', image_size=1024, colors=None, contact_viz_type='sphere', dataset_name='behave', kid=1, part_labels=None):
        if contact_viz_type not in ('sphere', 'face'):
            raise ValueError(f"contact_viz_type must be 'sphere' or 'face', not {contact_viz_type!r}")
        self.device = device
        self.contact_viz = None if part_labels is None else ContactVisualizer(part_labels, thres=0.04, radius=0.06, device=device)   # nr_utils.py:417
        self.colors = [list(c) for c in SMPL_OBJ_COLOR_LIST] if colors is None else colors
        self.smpl_color, self.obj_color = SMPL_OBJ_COLOR_LIST[0], SMPL_OBJ_COLOR_LIST[1]
        self.front_renderer = setup_renderer(image_size=image_size, dataset_name=dataset_name, kid=kid)
        self.image_size = image_size
        self.contact_viz_type = contact_viz_type
        self.raster = ShadedRasterizer(device)
        self._layers = {}

    def static_layer(self, renderer: RenderParams, checker: CheckerBoard) -> StaticLayer:
        """the checker of ``renderer`` as a static layer, built once per (checker, camera)"""
        key = (id(checker), renderer.key())
        if key not in self._layers:
            cv, cf, ct = checker.get_rends()
            self._layers[key] = (checker, StaticLayer(cv[0], cf[0], ct.reshape(-1, 3), renderer, self.device))
        return self._layers[key][1]

    def contacts(self):
        if self.contact_viz is None:
            raise ValueError("viz_contact=True needs the SMPL part labels: pass part_labels=(6890,) ints in [0, 14) (paths.load_part_labels(assets_root) "
                             "or synthetic.part_labels(model)) to NrWrapper / RendererSide2side")
        return self.contact_viz

    def prepare_render(self, meshes, viz_contact=False, colors=None, checker=None, radius=None):
        """nr_utils.py:760-799: verts (1,NV,3), faces (1,F,3), textures (1,F,1,1,1,3), ground appended last.  ``viz_contact`` counts for exactly two
        meshes [SMPL, object], like the reference: contact_viz_type 'sphere' appends one sphere per touching part, 'face' recolours the object."""
        render_color = self.colors if colors is None else colors
        verts_list = [torch.as_tensor(np.asarray(m.v), dtype=torch.float32).unsqueeze(0) for m in meshes]
        faces_list = [torch.as_tensor(np.asarray(m.f).astype(np.int32)) for m in meshes]
        color_list = [list(c) for c in list(render_color)[:len(meshes)]]
        regions = self.contacts().get_contact_spheres(meshes[0], meshes[1], radius) if viz_contact and len(meshes) == 2 else {}
        spheres = bool(regions) and self.contact_viz_type == 'sphere'
        if spheres:
            for part in sorted(regions):
                color, sphere, _ = regions[part]
                verts_list.append(torch.as_tensor(sphere.v, dtype=torch.float32).unsqueeze(0))
                faces_list.append(torch.as_tensor(sphere.f.astype(np.int32)))
                color_list.append(list(color))
        faces, textures = get_faces_and_textures(verts_list, faces_list, colors_list=color_list)
        if regions and not spheres:
            cv = self.contact_viz
            part = torch.full((1, verts_list[1].shape[1]), -1, dtype=torch.int32)
            for p, (_, _, ind) in regions.items():
                part[0, torch.as_tensor(ind)] = p
            textures = cv.face_colors(part.to(cv.device), faces_list[1], faces_list[0].shape[0], textures.reshape(-1, 3)).cpu().reshape(1, -1, 1, 1, 1, 3)
        verts = torch.cat(verts_list, 1)
        if checker is not None:
            cv, cf, ct = checker.get_rends()
            faces = torch.cat([faces, verts.shape[1] + cf.to(faces.dtype)], 1)
            textures = torch.cat([textures, ct], 1)
            verts = torch.cat([verts, cv], 1)
        return verts, faces, textures

    def render_meshes(self, renderer, meshes: list, viz_contact=False, ret_depth=False, checker=None, colors=None):
        """-> rend (H,W,3) float32 in [0, 1], mask (H,W) bool (and depth): NrWrapper.render of the meshes, checker as a static layer"""
        verts, faces, textures = self.prepare_render(meshes, viz_contact, colors=colors)
        layer = self.static_layer(renderer, checker) if checker is not None else None
        out = self.raster.render(verts, faces[0], textures.reshape(-1, 3), renderer, static=layer, want_depth=ret_depth)
        rend = np.clip(out["rgb"][0].cpu().numpy(), 0, 1)
        mask = out["alpha"][0].cpu().numpy().astype(bool)
        if ret_depth:
            return rend, mask, out["depth"][0].cpu().numpy()
        return rend, mask


# ---- contacts: render/nr_utils.py:359-404 (ContactVisualizer), :100-122 (contact-coloured faces) --------------------------------------------------
PARTS_NUM = 14
# this project's own palette for the 14 body parts: hues 360 / 14 degrees apart at alternating value, so that neighbours in the list differ clearly
PART_COLORS = np.array([[0.90, 0.10, 0.10], [0.55, 0.30, 0.05], [0.95, 0.75, 0.10], [0.45, 0.55, 0.05], [0.45, 0.90, 0.10], [0.05, 0.55, 0.15],
                        [0.10, 0.90, 0.55], [0.05, 0.50, 0.50], [0.10, 0.70, 0.95], [0.05, 0.25, 0.60], [0.35, 0.25, 0.95], [0.40, 0.05, 0.60],
                        [0.90, 0.15, 0.90], [0.60, 0.05, 0.30]], np.float64)


def icosphere(subdivisions=2):
    """Unit sphere template of the contact spheres: an icosahedron, every triangle split in four ``subdivisions`` times, vertices pushed to radius 1.
    -> verts (10 * 4^s + 2, 3) float64, faces (20 * 4^s, 3) int32, outward winding.  PARITY UNPINNED: stands in for psbody's Sphere.to_mesh."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    verts = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = verts[a] + verts[b]
                verts.append(x / np.linalg.norm(x)); mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.stack(verts), np.asarray(faces, np.int32)


def look_at_view_transform(eye, at, up):
    """World -> view rotation R (3,3) and translation T (3,) in float64, applied as ``v @ R + T``: z = normalize(at - eye), x = normalize(cross(up, z)),
    y = cross(z, x), R = [x y z] as columns, T = -(eye @ R).  PARITY UNPINNED: restated from pytorch3d's documented look_at_view_transform (not
    installed); its fallback for an ``up`` parallel to the viewing direction is left out -- that case raises."""
    eye, at, up = (np.asarray(a, np.float64).reshape(3) for a in (eye, at, up))
    z = at - eye
    if np.linalg.norm(z) < 1e-12:
        raise ValueError("look_at_view_transform: eye and at coincide")
    z = z / np.linalg.norm(z)
    x = np.cross(up, z)
    if np.linalg.norm(x) < 1e-5:
        raise ValueError("look_at_view_transform: up is parallel to the viewing direction")
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], 1)
    return R, -(eye @ R)


TOP_EYE, TOP_AT, TOP_UP = (0.0, -1.8, 2.5), (0.0, 0.0, 2.4), (0.0, -1.0, 0.0)        # render_side_comp.py:52-66 rend_topviews


class ContactVisualizer:
    """nr_utils.py:359-404 on the device (csrc/contact.hip).  ``part_labels`` (NVs,) ints in [0, P), P = len(part_colors) <= 32."""

    def __init__(self, part_labels, thres=0.04, radius=0.08, part_colors=None, device='cuda:0'):
        self.device = torch.device(device)
        self.part_colors = np.array(PART_COLORS if part_colors is None else part_colors, np.float64).reshape(-1, 3)
        self.P = len(self.part_colors)
        lab = np.asarray(part_labels.cpu() if torch.is_tensor(part_labels) else part_labels).astype(np.int64).reshape(-1)
        if not 0 < self.P <= 32 or lab.size == 0 or lab.min() < 0 or lab.max() >= self.P:
            raise ValueError(f"part labels must lie in [0, {self.P}) (one colour per part, at most 32 parts)")
        self.part_labels = lab.astype(np.int32)
        self.thres, self.radius = float(thres), float(radius)
        self.sphere_v, self.sphere_f = icosphere(2)
        self.labels_d = torch.as_tensor(self.part_labels, device=self.device).contiguous()
        self.unit_d = torch.as_tensor(self.sphere_v, dtype=torch.float32, device=self.device).contiguous()
        self.palette_d = torch.as_tensor(self.part_colors, dtype=torch.float32, device=self.device).contiguous()

    def _verts(self, v):
        v = torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).to(self.device, torch.float32)
        return (v[None] if v.dim() == 2 else v).contiguous()

    def regions(self, smpl_verts, obj_verts):
        """vt_contact_regions: smpl_verts (B,NVs,3), obj_verts (B,NVo,3) -> device tensors nn_idx (B,NVo) int32, nn_dist (B,NVo), part (B,NVo) int32
        (-1 = no contact), count (B,P) int32, centre (B,P,3)"""
        sv, ov = self._verts(smpl_verts), self._verts(obj_verts)
        if sv.shape[0] != ov.shape[0] or sv.shape[1] != len(self.part_labels) or sv.shape[2] != 3 or ov.shape[2] != 3:
            raise ValueError(f"regions: smpl_verts {tuple(sv.shape)} / obj_verts {tuple(ov.shape)} do not match {len(self.part_labels)} part labels")
        B, NVs, NVo, dev = sv.shape[0], sv.shape[1], ov.shape[1], self.device
        out = {"nn_idx": torch.empty(B, NVo, dtype=torch.int32, device=dev), "nn_dist": torch.empty(B, NVo, device=dev),
               "part": torch.empty(B, NVo, dtype=torch.int32, device=dev), "count": torch.empty(B, self.P, dtype=torch.int32, device=dev),
               "centre": torch.empty(B, self.P, 3, device=dev)}
        with torch.cuda.device(dev):
            L.check(L.lib().vt_contact_regions(L.dptr(sv), L.dptr(self.labels_d), L.dptr(ov), B, NVs, NVo, self.P, self.thres, L.dptr(out["nn_idx"]),
                                               L.dptr(out["nn_dist"]), L.dptr(out["part"]), L.dptr(out["count"]), L.dptr(out["centre"]), L.stream_ptr()))
        return out

    def spheres(self, regions, radius=None):
        """vt_contact_spheres -> (B, P * 162, 3): sphere p of every frame, collapsed to one point where part p does not touch"""
        centre, count = regions["centre"], regions["count"]
        B, NSV = centre.shape[0], self.unit_d.shape[0]
        out = torch.empty(B, self.P * NSV, 3, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().vt_contact_spheres(L.dptr(centre), L.dptr(count), B, self.P, L.dptr(self.unit_d), NSV,
                                               float(self.radius if radius is None else radius), L.dptr(out), L.stream_ptr()))
        return out

    def sphere_faces_colors(self, vert_offset):
        """faces (P * 320, 3) int32 of the P spheres appended at ``vert_offset``, and their colours (P * 320, 3) float32"""
        NSV, NSF = len(self.sphere_v), len(self.sphere_f)
        f = np.concatenate([self.sphere_f + vert_offset + p * NSV for p in range(self.P)]).astype(np.int32)
        return f, np.repeat(self.part_colors.astype(np.float32), NSF, 0)

    def face_colors(self, part, obj_faces, face_off, base_colors):
        """vt_contact_face_colors: part (B,NVo) -> (B,NF,3) colour tables, the object's faces (rows face_off.. of ``base_colors``) in contact recoloured"""
        part = part.contiguous()
        B, NVo = part.shape
        f = torch.as_tensor(np.asarray(obj_faces.cpu() if torch.is_tensor(obj_faces) else obj_faces).astype(np.int32), device=self.device).reshape(-1, 3).contiguous()
        if f.numel() == 0 or int(f.min()) < 0 or int(f.max()) >= NVo:
            raise ValueError("face_colors: object faces index outside the object's vertices")
        base = torch.as_tensor(base_colors, dtype=torch.float32, device=self.device).reshape(-1, 3).contiguous()
        out = torch.empty(B, base.shape[0], 3, device=self.device)
        with torch.cuda.device(self.device):
            L.check(L.lib().vt_contact_face_colors(L.dptr(part), B, NVo, L.dptr(f), f.shape[0], int(face_off), L.dptr(base), base.shape[0],
                                                   L.dptr(self.palette_d), self.P, L.dptr(out), L.stream_ptr()))
        return out

    def get_contact_spheres(self, smpl: Mesh, obj: Mesh, radius=None):
        """nr_utils.py:380-404 for one mesh pair: {part: (colour, sphere Mesh, indices of the object's contact vertices of that part)}, {} without contact"""
        reg = self.regions(np.asarray(smpl.v), np.asarray(obj.v))
        count = reg["count"][0].cpu().numpy()
        if count.sum() == 0:
            return {}
        part = reg["part"][0].cpu().numpy()
        sph = self.spheres(reg, radius).reshape(self.P, -1, 3).cpu().numpy()
        return {int(p): (self.part_colors[p], Mesh(v=sph[p].astype(np.float64), f=self.sphere_f.copy()), np.nonzero(part == p)[0])
                for p in np.nonzero(count)[0]}


# ---- behave/utils.py:41-70, behave/kinect_transform.py -------------------------------------------------------------------------------------------
def load_kinect_poses(config_folder, kids):
    pose_calibs = [json.load(open(osp.join(config_folder, f"{x}/config.json"))) for x in kids]
    rotations = [np.array(pose_calibs[x]['rotation']).reshape((3, 3)) for x in range(len(kids))]
    translations = [np.array(pose_calibs[x]['translation']) for x in range(len(kids))]
    return rotations, translations


def load_kinect_poses_back(config_folder, kids, rotate=False):
    """world (camera 1 colour frame) -> camera k: the inverse of each {k}/config.json pose"""
    rotations, translations = load_kinect_poses(config_folder, kids)
    rb, tb = [], []
    for r, t in zip(rotations, translations):
        trans = np.eye(4)
        trans[:3, :3] = r
        trans[:3, 3] = t
        back = np.linalg.inv(trans)
        r_back, t_back = back[:3, :3], back[:3, 3]
        if rotate:
            g = np.eye(4); g[0, 0] = g[1, 1] = -1
            rot = np.matmul(g, np.concatenate([np.concatenate([r_back, t_back[:, None]], 1), [[0, 0, 0, 1]]], 0))
            r_back, t_back = rot[:3, :3], rot[:3, 3]
        rb.append(r_back)
        tb.append(t_back)
    return rb, tb


def seq_config_folder(seq):
    """behave/seq_utils.py:48-60: the 'config' entry of <seq>/info.json, relative to the sequence unless that is no folder"""
    info = json.load(open(osp.join(seq, 'info.json')))
    path = osp.join(seq, info['config'])
    kids = list(range(len(info['kinects']) if 'kinects' in info else 3))
    return (path if osp.isdir(path) else info['config']), kids


class KinectTransform:
    """world (camera 1 colour frame) <-> camera k.  ``KinectTransform(seq)`` reads the sequence's config folder like the reference (intrinsics are not
    loaded: step 7 passes no_intrinsic=True); ``KinectTransform(world2local_R=[...], world2local_t=[...])`` takes the per-camera arrays directly."""

    def __init__(self, seq=None, kinect_count=4, no_intrinsic=True, world2local_R=None, world2local_t=None):
        if not no_intrinsic:
            raise NotImplementedError("Kinect intrinsics (behave/kinect_calib.py) are not needed by step 7")
        self.intrinsics = None
        if seq is not None:
            config, self.kids = seq_config_folder(seq)
            self.local2world_R, self.local2world_t = load_kinect_poses(config, self.kids)
            self.world2local_R, self.world2local_t = load_kinect_poses_back(config, self.kids)
        else:
            self.world2local_R = [np.asarray(r, np.float64).reshape(3, 3) for r in world2local_R]
            self.world2local_t = [np.asarray(t, np.float64).reshape(3) for t in world2local_t]
            self.kids = list(range(len(self.world2local_R)))
            inv = [np.linalg.inv(np.concatenate([np.concatenate([r, t[:, None]], 1), [[0, 0, 0, 1]]], 0)) for r, t in zip(self.world2local_R, self.world2local_t)]
            self.local2world_R, self.local2world_t = [m[:3, :3] for m in inv], [m[:3, 3] for m in inv]

    def world2local(self, points, kid):
        return np.matmul(points, self.world2local_R[kid].T) + self.world2local_t[kid]

    def local2world(self, points, kid):
        return np.matmul(points, self.local2world_R[kid].T) + self.local2world_t[kid]

    def world2color_mesh(self, mesh, kid):
        m = Mesh(v=self.world2local(mesh.v, kid), f=getattr(mesh, 'f', None))
        return m

    def world2local_meshes(self, meshes, kid):
        return [self.world2color_mesh(m, kid) for m in meshes]

    def world2local_torch(self, verts, kid):
        """device version for batches: verts (..., 3) tensor"""
        R = torch.as_tensor(self.world2local_R[kid], dtype=torch.float32, device=verts.device)
        t = torch.as_tensor(self.world2local_t[kid], dtype=torch.float32, device=verts.device)
        return verts @ R.T + t


def object_verts(temp_v, obj_angles, obj_trans, obj_scales):
    """render_recon.py:323-324 (prepare_verts): (temp.v @ obj_angles + obj_trans) * obj_scales, numpy in, numpy out (float64 like the reference)"""
    v = np.matmul(np.asarray(temp_v)[None], np.asarray(obj_angles)) + np.asarray(obj_trans)[:, None]
    return v * np.asarray(obj_scales).reshape(-1, 1, 1)


# ---- render/render_side_comp.py + render_recon.py:render_seq ---------------------------------------------------------------------------------
class RendererSide2side:
    """Side-by-side frames: [input rgb | camera kid recon_1 .. recon_n | camera kid + 1 recon_1 .. recon_n], each panel the rows [:0.75 size] and
    columns [0.2 size, 0.8 size) of a size x size render (render_side_comp.py:71-98, render_recon.py:41-160).  Camera 1's intrinsics render every
    view (the reference's single front renderer, NrWrapper(kid=1)).  ``part_labels`` / ``contact_viz_type``: see NrWrapper (for ``viz_contact``)."""

    def __init__(self, image_size=1200, gender='male', dataset_name='behave', kid=None, device='cuda:0', xcut_start=0.2, xcut_end=0.8,
                 part_labels=None, contact_viz_type='sphere'):
        self.test_id = (1 if dataset_name == 'behave' else 0) if kid is None else kid
        self.aspect_ratio = 0.75 if dataset_name == 'behave' else 9 / 16.
        self.nrwrapper = NrWrapper(image_size=image_size, colors=COLOR_LIST3, dataset_name=dataset_name, device=device, part_labels=part_labels,
                                   contact_viz_type=contact_viz_type)
        self._ground_xy = None
        R, T = look_at_view_transform(TOP_EYE, TOP_AT, TOP_UP)
        self.top_R, self.top_T = R.astype(np.float32), T.astype(np.float32)
        checker_xz = CheckerBoard()
        psize = 80.0
        checker_xz.init_checker(np.array([-psize / 2., 1.5, -psize / 2.]), 'xz', square_size=0.5, xlength=psize, ylength=psize)
        self.ground_xz = checker_xz
        self.image_size, self.device = image_size, device
        self.xcut_start, self.xcut_end = xcut_start, xcut_end

    def get_xcuts(self, image_size):
        return int(self.xcut_start * image_size), int(self.xcut_end * image_size)

    def frame_shape(self, n_recons, overlay=False):
        cs, ce = self.get_xcuts(self.image_size)
        return int(self.aspect_ratio * self.image_size), (ce - cs) * (1 + (3 if overlay else 2) * n_recons), 3

    @property
    def ground_xy(self):
        """render_recon.py:59-62: the xy board of the top view, built on first use"""
        if self._ground_xy is None:
            ck = CheckerBoard()
            ck.init_checker(np.array([-40., -40., 4.0]), 'xy', square_size=0.75, xlength=80, ylength=80)
            self._ground_xy = ck
        return self._ground_xy

    def top_shape(self, n_recons):
        """shape of a top-view strip [rgb panel | top view of recon_1 .. recon_n] after the cut of its top 0.3 (render_recon.py:172-178)"""
        H, _, _ = self.frame_shape(n_recons)
        cs, ce = self.get_xcuts(self.image_size)
        return H - int(0.3 * H), (ce - cs) * (1 + n_recons), 3

    def top_transform(self, verts):
        """packed coordinates -> the top view's camera (render_side_comp.py:52-66): v @ R + T of look_at_view_transform(TOP_EYE, TOP_AT, TOP_UP), in
        fp32, term by term (x R[0] + y R[1]) + z R[2] + T so that the result does not depend on the batch shape"""
        R = torch.as_tensor(self.top_R, device=verts.device); T = torch.as_tensor(self.top_T, device=verts.device)
        return (verts[..., 0:1] * R[0] + verts[..., 1:2] * R[1]) + verts[..., 2:3] * R[2] + T

    def _scene(self, temp_v, temp_f, smpl_handle, viz_contact=False):
        """what every chunk of a sequence shares: the face list [SMPL-H, object (, 14 contact spheres)] and its colours on the device, the object template"""
        dev = torch.device(self.device)
        temp_f = np.asarray(temp_f)
        smpl_f = np.asarray(smpl_handle.faces)
        nvs = 6890
        faces = np.concatenate([smpl_f, temp_f + nvs], 0).astype(np.int32)
        colors = np.concatenate([np.tile(np.asarray(self.nrwrapper.colors[0], np.float32), (len(smpl_f), 1)),
                                 np.tile(np.asarray(self.nrwrapper.colors[1], np.float32), (len(temp_f), 1))], 0)
        tv = torch.as_tensor(np.asarray(temp_v), dtype=torch.float32, device=dev)
        nv_mesh = nvs + tv.shape[0]
        cviz = self.nrwrapper.contacts() if viz_contact else None
        spheres = viz_contact and self.nrwrapper.contact_viz_type == 'sphere'
        if spheres:
            sf, sc = cviz.sphere_faces_colors(nv_mesh)
            faces, colors = np.concatenate([faces, sf], 0), np.concatenate([colors, sc], 0)
        return SimpleNamespace(temp_f=temp_f, nf_body=len(smpl_f), nf_obj=len(temp_f), tv=tv, nv_mesh=nv_mesh, cviz=cviz, spheres=spheres,
                               faces_d=torch.as_tensor(faces, device=dev), colors_d=torch.as_tensor(colors, device=dev))

    def _chunk_meshes(self, sc, recons, smpl_handle, idx):
        """frames ``idx`` of every recon in packed coordinates: per recon (len(idx), NV, 3) [SMPL-H, object (, spheres)] vertices, and, for contact-coloured
        faces, per recon (len(idx), NF, 3) colour tables (else an empty list)"""
        dev = sc.tv.device
        nc = len(idx)
        ii = torch.as_tensor(idx, device=dev)
        per_recon, per_colors = [], []
        for d in recons:
            T = len(d["poses"])
            g = lambda k, w: torch.as_tensor(np.asarray(d[k], np.float32).reshape(T, w), device=dev)[ii].contiguous()
            sv, _, _ = ops.smplh_forward(smpl_handle, g("poses", 156), g("betas", 10), g("trans", 3))
            R = g("obj_angles", 9).reshape(nc, 3, 3); t = g("obj_trans", 3); s = g("obj_scales", 1)
            ov = (sc.tv[None] @ R + t[:, None]) * s[:, :, None]
            block = [sv.detach(), ov]
            if sc.cviz is not None:
                reg = sc.cviz.regions(block[0], ov)
                if sc.spheres:
                    block.append(sc.cviz.spheres(reg))
                else:
                    per_colors.append(sc.cviz.face_colors(reg["part"], sc.temp_f, sc.nf_body, sc.colors_d))
            per_recon.append(torch.cat(block, 1))
        return per_recon, per_colors

    def fit_views(self, sc, per_recon, per_colors, kin):
        """the camera-``test_id`` view of every (frame, recon) of a chunk WITHOUT the ground: no static layer, background 0, the chunk's own face list (contact
        spheres or per-view colours included) -> vt_render_rgb's dict, views frame-major (frame j, recon r at j * n + r): rgb premultiplied by coverage, alpha,
        face_index (the owner map vt_mask_score reads).  What ``overlay`` composites and ``mask_scores`` scores."""
        renderer = self.nrwrapper.front_renderer
        bare = RenderParams(**{**vars(renderer), "background_color": [0.0, 0.0, 0.0]})
        views = torch.stack([kin.world2local_torch(v, self.test_id) for v in per_recon], 1)               # (nc, n, NV, 3)
        nc, n = views.shape[0], views.shape[1]
        views = views.reshape(nc * n, views.shape[-2], 3).contiguous()
        if bool((views[:, :sc.nv_mesh, 2].amin() < 0).item()):
            raise ValueError("a mesh lies behind the camera (render_side_comp.py:86-90 allows that for PHOSA only)")
        cols = torch.stack(per_colors, 1).reshape(nc * n, -1, 3) if per_colors else sc.colors_d
        return self.nrwrapper.raster.render(views, sc.faces_d, cols, bare, static=None, want_index=True)

    def mask_scores(self, recons, temp_v, temp_f, smpl_handle, kin, masks, start=0, end=None, interval=1, chunk=8, decode_workers=0):
        """Which frames went wrong, without ground truth: the overlap of the fit's owner map (``fit_views``: what is VISIBLE of the body and of the object from
        camera ``test_id``) with the frame's person and object masks, counted by vt_mask_score (csrc/overlay.hip) over the panel's rows [0, H) of the render.
        ``masks``: a sequence or a callable frame index -> a (person, object) pair of uint8 arrays ((h,w) or (h,w,C), channel 0 counts, on when > 127), the ``str``
        path of the frame's colour image (its masks are found and decoded by ``sequence_io.decode_masks``) or a pair of uint8 device tensors (read in place).
        Host masks of a chunk go through one pinned buffer and one upload; ``decode_workers=N`` fetches and decodes the next chunk's in the loader's pool (at most
        16 threads).  One synchronisation per chunk, the read-back of the counts.
        -> {"count": (n_frames, n_recons, 2, 4) int32: per class (0 body against the person mask, 1 object against the object mask) inter, fit, mask, hidden (the
        mask is on and the OTHER class owns the sample: discounts occlusion when the object mask is a full, unoccluded rendering); "iou": (n_frames, n_recons, 2)
        float64 inter / (fit + mask - inter), nan where that union is 0}."""
        dev = torch.device(self.device)
        size = self.image_size
        H = self.frame_shape(len(recons))[0]
        n = len(recons)
        T = len(recons[0]["poses"])
        end = T if end is None else end
        frames = list(range(start, end, interval))
        sc = self._scene(temp_v, temp_f, smpl_handle)
        F = int(sc.faces_d.shape[0])
        sources = mask_sources(masks, frames, chunk, decode_workers)
        counts = []
        with torch.cuda.device(dev):
            for c0 in range(0, len(frames), chunk):
                idx = frames[c0:c0 + chunk]
                pairs = next(sources)                                               # with a pool, the next chunk's are being decoded from here on
                per_recon, per_colors = self._chunk_meshes(sc, recons, smpl_handle, idx)
                fidx = self.fit_views(sc, per_recon, per_colors, kin)["face_index"]
                rows = H * fidx.shape[1] // size
                cnt = device_mask_scores(pairs, fidx, rows, F, sc.nf_body, sc.nf_obj, n)
                counts.append(cnt.cpu().numpy().reshape(len(idx), n, 2, 4))       # the one synchronisation of the chunk
        count = np.concatenate(counts) if counts else np.zeros((0, n, 2, 4), np.int32)
        c = count.astype(np.int64)
        union = c[..., 1] + c[..., 2] - c[..., 0]
        iou = np.where(union > 0, c[..., 0] / np.maximum(union, 1), np.nan)
        return {"count": count, "iou": iou}

    def render_frames(self, recons, temp_v, temp_f, smpl_handle, kin, rgb=None, start=0, end=None, interval=1, chunk=8, on_device=False,
                      viz_contact=False, add_top=False, device_panel=False, decode_workers=0, overlay=False, overlay_opacity=0.6):
        """Generator of uint8 frame chunks (n, H, W, 3) for frames start:end:interval of the packed ``recons`` (dicts with poses (T,156), betas,
        trans, obj_angles (T,3,3), obj_trans, obj_scales).  ``smpl_handle``: ops.SmplhHandle of the sequence's SMPL-H model; ``kin``: KinectTransform;
        ``rgb``: None (black panel), a sequence or a callable frame index -> (h,w,3) uint8 image of camera test_id.  Every chunk renders
        chunk x 2 x len(recons) views in one vt_render_rgb call, the ground as one static layer.  ``on_device=True`` yields the chunks as uint8 device
        tensors (for ``video.write_video``) instead of host arrays.

        ``viz_contact``: the contact search (ContactVisualizer.regions) runs once per (frame, recon) in packed coordinates; with contact_viz_type
        'sphere' the 14 spheres of every recon join its vertex block before the camera transforms (parts that do not touch collapse to a point:
        zero-area faces, culled by the rasteriser's set-up), with 'face' every view gets its own face-colour table.  ``add_top``: the generator
        yields (frames, top_frames) pairs, top_frames (n,) + top_shape(len(recons)): [rgb panel | top-down view of every recon] over the xy ground
        (render_side_comp.py:52-66, render_recon.py:172-178).  Every frame is written: the reference loses the first top-view frame while it opens
        its second writer, which is not copied.

        ``device_panel=True`` builds the camera panel with vt_resize_panel_u8 (csrc/inputs.hip) instead of ``resize_bilinear_hw`` on the host, frame by
        frame: ``rgb`` may then also give ``str`` paths (decoded with the loader's ``_load_image``) or uint8 device tensors (read in place); host images
        of a chunk are staged -- only the columns the panel reads -- into one pinned buffer and uploaded once.  ``decode_workers=N`` fetches and decodes
        the images of the next chunk in a pool of at most 16 threads while this one is rendered.  The frames are the default path's wherever the fp32
        blends are exact (e.g. 96 x 128 images for image_size 64), elsewhere within one grey level at pixels whose blend sits on a rounding boundary.

        ``overlay=True`` (needs ``rgb``) draws the fit ON the camera image: a frame becomes [rgb | overlay recon_1 .. recon_n | camera kid recon_1 .. | camera
        kid + 1 recon_1 ..], every overlay panel the frame's own camera panel with the ground-free camera-kid render of that recon (``fit_views``) composited at
        ``overlay_opacity`` by vt_overlay_panel_u8 (csrc/overlay.hip) -- the panel is that camera's image and the render uses that camera's intrinsics, so
        the two are pixel-aligned.  Every other panel, and the top strips, keep their bytes."""
        if decode_workers > 0 and not device_panel:
            raise ValueError("decode_workers needs device_panel=True")
        if overlay and rgb is None:
            raise ValueError("overlay=True needs the camera images (rgb): there is nothing to draw the fit on")
        if overlay and not 0.0 <= float(overlay_opacity) <= 1.0:
            raise ValueError(f"overlay_opacity {overlay_opacity} outside [0, 1]")
        dev = torch.device(self.device)
        size = self.image_size
        cs, ce = self.get_xcuts(size)
        H, W, _ = self.frame_shape(len(recons), overlay)
        pw = ce - cs
        n = len(recons)
        T = len(recons[0]["poses"])
        end = T if end is None else end
        frames = list(range(start, end, interval))
        renderer = self.nrwrapper.front_renderer
        layer = self.nrwrapper.static_layer(renderer, self.ground_xz)
        sc = self._scene(temp_v, temp_f, smpl_handle, viz_contact)
        faces_d, colors_d, nv_mesh = sc.faces_d, sc.colors_d, sc.nv_mesh
        first = 1 + (n if overlay else 0)                                   # panel index of camera kid's first render
        if add_top:
            top_layer = self.nrwrapper.static_layer(renderer, self.ground_xy)
            Ht, Wt, _ = self.top_shape(n)
            cut = H - Ht
        kids = [self.test_id, self.test_id + 1]
        sources = panel_sources(rgb, frames, chunk, decode_workers) if device_panel and rgb is not None else None
        with torch.cuda.device(dev):
            for c0 in range(0, len(frames), chunk):
                idx = frames[c0:c0 + chunk]
                nc = len(idx)
                images = next(sources) if sources is not None else None          # with a pool, the next chunk's are being decoded from here on
                per_recon, per_colors = self._chunk_meshes(sc, recons, smpl_handle, idx)
                views = torch.stack([torch.stack([kin.world2local_torch(v, k) for v in per_recon], 1) for k in kids], 1)   # (nc, 2, n, NV, 3)
                views = views.reshape(nc * 2 * n, views.shape[-2], 3).contiguous()
                if bool((views[:, :nv_mesh, 2].amin() < 0).item()):
                    raise ValueError("a mesh lies behind the camera (render_side_comp.py:86-90 allows that for PHOSA only)")
                cols = colors_d
                if per_colors:                                                      # (nc, n, NF, 3): the same table for both cameras of a frame
                    pc = torch.stack(per_colors, 1)
                    cols = pc[:, None].expand(nc, 2, n, *pc.shape[2:]).reshape(nc * 2 * n, -1, 3)
                out = self.nrwrapper.raster.render(views, faces_d, cols, renderer, static=layer)
                buf = torch.zeros(nc, H, W, 3, dtype=torch.uint8, device=dev)
                b = torch.arange(nc * 2 * n, device=dev)
                off = (b // (2 * n)) * (H * W * 3) + (first + b % (2 * n)) * (pw * 3)
                panels_u8(out["rgb"], buf, off, 0, H, cs, pw, W * 3)
                if images is not None:
                    device_panels(images, buf, size, cs, ce)
                elif rgb is not None:
                    for j, i in enumerate(idx):
                        img = rgb(i) if callable(rgb) else rgb[i]
                        img = resize_bilinear_hw(np.asarray(img), H, size)[:, cs:ce]
                        buf[j, :, :pw] = torch.as_tensor(np.ascontiguousarray(img), device=dev)
                if overlay:                                                          # behind the camera panel, on the same stream
                    fit = self.fit_views(sc, per_recon, per_colors, kin)
                    b = torch.arange(nc * n, device=dev)
                    src = (b // n) * (H * W * 3)
                    ops.overlay_panel_u8(fit["rgb"], fit["alpha"], buf, src, src + (1 + b % n) * (pw * 3), 0, H, cs, pw, W * 3, float(overlay_opacity))
                if not add_top:
                    yield buf if on_device else buf.cpu().numpy()
                    continue
                tviews = self.top_transform(torch.stack(per_recon, 1)).reshape(nc * n, -1, 3).contiguous()
                tcols = torch.stack(per_colors, 1).reshape(nc * n, -1, 3) if per_colors else colors_d
                tout = self.nrwrapper.raster.render(tviews, faces_d, tcols, renderer, static=top_layer)
                tbuf = torch.zeros(nc, Ht, Wt, 3, dtype=torch.uint8, device=dev)
                b = torch.arange(nc * n, device=dev)
                panels_u8(tout["rgb"], tbuf, (b // n) * (Ht * Wt * 3) + (1 + b % n) * (pw * 3), cut, Ht, cs, pw, Wt * 3)
                tbuf[:, :, :pw] = buf[:, cut:, :pw]
                yield (buf, tbuf) if on_device else (buf.cpu().numpy(), tbuf.cpu().numpy())


def write_frames(frames, outdir, start=0, prefix="frame"):
    """Write frames (an iterable of (H,W,3) uint8 frames or of (n,H,W,3) chunks) as PNG through PIL, or .npy where PIL is absent.  Returns the paths."""
    os.makedirs(outdir, exist_ok=True)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    paths, k = [], start
    for ch in frames:
        ch = np.asarray(ch)
        for fr in (ch if ch.ndim == 4 else ch[None]):
            if Image is not None:
                p = osp.join(outdir, f"{prefix}_{k:05d}.png"); Image.fromarray(fr).save(p)
            else:
                p = osp.join(outdir, f"{prefix}_{k:05d}.npy"); np.save(p, fr)
            paths.append(p); k += 1
    return paths
