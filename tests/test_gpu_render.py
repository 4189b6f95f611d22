"""GPU: the shaded rasteriser of demo step 7 (csrc/render.hip, vt_render_rgb) and RendererSide2side.render_frames.

The float64 numpy renderer below is written only from the RGB rule stated in render.hip's header (neural_renderer's published behaviour): it shares
no code with the HIP path.  Owner maps must agree except at pixels whose centre lies within rounding of a coverage edge, at the clipping planes,
or where two faces' depths tie; those are counted and bounded per view."""

import numpy as np
import pytest
import torch

from vistracker_amd import _lib as L
from vistracker_amd import ops, synthetic as syn
from vistracker_amd import visualize as V

pytestmark = pytest.mark.gpu
TOL_EDGE, TOL_Z = 1e-5, 1e-5
# owner differences allowed per view, as a share of the raster's pixels: every one must be explained as above.  Near the horizon the ground's
# sub-pixel faces meet many pixel centres on shared edges (measured: ~0.16 % of a 256^2 view with the reference ground)
MAX_AMBIGUOUS = 0.005


# ---- independent float64 renderer ------------------------------------------------------------------------------------------------------------
def np_render(verts, faces, colors, K, orig_size, size, aa, light, bg, window=None):
    """verts (NV,3) camera coordinates, faces (F,3), colors (F,3), K (9,).  Returns rgb (S,S,3), alpha (S,S), owner (rs,rs) int64 (-1 = background,
    image rows top first), ambiguous (rs,rs) bool.  window = (r0, r1, c0, c1) in image rows / columns of the rs x rs raster restricts the work."""
    v = np.asarray(verts, np.float64); K = np.asarray(K, np.float64).reshape(9); os_ = float(orig_size)
    rs = size * (2 if aa else 1)
    F = len(faces)
    fd = np.concatenate([faces, faces[:, ::-1]]).astype(np.int64)                    # fill_back: reversed copy [i2, i1, i0], ids F + f
    z = v[:, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x_, y_ = v[:, 0] / (z + 1e-9), v[:, 1] / (z + 1e-9)
        u = K[0] * x_ + K[1] * y_ + K[2]; w = os_ - (K[3] * x_ + K[4] * y_ + K[5])
    P = np.stack([2 * (u - os_ / 2) / os_, 2 * (w - os_ / 2) / os_, z], -1)
    tri, ptri = v[fd], P[fd]
    n = np.cross(tri[:, 0] - tri[:, 1], tri[:, 2] - tri[:, 1])
    n = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-5)
    Ia, Id, ca, cd, d = light[0], light[1], np.asarray(light[2:5]), np.asarray(light[5:8]), np.asarray(light[8:11])
    lit = np.concatenate([colors, colors]).astype(np.float64) * (Ia * ca + Id * cd * np.maximum(n @ d, 0)[:, None])
    x0, y0, x1, y1, x2, y2 = (ptri[:, k // 2, k % 2] for k in range(6))
    front = ~((y2 - y0) * (x1 - x0) < (y1 - y0) * (x2 - x0))
    # a corner exactly at z = 0 makes w / z infinite (zp = 0) or undefined for every pixel: such faces never pass near < z
    never = (ptri[:, :, 2] == 0).any(1) | (ptri[:, :, 2] < 0).all(1) | ~np.isfinite(ptri).all((1, 2))
    r0, r1, c0, c1 = window if window is not None else (0, rs, 0, rs)
    lo_y, hi_y = rs - r1, rs - 1 - r0                                              # internal y-up rows of the window
    with np.errstate(invalid="ignore", over="ignore"):
        bx0 = np.floor((np.minimum(np.minimum(x0, x1), x2) * rs + rs - 1) / 2) - 1
        bx1 = np.ceil((np.maximum(np.maximum(x0, x1), x2) * rs + rs - 1) / 2) + 1
        by0 = np.floor((np.minimum(np.minimum(y0, y1), y2) * rs + rs - 1) / 2) - 1
        by1 = np.ceil((np.maximum(np.maximum(y0, y1), y2) * rs + rs - 1) / 2) + 1
    bx0 = np.clip(bx0, c0, c1 - 1); bx1 = np.clip(bx1, c0 - 1, c1 - 1); by0 = np.clip(by0, lo_y, hi_y); by1 = np.clip(by1, lo_y - 1, hi_y)
    keep = front & ~never & (bx0 <= bx1) & (by0 <= by1)
    ids = np.nonzero(keep)[0]
    bw, bh = (bx1 - bx0 + 1)[ids].astype(np.int64), (by1 - by0 + 1)[ids].astype(np.int64)
    cf, cp = [], []
    small = bw * bh <= 64
    k = np.arange(64)
    si = ids[small]
    if len(si):
        wv, hv = bw[small][:, None], bh[small][:, None]
        ok = k[None] < wv * hv
        xi = bx0[si][:, None].astype(np.int64) + k[None] % wv; yi = by0[si][:, None].astype(np.int64) + k[None] // wv
        cf.append(np.broadcast_to(si[:, None], ok.shape)[ok]); cp.append((yi * rs + xi)[ok])
    for f, ww, hh in zip(ids[~small], bw[~small], bh[~small]):
        yy, xx = np.meshgrid(np.arange(hh) + int(by0[f]), np.arange(ww) + int(bx0[f]), indexing="ij")
        cf.append(np.full(yy.size, f)); cp.append((yy * rs + xx).reshape(-1))
    cand_f = np.concatenate(cf) if cf else np.zeros(0, np.int64); cand_p = np.concatenate(cp) if cp else np.zeros(0, np.int64)
    amb = np.zeros(rs * rs, bool)
    best_f = np.full(rs * rs, -1); best_z = np.full(rs * rs, np.inf)
    zs_all, fs_all, ps_all = [], [], []
    for s in range(0, len(cand_f), 1 << 22):
        f, p = cand_f[s:s + (1 << 22)], cand_p[s:s + (1 << 22)]
        xp = (2.0 * (p % rs) + 1 - rs) / rs; yp = (2.0 * (p // rs) + 1 - rs) / rs
        X0, Y0, Z0, X1, Y1, Z1, X2, Y2, Z2 = x0[f], y0[f], ptri[f, 0, 2], x1[f], y1[f], ptri[f, 1, 2], x2[f], y2[f], ptri[f, 2, 2]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            ea, eb = (yp - Y0) * (X1 - X0), (xp - X0) * (Y1 - Y0)
            fa, fb = (yp - Y1) * (X2 - X1), (xp - X1) * (Y2 - Y1)
            ga, gb = (yp - Y2) * (X0 - X2), (xp - X2) * (Y0 - Y2)
            m = np.minimum(np.minimum((ea - eb) / (np.abs(ea) + np.abs(eb) + 1e-300), (fa - fb) / (np.abs(fa) + np.abs(fb) + 1e-300)),
                           (ga - gb) / (np.abs(ga) + np.abs(gb) + 1e-300))
            inside = (ea >= eb) & (fa >= fb) & (ga >= gb)
            den = X0 * (Y1 - Y2) + X1 * (Y2 - Y0) + X2 * (Y0 - Y1)
            w0 = np.clip(((Y1 - Y2) * xp + (X2 - X1) * yp + (X1 * Y2 - X2 * Y1)) / den, 0, 1)
            w1 = np.clip(((Y2 - Y0) * xp + (X0 - X2) * yp + (X2 * Y0 - X0 * Y2)) / den, 0, 1)
            w2 = np.clip(((Y0 - Y1) * xp + (X1 - X0) * yp + (X0 * Y1 - X1 * Y0)) / den, 0, 1)
            ws = w0 + w1 + w2
            zp = 1.0 / (w0 / ws / Z0 + w1 / ws / Z1 + w2 / ws / Z2)
            ok = inside & (zp > V.NEAR) & (zp < V.FAR)
            inz = (zp > V.NEAR * (1 - TOL_Z)) & (zp < V.FAR * (1 + TOL_Z))          # an edge only matters where the face's depth is in range
            np.logical_or.at(amb, p[(np.abs(m) < TOL_EDGE) & inz], True)
            np.logical_or.at(amb, p[inside & ((np.abs(zp - V.NEAR) < TOL_Z * V.NEAR) | (np.abs(zp - V.FAR) < TOL_Z * V.FAR))], True)
        zs_all.append(zp[ok]); fs_all.append(f[ok]); ps_all.append(p[ok])
    zc, fc, pc = (np.concatenate(a) for a in (zs_all, fs_all, ps_all))
    o = np.lexsort((fc, zc, pc))
    zc, fc, pc = zc[o], fc[o], pc[o]
    first = np.ones(len(pc), bool); first[1:] = pc[1:] != pc[:-1]
    best_f[pc[first]] = fc[first]; best_z[pc[first]] = zc[first]
    second = np.zeros(len(pc), bool); second[1:] = first[:-1] & ~first[1:]
    tie = second & (np.abs(zc - np.roll(zc, 1)) <= TOL_Z * np.abs(zc))
    amb[pc[tie]] = True
    own = best_f.reshape(rs, rs)[::-1].copy(); amb = amb.reshape(rs, rs)[::-1].copy()
    img = np.where(own[..., None] >= 0, lit[np.maximum(own, 0)], np.asarray(bg, np.float64))
    alpha = (own >= 0).astype(np.float64)
    if aa:
        img = img.reshape(size, 2, size, 2, 3).mean((1, 3)); alpha = alpha.reshape(size, 2, size, 2).mean((1, 3))
    return img, alpha, own, amb


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def smpl_scene(n, seed=7):
    """n frames of a synthetic SMPL-H + object (camera coordinates, in front of the camera): verts (n,NV,3), faces, colours"""
    key = (n, seed)
    if key not in _CACHE:
        model = syn.smplh_model(0)
        h = ops.SmplhHandle(model)
        sp = syn.sequence_params(n, seed)
        t = lambda a: torch.tensor(a, device="cuda")
        sv, _, _ = ops.smplh_forward(h, t(sp["pose"]), t(sp["betas"]), t(sp["trans"]))
        tv, tf = syn.object_template()
        ov = np.einsum("vi,nij->nvj", tv, sp["obj_R"].transpose(0, 2, 1)) + sp["obj_t"][:, None]
        verts = np.concatenate([sv.detach().cpu().numpy(), ov], 1).astype(np.float32)
        faces = np.concatenate([model["f"], tf + 6890]).astype(np.int32)
        colors = np.concatenate([np.tile(V.COLOR_LIST3[0], (len(model["f"]), 1)), np.tile(V.COLOR_LIST3[1], (len(tf), 1))]).astype(np.float32)
        _CACHE[key] = (verts, faces, colors, h, model, sp, tv, tf)
    return _CACHE[key]


def ground(y=1.5, z0=-40.0, size=80.0, square=0.5):
    ck = V.CheckerBoard(); ck.init_checker(np.array([-size / 2, y, z0]), 'xz', square_size=square, xlength=size, ylength=size)
    v, f, t = ck.get_rends()
    return v[0].numpy(), f[0].numpy().astype(np.int32), t.reshape(-1, 3).numpy()


def params(size, aa, K=None, orig_size=None):
    p = V.setup_renderer(image_size=size, kid=1)
    if K is not None:
        p.K = torch.tensor(np.asarray(K, np.float32).reshape(1, 3, 3))
    if orig_size is not None:
        p.orig_size = orig_size
    p.anti_aliasing = aa
    return p


def concat(meshes):
    vs, fs, cs, o = [], [], [], 0
    for v, f, c in meshes:
        vs.append(v); fs.append(f + o); cs.append(c); o += v.shape[-2]
    return np.concatenate(vs, -2), np.concatenate(fs), np.concatenate(cs)


def gpu_render(verts, faces, colors, p, static=None, K=None):
    r = V.ShadedRasterizer()
    out = r.render(torch.tensor(np.asarray(verts, np.float32), device="cuda"), faces, colors, p, static=static, K=K, want_depth=True, want_index=True)
    return {k: (x.cpu().numpy() if x is not None else None) for k, x in out.items()}


def compare(g, ref, b=0, tag="", max_ambiguous=MAX_AMBIGUOUS):
    img, alpha, own, amb = ref
    fi = g["face_index"][b]
    diff = fi != own
    bad = diff & ~amb
    assert not bad.any(), f"{tag}: {int(bad.sum())} unexplained owner differences, e.g. {np.argwhere(bad)[:5].tolist()}"
    assert diff.sum() <= max_ambiguous * diff.size, f"{tag}: {int(diff.sum())} owner differences at tie / edge pixels"
    print(f"{tag}: {int(diff.sum())} owner differences of {diff.size} pixels, all at ties / edges")
    S = g["rgb"].shape[1]
    agree = ~diff if fi.shape[0] == S else ~diff.reshape(S, 2, S, 2).any((1, 3))
    err = np.abs(g["rgb"][b].astype(np.float64) - img)[agree].max(initial=0.0)
    assert err <= 1e-6, (tag, err)
    np.testing.assert_array_equal(g["alpha"][b][agree], alpha[agree].astype(np.float32))
    return int(diff.sum())


LIGHT = V.setup_renderer(image_size=8).light().astype(np.float64)
BG = [1.0, 1.0, 1.0]


@pytest.mark.parametrize("size,aa", [(256, False), (128, True)])
def test_matches_independent_renderer(size, aa):
    verts, faces, colors, *_ = smpl_scene(2)
    gv, gf, gc = ground()
    K, ratio = V.get_kinect_K(size, 1)
    p = params(size, aa)
    for b in range(2):
        sv, sf, sc = concat([(verts[b], faces, colors), (gv, gf, gc)])
        g = gpu_render(sv[None], sf, sc, p)
        ref = np_render(sv, sf, sc, K.numpy().reshape(9), 2048 * ratio, size, aa, LIGHT, BG)
        compare(g, ref, 0, f"frame {b}")
        assert (g["alpha"][0] > 0).mean() > 0.3                          # ground + body cover much of the view
        fi = g["face_index"][0]
        assert ((fi >= 0) & (fi % len(sf) < len(faces))).sum() > 50          # mesh pixels (either orientation)


def test_coverage_bit_identical_to_silhouette_rasteriser():
    verts, faces, colors, *_ = smpl_scene(4)
    B, size = 4, 256
    K = np.tile(np.float32([0.45, 0, 0.5, 0, 0.45, 0.52, 0, 0, 1]), (B, 1))
    vd = torch.tensor(verts, device="cuda"); fd = torch.tensor(faces, device="cuda"); Kd = torch.tensor(K, device="cuda")
    img = torch.empty(B, size, size, device="cuda"); fi = torch.empty(B, size, size, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.lib().vt_sil_workspace_floats(B, verts.shape[1], len(faces), size), device="cuda")
    L.check(L.lib().vt_sil_forward(L.dptr(vd), B, verts.shape[1], L.dptr(fd), len(faces), L.dptr(Kd), size, L.dptr(img), L.dptr(fi), L.dptr(ws), L.stream_ptr()))
    p = params(size, False, orig_size=1.0)
    g = gpu_render(verts, faces, colors, p, K=K)
    np.testing.assert_array_equal(g["alpha"], img.cpu().numpy())
    np.testing.assert_array_equal(g["face_index"], fi.cpu().numpy())
    assert (g["alpha"] > 0).mean() > 0.02


@pytest.mark.parametrize("case", ["reference", "straddling", "grazing"])
def test_hard_geometry(case):
    """the ground as the reference places it (a grid line at z = 0: faces from z = 0 through the near plane, projections far larger than the image),
    the same ground shifted by a quarter square so that faces straddle z = 0, and a camera looking along the ground plane.  Straddling faces project
    to coplanar overlapping triangles whose depths tie exactly: there every owner difference must be such a tie or an edge, without a count bound."""
    verts, faces, colors, *_ = smpl_scene(1)
    gv, gf, gc = {"reference": lambda: ground(), "straddling": lambda: ground(z0=-39.75), "grazing": lambda: ground(y=0.02)}[case]()
    size = 128
    K, ratio = V.get_kinect_K(size, 1)
    p = params(size, True)
    sv, sf, sc = concat([(verts[0], faces, colors), (gv, gf, gc)])
    g = gpu_render(sv[None], sf, sc, p)
    ref = np_render(sv, sf, sc, K.numpy().reshape(9), 2048 * ratio, size, True, LIGHT, BG)
    compare(g, ref, 0, case, max_ambiguous=MAX_AMBIGUOUS if case != "straddling" else 1.0)
    Z = gv[gf][:, :, 2]
    if case == "reference":
        assert ((Z.min(1) == 0) & (Z.max(1) > V.NEAR)).sum() >= 100
    if case == "straddling":
        assert ((Z.min(1) < 0) & (Z.max(1) > V.NEAR)).sum() >= 100


def test_static_layer_equals_concatenated_scene():
    verts, faces, colors, *_ = smpl_scene(3)
    gv, gf, gc = ground(y=1.5, z0=-39.75)
    for size, aa in ((128, True), (256, False)):
        p = params(size, aa)
        layer = V.StaticLayer(gv, gf, gc, p)
        a = gpu_render(verts, faces, colors, p, static=layer)
        sv = np.concatenate([verts, np.broadcast_to(gv, (3,) + gv.shape)], 1)
        sf = np.concatenate([faces, gf + verts.shape[1]]); sc = np.concatenate([colors, gc])
        b = gpu_render(sv, sf, sc, p)
        for k in ("rgb", "alpha", "depth", "face_index"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        assert (a["face_index"] >= len(faces)).any() and (a["face_index"] < len(faces)).any()


def test_deterministic_and_batch_invariant():
    verts, faces, colors, *_ = smpl_scene(12)
    gv, gf, gc = ground()
    size = 128
    p = params(size, True)
    layer = V.StaticLayer(gv, gf, gc, p)
    R2 = np.float32([[0.9, 0, 0.43589], [0, 1, 0], [-0.43589, 0, 0.9]])
    views = np.concatenate([verts, (verts - [0, 0, 2.4]) @ R2.T + [0, 0, 2.6]], 0).astype(np.float32)    # 12 frames x 2 views = 24
    a = gpu_render(views, faces, colors, p, static=layer)
    b = gpu_render(views, faces, colors, p, static=layer)
    for k in ("rgb", "alpha", "depth", "face_index"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for i in (0, 5, 13, 23):
        s = gpu_render(views[i:i + 1], faces, colors, p, static=layer)
        for k in ("rgb", "alpha", "depth", "face_index"):
            np.testing.assert_array_equal(s[k][0], a[k][i], err_msg=f"{k} view {i}")


def test_render_frames_end_to_end():
    n_frames = 8
    _, faces, colors, h, model, sp, tv, tf = smpl_scene(n_frames)
    recons = []
    for k in range(2):
        recons.append({"poses": sp["pose"], "betas": sp["betas"], "trans": sp["trans"] + np.float32([0.05 * k, 0, 0]), "obj_angles": sp["obj_R"].transpose(0, 2, 1),
                       "obj_trans": sp["obj_t"], "obj_scales": np.ones(n_frames, np.float32)})
    c, s = np.cos(0.35), np.sin(0.35)
    R1 = np.eye(3); R2 = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
    Rs = [np.eye(3), R1, R2]; ts = [np.zeros(3), np.zeros(3), np.array([0.8, 0, 0.3])]
    kin = V.KinectTransform(world2local_R=Rs, world2local_t=ts)
    r = V.RendererSide2side(image_size=1200)
    rgb_img = np.random.default_rng(0).integers(0, 256, (1536, 2048, 3), dtype=np.uint8)
    chunks = list(r.render_frames(recons, tv, tf, h, kin, rgb=lambda i: rgb_img, chunk=5))
    frames = np.concatenate(chunks)
    assert frames.shape == (n_frames, 900, 720 * 5, 3) and frames.dtype == np.uint8
    # the rgb panel
    from vistracker_amd.sequence_io import resize_bilinear_hw
    np.testing.assert_array_equal(frames[3, :, :720], resize_bilinear_hw(rgb_img, 900, 1200)[:, 240:960])
    # one frame's panels against the float64 renderer on the panel window
    f = 3
    K, ratio = V.get_kinect_K(1200, 1)
    gv, gf, gc = ground()
    ov = V.object_verts(tv, recons[0]["obj_angles"][f:f + 1], recons[0]["obj_trans"][f:f + 1], recons[0]["obj_scales"][f:f + 1])[0]
    for j, (kid, rc) in enumerate([(1, 0), (2, 0)]):
        d = recons[rc]
        sv, _, _ = ops.smplh_forward(h, *(torch.tensor(d[k][f:f + 1], device="cuda") for k in ("poses", "betas", "trans")))
        ov = V.object_verts(tv, d["obj_angles"][f:f + 1], d["obj_trans"][f:f + 1], d["obj_scales"][f:f + 1])[0]
        mesh = kin.world2local(np.concatenate([sv[0].detach().cpu().numpy(), ov]), kid)
        sv_, sf_, sc_ = concat([(mesh, faces, colors), (gv, gf, gc)])
        img, alpha, own, amb = np_render(sv_, sf_, sc_, K.numpy().reshape(9), 2048 * ratio, 1200, True, LIGHT, BG, window=(0, 1800, 480, 1920))
        panel = frames[f, :, 720 * (1 + j * 2 + rc):720 * (2 + j * 2 + rc)]
        ref = (np.clip(img[:900, 240:960], 0, 1).astype(np.float32) * 255).astype(np.uint8)
        win = own[:1800, 480:1920]; ambw = amb[:1800, 480:1920]
        unclear = ambw.reshape(900, 2, 720, 2).any((1, 3))
        diff = (panel != ref).any(-1)
        assert (diff & ~unclear).sum() == 0 or np.abs(panel.astype(int) - ref)[diff & ~unclear].max() <= 1, (kid, int((diff & ~unclear).sum()))
        assert diff.sum() <= MAX_AMBIGUOUS * diff.size, (kid, int(diff.sum()))
        # the SMPL colour, lit: body pixels are COLOR_LIST3[0] x (0.4 + 0.3 relu(n . d)), between 0.4 and 0.85 of it
        body = (win >= 0) & (win % len(sf_) < len(model["f"]))
        bp = body.reshape(900, 2, 720, 2).all((1, 3))
        assert bp.sum() > 1000
        col = panel[bp].astype(np.float64) / 255 / np.asarray(V.COLOR_LIST3[0])
        assert col.min() > 0.4 - 0.01 and col.max() < 0.85 + 0.01 and col.std() > 0.01
