"""GPU (-m gpu): the fit on the camera image (csrc/overlay.hip vt_overlay_panel_u8, ``render_frames(overlay=True)``) and its score on the input masks
(vt_mask_score, ``RendererSide2side.mask_scores``) against the float64 / integer models of tests/overlay_model.py.

Grey levels of the overlay must equal the model's except where the model's v lies within 1e-3 of a half-way point (fp32 carries a few ulp of 255, ~1e-4, on
such a value: the band leaves that a margin of more than ten), there within one level, and at most 1 % of the values may be that close (uniform inputs put
about 0.2 % there).  The score is integer arithmetic: exact equality."""
from types import SimpleNamespace

import numpy as np
import pytest

import overlay_model as M
import panel_model as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PW = P.CE - P.CS


# ---- the overlay kernel on random inputs ---------------------------------------------------------------------------------------------------------------------
B, S, R0, NR, C0, NC = 3, 16, 0, 12, 3, 10
BUF = (3, 12, 40, 3)
ROW = BUF[2] * 3
SRC = [b * BUF[1] * ROW + 3 * c for b, c in enumerate((0, 2, 1))]                  # source panels at columns 0, 2, 1 of frames 0, 1, 2
DST = [b * BUF[1] * ROW + 3 * c for b, c in enumerate((20, 30, 14))]               # destination panels at columns 20, 30, 14: disjoint from the sources


@pytest.fixture(scope="module")
def ov():
    rng = np.random.default_rng(11)
    rgb = rng.uniform(-0.2, 1.2, (B, S, S, 3)).astype(np.float32); alpha = rng.uniform(0, 1, (B, S, S)).astype(np.float32)
    empty = rng.random((B, S, S)) < 0.25                                             # uncovered pixels: alpha == 0 and rgb == 0
    rgb[empty] = 0; alpha[empty] = 0
    buf = rng.integers(0, 256, BUF, dtype=np.uint8)                                  # the sentinel pattern: every byte of the buffer is known
    return SimpleNamespace(rgb=rgb, alpha=alpha, empty=empty, buf=buf, rgb_d=torch.as_tensor(rgb).cuda(), alpha_d=torch.as_tensor(alpha).cuda())


def panel_of(buf, off):
    """(B, NR, NC, 3) panels at byte offsets ``off`` of a host buffer"""
    flat = buf.reshape(-1)
    return np.stack([np.stack([flat[o + y * ROW:o + y * ROW + 3 * NC].reshape(NC, 3) for y in range(NR)]) for o in off])


def run_overlay(ov, opacity, src=SRC, dst=DST):
    from vistracker_amd import ops
    d = torch.as_tensor(ov.buf).cuda()
    ops.overlay_panel_u8(ov.rgb_d, ov.alpha_d, d, src, dst, R0, NR, C0, NC, ROW, opacity)
    return d.cpu().numpy()


@pytest.mark.parametrize("opacity", [0.6, 1.0, 0.25])
def test_overlay_equals_the_model_and_touches_nothing_else(ov, opacity):
    got = run_overlay(ov, opacity)
    src = panel_of(ov.buf, SRC)
    crop = lambda a: a[:, R0:R0 + NR, C0:C0 + NC]
    out = panel_of(got, DST)
    M.assert_overlay(out, crop(ov.rgb), crop(ov.alpha), src, opacity, tag=f"opacity {opacity}")
    np.testing.assert_array_equal(out[crop(ov.empty)], src[crop(ov.empty)])          # alpha == 0 and rgb == 0: the source byte, bit for bit
    assert (out != src).mean() > 0.5                                                 # ... and the rest did change
    mask = np.ones(ov.buf.size, bool)
    for o in DST:
        for y in range(NR):
            mask[o + y * ROW:o + y * ROW + 3 * NC] = False
    np.testing.assert_array_equal(got.reshape(-1)[mask], ov.buf.reshape(-1)[mask])   # every byte outside the destination panels keeps its value


def test_overlay_opacity_zero_and_in_place(ov):
    got = run_overlay(ov, 0.0)
    np.testing.assert_array_equal(panel_of(got, DST), panel_of(ov.buf, SRC))         # opacity 0 copies the source panel
    out_of_place = panel_of(run_overlay(ov, 0.6), DST)
    in_place = run_overlay(ov, 0.6, src=SRC, dst=SRC)
    np.testing.assert_array_equal(panel_of(in_place, SRC), out_of_place)
    np.testing.assert_array_equal(panel_of(in_place, DST), panel_of(ov.buf, DST))    # in place: the other panels are not written


# ---- the score kernel: exact equality with the model ---------------------------------------------------------------------------------------------------------
F, NB, NO = 50, 20, 17


def run_score(owners, rows, masks, thres=127):
    """owners: list of (is,is) int32; masks: one (pm, om) pair per view, all packed into one device buffer (an (h,w,C) mask keeps its channels: pixel stride C)"""
    from vistracker_amd import ops
    parts, desc, total = [], [], 0
    for pm, om in masks:
        row = []
        for m in (pm, om):
            row.append((total, m.shape[2] if m.ndim == 3 else 1)); parts.append(m.reshape(-1)); total += m.size
        h, w = pm.shape[:2]
        desc.append([row[0][0], row[1][0], h, w, row[0][1], w * row[0][1], row[1][1], w * row[1][1]])
    src = torch.as_tensor(np.concatenate(parts)).cuda()
    fidx = torch.as_tensor(np.stack(owners)).cuda()
    return ops.mask_score(fidx, rows, F, NB, NO, src, src, desc, thres).cpu().numpy()


def model_score(owners, rows, masks):
    return np.stack([M.score(d, rows, F, NB, NO, pm, om) for d, (pm, om) in zip(owners, masks)])


def test_score_identity_mapping():
    rng = np.random.default_rng(21)
    d = [M.random_owners(rng, 32, F, NB, NO)]
    masks = [(M.random_mask(rng, 24, 32), M.random_mask(rng, 24, 32))]
    got = run_score(d, 24, masks)
    assert got.shape == (1, 2, 4) and got.dtype == np.int32
    np.testing.assert_array_equal(got, model_score(d, 24, masks))
    assert (got[0, :, :3] > 0).all() and (got[0, :, 3] > 0).all()


def test_score_ratio_pixel_stride_and_frames_of_different_sizes():
    rng = np.random.default_rng(22)
    d = [M.random_owners(rng, 32, F, NB, NO) for _ in range(3)]
    masks = [(M.random_mask(rng, 36, 48), M.random_mask(rng, 36, 48)),
             (M.random_mask(rng, 36, 48, 3), M.random_mask(rng, 36, 48)),            # (h,w,3): pixel stride 3, channel 0
             (M.random_mask(rng, 29, 41), M.random_mask(rng, 29, 41, 3))]            # another size in the same call
    got = run_score(d, 24, masks)
    np.testing.assert_array_equal(got, model_score(d, 24, masks))
    assert not (masks[1][0][..., 0] == masks[1][0][..., 1]).all()                    # reading another channel would have shown


def test_score_several_workgroups_positions_and_runs():
    rng = np.random.default_rng(23)
    x, y = M.random_owners(rng, 80, F, NB, NO), M.random_owners(rng, 80, F, NB, NO)  # 60 x 80 = 4800 samples: 19 workgroups, the last one part filled
    mx = (M.random_mask(rng, 90, 120), M.random_mask(rng, 90, 120)); my = (M.random_mask(rng, 45, 64), M.random_mask(rng, 45, 64))
    got = run_score([x, y, x], 60, [mx, my, mx])
    np.testing.assert_array_equal(got, model_score([x, y, x], 60, [mx, my, mx]))
    np.testing.assert_array_equal(got[0], got[2])                                    # a frame's place in the batch does not matter
    np.testing.assert_array_equal(run_score([x], 60, [mx])[0], got[0])               # nor does B
    np.testing.assert_array_equal(run_score([x, y, x], 60, [mx, my, mx]), got)       # nor the run
    many = run_score([x, y] * 9, 60, [mx, my] * 9)                                   # 18 views: more than one launch's descriptors
    np.testing.assert_array_equal(many, np.tile(got[:2], (9, 1, 1)))


# ---- through the real rasteriser ----------------------------------------------------------------------------------------------------------------------------
def make_scene(n, image_size, two_recons=False):
    from test_gpu_render import smpl_scene
    from vistracker_amd import visualize as V
    _, faces, colors, h, model, sp, tv, tf = smpl_scene(n)
    recon = {"poses": sp["pose"], "betas": sp["betas"], "trans": sp["trans"], "obj_angles": sp["obj_R"].transpose(0, 2, 1), "obj_trans": sp["obj_t"],
             "obj_scales": np.ones(n, np.float32)}
    recons = [recon]
    if two_recons:
        recons.append({**recon, "obj_trans": sp["obj_t"] + np.array([0.25, -0.1, 0.0], np.float32), "trans": sp["trans"] + np.array([-0.1, 0.0, 0.05], np.float32)})
    c, s = np.cos(0.35), np.sin(0.35)
    kin = V.KinectTransform(world2local_R=[np.eye(3), np.eye(3), np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])],
                            world2local_t=[np.zeros(3), np.zeros(3), np.array([0.8, 0, 0.3])])
    r = V.RendererSide2side(image_size=image_size)
    return SimpleNamespace(n=n, recons=recons, kin=kin, r=r, h=h, tv=tv, tf=tf, nb=len(np.asarray(h.faces)), no=len(tf))


def fit_of(sc, recons, idx):
    """``fit_views`` of frames ``idx`` on the host: rgb, alpha, face_index"""
    s = sc.r._scene(sc.tv, sc.tf, sc.h)
    with torch.cuda.device(0):
        per_recon, per_colors = sc.r._chunk_meshes(s, recons, sc.h, idx)
        out = sc.r.fit_views(s, per_recon, per_colors, sc.kin)
    return {k: out[k].cpu().numpy() for k in ("rgb", "alpha", "face_index")}


@pytest.fixture(scope="module")
def tiny():
    sc = make_scene(3, 16)
    sc.fit = fit_of(sc, sc.recons, [0, 1, 2])
    return sc


def test_alpha_is_where_the_owners_are(tiny):
    """pins the row order of face_index (image row 0 = top, as rgb / alpha) and the ground-free render: coverage is mesh faces only"""
    fi, alpha, rgb = tiny.fit["face_index"], tiny.fit["alpha"], tiny.fit["rgb"]
    assert fi.shape == (3, 32, 32) and alpha.shape == (3, 16, 16)
    Fm = tiny.nb + tiny.no
    assert fi.max() < 2 * Fm                                                         # no ground: every owner is a mesh face
    held = (fi >= 0).reshape(3, 16, 2, 16, 2)
    np.testing.assert_array_equal(alpha > 0, held.any((2, 4)))
    np.testing.assert_array_equal(alpha, held.mean((2, 4)).astype(np.float32))
    assert (rgb[alpha == 0] == 0).all() and (alpha > 0).sum() >= 6                   # background 0; something is there
    top, bottom = (alpha[:, :8] > 0).sum(), (alpha[:, 8:] > 0).sum()
    assert top != bottom                                                             # the scene is not symmetric: a flipped owner map could not pass


def test_masks_made_from_the_owner_map_score_one_and_a_moved_object_less(tiny):
    sc = tiny
    Fm, rows = sc.nb + sc.no, 24                                                     # H = 12 panel rows of the 16 x 16 render = 24 raster rows
    masks = [M.masks_of_owners(f, rows, Fm, sc.nb, sc.no) for f in sc.fit["face_index"]]
    assert masks[0][0].shape == (24, 32)
    res = sc.r.mask_scores(sc.recons, sc.tv, sc.tf, sc.h, sc.kin, masks, chunk=2)
    c = res["count"]
    print("counts of the fit against its own owner masks:", c[:, 0].tolist())
    assert c.shape == (3, 1, 2, 4) and c.dtype == np.int32 and res["iou"].shape == (3, 1, 2)
    np.testing.assert_array_equal(c[:, 0], np.stack([M.score(f, rows, Fm, sc.nb, sc.no, *m) for f, m in zip(sc.fit["face_index"], masks)]))
    assert (c[..., 0] == c[..., 1]).all() and (c[..., 1] == c[..., 2]).all() and (c[..., 3] == 0).all()
    assert (c[..., 1] > 0).all()                                                     # both classes are visible
    np.testing.assert_array_equal(res["iou"], np.ones((3, 1, 2)))
    moved = [{**sc.recons[0], "obj_trans": sc.recons[0]["obj_trans"] + np.array([0.08, 0.0, 0.0], np.float32)}]
    res2 = sc.r.mask_scores(moved, sc.tv, sc.tf, sc.h, sc.kin, masks, chunk=2)
    print("object moved by 8 cm:", res2["count"][:, 0].tolist(), res2["iou"][:, 0].tolist())
    assert (res2["iou"][:, 0, 1] < 1).all()
    np.testing.assert_array_equal(res2["count"][..., 2], c[..., 2])                  # the masks did not change


# ---- render_frames(overlay=True), mask_scores --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """image_size 64, 96 x 128 camera images (every blend of the panel exact in fp32), 4 frames, two recons; the overlay=False frames are the reference"""
    from PIL import Image
    sc = make_scene(4, P.SIZE, two_recons=True)
    sc.imgs = [P.image(40 + k, *P.EXACT) for k in range(sc.n)]
    sc.run = lambda rgb, **kw: list(sc.r.render_frames(sc.recons, sc.tv, sc.tf, sc.h, sc.kin, rgb=rgb, chunk=3, **kw))
    sc.default = np.concatenate(sc.run(sc.imgs))
    sc.overlay = np.concatenate(sc.run(sc.imgs, overlay=True))
    sc.fit = fit_of(sc, sc.recons, list(range(sc.n)))
    # masks: the first recon's own owner masks at 96 x 128, frame 1 with an (h,w,3) object mask; as arrays and as a sequence folder
    rng = np.random.default_rng(5)
    Fm = sc.nb + sc.no
    sc.masks = []
    root = tmp_path_factory.mktemp("overlay") / "seq"
    sc.paths = []
    for k in range(sc.n):
        pm, om = M.masks_of_owners(sc.fit["face_index"][2 * k], 96, Fm, sc.nb, sc.no)          # (96, 128): the raster's own size
        om = np.ascontiguousarray(np.roll(om, 3, 1))                                 # the object mask sits three samples to the right of the fit
        pm[rng.random(pm.shape) < 0.02] = 127                                        # 2 % of the person mask at the threshold: off
        if k == 1:
            om = np.ascontiguousarray(np.stack([om, 255 - om, om], -1))
        sc.masks.append((pm, om))
        d = root / f"t{k:04d}.000"; d.mkdir(parents=True)
        Image.fromarray(pm).save(d / "k1.person_mask.png"); Image.fromarray(om).save(d / "k1.obj_rend_mask.png")
        sc.paths.append(str(d / "k1.color.jpg"))
    return sc


def test_overlay_frames_keep_every_other_panel(scene):
    n = 2
    assert scene.default.shape == (scene.n, P.H, PW * (1 + 2 * n), 3) and scene.overlay.shape == (scene.n, P.H, PW * (1 + 3 * n), 3)
    assert scene.overlay.shape[1:] == scene.r.frame_shape(n, overlay=True)
    np.testing.assert_array_equal(scene.overlay[:, :, :PW], scene.default[:, :, :PW])
    np.testing.assert_array_equal(scene.overlay[:, :, PW * (1 + n):], scene.default[:, :, PW:])


@pytest.mark.parametrize("opacity", [0.6, 1.0])
def test_overlay_panels_equal_the_model_on_the_frames_own_panel(scene, opacity):
    n = 2
    frames = scene.overlay if opacity == 0.6 else np.concatenate(scene.run(scene.imgs, overlay=True, overlay_opacity=opacity))
    rgb = scene.fit["rgb"].reshape(scene.n, n, P.SIZE, P.SIZE, 3)[:, :, :P.H, P.CS:P.CE]
    alpha = scene.fit["alpha"].reshape(scene.n, n, P.SIZE, P.SIZE)[:, :, :P.H, P.CS:P.CE]
    assert (alpha > 0).mean() > 0.02 and ((alpha > 0) & (alpha < 1)).any()           # the fit is in the panel, anti-aliased edges included
    for r in range(n):
        got = frames[:, :, PW * (1 + r):PW * (2 + r)]
        M.assert_overlay(got, rgb[:, r], alpha[:, r], frames[:, :, :PW], opacity, tag=f"recon {r}, opacity {opacity}")
        out = alpha[:, r] == 0
        np.testing.assert_array_equal(got[out], frames[:, :, :PW][out])              # the camera image wherever the fit is not
        assert (got != frames[:, :, :PW]).any()
    assert (frames[:, :, PW:2 * PW] != frames[:, :, 2 * PW:3 * PW]).any()            # the two recons differ


def test_overlay_routes_agree(scene):
    dev = scene.run(scene.imgs, overlay=True, device_panel=True, decode_workers=2)
    assert [len(c) for c in dev] == [3, 1]
    np.testing.assert_array_equal(np.concatenate(dev), scene.overlay)                # 96 x 128 -> 48 x 64: the device panel is the host's bit for bit
    on = scene.run([torch.as_tensor(im).cuda() for im in scene.imgs], overlay=True, device_panel=True, on_device=True)
    assert all(torch.is_tensor(c) and c.is_cuda and c.dtype == torch.uint8 for c in on)
    np.testing.assert_array_equal(torch.cat(on).cpu().numpy(), scene.overlay)
    ref = scene.run(scene.imgs, add_top=True)
    got = scene.run(scene.imgs, add_top=True, overlay=True)
    for (f0, t0), (f1, t1) in zip(ref, got):
        np.testing.assert_array_equal(t1, t0)                                        # the top strips are unchanged
        np.testing.assert_array_equal(f1[:, :, PW * 3:], f0[:, :, PW:])
    np.testing.assert_array_equal(np.concatenate([f for f, _ in got]), scene.overlay)


def test_pipeline_forwards_overlay_and_mask_scores(scene):
    from vistracker_amd.pipeline import SequencePipeline
    fake = SimpleNamespace(device="cuda:0", ctx=SimpleNamespace(smpl=scene.h))
    one = {"recon": scene.recons[0]}
    gen = SequencePipeline.render(fake, one, scene.kin, rgb=scene.imgs, template=(scene.tv, scene.tf), chunk=3, image_size=P.SIZE, overlay=True,
                                  overlay_opacity=0.6)
    got = np.concatenate(list(gen))
    assert got.shape == (scene.n, P.H, PW * 4, 3)
    np.testing.assert_array_equal(got[:, :, :2 * PW], scene.overlay[:, :, :2 * PW])
    res = SequencePipeline.mask_scores(fake, one, scene.kin, scene.masks, (scene.tv, scene.tf), chunk=3, image_size=P.SIZE)
    ref = scene.r.mask_scores(scene.recons[:1], scene.tv, scene.tf, scene.h, scene.kin, scene.masks, chunk=3)
    np.testing.assert_array_equal(res["count"], ref["count"]); np.testing.assert_array_equal(res["iou"], ref["iou"])


def test_mask_scores_sources_agree_and_equal_the_model(scene):
    sc = scene
    run = lambda masks, **kw: sc.r.mask_scores(sc.recons, sc.tv, sc.tf, sc.h, sc.kin, masks, chunk=3, **kw)
    ref = run(sc.masks)
    Fm, rows = sc.nb + sc.no, 2 * P.H
    want = np.stack([M.score(f, rows, Fm, sc.nb, sc.no, *sc.masks[b // 2]) for b, f in enumerate(sc.fit["face_index"])]).reshape(sc.n, 2, 2, 4)
    np.testing.assert_array_equal(ref["count"], want)
    np.testing.assert_array_equal(ref["iou"], M.iou(want))
    print("iou (frame, recon, class):", np.round(ref["iou"], 3).tolist())
    assert (ref["iou"][:, 0, 0] > 0.9).all() and (ref["iou"][:, 1, 1] < ref["iou"][:, 0, 1]).all()       # own masks score high, the displaced recon lower
    on_dev = [tuple(torch.as_tensor(m).cuda() for m in pair) for pair in sc.masks]
    mixed = [on_dev[0], sc.masks[1], sc.paths[2], on_dev[3]]
    for masks, kw in ((lambda i: sc.masks[i], {}), (sc.paths, {}), (sc.paths, dict(decode_workers=2)), (on_dev, {}), (mixed, {})):
        got = run(masks, **kw)
        np.testing.assert_array_equal(got["count"], ref["count"]); np.testing.assert_array_equal(got["iou"], ref["iou"])
    part = run(sc.masks, start=1, end=4, interval=2)
    np.testing.assert_array_equal(part["count"], ref["count"][1:4:2])


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(scene, ov):
    from vistracker_amd import _lib as L, ops
    lib = L.lib()
    st = L.stream_ptr()
    with pytest.raises(ValueError, match="overlay"):
        scene.run(None, overlay=True)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="opacity"):
            scene.run(scene.imgs, overlay=True, overlay_opacity=bad)
    # vt_overlay_panel_u8
    buf = torch.as_tensor(ov.buf).cuda()
    so, do = torch.as_tensor(SRC).cuda(), torch.as_tensor(DST).cuda()

    def call(rgb=ov.rgb_d.data_ptr(), alpha=ov.alpha_d.data_ptr(), B_=B, S_=S, r0=R0, nr=NR, c0=C0, nc=NC, out=buf.data_ptr(), s=so.data_ptr(), d=do.data_ptr(), rs=ROW,
             op=0.6):
        return lib.vt_overlay_panel_u8(rgb, alpha, B_, S_, r0, nr, c0, nc, out, s, d, rs, op, st)
    for kw in (dict(rgb=None), dict(alpha=None), dict(out=None), dict(s=None), dict(d=None), dict(B_=0), dict(S_=0), dict(nr=0), dict(nc=0), dict(nr=-1),
               dict(r0=-1), dict(c0=-1), dict(r0=5), dict(c0=7), dict(nr=17), dict(nc=14), dict(r0=16, nr=1), dict(rs=3 * NC - 1),          # a crop outside the render
               dict(op=-0.01), dict(op=1.01), dict(op=float("nan")), dict(op=float("inf"))):
        assert call(**kw) == L.VT_ERR_ARG, kw
    assert b"vt_overlay_panel_u8" in lib.vt_last_error()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(buf.cpu().numpy(), ov.buf)                         # nothing was launched
    assert call(op=1.0) == L.VT_OK and call(op=0.0) == L.VT_OK
    with pytest.raises(L.VtError):
        ops.overlay_panel_u8(ov.rgb_d, ov.alpha_d, buf, SRC, DST, R0, 17, C0, NC, ROW, 0.6)
    # vt_mask_score
    fidx = torch.zeros(1, 32, 32, dtype=torch.int32, device="cuda")
    m = torch.zeros(2 * 24 * 32, dtype=torch.uint8, device="cuda")
    count = torch.full((1, 2, 4), -7, dtype=torch.int32, device="cuda")
    desc = lambda *row: np.array([row], np.int64)
    good = desc(0, 768, 24, 32, 1, 32, 1, 32)

    def score(d=good, f=fidx.data_ptr(), B_=1, is_=32, rows=24, F_=F, nb=NB, no=NO, pm=m.data_ptr(), pb=m.numel(), om=m.data_ptr(), ob=m.numel(), th=127,
              cnt=count.data_ptr()):
        return lib.vt_mask_score(f, B_, is_, rows, F_, nb, no, pm, pb, om, ob, d.ctypes.data if d is not None else None, th, cnt, st)
    for kw in (dict(f=None), dict(pm=None), dict(om=None), dict(d=None), dict(cnt=None), dict(B_=0), dict(is_=0), dict(rows=0), dict(rows=33), dict(F_=0),
               dict(nb=-1), dict(no=-1), dict(nb=40, no=11), dict(pb=0), dict(ob=0), dict(th=-1), dict(th=256),
               dict(d=desc(0, 768, 0, 32, 1, 32, 1, 32)), dict(d=desc(0, 768, 24, 0, 1, 32, 1, 32)), dict(d=desc(0, 768, 24, 32, 0, 32, 1, 32)),
               dict(d=desc(0, 768, 24, 32, 1, 31, 1, 32)), dict(d=desc(0, 768, 24, 32, 1, 32, 3, 95)),                          # rows that overlap
               dict(d=desc(-1, 768, 24, 32, 1, 32, 1, 32)), dict(d=desc(0, 769, 24, 32, 1, 32, 1, 32)), dict(d=desc(0, 768, 25, 32, 1, 32, 1, 32)),          # a mask that leaves its buffer
               dict(d=desc(0, 768, 24, 32, 1, 32, 3, 96)), dict(pb=767), dict(ob=1535), dict(d=desc(2 ** 62, 768, 24, 32, 1, 32, 1, 32)),
               dict(d=desc(0, 2 ** 63 - 100, 24, 32, 1, 32, 1, 32))):
        assert score(**kw) == L.VT_ERR_ARG, kw
    assert b"vt_mask_score" in lib.vt_last_error() and b"leaves" in lib.vt_last_error()
    torch.cuda.synchronize()
    assert (count == -7).all()                                                       # nothing was launched, nothing zeroed
    assert score() == L.VT_OK
    torch.cuda.synchronize()
    np.testing.assert_array_equal(count.cpu().numpy()[0], [[0, 768, 0, 0], [0, 0, 0, 0]])      # every sample is owned by face 0, a body face; the masks are off
    with pytest.raises(L.VtError):                                                   # no CPU route
        ops.mask_score(fidx, 24, F, NB, NO, m.cpu(), m, good)
    with pytest.raises(ValueError):
        scene.r.mask_scores(scene.recons, scene.tv, scene.tf, scene.h, scene.kin, [(mm[0].astype(np.float32), mm[1]) for mm in scene.masks], chunk=3)
    with pytest.raises(ValueError):
        scene.r.mask_scores(scene.recons, scene.tv, scene.tf, scene.h, scene.kin, [(mm[0][:-1], mm[1]) for mm in scene.masks], chunk=3)
