"""GPU (-m gpu): step 7's camera panel on the device (csrc/inputs.hip vt_resize_panel_u8, ``sequence_io.device_panels``, ``render_frames(device_panel=,
decode_workers=)``) against the host path it replaces (``sequence_io.resize_bilinear_hw``), bit for bit where fp32 blends are exact, and against the integer
model of tests/panel_model.py where they round.  Panels of image_size 64: H = 48, columns [12, 51)."""
from types import SimpleNamespace

import numpy as np
import pytest

import panel_model as P

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PW = P.CE - P.CS
SENTINEL = 0xA5


def device_panel_of(images, W=None, n=None):
    """``device_panels`` of ``images`` into sentinel-filled (n, H, W, 3) frames -> host array"""
    from vistracker_amd import sequence_io as SIO
    n = len(images) if n is None else n
    buf = torch.full((n, P.H, PW + 7 if W is None else W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    SIO.device_panels(images, buf, P.SIZE, P.CS, P.CE)
    return buf.cpu().numpy()


def host_panel(img):
    from vistracker_amd.sequence_io import resize_bilinear_hw
    return resize_bilinear_hw(np.asarray(img), P.H, P.SIZE)[:, P.CS:P.CE]


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------------
def test_exact_blends_equal_the_host_path_bit_for_bit():
    """96 x 128 -> 48 x 64: weights 1 / 4 and 3 / 4, every blend exact in fp32; 26 % of them sit exactly on a half-way point: the rounding rule"""
    img = P.image(1, *P.EXACT)
    got = device_panel_of([img])
    np.testing.assert_array_equal(got[0, :, :PW], host_panel(img))
    _, d = P.panel(img, P.H, P.SIZE, P.CS, P.CE)
    assert (d == 0).mean() > 0.2
    assert (got[:, :, PW:] == SENTINEL).all()


@pytest.mark.parametrize("h,w", P.ROUNDING)
def test_rounded_blends_against_the_integer_model(h, w):
    """fp32 tap positions and blends carry ~1e-4 grey levels (a few ulp of 255): equal to the exact model wherever the blend is more than 1e-3 from a half-way
    point, within one level everywhere, and at most 2 % of the values are that close (the whole resize on the CPU: 0.20 %, 0.20 %, 0.90 % for these images)"""
    img = P.image(2, h, w)
    got = device_panel_of([img])[0, :, :PW]
    q, d = P.panel(img, P.H, P.SIZE, P.CS, P.CE)
    clear = d > 1e-3
    print(f"{h} x {w}: device differs from the model in {int((got != q).sum())} of {q.size} values; {100 * (1 - clear.mean()):.2f} % excluded")
    np.testing.assert_array_equal(got[clear], q[clear])
    assert np.abs(got.astype(int) - q.astype(int)).max() <= 1
    assert 1 - clear.mean() <= 0.02


def test_mixed_chunk_strides_device_tensors_positions_and_untouched_bytes():
    """one chunk: two image sizes, a host view with a row stride, a device tensor, a device view of a larger allocation, the same image in several slots"""
    a, b = P.image(3, *P.EXACT), P.image(4, 83, 110)
    big = P.image(5, 100, 140)
    view = big[2:98, 5:133]                                                        # (96, 128, 3) with a row stride of 140 pixels
    dev_big = torch.as_tensor(big).cuda()
    images = [a, b, view, torch.as_tensor(a).cuda(), dev_big[2:98, 5:133], b, a, torch.as_tensor(b).cuda()]
    got = device_panel_of(images)
    ref_a, ref_view = host_panel(a), host_panel(np.ascontiguousarray(view))
    ref_b = got[1, :, :PW]                                                         # 83 x 110 rounds in fp32: the slots must agree with each other ...
    qb, db = P.panel(b, P.H, P.SIZE, P.CS, P.CE)
    np.testing.assert_array_equal(ref_b[db > 1e-3], qb[db > 1e-3])                 # ... and with the model
    for j, ref in enumerate([ref_a, ref_b, ref_view, ref_a, ref_view, ref_b, ref_a, ref_b]):
        np.testing.assert_array_equal(got[j, :, :PW], ref, err_msg=f"slot {j}")
    assert (got[:, :, PW:] == SENTINEL).all()
    # a single frame of a larger buffer: the other frames keep every byte
    one = device_panel_of([b], n=1)
    np.testing.assert_array_equal(one[0, :, :PW], ref_b)
    from vistracker_amd import ops
    buf = torch.full((3, P.H, PW + 2, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    ops.resize_panel_u8(torch.as_tensor(a).cuda(), [[0, 96, 128, 0, 128, 3 * 128]], P.H, P.SIZE, P.CS, PW, buf, [buf[1].numel()], (PW + 2) * 3)
    out = buf.cpu().numpy()
    np.testing.assert_array_equal(out[1, :, :PW], ref_a)
    assert (out[0] == SENTINEL).all() and (out[2] == SENTINEL).all() and (out[1, :, PW:] == SENTINEL).all()


def test_more_frames_than_one_launch_holds():
    """20 frames: the descriptors of 16 travel with one launch"""
    imgs = [P.image(20 + k, *P.EXACT) if k % 3 else P.image(20 + k, 30, 40) for k in range(20)]
    got = device_panel_of(imgs)
    for k in (0, 1, 15, 16, 17, 19):
        if k % 3:
            np.testing.assert_array_equal(got[k, :, :PW], host_panel(imgs[k]))
        else:
            q, d = P.panel(imgs[k], P.H, P.SIZE, P.CS, P.CE)
            np.testing.assert_array_equal(got[k, :, :PW][d > 1e-3], q[d > 1e-3])
    assert (got[:, :, PW:] == SENTINEL).all()


# ---- render_frames ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """the small render fixture of test_gpu_render at image_size 64, 5 frames with a camera image each (96 x 128; written as PNG too), and the default
    path's frames: the reference of the tests below, computed once"""
    from PIL import Image
    from test_gpu_render import smpl_scene
    from vistracker_amd import visualize as V
    n = 5
    _, faces, colors, h, model, sp, tv, tf = smpl_scene(n)
    recon = {"poses": sp["pose"], "betas": sp["betas"], "trans": sp["trans"], "obj_angles": sp["obj_R"].transpose(0, 2, 1), "obj_trans": sp["obj_t"],
             "obj_scales": np.ones(n, np.float32)}
    c, s = np.cos(0.35), np.sin(0.35)
    kin = V.KinectTransform(world2local_R=[np.eye(3), np.eye(3), np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])],
                            world2local_t=[np.zeros(3), np.zeros(3), np.array([0.8, 0, 0.3])])
    r = V.RendererSide2side(image_size=P.SIZE)
    imgs = [P.image(30 + k, *P.EXACT) for k in range(n)]
    root = tmp_path_factory.mktemp("panel")
    paths = []
    for k, im in enumerate(imgs):
        paths.append(str(root / f"k1.{k}.color.png")); Image.fromarray(im).save(paths[-1])
    run = lambda rgb, **kw: list(r.render_frames([recon], tv, tf, h, kin, rgb=rgb, chunk=3, **kw))
    sc = SimpleNamespace(n=n, recon=recon, kin=kin, r=r, imgs=imgs, paths=paths, run=run, h=h, tv=tv, tf=tf)
    sc.default = np.concatenate(run(imgs))
    assert sc.default.shape == (n, P.H, 3 * PW, 3)
    for k in range(n):
        np.testing.assert_array_equal(sc.default[k, :, :PW], host_panel(imgs[k]))
    assert len(np.unique(sc.default[:, :, PW:])) > 8                               # something is rendered next to the panel
    return sc


@pytest.mark.parametrize("source,workers", [("arrays", 0), ("callable", 0), ("paths", 0), ("paths", 2), ("arrays", 2), ("device", 0)])
def test_render_frames_device_panel_equals_the_default_path(scene, source, workers):
    rgb = {"arrays": scene.imgs, "callable": lambda i: scene.imgs[i], "paths": scene.paths, "device": [torch.as_tensor(im).cuda() for im in scene.imgs]}[source]
    chunks = scene.run(rgb, device_panel=True, decode_workers=workers)
    assert [len(c) for c in chunks] == [3, 2]                                      # the last chunk is shorter than `chunk`
    np.testing.assert_array_equal(np.concatenate(chunks), scene.default)


def test_render_frames_device_panel_with_top_view_and_on_device(scene):
    ref = scene.run(scene.imgs, add_top=True)
    got = scene.run(scene.paths, add_top=True, device_panel=True, decode_workers=2)
    assert len(ref) == len(got) == 2
    for (f0, t0), (f1, t1) in zip(ref, got):
        np.testing.assert_array_equal(f1, f0); np.testing.assert_array_equal(t1, t0)
    np.testing.assert_array_equal(np.concatenate([f for f, _ in ref]), scene.default)
    cut = P.H - ref[0][1].shape[1]
    np.testing.assert_array_equal(ref[0][1][:, :, :PW], ref[0][0][:, cut:, :PW])   # the strip's panel is the frame's
    dev = scene.run(scene.imgs, on_device=True, device_panel=True)
    assert all(torch.is_tensor(c) and c.is_cuda and c.dtype == torch.uint8 for c in dev)
    np.testing.assert_array_equal(torch.cat(dev).cpu().numpy(), scene.default)
    both = scene.run(scene.imgs, on_device=True, add_top=True, device_panel=True)
    np.testing.assert_array_equal(torch.cat([t for _, t in both]).cpu().numpy(), np.concatenate([t for _, t in ref]))


def test_pipeline_forwards_the_arguments(scene):
    from vistracker_amd.pipeline import SequencePipeline
    fake = SimpleNamespace(device="cuda:0", ctx=SimpleNamespace(smpl=scene.h))
    gen = SequencePipeline.render(fake, {"recon": scene.recon}, scene.kin, rgb=scene.paths, template=(scene.tv, scene.tf), chunk=3, image_size=P.SIZE,
                                  device_panel=True, decode_workers=2)
    np.testing.assert_array_equal(np.concatenate(list(gen)), scene.default)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(scene):
    from vistracker_amd import _lib as L, ops, sequence_io as SIO
    lib = L.lib()
    img = torch.as_tensor(P.image(1, *P.EXACT)).cuda()
    buf = torch.full((1, P.H, PW, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    off = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = L.stream_ptr()
    desc = lambda *row: np.array([row], np.int64)
    good = desc(0, 96, 128, 0, 128, 384)

    def call(d=good, src=img.data_ptr(), nbytes=img.numel(), n=1, H=P.H, size=P.SIZE, col0=P.CS, pw=PW, out=buf.data_ptr(), o=off.data_ptr(), rs=3 * PW):
        return lib.vt_resize_panel_u8(src, nbytes, d.ctypes.data if d is not None else None, n, H, size, col0, pw, out, o, rs, st)
    for kw in (dict(src=None), dict(d=None), dict(out=None), dict(o=None), dict(n=0), dict(n=-1), dict(H=0), dict(size=0), dict(pw=0), dict(col0=-1), dict(nbytes=0),
               dict(col0=30), dict(rs=3 * PW - 1),                                 # columns beyond the resize; output rows that overlap
               dict(d=desc(0, 0, 128, 0, 128, 384)), dict(d=desc(0, 96, 0, 0, 128, 384)), dict(d=desc(0, 96, 128, 0, 0, 384)), dict(d=desc(0, 96, 128, -1, 128, 384)),
               dict(d=desc(0, 96, 128, 0, 129, 387)), dict(d=desc(0, 96, 128, 0, 128, 383)),          # wider than the image; rows that overlap
               dict(d=desc(1, 96, 128, 0, 128, 384)), dict(d=desc(-1, 96, 128, 0, 128, 384)), dict(nbytes=img.numel() - 1), dict(d=desc(2 ** 63 - 200, 96, 128, 0, 128, 384)),      # rows that leave the source
               dict(d=desc(0, 96, 128, 25, 103, 309)), dict(d=desc(0, 96, 128, 0, 101, 303))):          # taps of columns [12, 51) are image columns 24 .. 101
        assert call(**kw) == L.VT_ERR_ARG, kw
    assert b"vt_resize_panel_u8" in lib.vt_last_error() and b"taps" in lib.vt_last_error()
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()                                                 # nothing was launched
    staged = img[:, 24:102].contiguous()                                           # exactly the taps' columns
    assert call(d=desc(0, 96, 128, 24, 78, 234), src=staged.data_ptr(), nbytes=staged.numel()) == L.VT_OK
    torch.cuda.synchronize()
    np.testing.assert_array_equal(buf[0].cpu().numpy(), host_panel(img.cpu().numpy()))
    with pytest.raises(L.VtError):                                                 # no CPU route
        ops.resize_panel_u8(img.cpu(), good, P.H, P.SIZE, P.CS, PW, buf, [0], 3 * PW)
    # the Python layer
    with pytest.raises(ValueError, match="decode_workers"):
        scene.run(scene.imgs, decode_workers=2)
    for bad in (scene.imgs[0].astype(np.float32), scene.imgs[0].astype(np.uint16), scene.imgs[0][..., 0], scene.imgs[0][..., :2], np.zeros((4, 96, 128, 3), np.uint8),
                img.float(), img[..., 0], img[:, ::2]):
        with pytest.raises(ValueError):
            scene.run([bad] * scene.n, device_panel=True)
    with pytest.raises(ValueError):
        SIO.device_panels([scene.imgs[0]], torch.zeros(2, P.H, PW, 3, dtype=torch.uint8, device="cuda"), P.SIZE, P.CS, P.CE)
