"""GPU (-m gpu): the network-input kernels of csrc/inputs.hip against the host loader they replace (``sequence_io.masks2bbox``, ``crop``, ``resize_bilinear``
and the compose of ``SequenceLoader.load_crop``), bit for bit; against the integer model of tests/inputs_model.py where fp32 blends round; and the loader
options ``device_prep`` / ``decode_workers`` on a small written sequence."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import inputs_model as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

cu = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host_compose(rgb, pm, om, center, crop_size, S):
    """the lines of SequenceLoader.load_crop behind the crop centre"""
    from vistracker_amd import sequence_io as SIO
    f = lambda a: SIO.resize_bilinear(SIO.crop(a, np.asarray(center), crop_size), S) / 255.0
    rgb, pm, om = f(rgb), f(pm), f(om)
    comb = (pm > 0.5) | (om > 0.5)
    return np.dstack((rgb * comb[..., None], pm, om)).transpose(2, 0, 1).astype(np.float32)


def corner_rows(centers, crop_size):
    return np.stack([np.concatenate(M.corners(c, crop_size)) for c in centers])


# ---- vt_mask_bbox -------------------------------------------------------------------------------------------------------------------------
def _bbox_cases(H, W):
    z = lambda: np.zeros((H, W), np.uint8)
    cases = []
    cases.append((z(), z()))                                                       # empty
    p = z(); p[0, 0] = 255; cases.append((p, z()))                                  # one pixel at (0, 0)
    o = z(); o[H - 1, W - 1] = 200; cases.append((z(), o))                          # one pixel at (W - 1, H - 1)
    p, o = z(), z(); p[5:9, 7:20] = 200; o[5:9, 7:20] = 100                         # 200 + 100 wraps to 44: empty ...
    p[20, 30] = 255; o[20, 30] = 255; cases.append((p, o))                          # ... but 255 + 255 = 254 counts
    p, o = z(), z(); p[3:30, 4:40] = 127; p[10:12, 11:17] = 128; o[15, 2] = 64; p[15, 2] = 64; cases.append((p, o))       # 127 no, 128 yes, 64 + 64 yes
    p = z(); p[H - 1, 10:21] = 255; cases.append((p, z()))                          # only the last row
    return cases


@pytest.mark.parametrize("H,W", [(37, 53), (48, 64)])           # 1 pixel per lane; 16 pixels per lane (rows of a multiple of 16 pixels)
def test_mask_bbox_equals_masks2bbox(H, W):
    from vistracker_amd import ops, sequence_io as SIO
    cases = _bbox_cases(H, W)
    for s in range(0, len(cases), 3):                                               # B = 3
        pm = np.stack([c[0] for c in cases[s:s + 3]]); om = np.stack([c[1] for c in cases[s:s + 3]])
        box = ops.mask_bbox(cu(pm), cu(om), 127).cpu().numpy()
        assert box.dtype == np.int32 and box.shape == (3, 4)
        for k in range(3):
            want = SIO.masks2bbox([pm[k], om[k]])
            got = SIO.bbox_from_device(box[k])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (s + k, box[k], want)
    assert tuple(box[2]) == (10, H - 1, 20, H - 1) and tuple(ops.mask_bbox(cu(cases[0][0][None]), cu(cases[0][1][None])).cpu().numpy()[0]) == (W, H, -1, -1)


def test_mask_bbox_random_masks_and_thresholds():
    from vistracker_amd import ops, sequence_io as SIO
    _, pm, om = M.frames(2, 4, 64, 80)
    pm[:, :9] = 0; om[:, :9] = 0; pm[:, :, 70:] = 0; om[:, :, 70:] = 0
    for thres in (127, 0, 254, 255):
        box = ops.mask_bbox(cu(pm), cu(om), thres).cpu().numpy()
        for k in range(4):
            want = SIO.masks2bbox([pm[k], om[k]], thres)
            got = SIO.bbox_from_device(box[k])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (thres, k)


# ---- vt_crop_resize_compose ---------------------------------------------------------------------------------------------------------------
H0, W0, CS, S0 = 96, 128, 75, 32
# interior; across the left, right (the dropped last column), top, bottom (the dropped last row) border; across two corners; odd / even centres
CENTERS = [(64, 48), (20, 48), (110, 50), (60, 12), (61, 85), (115, 88), (9, 10), (65, 47), (127, 95)]


@pytest.mark.parametrize("B", [1, 3, 5])
def test_crop_resize_compose_equals_the_host_loader(B):
    from vistracker_amd import ops
    rgb, pm, om = M.frames(20 + B, B, H0, W0)
    cs = [CENTERS[(2 * B + k) % len(CENTERS)] for k in range(B)] if B < 5 else CENTERS[1:6]
    want = np.stack([host_compose(rgb[k], pm[k], om[k], cs[k], CS, S0) for k in range(B)])
    out = torch.empty(B, 8, S0, S0, device="cuda")
    pattern = torch.arange(B * 3 * S0 * S0, device="cuda", dtype=torch.float32).view(B, 3, S0, S0) * 0.37 - 5.0
    out[:, 5:] = pattern; out[:, :5] = float("nan")
    ret = ops.crop_resize_compose(cu(rgb), cu(pm), cu(om), corner_rows(cs, CS), CS, S0, out=out)
    assert ret is out
    assert torch.equal(out[:, :5].cpu(), torch.from_numpy(want))
    assert torch.equal(out[:, 5:], pattern)
    q = np.rint(want[:, 3:] * 255).astype(int)
    assert (q == 127).any() and (q == 128).any()                                   # both sides of the composition threshold occur


def test_crop_resize_compose_every_centre_and_a_small_image():
    from vistracker_amd import ops
    B = len(CENTERS)
    rgb, pm, om = M.frames(31, B, H0, W0)
    want = np.stack([host_compose(rgb[k], pm[k], om[k], CENTERS[k], CS, S0) for k in range(B)])
    got = ops.crop_resize_compose(cu(rgb), cu(pm), cu(om), corner_rows(CENTERS, CS), CS, S0)
    assert tuple(got.shape) == (B, 5, S0, S0) and torch.equal(got.cpu(), torch.from_numpy(want))
    rgb, pm, om = M.frames(32, 2, 40, 50)                                           # smaller than the crop: padded on every side
    cs = [(25, 20), (44, 7)]
    want = np.stack([host_compose(rgb[k], pm[k], om[k], cs[k], CS, S0) for k in range(2)])
    got = ops.crop_resize_compose(cu(rgb), cu(pm), cu(om), corner_rows(cs, CS), CS, S0)
    assert torch.equal(got.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("crop_size,S", [(70, 32), (70, 30)])
def test_crop_resize_against_the_integer_model(crop_size, S):
    """70 -> 32 (the weights are still multiples of 1 / 64: every blend exact) and 70 -> 30 (ratio 7 / 3: fp32 blends round).  Grey levels equal the exact
    model's wherever the exact blend is more than 1e-3 grey levels from a half-way point (fp32 blend error: a few ulp of 255, ~1e-4), elsewhere within one
    level; at most 1 % of the values are that close (tests/test_host_inputs.py shows it for these frames from the model alone)."""
    from vistracker_amd import ops
    rgb, pm, om = M.frames(11, 2, H0, W0)
    cs = [(64, 48), (110, 80)]
    got = ops.crop_resize_compose(cu(rgb), cu(pm), cu(om), corner_rows(cs, crop_size), crop_size, S).cpu().numpy()
    table = ops.div255_table()
    near = total = 0
    for b in range(2):
        (q_rgb, d_rgb), (q_pm, d_pm), (q_om, d_om) = (M.crop_resize(a[b], cs[b], crop_size, S) for a in (rgb, pm, om))
        gq = np.rint(got[b, 3:] * 255).astype(int)                                  # mask channels are stored as they are
        assert np.array_equal(table[gq], got[b, 3:])
        for g, q, d in ((gq[0], q_pm, d_pm), (gq[1], q_om, d_om)):
            assert np.array_equal(g[d > 1e-3], q[d > 1e-3]) and np.abs(g - q.astype(int)).max() <= 1
            near += int((d <= 1e-3).sum()); total += d.size
        comb = (gq[0] >= 128) | (gq[1] >= 128)                                      # the device's own composition decision
        grgb = np.rint(got[b, :3] * 255).astype(int).transpose(1, 2, 0)
        assert np.array_equal(table[grgb], got[b, :3].transpose(1, 2, 0)) and not grgb[~comb].any()
        sel = comb[..., None] & (d_rgb > 1e-3)
        assert np.array_equal(grgb[sel], q_rgb[sel]) and np.abs(grgb - q_rgb.astype(int))[comb].max() <= 1
        near += int((d_rgb <= 1e-3).sum()); total += d_rgb.size
    assert near / total <= 0.01, near / total
    if S == 32:
        for b in range(2):
            q = [M.crop_resize(a[b], cs[b], crop_size, S)[0] for a in (rgb, pm, om)]
            assert np.array_equal(got[b], M.compose(*q, table))                     # exact blends: the whole tensor, bit for bit


# ---- the loader -----------------------------------------------------------------------------------------------------------------------------
def _write_sequence(root, T, H=240, W=320):
    from PIL import Image
    rng = np.random.default_rng(4)
    seq = os.path.join(root, "data", "Date03_Sub03_chairwood")
    frames, files = [], []
    boxes = [(60, 90, 140, 200), (0, 5, 120, 90), (150, 200, 239, 319), (100, 0, 200, 60), (30, 250, 110, 318), (90, 120, 150, 180)]
    for i in range(T):
        name = f"t{i:04d}.000"; frames.append(name)
        ff = os.path.join(seq, name); os.makedirs(ff)
        y0, x0, y1, x1 = boxes[i % len(boxes)]
        pm = np.zeros((H, W), np.uint8); pm[y0:y1, x0:x1] = 255; pm[y0:y1, x0:x0 + 3] = (60, 127, 128); pm[y0 + 5:y0 + 9, x0 + 5:x1 - 5] = 128
        om = np.zeros((H, W), np.uint8); om[(y0 + y1) // 2:y1, (x0 + x1) // 2:x1] = 255; om[(y0 + y1) // 2, (x0 + x1) // 2:x1] = 127
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        Image.fromarray(pm).save(os.path.join(ff, "k1.person_mask.png"))
        Image.fromarray(np.dstack([om, om // 2, om // 3]) if i % 2 else om).save(os.path.join(ff, "k1.obj_rend_mask.png"))       # a three-channel mask: channel 0 counts
        Image.fromarray(rgb).save(os.path.join(ff, "k1.color.jpg"), quality=90)
        files.append(os.path.join(ff, "k1.color.jpg"))
    return frames, files


@pytest.fixture(scope="module")
def written(synth, tmp_path_factory):
    """6 frames of 240 x 320 on disk, their SMPL-T parameters, and the batches of the host loader (device_prep=False): the reference of the tests below"""
    from vistracker_amd import ops, sequence_io as SIO, synthetic as syn
    T = 6
    frames, files = _write_sequence(str(tmp_path_factory.mktemp("inputs")), T)
    sp = syn.sequence_params(T, seed=7)
    smplt = {"poses": sp["pose"], "betas": sp["betas"], "trans": sp["trans"], "frames": frames}
    ctx = SimpleNamespace(smpl=ops.SmplhHandle(synth["model"]), b25=ops.LandmarkHandle(synth["regs"]["body25"]))
    make = lambda **kw: SIO.SequenceLoader(files, 4, smplt, ctx, synth["model"]["f"], image_size=64, crop_size=150, **kw)
    return {"files": files, "smplt": smplt, "make": make, "host": list(make(device_prep=False))}


@pytest.mark.parametrize("device_prep,decode_workers", [(True, 2), (True, 0), (False, 2)])
def test_loader_settings_give_the_same_batches(written, device_prep, decode_workers):
    ref = written["host"]
    got = list(written["make"](device_prep=device_prep, decode_workers=decode_workers))
    assert [b["images"].shape[0] for b in ref] == [4, 2] == [b["images"].shape[0] for b in got]
    for a, b in zip(ref, got):
        assert list(a.keys()) == list(b.keys())
        for k in a:
            if torch.is_tensor(a[k]):
                assert a[k].dtype == b[k].dtype and a[k].device == b[k].device and torch.equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k
    img = torch.cat([b["images"] for b in ref])
    assert float(img[:, :3].abs().sum()) > 0 and float(img[:, 3].sum()) > 0 and float(img[:, 4].sum()) > 0 and float(img[:, 5:].sum()) > 0


def test_prepare_crops_equals_the_loader(written):
    from vistracker_amd import sequence_io as SIO
    ref = written["host"]
    for kw in ({}, {"decode_workers": 2, "chunk": 4}, {"device_prep": False}):
        img, cc = SIO.prepare_crops(written["files"], image_size=64, crop_size=150, **kw)
        assert img.is_cuda and img.dtype == torch.float32 and cc.dtype == np.float32
        assert torch.equal(img, torch.cat([b["images"][:, :5] for b in ref])) and np.array_equal(cc, torch.cat([b["crop_center"] for b in ref]).numpy())


def test_from_paths_hands_the_options_to_its_loader(written, tmp_path):
    """``from_paths(device_prep=, decode_workers=)`` -> ``sequence_loader``: the options, the fitter's context, faces, device and network size reach the
    ``SequenceLoader``, and its batches equal those of a host loader on the same context"""
    from types import SimpleNamespace as NS
    from test_host_paths import _make_tree
    from vistracker_amd import sequence_io as SIO
    from vistracker_amd.recon_fit import ReconFitterTriVisFull
    t = _make_tree(tmp_path)
    args = NS(exp_name="tri-vis-l2", checkpoint=None, net_img_size=[512, 512], loadSize=1200)
    fitter = ReconFitterTriVisFull.from_paths(t["seq"], False, None, args, paths=t["paths"], device_prep=True, decode_workers=2)
    files, smplt = written["files"], written["smplt"]
    full = fitter.sequence_loader(files, 4, smplt)
    assert isinstance(full, SIO.SequenceLoader) and full.device_prep is True and full.decode_workers == 2 and full.ctx is fitter.ctx
    assert full.image_size == fitter.net_in_size == 512 and full.crop_size == 1200 and full.device == fitter.device and full.bs == 4
    plain = ReconFitterTriVisFull.from_paths(t["seq"], False, None, args, paths=t["paths"]).sequence_loader(files, 4, smplt)
    assert plain.device_prep is False and plain.decode_workers == 0
    got = list(fitter.sequence_loader(files, 4, smplt, image_size=64, crop_size=150))
    ref = list(SIO.SequenceLoader(files, 4, smplt, fitter.ctx, fitter.smpl_faces, image_size=64, crop_size=150))
    assert len(got) == len(ref) == 2
    for a, b in zip(ref, got):
        assert list(a.keys()) == list(b.keys())
        for k in a:
            assert (a[k].dtype == b[k].dtype and torch.equal(a[k], b[k])) if torch.is_tensor(a[k]) else a[k] == b[k], k
    for a, b in zip(written["host"], got):                                          # the image channels do not depend on the body model
        assert torch.equal(a["images"][:, :5], b["images"][:, :5]) and torch.equal(a["crop_center"], b["crop_center"])


def test_frames_of_two_sizes_in_one_chunk():
    from vistracker_amd import sequence_io as SIO
    a, b = M.frames(41, 2, 96, 128), M.frames(42, 1, 80, 112)
    for m in a[1:] + b[1:]:
        m[:, :10] = 0; m[:, -10:] = 0; m[:, :, :10] = 0; m[:, :, -10:] = 0
    decoded = [(a[0][0], a[1][0], a[2][0]), (b[0][0], b[1][0], b[2][0]), (a[0][1], a[1][1], a[2][1])]
    names = ["f0", "f1", "f2"]
    want = [SIO.host_crop(d, n, 76, 32) for d, n in zip(decoded, names)]
    out = torch.zeros(3, 8, 32, 32, device="cuda")
    cc = SIO.device_crops(decoded, names, out, 76, 32)
    assert torch.equal(out[:, :5].cpu(), torch.from_numpy(np.stack([w[0] for w in want]))) and np.array_equal(cc, np.stack([w[1] for w in want]))
    assert not out[:, 5:].any()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from vistracker_amd import _lib as L, ops
    lib = L.lib()
    rgb, pm, om = (cu(a) for a in M.frames(1, 1, 16, 16))
    box = torch.full((1, 4), 77, dtype=torch.int32, device="cuda")
    out = torch.full((1, 5, 8, 8), 3.0, device="cuda")
    corners = torch.tensor([[0, 0, 12, 12]], dtype=torch.int32, device="cuda")
    table = cu(ops.div255_table())
    st = L.stream_ptr()
    p = lambda t: t.data_ptr()
    assert lib.vt_mask_bbox(p(pm), p(om), 0, 16, 16, 127, p(box), st) == L.VT_ERR_ARG
    assert lib.vt_mask_bbox(p(pm), p(om), -1, 16, 16, 127, p(box), st) == L.VT_ERR_ARG
    assert lib.vt_mask_bbox(None, p(om), 1, 16, 16, 127, p(box), st) == L.VT_ERR_ARG
    assert lib.vt_mask_bbox(p(pm), p(om), 1, 16, 16, 127, None, st) == L.VT_ERR_ARG
    crc = lambda rgb_, B, cs, S, out_: lib.vt_crop_resize_compose(rgb_, p(pm), p(om), B, 16, 16, p(corners), cs, S, p(table), out_, 5 * 8 * 8, st)
    assert crc(p(rgb), 0, 12, 8, p(out)) == L.VT_ERR_ARG
    assert crc(None, 1, 12, 8, p(out)) == L.VT_ERR_ARG
    assert crc(p(rgb), 1, 12, 8, None) == L.VT_ERR_ARG
    assert crc(p(rgb), 1, 0, 8, p(out)) == L.VT_ERR_ARG
    assert crc(p(rgb), 1, -3, 8, p(out)) == L.VT_ERR_ARG
    assert crc(p(rgb), 1, 12, 0, p(out)) == L.VT_ERR_ARG
    assert b"vt_crop_resize_compose" in lib.vt_last_error()
    torch.cuda.synchronize()
    assert (box == 77).all() and (out == 3.0).all()                                 # nothing was launched
    assert crc(p(rgb), 1, 12, 8, p(out)) == L.VT_OK and lib.vt_mask_bbox(p(pm), p(om), 1, 16, 16, 127, p(box), st) == L.VT_OK
    torch.cuda.synchronize()
    assert not (out == 3.0).any() and not (box == 77).any()
    with pytest.raises(L.VtError):                                                  # no CPU route
        ops.mask_bbox(pm.cpu(), om.cpu())
    with pytest.raises(L.VtError):
        ops.crop_resize_compose(rgb.cpu(), pm.cpu(), om.cpu(), [[0, 0, 12, 12]], 12, 8)
    with pytest.raises(ValueError):                                                 # corners that are no crop of crop_size
        ops.crop_resize_compose(rgb, pm, om, [[0, 0, 20, 12]], 12, 8)
