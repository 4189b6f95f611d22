"""CPU: the contract of csrc/inputs.hip against the host loader it replaces -- the exact integer model of tests/inputs_model.py equals
``resize_bilinear(crop(...))`` where fp32 blends are exact, the / 255 table holds the host's values, and the new loader options default to today's path."""
import inspect
import os

import numpy as np
import pytest

import inputs_model as M
from vistracker_amd import sequence_io as SIO

# crop centres (x, y) in a W x H image: interior, across the left / right / top / bottom border, across a corner
centres = lambda W, H, c: [(W // 2, H // 2), (c // 4, H // 2), (W - c // 4, H // 2), (W // 2, c // 4), (W // 2, H - c // 4), (W - c // 8, H - c // 8), (c // 8, c // 8)]


@pytest.mark.parametrize("H,W,crop_size,S,channels", [(96, 128, 75, 32, 3), (97, 127, 75, 32, 1), (1536, 2048, 1200, 512, 1)])
def test_integer_model_equals_the_host_resize(H, W, crop_size, S, channels):
    """ratio 2.34375 (and 74 / 32, 76 / 32: numpy rounds the corners of an odd crop size to even): weights are multiples of 1 / 64, every fp32 blend is exact"""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (H, W, 3) if channels == 3 else (H, W), dtype=np.uint8)
    extents = set()
    for c in centres(W, H, crop_size) + [(W // 2 + 1, H // 2)]:
        want = SIO.resize_bilinear(SIO.crop(img, np.array(c), crop_size), S)
        got, _ = M.crop_resize(img, c, crop_size, S)
        assert got.dtype == np.uint8 and np.array_equal(got, want), c
        tl, br = M.corners(c, crop_size)
        extents.add(int(br[0] - tl[0]))
    assert extents == ({1200} if crop_size == 1200 else {74, 76})


def test_model_crop_is_the_host_crop():
    """the model's own zero-padded crop, the dropped last column / row included, and an image smaller than the crop"""
    rng = np.random.default_rng(6)
    for H, W, cs in ((96, 128, 75), (40, 50, 75), (96, 128, 70)):
        img = rng.integers(1, 256, (H, W), dtype=np.uint8)
        for c in centres(W, H, cs):
            if not (0 < c[0] < W and 0 < c[1] < H):
                continue
            tl, br = M.corners(c, cs)
            assert np.array_equal(M.padded_crop(img, tl, br), SIO.crop(img, np.array(c), cs)), (H, W, cs, c)


def test_div255_table_holds_the_host_values():
    from vistracker_amd import ops
    t = ops.div255_table()
    assert t.dtype == np.float32 and t.shape == (256,)
    for q in range(256):
        assert t[q] == np.float32(q / 255.0)
    assert np.array_equal(t, (np.arange(256, dtype=np.uint8) / 255.0).astype(np.float32))          # what load_crop stores


def test_excluded_share_of_the_non_dyadic_case():
    """the frames of test_gpu_inputs' crop 70 -> 30 case: at most 1 % of the exact blends lie within 1e-3 of a half-way point"""
    rgb, pm, om = M.frames(11, 2, 96, 128)
    near = total = 0
    for b, c in enumerate([(64, 48), (110, 80)]):
        for img in (rgb[b], pm[b], om[b]):
            _, dist = M.crop_resize(img, c, 70, 30)
            near += int((dist <= 1e-3).sum()); total += dist.size
    assert near / total <= 0.01, near / total


def test_new_loader_options_default_to_the_host_path():
    from vistracker_amd.recon_fit import ReconFitterTriVisFull
    p = inspect.signature(SIO.SequenceLoader.__init__).parameters
    assert p["device_prep"].default is False and p["decode_workers"].default == 0
    p = inspect.signature(SIO.prepare_crops).parameters
    assert p["device_prep"].default is True and p["decode_workers"].default == 0 and p["image_size"].default == 512 and p["crop_size"].default == 1200
    p = inspect.signature(ReconFitterTriVisFull.from_paths).parameters
    assert p["device_prep"].default is False and p["decode_workers"].default == 0


def _write_frames(root, n, H, W):
    from PIL import Image
    rgb, pm, om = M.frames(3, n, H, W)
    files = []
    for i in range(n):
        ff = os.path.join(root, "seq", f"t{i:04d}.000"); os.makedirs(ff)
        Image.fromarray(rgb[i]).save(os.path.join(ff, "k1.color.jpg"), quality=90)
        Image.fromarray(pm[i]).save(os.path.join(ff, "k1.person_mask.png")); Image.fromarray(om[i]).save(os.path.join(ff, "k1.obj_rend_mask.png"))
        files.append(os.path.join(ff, "k1.color.jpg"))
    return files


def test_decode_pool_keeps_order_and_is_capped(tmp_path):
    files = _write_frames(str(tmp_path), 5, 60, 80)
    assert [SIO.decode_threads(n) for n in (-1, 0, 2, 16, 64)] == [0, 0, 2, 16, 16] and SIO.MAX_DECODE_WORKERS == 16
    assert SIO._decode_pool(0) is None
    serial = list(SIO._decoded_chunks(files, 2, 0))
    pooled = list(SIO._decoded_chunks(files, 2, 3))
    assert [s for s, _, _ in serial] == [0, 2, 4] == [s for s, _, _ in pooled]
    for (_, fa, da), (_, fb, db) in zip(serial, pooled):
        assert fa == fb and len(da) == len(db) == len(fa)
        for x, y in zip(da, db):
            assert all(np.array_equal(u, v) for u, v in zip(x, y))


def test_device_path_refuses_images_that_are_not_8_bit():
    """raised before anything touches the device"""
    rgb, pm, om = M.frames(3, 1, 20, 24)
    with pytest.raises(ValueError, match="8-bit"):
        SIO.device_crops([(rgb[0], pm[0].astype(np.uint16) * 257, om[0])], ["f0"], None, 12, 8)
    with pytest.raises(ValueError, match="8-bit"):
        SIO.device_crops([(rgb[0], pm[0], om[0] > 127)], ["f0"], None, 12, 8)


def test_prepare_crops_host_path_is_load_crop(tmp_path):
    """device_prep=False on the CPU: the same values as the loader's load_crop, for every decode_workers"""
    files = _write_frames(str(tmp_path), 3, 60, 80)
    want = [SIO.host_crop(SIO.decode_frame(f), f, 40, 16) for f in files]
    for workers in (0, 2):
        img, cc = SIO.prepare_crops(files, image_size=16, crop_size=40, device="cpu", device_prep=False, decode_workers=workers, chunk=2)
        assert img.dtype.is_floating_point and tuple(img.shape) == (3, 5, 16, 16) and cc.dtype == np.float32
        assert np.array_equal(img.numpy(), np.stack([w[0] for w in want])) and np.array_equal(cc, np.stack([w[1] for w in want]))
