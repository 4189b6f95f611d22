"""CPU: the integer model of step 7's camera panel (tests/panel_model.py) against the host path it restates (``sequence_io.resize_bilinear_hw``), the staged
source columns (``sequence_io.panel_columns``, ``stage_panels``' descriptors) against the taps' true extent, and the new keyword arguments' defaults."""
import inspect

import numpy as np
import pytest

import panel_model as P

torch = pytest.importorskip("torch")


def test_model_equals_the_host_path_where_blends_are_exact():
    from vistracker_amd.sequence_io import resize_bilinear_hw
    img = P.image(1, *P.EXACT)
    q, d = P.resize_hw(img, P.H, P.SIZE)
    np.testing.assert_array_equal(q, resize_bilinear_hw(img, P.H, P.SIZE))
    # the rounding rule is exercised: a quarter of these blends sit exactly on a half-way point (sums of four bytes over 16 ... over 4)
    assert 0.2 < (d == 0).mean() < 0.32


@pytest.mark.parametrize("h,w", P.ROUNDING)
def test_model_against_the_host_path_where_fp32_rounds(h, w):
    """fp32 tap positions and blends carry a few ulp of 255 (~1e-4 grey levels): the host path equals the exact model except within 1e-3 of a half-way point,
    there within one level; at most 2 % of the values are that close"""
    from vistracker_amd.sequence_io import resize_bilinear_hw
    img = P.image(2, h, w)
    q, d = P.resize_hw(img, P.H, P.SIZE)
    got = resize_bilinear_hw(img, P.H, P.SIZE)
    clear = d > 1e-3
    print(f"{h} x {w}: host path differs from the model in {int((got != q).sum())} of {q.size} values; {100 * (1 - clear.mean()):.2f} % within 1e-3 of a half-way point")
    np.testing.assert_array_equal(got[clear], q[clear])
    assert np.abs(got.astype(int) - q.astype(int)).max() <= 1
    assert 1 - clear.mean() <= 0.02


def test_model_clamps_and_identity():
    img = P.image(3, 30, 40)
    q, d = P.resize_hw(img, 30, 40)                                                # same size: every tap has weight 1
    np.testing.assert_array_equal(q, img)
    assert (d == 0.5).all()
    q2, _ = P.resize_hw(img[..., 0], 60, 80)                                       # a grey image, up-scaled: corners are the source's corners
    assert q2.shape == (60, 80) and q2[0, 0] == img[0, 0, 0] and q2[-1, -1] == img[-1, -1, 0]


def fp32_taps(w, size):
    """i0, i1 of every output column by the fp32 tap rule of csrc/inputs.hip, op by op"""
    f = np.float32
    scale = f(w) / f(size)
    src = np.maximum(scale * (np.arange(size, dtype=f) + f(0.5)) - f(0.5), f(0))
    assert src.dtype == f
    i0 = np.minimum(src.astype(np.int64), w - 1)
    return i0, np.minimum(i0 + 1, w - 1)


@pytest.mark.parametrize("w,size,cs,ce", [(128, 64, 12, 51), (110, 64, 12, 51), (101, 64, 12, 51), (40, 64, 12, 51), (2048, 1200, 240, 960), (1920, 1200, 240, 960),
                                         (64, 64, 0, 64), (7, 64, 0, 64), (1, 64, 12, 51), (300, 100, 99, 100), (2048, 1200, 0, 1)])
def test_staged_columns_hold_every_tap_and_little_else(w, size, cs, ce):
    from vistracker_amd.sequence_io import panel_columns
    x0, x1 = panel_columns(w, size, cs, ce)
    assert 0 <= x0 < x1 <= w
    i0, i1 = fp32_taps(w, size)
    lo, hi = int(i0[cs:ce].min()), int(i1[cs:ce].max())                             # what the kernel reads ...
    elo, ehi = P.tap_extent(w, size, cs, ce)                                       # ... and what exact arithmetic would
    assert x0 <= min(lo, elo) and max(hi, ehi) < x1
    assert x0 >= max(min(lo, elo) - 1, 0) and x1 <= min(max(hi, ehi) + 2, w)       # one spare column on either side, no more
    assert (np.diff(i0) >= 0).all() and (np.diff(i1) >= 0).all()                   # the taps grow with the column: first and last column bound them


def test_staged_share_at_the_production_size():
    from vistracker_amd.sequence_io import panel_columns
    x0, x1 = panel_columns(2048, 1200, 240, 960)
    assert (x0, x1) == (408, 1640) and 0.6 <= (x1 - x0) / 2048 <= 0.61


def test_stage_descriptors():
    """``stage_panels`` on images of two sizes: offsets back to back, rows packed, the staged bytes are the images' columns (pinned memory needs a GPU runtime:
    ``pin=False`` gives an ordinary buffer)"""
    from vistracker_amd import sequence_io as SIO
    imgs = [P.image(4, 96, 128), P.image(5, 83, 110)[:, ::-1], P.image(6, 96, 128)]            # the second one is a view with negative strides
    stage, desc = SIO.stage_panels(imgs, P.SIZE, P.CS, P.CE, pin=False)
    host, total = stage.numpy(), 0
    for (off, h, w, x0, sw, rs), img in zip(desc.tolist(), imgs):
        assert (off, h, w, rs) == (total, img.shape[0], img.shape[1], 3 * sw) and (x0, x0 + sw) == SIO.panel_columns(w, P.SIZE, P.CS, P.CE)
        np.testing.assert_array_equal(host[off:off + h * rs].reshape(h, sw, 3), img[:, x0:x0 + sw])
        total += h * rs
    assert total == stage.numel() and desc.dtype == np.int64


def test_sources_fetch_in_order_with_and_without_the_pool(tmp_path):
    from PIL import Image
    from vistracker_amd import sequence_io as SIO
    imgs = [P.image(10 + k, 12, 16) for k in range(5)]
    paths = []
    for k, im in enumerate(imgs):
        paths.append(str(tmp_path / f"c{k}.png")); Image.fromarray(im).save(paths[-1])
    for rgb in (imgs, lambda i: imgs[i], paths, lambda i: paths[i]):
        for workers in (0, 2):
            chunks = list(SIO.panel_sources(rgb, [4, 0, 2, 1, 3], 2, workers))
            assert [len(c) for c in chunks] == [2, 2, 1]
            for got, i in zip([im for c in chunks for im in c], [4, 0, 2, 1, 3]):
                np.testing.assert_array_equal(got, imgs[i])
    calls = []
    gen = SIO.panel_sources(lambda i: calls.append(i) or imgs[i], range(5), 2, 0)
    next(gen)
    assert calls == [0, 1]                                                         # without a pool nothing is fetched ahead


def test_new_arguments_are_off_by_default():
    from vistracker_amd import visualize as V
    from vistracker_amd.pipeline import SequencePipeline
    for fn in (V.RendererSide2side.render_frames, SequencePipeline.render):
        p = inspect.signature(fn).parameters
        assert p["device_panel"].default is False and p["decode_workers"].default == 0
