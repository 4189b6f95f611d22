"""CPU: the overlay / mask-score models' own properties (tests/overlay_model.py), the frame layout with overlay panels, ``sequence_io.decode_masks`` and the
declarations of the two new entry points.  Nothing here needs a GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import overlay_model as M
from conftest import ROOT


def test_overlay_model_identities():
    rng = np.random.default_rng(0)
    rgb = rng.uniform(-0.2, 1.2, (5, 7, 3)).astype(np.float32); alpha = rng.uniform(0, 1, (5, 7)).astype(np.float32)
    panel = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    q, _ = M.overlay(rgb, alpha, panel, 0.0)
    np.testing.assert_array_equal(q, panel)                                          # opacity 0
    q, _ = M.overlay(np.zeros_like(rgb), np.zeros_like(alpha), panel, 0.6)
    np.testing.assert_array_equal(q, panel)                                          # nothing rendered
    q, _ = M.overlay(np.ones_like(rgb), np.ones_like(alpha), panel, 1.0)
    assert (q == 255).all()                                                          # full coverage, full opacity: the render
    q, d = M.overlay(np.full((1, 1, 3), 0.5, np.float32), np.ones((1, 1), np.float32), np.full((1, 1, 3), 100, np.uint8), 0.5)
    assert (q == 114).all() and np.allclose(d, 0.25)                                 # 63.75 + 50 = 113.75


def test_score_model_on_masks_made_from_the_owner_map():
    rng = np.random.default_rng(1)
    F, nb, no = 50, 20, 17
    d = M.random_owners(rng, 32, F, nb, no)
    pm, om = M.masks_of_owners(d, 24, F, nb, no)
    c = M.score(d, 24, F, nb, no, pm, om)
    assert (c[:, 0] == c[:, 1]).all() and (c[:, 1] == c[:, 2]).all() and (c[:, 3] == 0).all() and (c[:, 1] > 0).all()
    np.testing.assert_array_equal(M.iou(c), [1.0, 1.0])
    # the same masks at three times the resolution: nearest neighbour at half-pixel centres finds the same pixels
    c3 = M.score(d, 24, F, nb, no, np.kron(pm, np.ones((3, 3), np.uint8)), np.kron(om, np.ones((3, 3), np.uint8)))
    np.testing.assert_array_equal(c3, c)
    # swapped masks: nothing intersects, every mask pixel is hidden behind the other class
    cs = M.score(d, 24, F, nb, no, om, pm)
    assert (cs[:, 0] == 0).all() and (cs[:, 3] == cs[:, 2]).all()
    assert np.isnan(M.iou(np.zeros((2, 4), np.int64))).all()
    # ids: reversed copies map back, -1 / >= 2 F / the third range are neither class
    np.testing.assert_array_equal(M.classes(np.array([0, nb - 1, nb, nb + no - 1, nb + no, F - 1, F, F + nb, 2 * F - 1, 2 * F, -1]), F, nb, no),
                                  [0, 0, 1, 1, -1, -1, 0, 1, -1, -1, -1])


def test_frame_shape_with_overlay():
    from vistracker_amd.visualize import RendererSide2side as R
    for size, pw, H in ((1200, 720, 900), (64, 39, 48), (16, 9, 12)):
        r = SimpleNamespace(image_size=size, aspect_ratio=0.75, xcut_start=0.2, xcut_end=0.8)
        r.get_xcuts = lambda s, r=r: R.get_xcuts(r, s)
        for n in (1, 2, 3):
            assert R.frame_shape(r, n) == (H, pw * (1 + 2 * n), 3)
            assert R.frame_shape(r, n, overlay=False) == R.frame_shape(r, n)
            assert R.frame_shape(r, n, overlay=True) == (H, pw * (1 + 3 * n), 3)
            r.frame_shape = lambda k, overlay=False, r=r: R.frame_shape(r, k, overlay)
            assert R.top_shape(r, n) == (H - int(0.3 * H), pw * (1 + n), 3)          # the strips do not grow


def test_decode_masks_finds_and_decodes_like_the_loader(tmp_path):
    from PIL import Image
    from vistracker_amd import sequence_io as SIO
    rng = np.random.default_rng(2)
    pm, om3 = M.random_mask(rng, 9, 11), M.random_mask(rng, 9, 11, 3)
    a = tmp_path / "seq" / "t0001.000"; a.mkdir(parents=True)
    Image.fromarray(pm).save(a / "k1.person_mask.png"); Image.fromarray(om3).save(a / "k1.obj_rend_mask.png")
    Image.fromarray(np.zeros((9, 11), np.uint8)).save(a / "k1.obj_mask.png")        # the rendered mask comes first in the loader's rule
    got = SIO.decode_masks(str(a / "k1.color.jpg"))                                  # the colour image does not exist: it is not opened
    assert got[0].shape == (9, 11) and got[1].shape == (9, 11, 3)
    np.testing.assert_array_equal(got[0], pm); np.testing.assert_array_equal(got[1], om3)
    b = tmp_path / "seq" / "t0002.000"; b.mkdir()
    Image.fromarray(pm).save(b / "k1.person_mask.png"); Image.fromarray(om3[..., 0]).save(b / "k1.obj_mask.png")
    Image.fromarray(rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)).save(b / "k1.color.jpg")
    got = SIO.decode_masks(str(b / "k1.color.jpg"))
    np.testing.assert_array_equal(got[1], om3[..., 0])
    rgb, p2, o2 = SIO.decode_frame(str(b / "k1.color.jpg"))                          # decode_frame shares the rule
    assert rgb.shape == (9, 11, 3)
    np.testing.assert_array_equal(p2, got[0]); np.testing.assert_array_equal(o2, got[1])
    with pytest.raises(FileNotFoundError):
        SIO.decode_masks(str(tmp_path / "seq" / "t0003.000" / "k1.color.jpg"))
    # staging: channel 0, packed, back to back
    stage, desc = SIO.stage_masks([(pm, om3), (om3, pm)], pin=False)
    host = stage.numpy()
    assert desc.tolist() == [[0, 99, 9, 11, 1, 11, 1, 11], [198, 297, 9, 11, 1, 11, 1, 11]] and host.size == 396
    np.testing.assert_array_equal(host[99:198].reshape(9, 11), om3[..., 0]); np.testing.assert_array_equal(host[198:297].reshape(9, 11), om3[..., 0])
    # sources: sequences and callables, paths decoded
    pairs = [c for c in SIO.mask_sources(lambda i: str((a if i == 0 else b) / "k1.color.jpg"), [0, 1, 0], 2)]
    assert [len(c) for c in pairs] == [2, 1]
    np.testing.assert_array_equal(pairs[0][1][1], om3[..., 0]); np.testing.assert_array_equal(pairs[1][0][1], om3)


def test_new_symbols_are_declared():
    from vistracker_amd import _lib, ops, pipeline, visualize
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vistracker.h")).read(), flags=re.S)
    for name, nargs in (("vt_overlay_panel_u8", 14), ("vt_mask_score", 15)):
        assert re.search(rf"\bint {name}\s*\(", src), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        decl = re.search(rf"\bint {name}\s*\((.*?)\);", src, flags=re.S).group(1)
        assert len(decl.split(",")) == nargs
    assert callable(ops.overlay_panel_u8) and callable(ops.mask_score)
    assert callable(visualize.RendererSide2side.mask_scores) and callable(pipeline.SequencePipeline.mask_scores)
    import inspect
    for fn in (visualize.RendererSide2side.render_frames, pipeline.SequencePipeline.render):
        p = inspect.signature(fn).parameters
        assert p["overlay"].default is False and p["overlay_opacity"].default == 0.6
    mk = open(os.path.join(ROOT, "vistracker_amd", "csrc", "Makefile")).read()
    assert "overlay.hip" in mk
