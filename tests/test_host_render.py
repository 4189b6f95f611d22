"""CPU: the host side of demo step 7 (vistracker_amd.visualize) against tests/golden/render_host.npz (tools/gen_golden_render.py ran the reference's
render/checkerboard.py, render/nr_utils.py, render/render_recon.py:prepare_verts and behave/utils.py:load_kinect_poses_back), and the panel arithmetic."""
import json
import os

import numpy as np
import torch

from conftest import golden
from vistracker_amd import visualize as V
from vistracker_amd.sequence_io import resize_bilinear, resize_bilinear_hw


def test_checkerboards_match_reference():
    g = golden("render_host")
    for name, args, kw in (("xz", (np.array([-40., 1.5, -40.]), 'xz'), dict(square_size=0.5, xlength=80.0, ylength=80.0)),
                           ("xy", (np.array([-40., -40., 4.0]), 'xy'), dict(square_size=0.75, xlength=80, ylength=80))):
        ck = V.CheckerBoard(); ck.init_checker(*args, **kw)
        v, f, t = (x.numpy() for x in ck.get_rends())
        assert v.dtype == np.float32 and t.shape[2:] == (1, 1, 1, 3)
        np.testing.assert_array_equal([v.shape[1], f.shape[1]], g[f"{name}_counts"])
        for part, sl in (("head", slice(0, 64)), ("tail", slice(-64, None))):
            np.testing.assert_array_equal(v[0, sl], g[f"{name}_v_{part}"])
            np.testing.assert_array_equal(f[0, sl], g[f"{name}_f_{part}"])
            np.testing.assert_array_equal(t[0, sl, 0, 0, 0], g[f"{name}_t_{part}"])
        np.testing.assert_allclose(v[0].astype(np.float64).sum(0), g[f"{name}_v_sum"], rtol=1e-12)
        np.testing.assert_array_equal(f[0].astype(np.int64).sum(0), g[f"{name}_f_sum"])
        np.testing.assert_allclose(t[0, :, 0, 0, 0].astype(np.float64).sum(0), g[f"{name}_t_sum"], rtol=1e-12)
    ck = V.CheckerBoard(); ck.init_checker(np.array([-1., 0.5, -2.]), 'xz', square_size=0.5, xlength=2.0, ylength=1.5)
    for x, k in zip(ck.get_rends(), ("small_v", "small_f", "small_t")):
        np.testing.assert_array_equal(x.numpy(), g[k])


def test_intrinsics_match_reference():
    g = golden("render_host")
    for k in range(4):
        K, r = V.get_kinect_K(1200, k)
        np.testing.assert_array_equal(K.numpy()[0], g["kinect_K"][k]); assert r == g["kinect_ratio"][k]
    for k in range(6):
        K, r = V.get_intercap_K(1200, k)
        np.testing.assert_array_equal(K.numpy()[0], g["intercap_K"][k]); assert r == g["intercap_ratio"][k]
    p = V.setup_renderer(image_size=1200, kid=1)
    assert p.orig_size == 1200.0 and p.anti_aliasing and p.fill_back and p.light_direction == [1, 0.5, 1]
    np.testing.assert_array_equal(p.light(), np.float32([0.4, 0.3, 1, 1, 1, 1, 1, 1, 1, 0.5, 1]))


def test_face_layout_matches_reference():
    g = golden("render_host")
    faces, tex = V.get_faces_and_textures([torch.tensor(g["scene_va"]), torch.tensor(g["scene_vb"])],
                                          [torch.tensor(g["scene_fa"]), torch.tensor(g["scene_fb"])], V.COLOR_LIST3)
    np.testing.assert_array_equal(faces.numpy(), g["scene_faces"])
    np.testing.assert_array_equal(tex.numpy()[0, :, 0, 0, 0], g["scene_tex"])
    # NrWrapper.prepare_render: meshes then the ground, offsets shifted by the mesh vertices
    w = V.NrWrapper.__new__(V.NrWrapper); w.colors = V.COLOR_LIST3
    ms = [V.Mesh(g["scene_va"][0], g["scene_fa"]), V.Mesh(g["scene_vb"][0], g["scene_fb"])]
    ck = V.CheckerBoard(); ck.init_checker(np.array([-1., 0.5, -2.]), 'xz', square_size=0.5, xlength=2.0, ylength=1.5)
    v, f, t = w.prepare_render(ms, checker=ck)
    np.testing.assert_array_equal(f[0, :10].numpy(), g["scene_faces"][0])
    np.testing.assert_array_equal(f[0, 10:].numpy(), g["small_f"][0] + 12)
    np.testing.assert_array_equal(t[0, 10:, 0, 0, 0].numpy(), g["small_t"][0, :, 0, 0, 0])
    assert v.shape == (1, 12 + g["small_v"].shape[1], 3)


def test_object_verts_match_reference():
    g = golden("render_host")
    ov = V.object_verts(g["obj_temp_v"], g["obj_angles"], g["obj_trans"], g["obj_scales"])
    np.testing.assert_allclose(ov, g["obj_verts"], rtol=0, atol=1e-12)


def test_kinect_poses_match_reference(tmp_path):
    g = golden("render_host")
    cfg = tmp_path / "calibs" / "config"
    for k, p in enumerate(g["kinect_poses"]):
        (cfg / str(k)).mkdir(parents=True)
        json.dump({"rotation": p[:9].tolist(), "translation": p[9:].tolist()}, open(cfg / str(k) / "config.json", "w"))
    rb, tb = V.load_kinect_poses_back(str(cfg), [0, 1])
    np.testing.assert_allclose(np.stack(rb), g["kinect_R_back"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.stack(tb), g["kinect_t_back"], rtol=0, atol=1e-12)
    seq = tmp_path / "Date01_Sub01_chair"; seq.mkdir()
    json.dump({"config": "../calibs/config", "kinects": [0, 1], "gender": "male", "cat": "chairwood", "empty": None, "intrinsic": None},
              open(seq / "info.json", "w"))
    kin = V.KinectTransform(str(seq))
    pts = np.random.default_rng(0).normal(size=(5, 3))
    for k in range(2):
        np.testing.assert_allclose(kin.world2local(pts, k), pts @ g["kinect_R_back"][k].T + g["kinect_t_back"][k], atol=1e-12)
        np.testing.assert_allclose(kin.local2world(kin.world2local(pts, k), k), pts, atol=1e-9)
    kin2 = V.KinectTransform(world2local_R=list(g["kinect_R_back"]), world2local_t=list(g["kinect_t_back"]))
    np.testing.assert_allclose(kin2.world2local(pts, 1), kin.world2local(pts, 1), atol=1e-12)
    kt = kin2.world2local_torch(torch.tensor(pts, dtype=torch.float32), 1)
    np.testing.assert_allclose(kt.numpy(), kin.world2local(pts, 1), atol=1e-5)


def test_panel_arithmetic():
    r = V.RendererSide2side.__new__(V.RendererSide2side)
    r.image_size, r.aspect_ratio, r.xcut_start, r.xcut_end = 1200, 0.75, 0.2, 0.8
    assert r.get_xcuts(1200) == (240, 960)
    for n in (1, 2, 3):
        assert r.frame_shape(n) == (900, 720 * (1 + 2 * n), 3)
    # (clip(rend, 0, 1) * 255).astype(uint8) truncates
    x = np.float32([-0.5, 0.0, 0.0039, 0.5, 0.99999, 1.0, 3.0])
    np.testing.assert_array_equal((np.clip(x, 0, 1) * 255).astype(np.uint8), [0, 0, 0, 127, 254, 255, 255])


def test_resize_bilinear_hw():
    img = np.random.default_rng(1).integers(0, 256, (48, 64, 3), dtype=np.uint8)
    out = resize_bilinear_hw(img, 30, 40)
    assert out.shape == (30, 40, 3) and out.dtype == np.uint8
    np.testing.assert_array_equal(resize_bilinear_hw(img, 24, 24), resize_bilinear(img, 24))
    # 2x down-sampling with half-pixel centres is the mean of 2 x 2 blocks (rounded)
    ref = np.floor(img.reshape(24, 2, 32, 2, 3).astype(np.float64).mean((1, 3)) + 0.5)
    assert np.abs(resize_bilinear_hw(img, 24, 32).astype(np.int32) - ref).max() <= 1


def test_write_frames(tmp_path):
    fr = np.zeros((2, 4, 6, 3), np.uint8); fr[1] = 200
    paths = V.write_frames([fr, fr[0]], str(tmp_path / "out"))
    assert len(paths) == 3 and all(os.path.exists(p) for p in paths)
