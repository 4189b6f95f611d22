"""Golden vectors of the host side of demo step 7 (render/checkerboard.py, render/nr_utils.py:381-415,480-525, render/render_recon.py:prepare_verts,
behave/utils.py:load_kinect_poses_back).  The rasteriser itself is neural_renderer (absent: parity unpinned, see csrc/render.hip).  psbody.mesh.Mesh is
replaced by a stand-in that stores v, f, fc.  Build container only: writes tests/golden/render_host.npz."""
import json
import os
import sys
import tempfile
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

torch = rh.enter_reference()


class Mesh:
    def __init__(self, v=None, f=None, fc=None, vc=None):
        self.v, self.f, self.fc = v, f, fc


sys.modules["psbody.mesh"].Mesh = Mesh
for name in ("imageio", "joblib", "pytorch3d.renderer", "lib_smpl", "recon.eval.pose_utils"):
    sys.modules.setdefault(name, MagicMock())
torch.cuda.FloatTensor = lambda data: torch.tensor(data, dtype=torch.float32)

from render.checkerboard import CheckerBoard  # noqa: E402
from render import nr_utils  # noqa: E402
from behave.utils import load_kinect_poses_back  # noqa: E402
from render.render_recon import RendererBase  # noqa: E402

out = {}
# the two boards of RendererBase.__init__ (render_recon.py:55-62): counts + first / last 64 rows of the large ones
for name, args, kw in (("xz", (np.array([-40., 1.5, -40.]), 'xz'), dict(square_size=0.5, xlength=80.0, ylength=80.0)),
                       ("xy", (np.array([-40., -40., 4.0]), 'xy'), dict(square_size=0.75, xlength=80, ylength=80))):
    ck = CheckerBoard(); ck.init_checker(*args, **kw)
    v, f, t = (x.cpu().numpy() for x in ck.get_rends())
    out[f"{name}_counts"] = np.array([v.shape[1], f.shape[1]])
    for part, sl in (("head", slice(0, 64)), ("tail", slice(-64, None))):
        out[f"{name}_v_{part}"] = v[0, sl]; out[f"{name}_f_{part}"] = f[0, sl]; out[f"{name}_t_{part}"] = t[0, sl, 0, 0, 0]
    out[f"{name}_v_sum"] = v[0].astype(np.float64).sum(0); out[f"{name}_f_sum"] = f[0].astype(np.int64).sum(0)
    out[f"{name}_t_sum"] = t[0, :, 0, 0, 0].astype(np.float64).sum(0)
# a small board in full
ck = CheckerBoard(); ck.init_checker(np.array([-1., 0.5, -2.]), 'xz', square_size=0.5, xlength=2.0, ylength=1.5)
out["small_v"], out["small_f"], out["small_t"] = (x.cpu().numpy() for x in ck.get_rends())
# intrinsics at 1200
out["kinect_K"] = np.stack([nr_utils.get_kinect_K(1200, k)[0].numpy()[0] for k in range(4)])
out["kinect_ratio"] = np.array([nr_utils.get_kinect_K(1200, k)[1] for k in range(4)])
out["intercap_K"] = np.stack([nr_utils.get_intercap_K(1200, k)[0].numpy()[0] for k in range(6)])
out["intercap_ratio"] = np.array([nr_utils.get_intercap_K(1200, k)[1] for k in range(6)])
# face / colour layout of a two-mesh scene
rng = np.random.default_rng(21)
va, vb = rng.normal(size=(1, 7, 3)).astype(np.float32), rng.normal(size=(1, 5, 3)).astype(np.float32)
fa, fb = rng.integers(0, 7, (6, 3)).astype(np.int32), rng.integers(0, 5, (4, 3)).astype(np.int32)
faces, tex = nr_utils.get_faces_and_textures([torch.tensor(va), torch.tensor(vb)], [torch.tensor(fa), torch.tensor(fb)], nr_utils.COLOR_LIST3)
out.update(scene_va=va, scene_vb=vb, scene_fa=fa, scene_fb=fb, scene_faces=faces.numpy(), scene_tex=tex.numpy()[0, :, 0, 0, 0])
# object vertices of packed rows (render_recon.py:prepare_verts, a recon that is not 'gt')
T, NV = 4, 9
temp_v = rng.normal(0, 0.3, (NV, 3))
A = rng.normal(size=(T, 3, 3)); Q = np.linalg.qr(A)[0]
pack = {"frames": [f"t{i}" for i in range(T)], "poses": np.zeros((T, 156), np.float32), "betas": np.zeros((T, 10), np.float32),
        "trans": np.zeros((T, 3), np.float32), "gender": "male", "obj_angles": Q.astype(np.float32),
        "obj_trans": rng.normal(0, 1, (T, 3)).astype(np.float32), "obj_scales": rng.uniform(0.8, 1.2, T).astype(np.float32)}
fake = MagicMock(); fake.smplh_layer = lambda p, b, t: (torch.zeros(len(p), 6890, 3),)
_, verts_obj = RendererBase.prepare_verts(fake, [pack], ["recon"], Mesh(v=temp_v))
out.update(obj_temp_v=temp_v, obj_angles=pack["obj_angles"], obj_trans=pack["obj_trans"], obj_scales=pack["obj_scales"], obj_verts=verts_obj[0])
# inverse Kinect poses of a synthetic two-camera config folder
poses = []
with tempfile.TemporaryDirectory() as d:
    for k in range(2):
        R = np.linalg.qr(rng.normal(size=(3, 3)))[0]; t = rng.normal(0, 1.5, 3)
        os.makedirs(os.path.join(d, str(k)))
        json.dump({"rotation": R.reshape(-1).tolist(), "translation": t.tolist()}, open(os.path.join(d, str(k), "config.json"), "w"))
        poses.append(np.concatenate([R.reshape(-1), t]))
    rb, tb = load_kinect_poses_back(d, [0, 1])
out.update(kinect_poses=np.stack(poses), kinect_R_back=np.stack(rb), kinect_t_back=np.stack(tb))
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "render_host.npz"), **out)
print("wrote tests/golden/render_host.npz", os.path.getsize(os.path.join(ROOT, "tests", "golden", "render_host.npz")), "bytes")
