"""Golden vectors of the contact search of demo step 7: the reference's own ContactVisualizer.get_contact_spheres (render/nr_utils.py:380-404, a scipy
cKDTree of the SMPL vertices queried with the object's) on the four frames of tests/contact_model.scene(4, FIXTURE_TOUCH, FIXTURE_SEED): three where
2-4 body parts touch the object, one where none does.  psbody is stubbed (the sphere mesh is not recorded: its tessellation is parity unpinned) and the
visualizer is built without its constructor, so no asset file is read; labels are synthetic.part_labels.  Recorded: the inputs, and per frame the
kd-tree's idx and dist (recomputed the way :382-383 does), the contact mask, and the per-part counts and centres get_contact_spheres returns.
Build container only: writes tests/golden/contact.npz (data only)."""
import os
import sys
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(ROOT, "tests"))
import contact_model as M  # noqa: E402
import ref_harness as rh  # noqa: E402

sc = M.scene(4, M.FIXTURE_TOUCH, M.FIXTURE_SEED)          # before the reference is entered (it changes the working directory)
torch = rh.enter_reference()


class Mesh:
    def __init__(self, v=None, f=None, fc=None, vc=None):
        self.v, self.f = v, f


class Sphere:
    def __init__(self, center, radius):
        self.center, self.radius = np.asarray(center), radius

    def to_mesh(self):
        return self


sys.modules["psbody.mesh"].Mesh = Mesh
sys.modules["psbody.mesh.sphere"].Sphere = Sphere
for name in ("imageio", "joblib", "pytorch3d.renderer", "lib_smpl", "recon.eval.pose_utils"):
    sys.modules.setdefault(name, MagicMock())
from render import nr_utils  # noqa: E402

THRES, RADIUS, P = 0.04, 0.06, 14
cv = nr_utils.ContactVisualizer.__new__(nr_utils.ContactVisualizer)
cv.part_labels, cv.part_colors, cv.thres, cv.radius = sc["labels"], np.zeros((P, 3)), THRES, RADIUS
B, NVo = sc["obj"].shape[:2]
idx, dist = np.zeros((B, NVo), np.int64), np.zeros((B, NVo))
mask = np.zeros((B, NVo), bool); count = np.zeros((B, P), np.int64); centre = np.zeros((B, P, 3)); part = np.full((B, NVo), -1, np.int64)
for b in range(B):
    smpl, obj = Mesh(v=sc["smpl"][b].astype(np.float64)), Mesh(v=sc["obj"][b].astype(np.float64))
    dist[b], idx[b] = nr_utils.KDTree(smpl.v).query(obj.v)
    mask[b] = dist[b] < cv.thres
    for p, (_, sphere, ind) in cv.get_contact_spheres(smpl, obj).items():
        assert sphere.radius == RADIUS
        count[b, p], centre[b, p], part[b, ind] = len(ind), sphere.center, p
    assert (part[b] >= 0).tolist() == mask[b].tolist()
    print(f"frame {b}: parts {np.nonzero(count[b])[0].tolist()} with {count[b][count[b] > 0].tolist()} vertices")
out = dict(smpl=sc["smpl"], obj=sc["obj"], labels=sc["labels"].astype(np.int32), thres=np.float64(THRES), radius=np.float64(RADIUS), idx=idx.astype(np.int32),
           dist=dist, mask=mask, part=part.astype(np.int32), count=count.astype(np.int32), centre=centre)
path = os.path.join(ROOT, "tests", "golden", "contact.npz")
np.savez_compressed(path, **out)
print("wrote tests/golden/contact.npz", os.path.getsize(path), "bytes")
