"""Golden vectors of HVOP-Net's training data set: the reference's ``TrainDataCMotionFiller.get_item`` on small synthetic packed sequences, with what
``np.random.randint`` and ``torch.randn`` returned recorded next to every returned array.  Build container only; writes tests/golden/clipdata.npz (data only).

The sequences are tests/clipdata_cases.py's, dumped with joblib into a temporary folder (plus the joint and occlusion arrays ``load_data`` insists on, which the
'params' representation never reads).  ``behave.kinect_transform.KinectTransform`` is replaced by a stand-in that only HOLDS seeded ``world2local_R`` /
``world2local_t``: the calibration reader is not pinned by this fixture.  ``get_item`` casts to float32 at its end (``astype(self.dtype)``); the data set is built
with ``dtype=np.float64`` so that the arrays are kept as the reference computed them.  Settings: T = 20, window 7; obj_repre '6d' and '9d'; aug_num 0 and 4; every
camera (``np.random.randint(0, 4)`` is steered through 0, 1, 2, 3 -- all other draws are numpy's own) and windows that overlap (recorded as drawn, one clip
steered onto overlapping starts).  Per setting k the file holds s<k>/<name> arrays stacked over four clips; gt_smpl equals
data_smpl element for element (asserted here) and is left out, which keeps the file under 1 MiB."""
import os, sys, tempfile, types
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(ROOT, "tests"))
import clipdata_cases as CC  # noqa: E402
import ref_harness as rh  # noqa: E402
torch = rh.enter_reference()
from unittest.mock import MagicMock  # noqa: E402
for m_ in ("behave", "behave.utils", "sklearn", "sklearn.decomposition", "sklearn.neighbors", "lib_smpl", "yacs", "yacs.config", "tensorboardX", "PIL", "PIL.Image",
           "PIL.ImageFilter", "interp", "interp.lib", "interp.lib.quaternions"):
    if m_ not in sys.modules:
        try:
            __import__(m_)
        except Exception:       # noqa: BLE001 -- an absent wheel, or a module that needs one
            sys.modules[m_] = MagicMock()

T, WINDOW, AUG = 20, 7, 4
K = CC.kinect()


class KinectTransform:
    """stand-in: holds the seeded world-to-local transforms of tests/clipdata_cases.kinect(), reads nothing"""

    def __init__(self, seq, no_intrinsic=True):
        date = [d for d in K if d in str(seq)]
        R, t = K[date[0]] if date else (np.tile(np.eye(3), (4, 1, 1)), np.zeros((4, 3)))
        self.world2local_R, self.world2local_t = [r.copy() for r in R], [x.copy() for x in t]


kt = types.ModuleType("behave.kinect_transform"); kt.KinectTransform = KinectTransform
sys.modules["behave.kinect_transform"] = kt
import data.data_paths as dp  # noqa: E402
dp.date_seqs = {f"Date{d:02d}": f"Date{d:02d}_stand_in" for d in range(1, 8)}
from data.traindata_cmfiller import TrainDataCMotionFiller  # noqa: E402

seqs, names = CC.sequences()
tmp = tempfile.mkdtemp()
import joblib  # noqa: E402
paths = []
for d, name in zip(seqs, names):
    n = len(d["frames"])
    full = dict(d, occ_ratios=np.zeros((n, 4)), joints_smpl=np.zeros((n, 52, 3)), joints_body=np.zeros((n, 25, 3)), joints_hand=np.zeros((n, 42, 3)),
                joints_face=np.zeros((n, 70, 3)))
    full["joints_smpl"][:, 0] = d["root_joints"]
    if n >= T:            # load_data skips a shorter sequence but still counts its frames (traindata_mfiller.py:92-93, 120, 130) and fails: the reference never sees it
        paths.append(os.path.join(tmp, name)); joblib.dump(full, paths[-1])

out = {"T": np.array(T), "window": np.array(WINDOW), "names": np.array(names), "kinect_dates": np.array(sorted(K)),
       "w2c_R": np.stack([K[d][0] for d in sorted(K)]), "w2c_t": np.stack([K[d][1] for d in sorted(K)])}
for i, d in enumerate(seqs):
    for k in ("poses", "trans", "root_joints", "obj_angles", "obj_trans"):
        out[f"seq{i}/{k}"] = d[k].astype(np.float32)
    out[f"seq{i}/n"] = np.array(len(d["frames"]))

real_randint, real_randn = np.random.randint, torch.randn
SETTINGS = [("6d", 0), ("9d", 0), ("6d", AUG), ("9d", AUG)]
for s, (repre, aug) in enumerate(SETTINGS):
    ds = TrainDataCMotionFiller(paths, T, WINDOW, 4, 0, phase="train", dtype=np.float64, start_fr_min=2, start_fr_max=12, min_drop_len=3, max_drop_len=8,
                                smpl_repre="params", obj_repre=repre, aug_num=aug, multi_kinects=True)
    clips = [0, 3, len(ds) // 2, len(ds) - 1]
    rec = {k: [] for k in ("clip", "kid", "drop_len", "start_fr", "aug_start", "noise", "data_smpl", "data_obj", "gt_smpl", "gt_obj", "mask_obj", "mask_smpl")}
    np.random.seed(1000 + s); torch.manual_seed(2000 + s)
    for n, c in enumerate(clips):
        ints, normals = [], []

        def randint(lo, hi=None, *a, **k):
            if len(ints) == 0 and ds.multi_kinects:
                v = n % 4                                               # the camera draw, steered through all four
            elif aug and n == 1 and len(ints) in (4, 6):
                v = ints[-1] + 1                                        # clip 1: windows 1 and 3 start one frame after windows 0 and 2 -- they overlap
                v = int(v) % (T - aug)
            else:
                v = real_randint(lo, hi, *a, **k)
            ints.append(int(np.asarray(v).reshape(-1)[0]))
            return v

        def randn(*a, **k):
            v = real_randn(*a, **k); normals.append(v.numpy().astype(np.float64)); return v

        np.random.randint, torch.randn = randint, randn
        try:
            item = ds.get_item(c)
        finally:
            np.random.randint, torch.randn = real_randint, real_randn
        assert len(ints) == 3 + aug and len(normals) == (1 if aug else 0), (ints, len(normals))
        assert ints[1] == item["drop_len"] and ints[2] == item["drop_start"]
        rec["clip"].append(c); rec["kid"].append(ints[0]); rec["drop_len"].append(ints[1]); rec["start_fr"].append(ints[2]); rec["aug_start"].append(ints[3:])
        rec["noise"].append(normals[0] if aug else np.zeros((0, 3)))
        for k in ("data_smpl", "data_obj", "gt_smpl", "gt_obj", "mask_obj", "mask_smpl"):
            assert item[k].dtype == (bool if k.startswith("mask") else np.float64), (k, item[k].dtype)
            rec[k].append(item[k])
        assert np.array_equal(item["gt_smpl"], item["data_smpl"])
    out[f"s{s}/obj_repre"], out[f"s{s}/aug_num"], out[f"s{s}/len"] = np.array(repre), np.array(aug), np.array(len(ds))
    for k, v in rec.items():
        if k == "gt_smpl":            # equal to data_smpl element for element (asserted above); left out to keep the file under 1 MiB
            continue
        a = np.stack(v)
        out[f"s{s}/{k}"] = a.astype(np.int32) if k in ("clip", "kid", "drop_len", "start_fr", "aug_start") else a
    out[f"s{s}/start_inds"], out[f"s{s}/clip_dates"] = np.asarray(ds.start_inds, np.int32), np.array(ds.clip_dates)
path = os.path.join(ROOT, "tests", "golden", "clipdata.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
