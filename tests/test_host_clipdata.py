"""CPU: the numpy model of the clip data set (tests/clipdata_model.py) against the reference's recorded ``get_item`` (tests/golden/clipdata.npz,
tools/gen_golden_clipdata.py), against scipy's ``Rotation``, and the hashed draws against a plain-Python restatement; the float32 model and the named mutants
against the gates of tests/test_gpu_clipdata.py.  Measured figures: tests/golden/clipdata.md."""
import numpy as np
import pytest

import clipdata_cases as CC
import clipdata_model as M
from conftest import golden

# The recording is float64 throughout (the data set was built with dtype float64) and the model's float64 run restates it with equivalent formulas (Rodrigues'
# formula against scipy's quaternion route): what separates them is float64 rounding through a chain of about a hundred operations on values of at most 4, the
# logarithm's 1 / w <= 3 included: 4096 eps x 4 = 3.6e-12 is a generous ceiling for that and 1e-4 of the float32 scale.
F64_BOUND = 4096 * np.finfo(np.float64).eps * 4.0


def golden_setting(g, s):
    """-> (tables, clip starts, clip dates, recorded clips / decisions / noise / arrays, T, obj_dim)"""
    names = [str(n) for n in g["names"]]
    seqs = [dict({k: g[f"seq{i}/{k}"].astype(np.float64) for k in ("poses", "trans", "root_joints", "obj_angles", "obj_trans")}, frames=[0] * int(g[f"seq{i}/n"]))
            for i in range(len(names))]
    T = int(g["T"])
    tab, starts, dates, date_names, n_seq = CC.clip_table(seqs, names, T, int(g["window"]))
    assert date_names == [str(d) for d in g["kinect_dates"]]
    tab["w2c_R"], tab["w2c_t"] = g["w2c_R"], g["w2c_t"]
    rec = {k: g[f"s{s}/{k}"] for k in ("clip", "kid", "drop_len", "start_fr", "aug_start", "noise", "data_smpl", "data_obj", "gt_obj", "mask_obj", "mask_smpl")}
    rec["gt_smpl"] = rec["data_smpl"]
    return tab, starts, dates, rec, T, 6 if str(g[f"s{s}/obj_repre"]) == "6d" else 9, n_seq


@pytest.mark.parametrize("s", range(4))
def test_float64_model_equals_the_recording(s):
    g = golden("clipdata")
    tab, starts, dates, rec, T, od, n_seq = golden_setting(g, s)
    # the clip table: the short sequence is skipped, the reference (which was given the long ones only) agrees on every start and date
    assert np.array_equal(starts, g[f"s{s}/start_inds"]) and len(starts) == int(g[f"s{s}/len"]) and n_seq == 2
    assert [sorted(set(map(str, g[f"s{s}/clip_dates"])))[d] for d in dates] == [str(x) for x in g[f"s{s}/clip_dates"]]
    assert sorted(set(rec["kid"].tolist())) == [0, 1, 2, 3]
    idx = rec["clip"]
    m = M.build(tab, starts[idx], dates[idx], rec, T, od, rec["noise"], np.float64)
    worst = 0.0
    for k in ("data_smpl", "data_obj", "gt_smpl", "gt_obj"):
        d = float(np.abs(m[k] - rec[k]).max()); worst = max(worst, d)
        print(f"\n[recording] setting {s} ({od}d, aug {rec['aug_start'].shape[1]}) {k}: max |model - recording| = {d:.3e}", end="")
        assert d <= F64_BOUND, (k, d)
    assert np.array_equal(m["mask_obj"], rec["mask_obj"]) and not rec["mask_smpl"].any() and not m["mask_smpl"].any()
    if rec["aug_start"].shape[1]:
        a = rec["aug_start"][1]
        assert a[1] == a[0] + 1 and a[3] == a[2] + 1, "the recorded clip 1 has overlapping windows"
        assert CC.min_aug_w(m) >= CC.W_MIN
    # the recorded draws lie in the ranges the reference's calls define
    assert ((rec["drop_len"] >= 3) & (rec["drop_len"] <= 8) & (rec["start_fr"] >= 2) & (rec["start_fr"] < np.minimum(T - rec["drop_len"], 12))).all()


def test_rotations_equal_scipy():
    R = pytest.importorskip("scipy.spatial.transform").Rotation
    r = np.random.RandomState(5)
    a = np.concatenate([r.randn(200, 3), 1e-6 * r.randn(20, 3), np.zeros((1, 3)), 3.0 * r.randn(50, 3) / 1.7])
    a = a[np.abs(np.linalg.norm(a, axis=1) % (2 * np.pi) - np.pi) > 0.05]
    m = R.from_rotvec(a).as_matrix()
    assert np.abs(M.rotvec_to_matrix(a) - m).max() < 1e-14
    assert np.abs(M.matrix_to_rotvec(m) - R.from_matrix(m).as_rotvec()).max() < 1e-12
    # axis -> 6D is the first two columns of that matrix up to the reference's 1e-8 quirks; 6D -> axis inverts it away from the angle pi
    six = M.axis_to_6d(a)
    assert np.abs(six - m[:, :, :2].reshape(-1, 6)).max() < 1e-7
    back, w = M.rot6d_to_axis(m[:, :, :2].reshape(-1, 6))
    assert np.abs(back - R.from_matrix(m).as_rotvec()).max() < 1e-9
    # a zeroed row sits exactly on (0, pi, 0) in both dtypes
    for dt in (np.float64, np.float32):
        z, wz = M.rot6d_to_axis(np.zeros((1, 6), dt))
        assert z[0, 0] == 0 and z[0, 2] == 0 and z[0, 1] == dt(2) * np.arctan2(dt(0.5), dt(0)) / dt(0.5) * dt(0.5) and wz[0] == 0


DRAW = dict(T=180, multi_kinects=True, min_drop_len=10, max_drop_len=40, start_fr_min=10, start_fr_max=50, aug_num=4)


def test_draws_equal_a_plain_python_restatement():
    from vistracker_amd import infill_training as IT
    clips = [0, 1, 2, 77, 2 ** 31 - 1]
    for seed, epoch in ((0, 0), (7, 3), (0x9abcdef012345678, 2 ** 32 - 1)):
        a, b = M.draw(clips, seed, epoch, **DRAW), M.draw(clips, seed, epoch, hash_fn=IT.dropout_hash, **DRAW)
        for k in a:
            assert a[k].dtype == np.int32 and np.array_equal(a[k], b[k])
        # by hand, for one clip
        e = (epoch << 32) | 77
        key = IT.dropout_hash(seed, 16, e) | (IT.dropout_hash(seed, 17, e) << 32)
        dl = 10 + ((IT.dropout_hash(key, 19, 0) * 31) >> 32)
        assert a["drop_len"][3] == dl and a["kid"][3] == (IT.dropout_hash(key, 18, 0) * 4) >> 32
        assert a["start_fr"][3] == 10 + ((IT.dropout_hash(key, 20, 0) * (min(180 - dl, 50) - 10)) >> 32)
        assert a["aug_start"][3, 2] == (IT.dropout_hash(key, 21, 2) * 176) >> 32
    # a decision depends on (seed, epoch, clip) only: not on the position in the batch nor on its size
    one = M.draw([77], 7, 3, **DRAW)
    assert all(np.array_equal(one[k][0], M.draw(clips, 7, 3, **DRAW)[k][3]) for k in one)
    assert not np.array_equal(M.draw(clips, 7, 4, **DRAW)["aug_start"], M.draw(clips, 7, 3, **DRAW)["aug_start"])
    assert (M.draw(clips, 7, 3, **dict(DRAW, multi_kinects=False))["kid"] == 1).all()


def test_draws_stay_in_range_and_hit_both_ends():
    d = M.draw(range(10000), 12345, 1, **DRAW)
    assert set(d["kid"].tolist()) == {0, 1, 2, 3}
    assert d["drop_len"].min() == 10 and d["drop_len"].max() == 40
    hi = np.minimum(180 - d["drop_len"], 50)
    assert (d["start_fr"] >= 10).all() and (d["start_fr"] < hi).all() and d["start_fr"].min() == 10 and (d["start_fr"] == hi - 1).any()
    assert d["aug_start"].min() == 0 and d["aug_start"].max() == 175
    # a short clip, where T - drop_len is what bounds the start
    s = M.draw(range(10000), 5, 0, T=20, multi_kinects=False, min_drop_len=3, max_drop_len=8, start_fr_min=2, start_fr_max=50, aug_num=2)
    hi = 20 - s["drop_len"]
    assert (s["start_fr"] >= 2).all() and (s["start_fr"] < hi).all() and (s["start_fr"] == hi - 1).any() and s["aug_start"].max() == 17
    z = M.hashed_noise(range(64), 9, 2, 4)
    assert z.shape == (64, 16, 3) and np.isfinite(z).all() and abs(z.mean()) < 0.1 and abs(z.std() - 1) < 0.1
    z32 = M.hashed_noise(range(64), 9, 2, 4, np.float32)
    assert z32.dtype == np.float32 and np.abs(z32 - z).max() < 1e-5


@pytest.mark.parametrize("c", CC.build_cases(), ids=lambda c: c["id"])
def test_float32_model_meets_the_gates_and_cases_keep_clear_of_pi(c):
    b = CC.build(c)
    res, bad = M.gate(b["ref32"], b["ref64"], b["ref32"], c["obj_dim"])
    assert not bad, bad
    # no un-masked augmented frame within reach of the discontinuity (w = 0): nothing has to be left out of a case, in either dtype
    assert CC.min_aug_w(b["ref64"]) >= CC.W_MIN and CC.min_aug_w(b["ref32"]) >= CC.W_MIN
    # masked rows are exact zeros, their mask set; gt is data where a frame is neither masked nor augmented
    free = ~b["ref64"]["mask_obj"] & ~b["ref64"]["aug"]
    assert (b["ref64"]["data_obj"][b["ref64"]["mask_obj"] & ~b["ref64"]["aug"]] == 0).all()
    assert np.array_equal(b["ref64"]["data_obj"][free], b["ref64"]["gt_obj"][free])
    if c["T"] > 1:
        d = b["dec"]
        assert d["start_fr"][0] == 0 and d["start_fr"][1] + d["drop_len"][1] == c["T"] - 1
    if c["aug_num"]:
        assert (b["ref64"]["aug"] & b["ref64"]["mask_obj"]).any(), "a window reaches into the dropped frames"


def test_every_camera_is_taken():
    assert sorted({int(k) for c in CC.build_cases() for k in CC.decisions(c["B"], c["T"], c["aug_num"], c["kid0"])["kid"]}) == [0, 1, 2, 3]


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_mutants_fail_the_gates(mutant):
    c = next(c for c in CC.build_cases() if c["id"].startswith("B3-T17-9d-aug4"))
    b = CC.build(c)
    res, bad = M.gate(b["run"](np.float64, mutant), b["ref64"], b["ref32"], c["obj_dim"])
    print(f"\n[mutant] {mutant}: fails {[(k, f'{e:.2e}' if not isinstance(e, str) else e) for k, e, _ in bad]}", end="")
    assert bad, mutant
    # and in float32 as well: the mistake is not hidden by rounding
    assert M.gate(b["run"](np.float32, mutant), b["ref64"], b["ref32"], c["obj_dim"])[1]
