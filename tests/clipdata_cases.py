"""The inputs of the clip data set's tests (tests/clipdata_model.py is the model): seeded synthetic packed sequences, world-to-local transforms, explicit
decisions that reach every edge, and the clip table restated from traindata_mfiller.py:85-99.

Rotation magnitudes are bounded so that no rotation the chain takes the logarithm of comes near the angle pi, where that map is discontinuous: the root and the
object turn by at most 1.2 rad, a camera by at most 1.2 rad, so a composed rotation stays below 2.4 rad and its quaternion's scalar part above cos(1.2) = 0.36."""
import numpy as np

import clipdata_model as M

SEQS = (("Date01_Sub01_chairwood_hand", 200), ("Date03_Sub04_boxtiny", 15), ("Date03_Sub03_yogamat", 230))        # (name, frames); the second is shorter than most clips
SHAPES = ((1, 1), (3, 17), (2, 180))                                                                                # (B, T)
AUG = 4
W_MIN = 0.05          # the least |w| an un-masked augmented frame may have in a case (float32 reach of w = 0 is ~1e-6)

f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)          # noqa: E731 -- float32 values in float64 storage: both dtypes start from the same numbers


def _bounded(r, n, lim):
    """a smooth (n, 3) rotation-vector track of norm <= lim"""
    t = np.linspace(0, 1, n)[:, None]
    v = np.sin(2 * np.pi * (t * r.uniform(0.5, 2, (1, 3)) + r.uniform(0, 1, (1, 3)))) + 0.05 * r.randn(n, 3)
    return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-9) * (lim * (0.15 + 0.85 * np.abs(np.sin(3 * t + r.uniform(0, 3)))))


def sequence(name, n, seed):
    """one packed sequence file's dict (packing.pack_recon's keys that the data set reads, obj_angles as rotation vectors)"""
    r = np.random.RandomState(seed)
    t = np.linspace(0, 1, n)[:, None]
    pose = 0.6 * np.sin(2 * np.pi * (t * r.uniform(0.3, 2, (1, 156)) + r.uniform(0, 1, (1, 156)))) + 0.02 * r.randn(n, 156)
    pose[:, :3] = _bounded(r, n, 1.2)
    pose[0, 3:6] = 0.0                                              # an exact zero rotation: the 1e-8 quirk of the norm
    trans = np.cumsum(0.01 * r.randn(n, 3), 0) + r.uniform(-1, 1, 3) + [0, 0, 2.5]
    return dict(poses=f32(pose), trans=f32(trans), root_joints=f32(trans + [0.0, -0.25, 0.03] + 0.01 * r.randn(n, 3)), obj_angles=f32(_bounded(r, n, 1.2)),
                obj_trans=f32(trans + r.uniform(-0.5, 0.5, 3) + 0.02 * np.cumsum(r.randn(n, 3), 0)), frames=[f"t{i:04d}.000" for i in range(n)])


def sequences():
    return [sequence(name, n, 900 + i) for i, (name, n) in enumerate(SEQS)], [f"{name}.pkl" for name, _ in SEQS]


def kinect(seed=77):
    """{date: (R (4, 3, 3), t (4, 3))}: proper rotations by at most 1.2 rad"""
    r = np.random.RandomState(seed)
    out = {}
    for date in ("Date01", "Date03"):
        rv = np.stack([_bounded(r, 1, 1.2)[0] * (1.0 if r.rand() < 0.5 else 0.7) for _ in range(4)])
        R = f32(M.rotvec_to_matrix(rv))
        out[date] = (R, f32(r.uniform(-2, 2, (4, 3))))
    return out


def clip_table(seqs, names, clip_len, window):
    """traindata_mfiller.py:85-99 -> (tables of the kept sequences, clip starts, clip date numbers, sorted dates, number of kept sequences)"""
    cols = {k: [] for k in ("poses", "trans", "roots", "obj_angles", "obj_trans")}
    starts, dates, offset, n_seq = [], [], 0, 0
    for d, name in zip(seqs, names):
        n = len(d["frames"])
        if n < clip_len:
            continue
        for i in range(0, n - clip_len + 1, window):
            starts.append(i + offset); dates.append(name.split("_")[0])
        offset += n; n_seq += 1
        cols["poses"].append(np.concatenate([d["poses"][:, :69], d["poses"][:, 111:114]], 1))
        for k, src in (("trans", "trans"), ("roots", "root_joints"), ("obj_angles", "obj_angles"), ("obj_trans", "obj_trans")):
            cols[k].append(d[src])
    names_sorted = sorted(set(dates))
    return {k: np.concatenate(v) for k, v in cols.items()}, np.asarray(starts, np.int32), np.asarray([names_sorted.index(x) for x in dates], np.int32), names_sorted, n_seq


def model_data(clip_len, window, K=None):
    seqs, names = sequences()
    tab, starts, dates, date_names, n_seq = clip_table(seqs, names, clip_len, window)
    K = kinect() if K is None else K
    tab["w2c_R"], tab["w2c_t"] = np.stack([K[d][0] for d in date_names]), np.stack([K[d][1] for d in date_names])
    return tab, starts, dates, n_seq


def decisions(B, T, aug_num, kid0):
    """explicit decisions reaching the edges: every camera over the cases (kid = (b + kid0) % 4); clip 0 dropped from frame 0, clip 1's drop ending on the last
    frame the rule allows (start_fr = T - drop_len - 1); windows that overlap each other (two of them start on the same frame) and the dropped frames"""
    kid = np.asarray([(b + kid0) % 4 for b in range(B)], np.int32)
    if T == 1:
        dl, sf = np.asarray([kid0 % 2] * B, np.int32), np.zeros(B, np.int32)
    else:
        dl = np.asarray([min(5 + 2 * b, T - 2) for b in range(B)], np.int32)
        sf = np.asarray([0 if b == 0 else (T - dl[b] - 1 if b == 1 else 3) for b in range(B)], np.int32)
    au = np.zeros((B, aug_num), np.int32)
    for b in range(B):
        if aug_num:
            hi = T - aug_num
            au[b] = [(3 + b) % hi, (5 + b) % hi, (hi - 1), (5 + b) % hi][:aug_num] if aug_num == 4 else [(3 * j + b) % hi for j in range(aug_num)]
    return dict(kid=kid, drop_len=dl, start_fr=sf, aug_start=au)


def build_cases():
    """(B, T) x obj_repre x aug_num in {0, 4} (no window fits T = 1), the cameras cycling so that each is taken"""
    out, n = [], 0
    for B, T in SHAPES:
        for repre in ("6d", "9d"):
            for aug in (0, AUG):
                if aug and T - aug <= 0:
                    continue
                out.append(dict(id=f"B{B}-T{T}-{repre}-aug{aug}-kid{n % 4}", B=B, T=T, obj_repre=repre, obj_dim=6 if repre == "6d" else 9, aug_num=aug, kid0=n % 4,
                                window=7, seed=400 + n))
                n += 1
    return out


_built = {}


def build(c):
    """the case's inputs, its float64 reference and its float32 run, computed once"""
    if c["id"] not in _built:
        tab, starts, dates, _ = model_data(c["T"], c["window"])
        r = np.random.RandomState(c["seed"])
        idx = r.choice(len(starts), c["B"], replace=False).astype(np.int32)
        dec = decisions(c["B"], c["T"], c["aug_num"], c["kid0"])
        noise = f32(r.randn(c["B"], c["aug_num"] ** 2, 3))
        run = lambda dt, mutant=None: M.build(tab, starts[idx], dates[idx], dec, c["T"], c["obj_dim"], noise, dt, mutant)          # noqa: E731
        _built[c["id"]] = dict(c, tab=tab, idx=idx, dec=dec, noise=noise, ref64=run(np.float64), ref32=run(np.float32), run=run)
    return _built[c["id"]]


def min_aug_w(ref):
    """the least |w| over the un-masked augmented frames of a model run (inf without one)"""
    sel = ref["aug"] & ~ref["mask_obj"]
    return float(np.abs(ref["aug_w"][sel]).min()) if sel.any() else float("inf")
