"""Float64 model of the contact step (csrc/contact.hip, visualize.ContactVisualizer / look_at_view_transform): brute-force nearest neighbour with the
smaller index on exact ties, threshold, per-part counts and means, face recolouring, sphere placement, the look-at matrices -- written from
render/nr_utils.py:380-404, :100-122 and the issue's definitions, sharing no code with the package.  Also the two 'near case' masks the GPU tests
exclude: vertices whose answer an fp32 rounding may legitimately change."""
import numpy as np

NEAR_TIE_REL = 1e-5         # best and second-best squared distances closer than this (relative): the fp32 argmin may differ
NEAR_THRES_ABS = 4e-6       # |dist - thres| below this (metres): the fp32 compare may differ (fp32 error of a distance at <= 4 m ~ 5e-7)
MAX_NEAR_SHARE = 0.01


def nearest(smpl_v, obj_v, block=128):
    """smpl_v (NVs,3), obj_v (NVo,3) -> idx (NVo,) int64 (smaller index on exact ties), d2 best (NVo,), d2 second best (NVo,), float64"""
    s, o = np.asarray(smpl_v, np.float64), np.asarray(obj_v, np.float64)
    idx, d1, d2 = np.zeros(len(o), np.int64), np.zeros(len(o)), np.zeros(len(o))
    for i in range(0, len(o), block):
        q = o[i:i + block]
        D = ((q[:, None, 0] - s[None, :, 0]) ** 2 + (q[:, None, 1] - s[None, :, 1]) ** 2) + (q[:, None, 2] - s[None, :, 2]) ** 2
        j = D.argmin(1)                                             # numpy: the first (smallest) index among equal minima
        r = np.arange(len(j))
        idx[i:i + block], d1[i:i + block] = j, D[r, j]
        D[r, j] = np.inf
        d2[i:i + block] = D.min(1)
    return idx, d1, d2


def regions(smpl_v, labels, obj_v, thres, P=14):
    """-> dict: idx, dist, part (-1 = none), count (P,), centre (P,3) float64 (0 where count == 0), near (NVo,) bool near-tie | near-threshold"""
    labels = np.asarray(labels)
    idx, d1, d2 = nearest(smpl_v, obj_v)
    dist = np.sqrt(d1)
    part = np.where(dist < thres, labels[idx], -1)
    near_tie = (d2 - d1) < NEAR_TIE_REL * d2
    near_thres = np.abs(dist - thres) < NEAR_THRES_ABS
    o = np.asarray(obj_v, np.float64)
    count = np.array([(part == p).sum() for p in range(P)])
    centre = np.stack([o[part == p].mean(0) if count[p] else np.zeros(3) for p in range(P)])
    return {"idx": idx, "dist": dist, "part": part, "count": count, "centre": centre, "near_tie": near_tie, "near_thres": near_thres,
            "near": near_tie | near_thres}


def face_colors(part, obj_faces, face_off, base, palette):
    """(NF,3) colours: base, the object's faces with a corner in contact recoloured, parts applied in ascending order (the highest wins)"""
    out = np.array(base, np.float64)
    f = np.asarray(obj_faces)
    for p in range(len(palette)):
        hit = np.isin(f[:, 0], np.nonzero(part == p)[0]) | np.isin(f[:, 1], np.nonzero(part == p)[0]) | np.isin(f[:, 2], np.nonzero(part == p)[0])
        out[face_off + np.nonzero(hit)[0]] = palette[p]
    return out


def spheres(centre, count, unit, radius):
    """(P * NSV, 3): centre + radius * unit per part, collapsed to the centre where count == 0"""
    c = np.asarray(centre, np.float64)
    return np.concatenate([c[p] + (radius if count[p] else 0.0) * np.asarray(unit, np.float64) for p in range(len(c))])


def look_at(eye, at, up):
    eye, at, up = (np.asarray(a, np.float64) for a in (eye, at, up))
    z = (at - eye) / np.linalg.norm(at - eye)
    x = np.cross(up, z); x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], 1)
    return R, -(eye @ R)


# ---- inputs shared by the fixture script, the host tests and the GPU tests -------------------------------------------------------------------
def place_object(sv, tv, touch, rng):
    """Pose the object template ``tv`` against one frame's SMPL vertices ``sv``: with ``touch`` a random object orientation whose vertex facing the
    body sits 1 cm outside a random SMPL vertex (so a handful of parts are within the 4 cm threshold), else the same pose 2 m away.
    -> obj_angles (3,3) float32 (verts = tv @ obj_angles + obj_trans, render_recon.py:323-324), obj_trans (3,) float32"""
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    a = int(rng.integers(len(sv)))
    d = sv[a].astype(np.float64) - sv.astype(np.float64).mean(0); d /= np.linalg.norm(d)
    rv = tv.astype(np.float64) @ R.T
    k = int(np.argmin(rv @ d))
    t = sv[a] + 0.01 * d - rv[k] + (0.0 if touch else 2.0) * d
    return R.T.astype(np.float32), t.astype(np.float32)


def scene(n, touch, seed=7):
    """n frames: SMPL vertices of synthetic.sequence_params(n, seed) through the CPU oracle, part labels, the object template posed by place_object.
    -> dict smpl (n,6890,3) f32, labels (6890,) i32, obj (n,NVo,3) f32, tv, tf, sp (the sequence parameters), obj_angles (n,3,3), obj_trans (n,3)"""
    from oracle import oracle as O
    from vistracker_amd import synthetic as syn
    model = syn.smplh_model(0)
    sp = syn.sequence_params(n, seed)
    sv = np.asarray(O.SmplModel(model).forward(sp["pose"], sp["betas"], sp["trans"])[0], np.float32)
    tv, tf = syn.object_template()
    rng = np.random.default_rng(seed + 100)
    poses = [place_object(sv[b], tv, bool(touch[b]), rng) for b in range(n)]
    A, t = np.stack([p[0] for p in poses]), np.stack([p[1] for p in poses])
    ov = (np.einsum("vi,nij->nvj", tv, A) + t[:, None]).astype(np.float32)
    return {"smpl": sv, "labels": syn.part_labels(model), "obj": ov, "tv": tv, "tf": tf, "sp": sp, "obj_angles": A, "obj_trans": t, "model": model}


FIXTURE_TOUCH = (True, True, True, False)
FIXTURE_SEED = 8
BATCH_N = 96
BATCH_TOUCH = tuple(b % 2 == 0 for b in range(BATCH_N))      # 48 of 96 frames posed to touch
