"""Test helper (not a test file): the SMPL-H cases tests/test_host_smplh_model.py and tests/test_gpu_smplh_perjoint.py share, and their references -- the float64
model's outputs and gradients (tests/smplh_model.py), the float32 CPU oracle's gradients and its per-row error e32 against the model, which sizes the gate.
A reference is computed once per case and session and handed out read-only."""
import numpy as np

import smplh_model as M

B_SIZES = (1, 6, 7, 16, 17, 96, 97)     # 6 | 7: frames per block of the backward tile kernel; 16 | 17: of the forward vertex kernel; 96 | 97: M block of the blend GEMM
TREES = ("heap3", "chain", "star", "wide11")
SCHEDULED = {"heap3": True, "chain": False, "star": False, "wide11": False}     # does the tree fit the 32 x 10 reverse-chain schedule (else: the serial loop)
CASES = tuple(f"batch{B}" for B in B_SIZES) + ("joint_only", "pose_edges") + tuple(f"tree_{t}" for t in TREES) + ("dense",)
MODES = ("djtr", "none")                # with a random djtr | with no gradient into jtr


def parents_of(tree):
    """52 parents with parents[j] < j (parents[0] = -1 as in the model files)"""
    j = np.arange(52)
    if tree == "heap3":          # ternary heap: 12 schedule steps, at most 9 joints in one
        p = (j - 1) // 3
    elif tree == "chain":        # 51 levels: more steps than the schedule has
        p = j - 1
    elif tree == "star":         # 51 sibling ranks in one level: ditto
        p = np.zeros(52, np.int64)
    elif tree == "wide11":       # joints 1..11 under the root, then j under j - 11: eleven first-ranked joints in level 2, one more than a step holds
        p = np.where(j <= 11, 0, j - 11)
    else:
        raise KeyError(tree)
    p = p.astype(np.int64); p[0] = -1
    return p


def schedule_shape(parents):
    """(steps, widest step) of the reverse-chain schedule vt_smplh_create builds: one step per (tree level, rank among siblings by descending index)"""
    par = [0 if j == 0 else int(parents[j]) for j in range(52)]
    lvl = [0] * 52
    for j in range(1, 52):
        lvl[j] = lvl[par[j]] + 1
    rank = [sum(par[k] == par[j] for k in range(j + 1, 52)) for j in range(52)]
    slots = {}
    for j in range(1, 52):
        slots[(lvl[j], rank[j])] = slots.get((lvl[j], rank[j]), 0) + 1
    return len(slots), max(slots.values())


def _random(B, seed):
    rng = np.random.default_rng(seed)
    f = np.float32
    return {"pose": rng.normal(0, 0.3, (B, 156)).astype(f), "betas": rng.normal(0, 1, (B, 10)).astype(f), "trans": rng.normal(0, 0.3, (B, 3)).astype(f),
            "dverts": rng.normal(0, 1, (B, 6890, 3)).astype(f), "djtr": rng.normal(0, 1, (B, 52, 3)).astype(f)}


def dense_model(base):
    """the model of test_smplh_dense_weights_take_the_dense_lbs: 100 vertices with 52 non-zero weights -> the dense LBS for the whole model"""
    rng = np.random.default_rng(3)
    dense = dict(base)
    W = np.asarray(dense["weights"], np.float32).copy()
    W[:100] = rng.dirichlet(np.ones(52), 100).astype(np.float32)
    dense["weights"] = W
    return dense


def inputs(name, base):
    """-> dict: model, pose, betas, trans, dverts, djtr (float32), modes, zero_joints (the rows of dpose the case makes exactly zero)"""
    modes = MODES
    model = base
    zero_joints = ()
    if name.startswith("batch"):
        B = int(name[5:])
        c = _random(B, 1000 + B)
    elif name == "joint_only":          # every vertex-path partial is zero: dpose, dbetas come from the chain alone
        c = _random(7, 2001)
        c["dverts"][:] = 0
        modes = ("djtr",)
        # a joint without children moves no joint: its rotation has no path to jtr, and with dverts = 0 none to anything -- exactly zero rows of dpose
        zero_joints = tuple(j for j in range(52) if j not in set(int(p) for p in np.asarray(base["parents"])[1:]))
    elif name == "pose_edges":
        c = _random(7, 2002)
        pose = c["pose"].reshape(7, 52, 3)
        axis = np.array([2.0, -1.0, 2.0], np.float32) / 3
        pose[0, 22:] = 0                                    # both hands exactly at rest
        pose[1, 5] = 1e-6                                   # the size of the 1e-8 shift matters
        pose[2, 3] = axis * np.float32(np.pi - 1e-3)        # half angle at pi / 2: quaternion w ~ 0
        pose[3, 16] = axis * np.float32(4.0)                # beyond pi
        pose[4] = 0                                         # the rest pose, root included
        c["betas"][5] = 3
    elif name.startswith("tree_"):
        c = _random(7, 1007)                                # the inputs of batch7
        model = dict(base); model["parents"] = parents_of(name[5:])
    elif name == "dense":
        c = _random(5, 2003)
        model = dense_model(base)
    else:
        raise KeyError(name)
    c["model"] = model; c["modes"] = modes; c["zero_joints"] = zero_joints
    return c


_REF = {}


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, (tuple, list)):
        for y in x:
            _freeze(y)
    elif isinstance(x, dict):
        for y in x.values():
            _freeze(y)
    return x


def reference(name, base):
    """-> dict: inputs (as ``inputs``), fwd = (verts, jtr, v_posed) of the float64 model, and per mode: ref = the model's (dpose, dbetas, dtrans),
    o32 = the float32 oracle's, err32 = its per-row errors, e32 = their maximum, gate = M.GATE * e32"""
    if name in _REF:
        return _REF[name]
    from oracle import oracle as O
    c = inputs(name, base)
    m = M.SmplhModel(c["model"])
    args = (c["pose"], c["betas"], c["trans"])
    cots = [(c["dverts"], c["djtr"] if mode == "djtr" else None) for mode in c["modes"]]
    out = {"inputs": c, "fwd": m.forward(*args)}
    o = O.SmplModel(c["model"])
    for mode, cot, ref in zip(c["modes"], cots, m.backward_many(*args, cots)):
        o32 = o.backward(*args, *cot)
        err32 = M.grad_errs(o32, ref, c["zero_joints"])
        e32 = M.worst(err32)
        out[mode] = {"ref": ref, "o32": o32, "err32": err32, "e32": e32, "gate": M.GATE * e32}
    _REF[name] = _freeze(out)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels' side (needs the GPU): shared by tests/test_gpu_smplh_perjoint.py and tools/smplh_perjoint_report.py
# ---------------------------------------------------------------------------------------------------------------------------------
def cu(x):
    import torch
    return torch.tensor(np.asarray(x)).cuda()               # a copy: the references are handed out read-only


_HANDLES = {}


def handle_of(name, model):
    """one SmplhHandle per distinct model: the base model, each tree, the dense-weights model"""
    key = name if name.startswith("tree_") or name == "dense" else "base"
    if key not in _HANDLES:
        import torch
        from vistracker_amd import ops
        assert torch.cuda.is_available(), "GPU tests need the MI355X box"
        _HANDLES[key] = ops.SmplhHandle(model)
    return _HANDLES[key]


def run_kernels(handle, c, mode):
    """-> (verts, jtr, v_posed), (dpose, dbetas, dtrans) of ops.smplh_forward and its backward, numpy"""
    from vistracker_amd import ops
    p, b, t = (cu(c[k]).requires_grad_(True) for k in ("pose", "betas", "trans"))
    verts, jtr, vposed = ops.smplh_forward(handle, p, b, t)
    loss = (verts * cu(c["dverts"])).sum()
    if mode == "djtr":
        loss = loss + (jtr * cu(c["djtr"])).sum()
    loss.backward()
    return tuple(x.detach().cpu().numpy() for x in (verts, jtr, vposed)), tuple(x.grad.cpu().numpy() for x in (p, b, t))
