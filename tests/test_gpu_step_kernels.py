"""GPU (-m gpu): the fused Adam-step kernels of csrc/step.hip and the single-purpose ones of csrc/misc.hip, each called through the C ABI and compared, buffer by buffer, with the float64 model of
its operation (tests/step_model.py).  Buffers the contract leaves alone start from a sentinel and are compared bit for bit.

Tolerances: the bar test_gpu_parity.py holds the same operation to is the floor (rigid 1e-5 abs / 1e-4 rel on gradients, SO(3) 3e-6 / 2e-4, stencils and
keypoints 1e-5 rel on terms / 1e-4 on gradients, Adam 1e-6 on parameters); above it a kernel gets 4 x e32, e32 being the distance of the MODEL's float32
evaluation from its float64 one on the same inputs (never anything the kernel produced).  Adam's moments have no bar of their own there: m is linear and v
quadratic in the gradient, so they take the gradient's relative bar (twice it for v).  Stepped parameters are compared frame by frame, in absolute
terms, each frame against max(1e-6, 4 x its own e32): the SO(3) inputs put matrices of size 1e-3 and 1e3 into one tensor, and a float32 of size 1e3
cannot be within 1e-6 of anything.  Every comparison prints a PARITY line (pytest -s).
"""
import numpy as np
import pytest

import step_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = np.float32(-7.25e11)         # what an untouched float32 buffer holds
SENT64 = -3.5e101                    # ... and an untouched float64 one
NT, I_ACC, I_VEL, I_TRANS = 8, 1, 2, 4          # terms of an object-stage step: count, and the slots the tail's own workgroups add to
I_PRIOR, I_PINIT = 2, 3                          # ... of a SMPL-stage step
CAM = np.array([979.7844, 979.840, 1018.952, 779.486, 1200.0], np.float32)


@pytest.fixture(scope="module")
def lib():
    from vistracker_amd import _lib as L
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return L


def cu(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).cuda()


def npy(t):
    return t.detach().cpu().numpy()


def P(t, off=0):
    return None if t is None else t.data_ptr() + off


def sent(*shape):
    return torch.full(shape, float(SENT), device="cuda")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def untouched(a):
    return same_bits(a, np.full(a.shape, SENT if a.dtype == np.float32 else SENT64, a.dtype))


def metric(kind, a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    if kind == "abs":
        return float(np.abs(a - b).max())
    if kind == "rel":
        return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))
    if kind == "relrow":                              # per frame: frames of very different scale share a tensor
        a = a.reshape(a.shape[0], -1); b = b.reshape(b.shape[0], -1)
        return float((np.abs(a - b).max(1) / (np.abs(b).max(1) + 1e-300)).max())
    raise ValueError(kind)


def check(op, shape, name, kind, got, ref64, ref32, floor):
    err, e32 = metric(kind, got, ref64), metric(kind, ref32, ref64)
    bar = max(floor, 4 * e32)
    print(f"PARITY {op} {shape} {name} [{kind}] e32={e32:.3e} err={err:.3e} bar={bar:.3e} err/bar={err / bar:.3f}")
    assert np.isfinite(err) and err <= bar, (op, shape, name, err, e32, bar)


def check_rows(op, shape, name, got, ref64, ref32, floor):
    """absolute error per frame, every frame against max(floor, 4 x the frame's own e32)"""
    B = np.asarray(ref64).shape[0]
    err = np.abs(np.asarray(got, np.float64).reshape(B, -1) - np.asarray(ref64, np.float64).reshape(B, -1)).max(1)
    e32 = np.abs(np.asarray(ref32, np.float64).reshape(B, -1) - np.asarray(ref64, np.float64).reshape(B, -1)).max(1)
    bar = np.maximum(floor, 4 * e32)
    b = int(np.argmax(err / bar))
    print(f"PARITY {op} {shape} {name} [abs per frame, worst frame {b}] e32={e32[b]:.3e} err={err[b]:.3e} bar={bar[b]:.3e} err/bar={err[b] / bar[b]:.3f}")
    assert np.isfinite(err).all() and (err <= bar).all(), (op, shape, name, b, err[b], e32[b], bar[b])


def exact_loss(hist, terms, w):
    """the closed loss against the terms read back after the launch: the same fp64 operations on the same values"""
    fused, plain = M.weighted_loss(terms, w)
    return same_bits(np.float32(hist), fused) or same_bits(np.float32(hist), plain)


# =====================================================================================================================================
# vt_objstep_head
# =====================================================================================================================================
def head_case(seed, so3_seed, B, N, NV):
    rng = np.random.default_rng(seed)
    assert so3_seed in M.SO3_SEEDS and B in M.SO3_BATCHES            # the pairs whose conditions tests/test_host_step_model.py asserts
    M0, noise, kinds, rejected = M.so3_inputs(so3_seed, B)
    assert rejected <= M.SO3_MAX_REJECT, (so3_seed, B, rejected)
    c = {"M0": M0, "noise": noise, "kinds": kinds, "t": (rng.normal(0, 0.5, (B, 3)) + [0, 0, 2.2]).astype(np.float32),
         "s": rng.uniform(0.8, 1.2, B).astype(np.float32), "X0_points": rng.normal(0, 0.3, (N, 3)).astype(np.float32), "B": B, "N": N, "NV": NV}
    c["X0_verts"] = rng.normal(0, 0.3, (NV, 3)).astype(np.float32) if NV else None
    return c


def run_head(L, c, nzero=7, noise=True, svd=True, terms=True, verts=True):
    B, N, NV = c["B"], c["N"], c["NV"]
    d = {"M0": cu(c["M0"]), "noise": cu(c["noise"]) if noise else None, "t": cu(c["t"]), "s": cu(c["s"]), "X0p": cu(c["X0_points"]),
         "X0v": cu(c["X0_verts"]) if NV else None, "X": sent(B, N, 3), "Xv": sent(B, max(NV, 1), 3), "R": sent(B, 9), "svd": sent(B, 22),
         "terms": torch.full((16,), SENT64, dtype=torch.float64, device="cuda")}
    use_v = bool(NV) and verts
    L.check(L.lib().vt_objstep_head(P(d["M0"]), P(d["noise"]), P(d["t"]), P(d["s"]), B, P(d["X0p"]), N, P(d["X"]), P(d["X0v"]) if use_v else None, NV if use_v else 0,
                                    P(d["Xv"]) if use_v else None, P(d["R"]), P(d["terms"]) if terms else None, nzero, P(d["svd"]) if svd else None, L.stream_ptr()))
    torch.cuda.synchronize()
    return {k: npy(d[k]) for k in ("X", "Xv", "R", "svd", "terms")}, d


HEAD_SHAPES = [(96, 3000, 2502), (97, 257, 1), (1, 1, 0), (3, 255, 0), (4, 256, 2502), (5, 1023, 1), (4, 1024, 0), (3, 1025, 1)]


@pytest.mark.parametrize("B,N,NV", HEAD_SHAPES)
def test_objstep_head_vs_model(lib, B, N, NV):
    shape = (B, N, NV)
    c = head_case(100 + B + N, M.SO3_SEEDS[0], B, N, NV)
    out, _ = run_head(lib, c, nzero=7)
    ref, r32 = M.objstep_head(c), M.objstep_head(c, fp32=True)
    check("head", shape, "R", "abs", out["R"].reshape(B, 3, 3), ref["R"], r32["R"], 3e-6)
    check("head", shape, "X_points", "abs", out["X"], ref["X_points"], r32["X_points"], 1e-5)
    if NV:
        check("head", shape, "X_verts", "abs", out["Xv"], ref["X_verts"], r32["X_verts"], 1e-5)
    else:
        assert untouched(out["Xv"])
    R = out["R"].reshape(B, 3, 3).astype(np.float64)
    assert np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max() < 3e-6 and np.abs(np.linalg.det(R) - 1).max() < 3e-6
    # the hand-over rows: U diag(s) V^T is the projected matrix, d = +-1 and the sign of the model's
    ws = out["svd"].astype(np.float64)
    U, V, s, dd = ws[:, :9].reshape(B, 3, 3), ws[:, 9:18].reshape(B, 3, 3), ws[:, 18:21], ws[:, 21]
    Min = M.so3_input(c["M0"], c["noise"])
    rec = (U * s[:, None, :]) @ np.swapaxes(V, 1, 2)
    assert metric("relrow", rec, Min) < 3e-6, metric("relrow", rec, Min)
    assert np.abs(np.abs(dd) - 1).max() < 3e-6 and np.array_equal(np.sign(dd), ref["svd"]["d"])
    assert (s[:, 0] >= s[:, 1]).all() and (s[:, 1] >= s[:, 2]).all()
    assert (out["terms"][:7] == 0).all() and untouched(out["terms"][7:])


@pytest.mark.parametrize("nzero", [0, 1, 7, 16])
def test_objstep_head_zeroes_exactly_nzero_terms(lib, nzero):
    c = head_case(7, M.SO3_SEEDS[1], 4, 300, 0)
    out, _ = run_head(lib, c, nzero=nzero)
    assert (out["terms"][:nzero] == 0).all() and untouched(out["terms"][nzero:])


def test_objstep_head_optional_arguments(lib):
    c = head_case(8, M.SO3_SEEDS[1], 5, 700, 33)
    full, _ = run_head(lib, c)
    for off in ("noise", "svd", "terms", "verts"):
        out, _ = run_head(lib, c, **{off: False})
        if off == "noise":
            c0 = dict(c, noise=None)
            ref, r32 = M.objstep_head(c0), M.objstep_head(c0, fp32=True)
            check("head", "no-noise", "R", "abs", out["R"].reshape(5, 3, 3), ref["R"], r32["R"], 3e-6)
            check("head", "no-noise", "X_points", "abs", out["X"], ref["X_points"], r32["X_points"], 1e-5)
            continue
        assert same_bits(out["R"], full["R"]) and same_bits(out["X"], full["X"])
        assert untouched(out["svd"]) if off == "svd" else same_bits(out["svd"], full["svd"])
        assert untouched(out["terms"]) if off == "terms" else same_bits(out["terms"], full["terms"])
        assert untouched(out["Xv"]) if off == "verts" else same_bits(out["Xv"], full["Xv"])


# =====================================================================================================================================
# vt_objstep_tail / vt_objstep_tail_temporal
# =====================================================================================================================================
LR = {"object": (0.002, 0.006), "sil": (0.006, 0.006), "joint": (0.0, 0.002), "plain": (0.002, 0.006)}


def tail_case(seed, so3_seed, B, N, NV, form, adam_step=1, nzero=0, armed=0, prev=np.inf, tol=1e-4, stop0=0):
    """form: 'object' (temporal tail, dX accumulated), 'sil' (temporal tail, init_zero, vertex pass, translation regulariser, dX_points = NaN),
    'joint' (plain tail, no rotation group), 'plain' (plain tail, both groups)"""
    rng = np.random.default_rng(seed)
    c = head_case(seed + 1, so3_seed, B, N, NV if form == "sil" else 0)
    c.update(form=form, adam_step=adam_step, nzero=nzero, armed=armed, prev=np.float32(prev), tol=tol, stop0=stop0, slot=3,
             rot=form != "joint", trans=True, lrR=LR[form][0], lrT=LR[form][1], w_trans=2.5)
    c["dX_points"] = (rng.normal(0, 1, (B, N, 3)) / np.sqrt(N)).astype(np.float32)
    if form in ("object", "sil"):
        X = M.objstep_head(c)["X_points"].astype(np.float32)
        c["temporal"] = {"X": X, "w_accel": 1.5, "w_velocity": 0.75, "init_zero": int(form == "sil")}
    if form == "sil":
        c["dX_verts"] = (rng.normal(0, 1, (B, NV, 3)) / np.sqrt(NV)).astype(np.float32)
        c["t_init"] = (c["t"] + rng.normal(0, 0.05, (B, 3))).astype(np.float32)
    # starting moments of the size of the gradients the model computes for this case
    probe = M.objstep_tail(dict(c, mR=np.ones((B, 9)), vR=np.ones((B, 9)), mT=np.ones((B, 3)), vT=np.ones((B, 3))))
    c["mT"], c["vT"] = M.adam_moments(rng, probe["dt"])
    if c["rot"]:
        c["mR"], c["vR"] = M.adam_moments(rng, probe["dM"])
    c["terms_in"] = rng.uniform(0.1, 2.0, NT)
    c["w"] = rng.uniform(0.5, 2.0, NT).astype(np.float32)
    return c


def tail_buffers(c):
    B, N, NV = c["B"], c["N"], c["NV"]
    dXp = c["dX_points"] if c["form"] != "sil" else np.full((B, N, 3), np.nan, np.float32)        # phase 'sil': must not be read
    d = {"X0v": cu(c.get("X0_verts")), "dXv": cu(c.get("dX_verts")), "X0p": cu(c["X0_points"]), "dXp": cu(dXp), "s": cu(c["s"]), "M0": cu(c["M0"].reshape(B, 9)),
         "noise": cu(c["noise"]), "t": cu(c["t"]), "t_init": cu(c.get("t_init")), "dR": sent(B, 9), "dt": sent(B, 3), "dM": sent(B, 9),
         "mR": cu(c["mR"]) if c["rot"] else sent(B, 9), "vR": cu(c["vR"]) if c["rot"] else sent(B, 9), "mT": cu(c["mT"]), "vT": cu(c["vT"]),
         "terms": cu(c["terms_in"]), "state": cu(np.array([c["prev"], SENT, SENT, SENT], np.float32)), "stop": cu(np.array([c["stop0"]], np.int32)),
         "hist": sent(8), "ticket": torch.zeros(1, dtype=torch.int32, device="cuda"), "X": cu(c["temporal"]["X"]) if "temporal" in c else None}
    return d


def launch_tail(L, c, d, svd_ws=None, ticket=None):
    B, N, NV = c["B"], c["N"], c["NV"]
    tp = lambda i: P(d["terms"], 8 * i)
    pre, fn = (), L.lib().vt_objstep_tail
    if "temporal" in c:
        tm = c["temporal"]
        pre, fn = (P(d["X"]), tm["w_accel"], tp(I_ACC), tm["w_velocity"], tp(I_VEL), tm["init_zero"]), L.lib().vt_objstep_tail_temporal
    rot = (P(d["M0"]), P(d["mR"]), P(d["vR"]), c["lrR"]) if c["rot"] else (None, None, None, 0.0)
    return fn(*pre, P(d["X0v"]), NV, P(d["dXv"]), P(d["X0p"]), N, P(d["dXp"]), P(d["s"]), B, P(d["M0"]), P(d["noise"]), P(d["t"]), P(d["t_init"]), c["w_trans"], tp(I_TRANS),
              P(d["dR"]), P(d["dt"]), P(d["dM"]), *rot, P(d["t"]), P(d["mT"]), P(d["vT"]), c["lrT"], c["adam_step"], 0.9, 0.999, 1e-8,
              P(d["terms"]), c["w"].ctypes.data, c.get("nterms", NT), c["tol"], c["armed"], P(d["state"]), P(d["stop"]), P(d["hist"]), c["slot"],
              P(ticket if ticket is not None else d["ticket"]), c["nzero"], P(svd_ws), L.stream_ptr())


def run_tail(L, c, svd_ws=None):
    d = tail_buffers(c)
    L.check(launch_tail(L, c, d, svd_ws))
    torch.cuda.synchronize()
    return {k: npy(v) for k, v in d.items() if v is not None}


def check_close(c, out, want):
    """what closing a step leaves: ticket back at zero, one history slot, state[0:2], the stop flag -- or, on the stopped branch, NaN and nothing else"""
    assert int(out["ticket"][0]) == 0
    hist, stopped = out["hist"], bool(c["stop0"])
    assert untouched(np.delete(hist, c["slot"])) and untouched(out["state"][2:])
    if stopped:
        assert np.isnan(hist[c["slot"]]) and same_bits(out["state"][:1], np.array([c["prev"]], np.float32)) and untouched(out["state"][1:2]) and int(out["stop"][0]) == 1
        return
    if c["nzero"] == 0:
        assert exact_loss(hist[c["slot"]], out["terms"], c["w"]), (hist[c["slot"]], M.weighted_loss(out["terms"], c["w"]), out["terms"].tolist())
    loss_m, stop_m, ratio = M.close_step(want, c["w"], c["prev"], c["tol"], c["armed"])
    assert abs(float(hist[c["slot"]]) - float(loss_m)) <= 1e-5 * abs(float(loss_m)), (hist[c["slot"]], loss_m)
    assert same_bits(out["state"][0], hist[c["slot"]]) and same_bits(out["state"][1], hist[c["slot"]])
    if c["armed"] and np.isfinite(c["prev"]):
        assert abs(ratio - 1) >= 0.01, ratio                      # a condition on the inputs: the decision is not within rounding of the threshold
    assert int(out["stop"][0]) == int(stop_m), (out["stop"], stop_m, ratio)


def check_tail(c, out, tag):
    B, shape = c["B"], (tag, c["B"], c["N"], c["NV"], c["form"], "step", c["adam_step"])
    ref, r32 = M.objstep_tail(c), M.objstep_tail(c, fp32=True)
    stopped = bool(c["stop0"])
    check("tail", shape, "dt", "rel", out["dt"], ref["dt"], r32["dt"], 1e-4)
    if c["rot"]:
        check("tail", shape, "dR", "relrow", out["dR"], ref["dR"], r32["dR"], 1e-4)
        check("tail", shape, "dM", "relrow", out["dM"], ref["dM"], r32["dM"], 2e-4)
    else:
        assert untouched(out["dR"]) and untouched(out["dM"]) and untouched(out["mR"]) and untouched(out["vR"]) and same_bits(out["M0"], c["M0"].reshape(B, 9))
    groups = [("T", "t", 1e-4)] + ([("R", "M0", 2e-4)] if c["rot"] else [])
    for g, pbuf, gbar in groups:
        if stopped:
            assert same_bits(out[pbuf], (c["t"] if g == "T" else c["M0"]).reshape(out[pbuf].shape)) and same_bits(out["m" + g], c["m" + g]) and same_bits(out["v" + g], c["v" + g])
            continue
        check_rows("tail", shape, "p" + g, out[pbuf], ref["p" + g], r32["p" + g], 1e-6)
        check("tail", shape, "m" + g, "rel", out["m" + g], ref["m" + g], r32["m" + g], gbar)
        check("tail", shape, "v" + g, "rel", out["v" + g], ref["v" + g], r32["v" + g], 2 * gbar)
    # terms: the tail's own workgroups add to three of them; with nzero = 0 they survive the launch
    want = c["terms_in"].copy()
    for name, idx in (("term_accel", I_ACC), ("term_velocity", I_VEL), ("term_trans", I_TRANS)):
        if name in ref:
            want[idx] += ref[name]
            if idx >= c["nzero"]:
                add = out["terms"][idx] - c["terms_in"][idx]
                check("tail", shape, name, "rel", add, ref[name], float(r32[name]), 1e-5)
        elif idx >= c["nzero"]:
            assert out["terms"][idx] == c["terms_in"][idx]
    for k in range(NT):
        if k < c["nzero"]:
            assert out["terms"][k] == 0.0, (k, out["terms"][k])
        elif k not in (I_ACC, I_VEL, I_TRANS):
            assert out["terms"][k] == c["terms_in"][k]
    check_close(c, out, want)

TAIL_CASES = [  # (B, N, NV, form, adam_step, nzero)
    (96, 3000, 2502, "object", 1, 0), (96, 3000, 2502, "sil", 2, 7), (96, 3000, 2502, "sil", 1, 0), (96, 3000, 2502, "joint", 1000, 0), (96, 3000, 2502, "plain", 1, 0),
    (97, 257, 1, "object", 2, 7), (97, 257, 1, "sil", 1, 0), (97, 257, 1, "joint", 1, 7), (97, 257, 1, "plain", 1000, 3),
    (3, 255, 1, "sil", 1, 0), (4, 256, 2502, "sil", 1000, 0), (5, 1023, 1, "object", 1, 0), (3, 1024, 0, "object", 2, 0), (4, 1025, 0, "object", 1, 6),
    (5, 1, 1, "sil", 1, 0), (1, 255, 0, "plain", 1, 0), (1, 1, 0, "joint", 2, 0), (3, 3000, 0, "plain", 2, 0),
]


@pytest.mark.parametrize("B,N,NV,form,adam_step,nzero", TAIL_CASES)
def test_objstep_tails_vs_model(lib, B, N, NV, form, adam_step, nzero):
    c = tail_case(1000 + 7 * B + N + adam_step, M.SO3_SEEDS[2 + (B + N) % 3], B, N, NV, form, adam_step=adam_step, nzero=nzero)
    check_tail(c, run_tail(lib, c), "tail")


@pytest.mark.parametrize("B,N,form", [(96, 3000, "plain"), (97, 257, "object"), (5, 700, "sil")])
def test_objstep_tail_svd_handover_is_bit_identical(lib, B, N, form):
    """the tail with the head's decomposition (svd_ws of a head call on the same M0 / noise) and the tail that decomposes the matrix itself"""
    c = tail_case(50 + B, M.SO3_SEEDS[5], B, N, 9, form)
    _, hd = run_head(lib, c)
    a, b = run_tail(lib, c, svd_ws=None), run_tail(lib, c, svd_ws=hd["svd"])
    for k in a:
        if k in ("terms", "hist", "state"):          # the frames' fp64 shares reach a term in whatever order the workgroups finish: last bits only
            assert np.allclose(a[k], b[k], rtol=2e-6, atol=0, equal_nan=True), k
        else:
            assert same_bits(a[k], b[k]), k
    check_tail(c, b, "tail+svd_ws")


def _prev_for(c, ratio_target):
    """prev such that abs(prev - loss) / prev = ratio_target * prev * tol in the model: solve p - loss = r tol p^2 for the root next to loss"""
    want = c["terms_in"].copy()
    ref = M.objstep_tail(c) if "pose" not in c else M.smplstep_tail(c)
    for name, idx in c["own_terms"]:
        if name in ref:
            want[idx] += ref[name]
    loss = float(M.weighted_loss(want, c["w"])[1])
    a = ratio_target * c["tol"]
    assert 4 * a * loss < 0.5, (a, loss)
    return (1 - np.sqrt(1 - 4 * a * loss)) / (2 * a)


OBJ_OWN = (("term_accel", I_ACC), ("term_velocity", I_VEL), ("term_trans", I_TRANS))


@pytest.mark.parametrize("form", ["object", "sil", "joint"])
def test_objstep_tail_stop_rule(lib, form):
    B, N, NV = 5, 300, 40
    base = dict(seed=77, so3_seed=M.SO3_SEEDS[6], B=B, N=N, NV=NV, form=form, tol=1e-4)
    c0 = tail_case(**base); c0["own_terms"] = OBJ_OWN
    for ratio, armed, expect in ((0.9, 1, 1), (1.1, 1, 0), (0.5, 0, 0)):
        c = tail_case(**base, armed=armed, prev=_prev_for(c0, ratio))
        out = run_tail(lib, c)
        check_tail(c, out, f"stop r={ratio} armed={armed}")
        assert int(out["stop"][0]) == expect
    c = tail_case(**base, armed=1, prev=np.inf)
    out = run_tail(lib, c); check_tail(c, out, "stop prev=inf")
    assert int(out["stop"][0]) == 0
    for nzero in (0, 6):                                            # flag already set on entry
        c = tail_case(**base, armed=1, prev=1.25, stop0=1, nzero=nzero)
        check_tail(c, run_tail(lib, c), f"stopped nzero={nzero}")


# =====================================================================================================================================
# closing a step: the loss the last workgroup computes against the terms it must have seen complete
# =====================================================================================================================================
def test_step_end_loss_is_exact_over_282_object_steps(lib):
    """282 consecutive launches of the temporal tail in its 'sil' form -- vertex pass, stencils, translation regulariser: its workgroups add to all THREE of
    the tail's terms, the regulariser's atomic being the last one a workgroup issues before it takes its ticket -- on one stream, new inputs for each launch,
    B = 96 / 4 / 97 sharing one ticket: history[slot] must be float32(sum_k float64(w_k) terms_k) of the terms read back, to the bit -- any difference is a
    term read before it was complete"""
    L = lib
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    cases = {B: tail_case(300 + B, M.SO3_SEEDS[7], B, 3000 if B != 4 else 600, 2502 if B != 4 else 40, "sil") for B in (96, 4, 97)}
    bufs = {B: tail_buffers(c) for B, c in cases.items()}
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    for k in range(282):
        B = (96, 4, 97)[k % 3] if k < 30 else (96, 97)[k % 2]
        c, d = cases[B], bufs[B]
        d["dXv"].normal_(generator=gen); d["X"].normal_(generator=gen); d["t_init"].normal_(generator=gen)
        tin = torch.rand(NT, dtype=torch.float64, device="cuda", generator=gen) + 0.1
        d["terms"].copy_(tin)
        L.check(launch_tail(L, c, d, ticket=ticket))
        torch.cuda.synchronize()
        terms, hist, tin = npy(d["terms"]), npy(d["hist"]), npy(tin)
        assert int(ticket.item()) == 0, k
        moved = [i for i in range(NT) if terms[i] != tin[i]]
        assert moved == [I_ACC, I_VEL, I_TRANS], (k, moved)
        assert exact_loss(hist[c["slot"]], terms, c["w"]), (k, B, hist[c["slot"]], M.weighted_loss(terms, c["w"]), terms.tolist(), tin.tolist())


# =====================================================================================================================================
# vt_smplstep_tail
# =====================================================================================================================================
SMPL_LAYOUTS = {   # AdamState.smpl_tail_groups: (name, columns, lr) per group, unused groups NULL
    "smplt-global": (("trans", 3, 0.01), ("pose", 3, 0.01), ("betas", 2, 0.01)),
    "smplt-all": (("trans", 3, 0.004), ("pose", 66, 0.004), ("betas", 10, 0.004)),
    "smpl-global": (("betas", 2, 0.02), ("trans", 3, 0.02)),
    "smpl-all": (("trans", 3, 0.006), ("pose", 66, 0.006), ("betas", 10, 0.006)),
}
WIDTH = {"trans": 3, "pose": 156, "betas": 10}


def smpl_case(seed, B, layout, synth, adam_step=1, nzero=0, armed=0, prev=np.inf, tol=1e-3, stop0=0):
    rng = np.random.default_rng(seed)
    c = {"B": B, "layout": layout, "adam_step": adam_step, "nzero": nzero, "armed": armed, "prev": np.float32(prev), "tol": tol, "stop0": stop0, "slot": 5,
         "pose": rng.normal(0, 0.3, (B, 156)).astype(np.float32), "mean": synth["priors"]["body_mean"], "prec": synth["priors"]["body_prec"],
         "gscale_prior": 0.8 / B, "w_pinit": 1.7, "dpose": rng.normal(0, 1, (B, 156)).astype(np.float32),
         "trans": rng.normal(0, 1, (B, 3)).astype(np.float32), "dtrans": rng.normal(0, 1, (B, 3)).astype(np.float32),
         "betas": rng.normal(0, 1, (B, 10)).astype(np.float32), "dbetas": rng.normal(0, 1, (B, 10)).astype(np.float32)}
    c["pose_init"] = (c["pose"] + rng.normal(0, 0.1, (B, 156))).astype(np.float32)
    probe = M.smplstep_tail(dict(c, groups=[]))["dpose"]
    c["groups"] = []
    for name, n, lr in SMPL_LAYOUTS[layout]:
        g = probe if name == "pose" else c["d" + name]
        m, v = M.adam_moments(rng, g[:, :n])
        c["groups"].append({"name": name, "p": c[name], "g": g, "m": m, "v": v, "ncols": n, "lr": lr})
    c["terms_in"] = rng.uniform(0.1, 2.0, NT); c["w"] = rng.uniform(0.5, 2.0, NT).astype(np.float32)
    c["own_terms"] = (("term_prior", I_PRIOR), ("term_pinit", I_PINIT))
    return c


def smpl_buffers(c, synth):
    d = {k: cu(c[k]) for k in ("pose", "pose_init", "dpose", "trans", "dtrans", "betas", "dbetas")}
    d.update(mean=cu(c["mean"]), prec=cu(c["prec"]), terms=cu(c["terms_in"]), state=cu(np.array([c["prev"], SENT, SENT, SENT], np.float32)),
             stop=cu(np.array([c["stop0"]], np.int32)), hist=sent(8), ticket=torch.zeros(1, dtype=torch.int32, device="cuda"))
    for i, g in enumerate(c["groups"]):
        d[f"m{i}"], d[f"v{i}"] = cu(g["m"]), cu(g["v"])
    return d


def launch_smpl(L, c, d, ticket=None):
    groups = ()
    for i, g in enumerate(c["groups"]):
        groups += (P(d[g["name"]]), WIDTH[g["name"]], P(d["d" + g["name"]]), WIDTH[g["name"]], P(d[f"m{i}"]), P(d[f"v{i}"]), g["ncols"], g["lr"])
    groups += (None, 0, None, 0, None, None, 0, 0.0) * (3 - len(c["groups"]))
    return L.lib().vt_smplstep_tail(P(d["pose"]), P(d["pose_init"]), P(d["dpose"]), c["B"], P(d["mean"]), P(d["prec"]), c["gscale_prior"], P(d["terms"], 8 * I_PRIOR),
                                    c["w_pinit"], P(d["terms"], 8 * I_PINIT), *groups, c["adam_step"], 0.9, 0.999, 1e-8, P(d["terms"]), c["w"].ctypes.data, c.get("nterms", NT),
                                    c["tol"], c["armed"], P(d["state"]), P(d["stop"]), P(d["hist"]), c["slot"], P(ticket if ticket is not None else d["ticket"]), c["nzero"],
                                    L.stream_ptr())


def check_smpl(c, out, tag):
    B, shape = c["B"], (tag, c["B"], c["layout"], "step", c["adam_step"])
    ref, r32 = M.smplstep_tail(c), M.smplstep_tail(c, fp32=True)
    stopped = bool(c["stop0"])
    check("smpltail", shape, "dpose", "rel", out["dpose"][:, 3:72], ref["dpose"][:, 3:72], r32["dpose"][:, 3:72], 1e-4)
    assert same_bits(out["dpose"][:, :3], c["dpose"][:, :3]) and same_bits(out["dpose"][:, 72:], c["dpose"][:, 72:])
    for i, g in enumerate(c["groups"]):
        n, name = g["ncols"], g["name"]
        assert same_bits(out[name][:, n:], c[name][:, n:]), name                   # columns outside the slice keep their bits
        if stopped:
            assert same_bits(out[name], c[name]) and same_bits(out[f"m{i}"], g["m"]) and same_bits(out[f"v{i}"], g["v"])
            continue
        check_rows("smpltail", shape, f"p[{name}:{n}]", out[name][:, :n], ref["groups"][i][0], r32["groups"][i][0], 1e-6)
        check("smpltail", shape, f"m[{name}:{n}]", "rel", out[f"m{i}"], ref["groups"][i][1], r32["groups"][i][1], 1e-4)
        check("smpltail", shape, f"v[{name}:{n}]", "rel", out[f"v{i}"], ref["groups"][i][2], r32["groups"][i][2], 2e-4)
    for name in ("trans", "betas", "pose"):
        if name not in [g["name"] for g in c["groups"]]:
            assert same_bits(out[name], c[name]), name
    want = c["terms_in"].copy()
    for name, idx in c["own_terms"]:
        want[idx] += ref[name]
        if idx >= c["nzero"]:
            check("smpltail", shape, name, "rel", out["terms"][idx] - c["terms_in"][idx], ref[name], float(r32[name]), 1e-5)
    for k in range(NT):
        if k < c["nzero"]:
            assert out["terms"][k] == 0.0
        elif k not in (I_PRIOR, I_PINIT):
            assert out["terms"][k] == c["terms_in"][k]
    check_close(c, out, want)

def run_smpl(L, c, synth):
    d = smpl_buffers(c, synth)
    L.check(launch_smpl(L, c, d))
    torch.cuda.synchronize()
    return {k: npy(v) for k, v in d.items()}


@pytest.mark.parametrize("B,layout,adam_step,nzero", [(1, "smpl-global", 1, 0), (2, "smplt-global", 2, 6), (3, "smplt-all", 1000, 0), (96, "smpl-all", 1, 0),
                                                      (97, "smpl-all", 2, 6), (96, "smpl-global", 1000, 6), (97, "smplt-global", 1, 0)])
def test_smplstep_tail_vs_model(lib, synth, B, layout, adam_step, nzero):
    c = smpl_case(2000 + B + adam_step, B, layout, synth, adam_step=adam_step, nzero=nzero)
    check_smpl(c, run_smpl(lib, c, synth), "smpltail")


def test_smplstep_tail_stop_rule(lib, synth):
    base = dict(seed=78, B=5, layout="smpl-all", synth=synth, tol=1e-6)      # (the prior term is ~1e3: with the fits' 1e-3 every step would stop)
    c0 = smpl_case(**base)
    for ratio, armed, expect in ((0.9, 1, 1), (1.1, 1, 0), (0.5, 0, 0)):
        c = smpl_case(**base, armed=armed, prev=_prev_for(c0, ratio))
        out = run_smpl(lib, c, synth); check_smpl(c, out, f"stop r={ratio} armed={armed}")
        assert int(out["stop"][0]) == expect
    c = smpl_case(**base, armed=1, prev=np.inf)
    out = run_smpl(lib, c, synth); check_smpl(c, out, "stop prev=inf")
    assert int(out["stop"][0]) == 0
    for nzero in (0, 6):
        c = smpl_case(**base, armed=1, prev=1.25, stop0=1, nzero=nzero)
        check_smpl(c, run_smpl(lib, c, synth), f"stopped nzero={nzero}")


def test_step_end_loss_is_exact_over_282_smpl_steps(lib, synth):
    """as test_step_end_loss_is_exact_over_282_object_steps, for the 64-thread SMPL tail (two terms from its own workgroups)"""
    L = lib
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    cases = {B: smpl_case(400 + B, B, "smpl-all", synth) for B in (96, 4, 97)}
    bufs = {B: smpl_buffers(c, synth) for B, c in cases.items()}
    gen = torch.Generator(device="cuda"); gen.manual_seed(6)
    for k in range(282):
        B = (96, 4, 97)[k % 3] if k < 30 else (96, 97)[k % 2]
        c, d = cases[B], bufs[B]
        d["pose"].normal_(0, 0.3, generator=gen); d["dpose"].normal_(generator=gen)
        tin = torch.rand(NT, dtype=torch.float64, device="cuda", generator=gen) + 0.1
        d["terms"].copy_(tin)
        L.check(launch_smpl(L, c, d, ticket=ticket))
        torch.cuda.synchronize()
        terms, hist = npy(d["terms"]), npy(d["hist"])
        assert int(ticket.item()) == 0, k
        assert [i for i in range(NT) if terms[i] != npy(tin)[i]] == [I_PRIOR, I_PINIT], k
        assert exact_loss(hist[c["slot"]], terms, c["w"]), (k, B, hist[c["slot"]], M.weighted_loss(terms, c["w"]), terms.tolist())


# =====================================================================================================================================
# vt_loss_reduce_and_stop
# =====================================================================================================================================
def test_loss_reduce_and_stop(lib):
    L = lib; rng = np.random.default_rng(9)
    terms = rng.uniform(0.1, 2, NT); w = rng.uniform(0.5, 2, NT).astype(np.float32); tol = 1e-3
    loss = float(M.weighted_loss(terms, w)[1])
    prev_of = lambda r: (1 - np.sqrt(1 - 4 * r * tol * loss)) / (2 * r * tol)
    for prev, armed, stop0 in ((prev_of(0.9), 1, 0), (prev_of(1.1), 1, 0), (prev_of(0.5), 0, 0), (np.inf, 1, 0), (1.25, 1, 1)):
        t, st, fl, hist = cu(terms), cu(np.array([prev, SENT, SENT], np.float32)), cu(np.array([stop0], np.int32)), sent(6)
        L.check(L.lib().vt_loss_reduce_and_stop(P(t), w.ctypes.data, NT, tol, armed, P(st), P(fl), P(hist), 2, L.stream_ptr()))
        torch.cuda.synchronize()
        h, s = npy(hist), npy(st)
        assert untouched(np.delete(h, 2)) and untouched(s[2:]) and same_bits(npy(t), terms)
        if stop0:
            assert np.isnan(h[2]) and same_bits(s[:1], np.array([prev], np.float32)) and untouched(s[1:2]) and int(fl.item()) == 1
            continue
        loss_m, stop_m, ratio = M.close_step(terms, w, prev, tol, armed)
        assert exact_loss(h[2], terms, w) and same_bits(s[0], h[2]) and same_bits(s[1], h[2])
        assert not (armed and np.isfinite(prev)) or abs(ratio - 1) >= 0.01
        assert int(fl.item()) == int(stop_m), (prev, armed, ratio)


# =====================================================================================================================================
# temporal stencils, Adam on strided slices, small utilities
# =====================================================================================================================================
@pytest.mark.parametrize("B,D", [(3, 3), (4, 257), (5, 9000), (96, 9000), (96, 257), (3, 9000)])
@pytest.mark.parametrize("init_zero", [0, 1])
def test_temporal_loss2_vs_model(lib, B, D, init_zero):
    L = lib; rng = np.random.default_rng(B * D + init_zero)
    v = rng.normal(0, 1, (B, D)).astype(np.float32); dv0 = rng.normal(0, 1, (B, D)).astype(np.float32)
    wa, wv = 1.5, 0.75
    vt, dv = cu(v), cu(dv0 if not init_zero else np.full((B, D), np.nan, np.float32)); terms = cu(np.array([0.25, 0.5, SENT64]))
    L.check(L.lib().vt_temporal_loss2(P(vt), B, D, wa, P(terms), wv, P(terms, 8), P(dv), init_zero, L.stream_ptr()))
    torch.cuda.synchronize()
    res = {}
    for q in (False, True):
        ta, ga = M.accel_term(v, wa, None, q); tv, gv = M.velocity_term(v, wv, q)
        res[q] = (ta, tv, (0 if init_zero else dv0.astype(ga.dtype)) + ga + gv)
    t = npy(terms)
    check("temporal2", (B, D, init_zero), "term_accel", "rel", t[0] - 0.25, res[False][0], float(res[True][0]), 1e-5)
    check("temporal2", (B, D, init_zero), "term_velocity", "rel", t[1] - 0.5, res[False][1], float(res[True][1]), 1e-5)
    check("temporal2", (B, D, init_zero), "dv", "rel", npy(dv), res[False][2], res[True][2], 1e-4)
    assert t[2] == SENT64


@pytest.mark.parametrize("B,D,stride", [(3, 3, 5), (4, 257, 300), (5, 9000, 9003), (96, 257, 257)])
def test_accel_loss_strided_vs_model(lib, B, D, stride):
    L = lib; rng = np.random.default_rng(B + D)
    v = np.full((B, stride), SENT, np.float32); v[:, :D] = rng.normal(0, 1, (B, D))
    dv0 = np.full((B, stride), SENT, np.float32); dv0[:, :D] = rng.normal(0, 1, (B, D))
    for ew in (None, rng.uniform(1, 10, D).astype(np.float32)):
        vt, dv, term, ewt = cu(v), cu(dv0), cu(np.array([0.25, SENT64])), cu(ew)
        L.check(L.lib().vt_accel_loss_strided(P(vt), B, D, stride, P(ewt), 0.7, P(term), P(dv), L.stream_ptr()))
        torch.cuda.synchronize()
        (t64, g64), (t32, g32) = M.accel_term(v[:, :D], 0.7, ew), M.accel_term(v[:, :D], 0.7, ew, True)
        check("accel_strided", (B, D, stride), "term", "rel", npy(term)[0] - 0.25, t64, float(t32), 1e-5)
        check("accel_strided", (B, D, stride), "dv", "rel", npy(dv)[:, :D], dv0[:, :D] + g64, dv0[:, :D] + g32, 1e-4)
        assert untouched(npy(dv)[:, D:]) and npy(term)[1] == SENT64 and same_bits(npy(vt), v)


@pytest.mark.parametrize("rows,cols,ps,gs,step", [(3, 9, 9, 9, 1), (96, 66, 156, 156, 2), (97, 3, 3, 5, 1000), (5, 10, 10, 12, 1), (1, 1, 4, 1, 2)])
def test_adam_step_2d_vs_model(lib, rows, cols, ps, gs, step):
    L = lib; rng = np.random.default_rng(rows + cols)
    p = np.full((rows, ps), SENT, np.float32); p[:, :cols] = rng.normal(0, 1, (rows, cols))
    g = np.full((rows, gs), SENT, np.float32); g[:, :cols] = rng.normal(0, 1, (rows, cols)) * rng.choice([1e-3, 1.0, 1e3], (rows, 1))
    m, v = M.adam_moments(rng, g[:, :cols])
    for stop0 in (0, 1):
        pt, gt, mt, vt, fl = cu(p), cu(g), cu(m), cu(v), cu(np.array([stop0], np.int32))
        L.check(L.lib().vt_adam_step_2d(P(pt), ps, P(gt), gs, P(mt), P(vt), rows, cols, step, 0.006, 0.9, 0.999, 1e-8, P(fl), L.stream_ptr()))
        torch.cuda.synchronize()
        assert untouched(npy(pt)[:, cols:]) and same_bits(npy(gt), g)
        if stop0:
            assert same_bits(npy(pt), p) and same_bits(npy(mt), m) and same_bits(npy(vt), v)
            continue
        r64, r32 = M.adam(p[:, :cols], g[:, :cols], m, v, step, 0.006), M.adam(p[:, :cols], g[:, :cols], m, v, step, 0.006, fp32=True)
        check("adam2d", (rows, cols, step), "p", "abs", npy(pt)[:, :cols], r64[0], r32[0], 1e-6)
        check("adam2d", (rows, cols, step), "m", "rel", npy(mt), r64[1], r32[1], 1e-6)
        check("adam2d", (rows, cols, step), "v", "rel", npy(vt), r64[2], r32[2], 1e-6)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_sum_to_term_and_fills(lib, n):
    L = lib; rng = np.random.default_rng(n)
    x = rng.normal(0, 1, n + 3).astype(np.float32); xt, term = cu(x), cu(np.array([0.5, SENT64]))
    L.check(L.lib().vt_sum_to_term(P(xt), n, 0.3, P(term), L.stream_ptr()))
    torch.cuda.synchronize()
    want = np.sum(x[:n].astype(np.float64)) * float(np.float32(0.3))
    assert abs(npy(term)[0] - 0.5 - want) <= 1e-12 * np.abs(x[:n]).sum() and npy(term)[1] == SENT64      # fp64 sums of float32 values: order only
    a, b = sent(n + 2), torch.full((n + 2,), SENT64, dtype=torch.float64, device="cuda")
    L.check(L.lib().vt_fill(P(a, 4), n, 1.5, L.stream_ptr())); L.check(L.lib().vt_fill_f64(P(b, 8), n, -2.5, L.stream_ptr()))
    torch.cuda.synchronize()
    a, b = npy(a), npy(b)
    assert (a[1:n + 1] == np.float32(1.5)).all() and untouched(a[[0, n + 1]]) and (b[1:n + 1] == -2.5).all() and untouched(b[[0, n + 1]])


# =====================================================================================================================================
# vt_kpts_step
# =====================================================================================================================================
def _csr(rng, K, V, nnz_row):
    ind = np.stack([np.sort(rng.choice(V, min(nnz_row, V), replace=False)) for _ in range(K)]).astype(np.int32)
    data = rng.uniform(0.2, 1, ind.shape); data /= data.sum(1, keepdims=True)
    return {"indptr": (np.arange(K + 1) * ind.shape[1]).astype(np.int32), "indices": ind.ravel(), "data": data.astype(np.float32).ravel(), "shape": (K, V)}


@pytest.mark.parametrize("reg,B", [("body25", 96), ("body25", 3), ((1, 7), 5), ((64, 1500), 4), ((64, 7), 1), ((1, 1500), 97)])
def test_kpts_step_vs_model(lib, synth, reg, B):
    from vistracker_amd import ops
    L = lib; rng = np.random.default_rng(B + 31)
    csr = synth["regs"]["body25"] if reg == "body25" else _csr(rng, reg[0], reg[1], 5)
    K, V = csr["shape"]
    h = ops.LandmarkHandle(csr)
    A = M.csr_dense(csr["indptr"], csr["indices"], csr["data"], K, V)
    verts = (rng.normal(0, 0.3, (B, V, 3)) + [0, 0, rng.uniform(1.8, 2.7)]).astype(np.float32)
    verts[..., 2] = np.clip(verts[..., 2], 1.5, 3.0)                                             # joint depths in [1.5, 3] m
    k2 = np.concatenate([rng.uniform(0, 2000, (B, K, 2)), rng.uniform(0, 1, (B, K, 1))], -1).astype(np.float32)
    cc = rng.uniform(900, 1100, (B, 2)).astype(np.float32)
    dv0 = rng.normal(0, 1, (B, V, 3)).astype(np.float32)
    touched = A.any(0)
    for mode, accumulate, withJ in ((0, 0, True), (1, 0, True), (1, 1, True), (0, 1, False)):
        vt, kt, cct, term = cu(verts), cu(k2), cu(cc), cu(np.array([0.25, SENT64]))
        J, dv = sent(B, K, 3), cu(dv0) if accumulate else sent(B, V, 3)
        L.check(L.lib().vt_kpts_step(h.h, P(vt), P(kt), P(cct), B, mode, CAM.ctypes.data, 512.0, 0.7, P(term), P(J) if withJ else None, P(dv), accumulate, L.stream_ptr()))
        torch.cuda.synchronize()
        (J64, t64, g64), (J32, t32, g32) = M.kpts_chain(A, verts, k2, cc, mode, CAM, 512.0, 0.7), M.kpts_chain(A, verts, k2, cc, mode, CAM, 512.0, 0.7, fp32=True)
        shape = (reg, B, "mode", mode, "acc", accumulate)
        if withJ:
            check("kpts_step", shape, "J", "abs", npy(J), J64, J32, 2e-5)
        else:
            assert untouched(npy(J))
        check("kpts_step", shape, "term", "rel", npy(term)[0] - 0.25, t64, float(t32), 1e-5)
        base = dv0 if accumulate else np.float32(0)
        check("kpts_step", shape, "dverts", "rel", npy(dv), base + g64, base + g32, 1e-4)
        if accumulate:
            assert same_bits(npy(dv)[:, ~touched], dv0[:, ~touched])                              # vertices no landmark touches keep their bits
        else:
            assert (npy(dv)[:, ~touched] == 0).all()
        assert npy(term)[1] == SENT64 and same_bits(npy(vt), verts)


def test_kpts_step_refuses_more_than_64_landmarks(lib):
    from vistracker_amd import ops
    L = lib; rng = np.random.default_rng(3)
    h = ops.LandmarkHandle(_csr(rng, 65, 70, 3))
    vt, kt, cct, term, dv = cu(rng.normal(0, 1, (2, 70, 3)).astype(np.float32)), sent(2, 65, 3), sent(2, 2), cu(np.array([SENT64])), sent(2, 70, 3)
    rc = L.lib().vt_kpts_step(h.h, P(vt), P(kt), P(cct), 2, 1, CAM.ctypes.data, 512.0, 0.7, P(term), None, P(dv), 0, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == L.VT_ERR_ARG and b"vt_kpts_step" in L.lib().vt_last_error() and untouched(npy(dv)) and untouched(npy(term))


# =====================================================================================================================================
# fused == single-purpose launches, per kernel ("element for element and in the same order")
# =====================================================================================================================================
@pytest.mark.parametrize("B,N,NV", [(96, 3000, 2502), (97, 257, 1)])
def test_fused_equals_single_purpose_launches(lib, B, N, NV):
    L = lib; l = L.lib(); st = L.stream_ptr()
    c = head_case(500 + B, M.SO3_SEEDS[4], B, N, NV)
    out, hd = run_head(L, c)
    R, X, Xv = sent(B, 9), sent(B, N, 3), sent(B, NV, 3)
    L.check(l.vt_so3_project_forward(P(hd["M0"]), P(hd["noise"]), B, P(R), st))
    L.check(l.vt_rigid_forward(P(hd["X0p"]), 1, P(R), P(hd["t"]), P(hd["s"]), B, N, P(X), st))
    L.check(l.vt_rigid_forward(P(hd["X0v"]), 1, P(R), P(hd["t"]), P(hd["s"]), B, NV, P(Xv), st))
    torch.cuda.synchronize()
    assert np.array_equal(npy(R), out["R"]) and np.array_equal(npy(X), out["X"]) and np.array_equal(npy(Xv), out["Xv"])
    for form in ("plain", "sil", "object"):
        c = tail_case(600 + B, M.SO3_SEEDS[4], B, N, NV, form, adam_step=2)
        fused = run_tail(L, c)
        d = tail_buffers(c)
        tp = lambda i: P(d["terms"], 8 * i)
        if form == "sil":
            d["dXp"].zero_()                                   # the single-purpose sequence starts the point gradient from a fill
        if "temporal" in c:
            L.check(l.vt_temporal_loss2(P(d["X"]), B, N * 3, c["temporal"]["w_accel"], tp(I_ACC), c["temporal"]["w_velocity"], tp(I_VEL), P(d["dXp"]), 0, st))
        acc = 0
        if form == "sil":
            L.check(l.vt_rigid_backward(P(d["X0v"]), 1, P(d["s"]), B, NV, P(d["dXv"]), P(d["dR"]), P(d["dt"]), 0, st)); acc = 1
            L.check(l.vt_sqdiff_loss(P(d["t"]), 3, P(d["t_init"]), 3, B, 3, float(3 * B), c["w_trans"], tp(I_TRANS), P(d["dt"]), st))
        L.check(l.vt_rigid_backward(P(d["X0p"]), 1, P(d["s"]), B, N, P(d["dXp"]), P(d["dR"]), P(d["dt"]), acc, st))
        L.check(l.vt_so3_project_backward(P(d["M0"]), P(d["noise"]), B, P(d["dR"]), P(d["dM"]), st))
        L.check(l.vt_adam_step_2d(P(d["M0"]), 9, P(d["dM"]), 9, P(d["mR"]), P(d["vR"]), B, 9, c["adam_step"], c["lrR"], 0.9, 0.999, 1e-8, P(d["stop"]), st))
        L.check(l.vt_adam_step_2d(P(d["t"]), 3, P(d["dt"]), 3, P(d["mT"]), P(d["vT"]), B, 3, c["adam_step"], c["lrT"], 0.9, 0.999, 1e-8, P(d["stop"]), st))
        L.check(l.vt_loss_reduce_and_stop(P(d["terms"]), c["w"].ctypes.data, NT, c["tol"], c["armed"], P(d["state"]), P(d["stop"]), P(d["hist"]), c["slot"], st))
        torch.cuda.synchronize()
        for k in ("dR", "dt", "dM", "M0", "mR", "vR", "t", "mT", "vT", "stop"):
            assert np.array_equal(npy(d[k]), fused[k]), (form, k, float(np.abs(npy(d[k]) - fused[k]).max()))
        assert np.allclose(npy(d["terms"]), fused["terms"], rtol=2e-6, atol=0) and np.allclose(npy(d["hist"])[c["slot"]], fused["hist"][c["slot"]], rtol=2e-6, atol=0)


# =====================================================================================================================================
# refusals: VT_ERR_ARG, a message, nothing written
# =====================================================================================================================================
def test_step_entry_points_refuse_bad_arguments(lib, synth):
    L = lib
    def refused(c, d, launch, what):
        before = {k: npy(v) for k, v in d.items() if v is not None}
        rc = launch(L, c, d)
        torch.cuda.synchronize()
        assert rc == L.VT_ERR_ARG and len(L.lib().vt_last_error()) > 0, (what, rc)
        for k, v in before.items():
            assert same_bits(npy(d[k]), v), (what, k)
    for B in (1, 2):                                                   # temporal entry points need an interior frame
        c = tail_case(1, M.SO3_SEEDS[0], 3, 50, 0, "object"); d = tail_buffers(c)
        refused(dict(c, B=B), d, launch_tail, f"temporal tail B={B}")
        v, dv, t = sent(3, 10), sent(3, 10), cu(np.array([SENT64, SENT64]))
        rc = L.lib().vt_temporal_loss2(P(v), B, 10, 1.0, P(t), 1.0, P(t, 8), P(dv), 0, L.stream_ptr())
        rc2 = L.lib().vt_accel_loss_strided(P(v), B, 10, 10, None, 1.0, P(t), P(dv), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc == L.VT_ERR_ARG and rc2 == L.VT_ERR_ARG and untouched(npy(dv)) and untouched(npy(t))
    for form, mk, bufs, launch in (("plain", lambda: tail_case(2, M.SO3_SEEDS[0], 4, 50, 0, "plain"), tail_buffers, launch_tail),
                                   ("object", lambda: tail_case(2, M.SO3_SEEDS[0], 4, 50, 0, "object"), tail_buffers, launch_tail),
                                   ("smpl", lambda: smpl_case(3, 4, "smpl-all", synth), lambda c: smpl_buffers(c, synth), launch_smpl)):
        c = mk()
        refused(dict(c, adam_step=0), bufs(c), launch, form + " adam_step=0")
        refused(dict(c, nzero=NT + 1), bufs(c), launch, form + " nzero > nterms")
        for nterms in (0, 17):
            refused(dict(c, nzero=0, nterms=nterms), bufs(c), launch, f"{form} nterms={nterms}")
        if form == "smpl":
            d = bufs(c); d["m1"] = None
            refused(c, d, launch, "smpl group without m")
            d = bufs(c); d["dtrans"] = None
            refused(c, d, launch, "smpl group without gradient")
            for what, grp in (("more columns than the parameter stride", dict(c["groups"][0], ncols=4)), ("no columns", dict(c["groups"][0], ncols=0))):
                refused(dict(c, groups=[grp] + c["groups"][1:]), bufs(c), launch, "smpl group with " + what)      # (trans: stride 3)
        else:
            d = bufs(c); d["mT"] = None
            refused(c, d, launch, form + " pT without mT")
            d = bufs(c); d["vR"] = None
            refused(c, d, launch, form + " pR without vR")
