"""GPU (-m gpu): SMPL-H with the hand joints' share taken out of the step (vt_smplh_prefix / vt_smplh_forward_prefixed / vt_smplh_backward_free).

The fits never move pose[:, 66:], so the library computes the hand rotations and the frozen K steps of the blend-shape GEMM once per fit and the backward
leaves the hand columns out.  What is asked of it:
  * prefix + prefixed forward == vt_smplh_forward, bit for bit (the same MFMAs per accumulator in the same order), at both sides of the frame-block edges;
  * the restricted backward's dpose[:, :66], dbetas, dtrans == vt_smplh_backward's, bit for bit; dpose[:, 66:] is not written (a sentinel survives);
  * both within the common gate of the float64 model (tests/smplh_model.py: 8 x the float32 oracle's worst row on the same case) -- which also holds the plain
    forward in its new K order to the model;
  * a prefix is a function of the hand pose: another hand pose with the old prefix gives another result, with a rebuilt prefix the plain forward's again;
  * a short SMPL-stage fit ends on the same bits with the prefix path on and off.
The hand poses are the synthetic GRAB means plus noise: with hands at rest the frozen rows multiply R - I = 0 and nothing here would be tested."""
import numpy as np
import pytest

import smplh_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B_SIZES = (1, 6, 7, 16, 17)       # 6 | 7: frames per block of smplh_bwd_tile_kernel; 16 | 17: of smplh_verts_kernel
N_FREE = 66                       # pose columns of the fits' Adam groups
SENTINEL = -12345.0


def cu(x):
    return torch.tensor(np.asarray(x)).cuda()


def case_inputs(synth, B):
    """random body, hands = GRAB means + noise (never at rest), random cotangents"""
    rng = np.random.default_rng(4200 + B)
    f = np.float32
    pose = rng.normal(0, 0.3, (B, 156)).astype(f)
    hands = np.concatenate([synth["priors"]["lhand_mean"], synth["priors"]["rhand_mean"]]).astype(f)
    pose[:, 66:] = hands + rng.normal(0, 0.2, (B, 90)).astype(f)
    assert (np.abs(pose[:, 66:].reshape(B, 30, 3)).max(-1) > 1e-3).all()
    return {"pose": pose, "betas": rng.normal(0, 1, (B, 10)).astype(f), "trans": rng.normal(0, 0.3, (B, 3)).astype(f),
            "dverts": rng.normal(0, 1, (B, 6890, 3)).astype(f), "djtr": rng.normal(0, 1, (B, 52, 3)).astype(f)}


_HANDLE = {}


def handle(synth):
    if "h" not in _HANDLE:
        from vistracker_amd import ops
        _HANDLE["h"] = ops.SmplhHandle(synth["model"])
    return _HANDLE["h"]


class Run:
    """the C ABI on one case: every call gets buffers of its own, so that nothing can be right by leftovers of another call"""

    def __init__(self, synth, c):
        from vistracker_amd import _lib as L
        self.L, self.lib, self.h = L, L.lib(), handle(synth).h
        self.B = c["pose"].shape[0]
        self.p, self.b, self.t, self.dv, self.dj = (cu(c[k]) for k in ("pose", "betas", "trans", "dverts", "djtr"))

    def _out(self):
        B = self.B
        return [torch.full((B, 6890, 3), float("nan"), device="cuda"), torch.full((B, 52, 3), float("nan"), device="cuda"),
                torch.full((B, 6890, 3), float("nan"), device="cuda"), torch.full((self.lib.vt_smplh_workspace_floats(B),), float("nan"), device="cuda")]

    def plain(self, pose=None):
        L = self.L; p = self.p if pose is None else pose
        v, j, vp, ws = self._out()
        L.check(self.lib.vt_smplh_forward(self.h, L.dptr(p), L.dptr(self.b), L.dptr(self.t), self.B, L.dptr(v), L.dptr(j), L.dptr(vp), L.dptr(ws), L.stream_ptr()))
        return v, j, vp, ws

    def prefix(self, pose=None):
        """-> (ws, prefix) of a vt_smplh_prefix call"""
        L = self.L; p = self.p if pose is None else pose
        ws = self._out()[3]
        pre = torch.full((self.lib.vt_smplh_prefix_floats(self.B),), float("nan"), device="cuda")
        L.check(self.lib.vt_smplh_prefix(self.h, L.dptr(p), self.B, L.dptr(ws), L.dptr(pre), L.stream_ptr()))
        return ws, pre

    def prefixed(self, ws, pre, pose=None, steps=1):
        """the prefixed forward on (ws, pre); ``steps`` calls in a row, as a fit makes them"""
        L = self.L; p = self.p if pose is None else pose
        v, j, vp, _ = self._out()
        for _ in range(steps):
            L.check(self.lib.vt_smplh_forward_prefixed(self.h, L.dptr(p), L.dptr(self.b), L.dptr(self.t), self.B, L.dptr(pre), L.dptr(v), L.dptr(j), L.dptr(vp),
                                                       L.dptr(ws), L.stream_ptr()))
        return v, j, vp, ws

    def _grads(self):
        B = self.B
        return (torch.full((B, 156), SENTINEL, device="cuda"), torch.full((B, 10), SENTINEL, device="cuda"), torch.full((B, 3), SENTINEL, device="cuda"),
                torch.full((self.lib.vt_smplh_bwd_scratch_floats(B),), float("nan"), device="cuda"))

    def backward(self, vp, ws, djtr):
        L = self.L; dp, db, dt, scratch = self._grads()
        L.check(self.lib.vt_smplh_backward(self.h, L.dptr(self.p), L.dptr(self.b), self.B, L.dptr(self.dv), L.dptr(self.dj) if djtr else None, L.dptr(vp), L.dptr(ws),
                                           L.dptr(scratch), L.dptr(dp), L.dptr(db), L.dptr(dt), L.stream_ptr()))
        return dp, db, dt

    def backward_free(self, vp, ws, djtr, n_free=N_FREE):
        L = self.L; dp, db, dt, scratch = self._grads()
        L.check(self.lib.vt_smplh_backward_free(self.h, L.dptr(self.p), self.B, L.dptr(self.dv), L.dptr(self.dj) if djtr else None, L.dptr(vp), L.dptr(ws),
                                                L.dptr(scratch), n_free, L.dptr(dp), L.dptr(db), L.dptr(dt), L.stream_ptr()))
        return dp, db, dt


def n(*ts):
    return [x.cpu().numpy() for x in ts]


@pytest.mark.parametrize("B", B_SIZES)
def test_forward_is_bit_identical(synth, B):
    r = Run(synth, case_inputs(synth, B))
    want = n(*r.plain()[:3])
    ws, pre = r.prefix()
    got = n(*r.prefixed(ws, pre, steps=2)[:3])          # twice: the second call must find the hand rotations of the prefix call, not ruins of the first
    for what, g, w in zip(("verts", "jtr", "v_posed"), got, want):
        assert np.isfinite(w).all() and np.array_equal(g, w), (what, float(np.abs(g - w).max()))


@pytest.mark.parametrize("djtr", (True, False))
@pytest.mark.parametrize("B", B_SIZES)
def test_backward_is_bit_identical(synth, B, djtr):
    r = Run(synth, case_inputs(synth, B))
    _, _, vp, ws = r.plain()
    want = n(*r.backward(vp, ws, djtr))
    ws2, pre = r.prefix()
    _, _, vp2, ws2 = r.prefixed(ws2, pre)
    for name, (v_, w_) in (("behind the plain forward", (vp, ws)), ("behind the prefixed forward", (vp2, ws2))):
        dp, db, dt = n(*r.backward_free(v_, w_, djtr))
        assert np.isfinite(want[0]).all() and (want[0] != SENTINEL).all()
        assert np.array_equal(dp[:, :N_FREE], want[0][:, :N_FREE]), (name, float(np.abs(dp[:, :N_FREE] - want[0][:, :N_FREE]).max()))
        assert np.array_equal(db, want[1]) and np.array_equal(dt, want[2]), name
        assert (dp[:, N_FREE:] == SENTINEL).all(), f"{name}: dpose[:, {N_FREE}:] was written"


def test_backward_free_takes_fewer_columns_and_refuses_frozen_ones(synth):
    """n_free_pose_cols = 3 (the global rotation alone, the first phase of the SMPL-T pre-fit): same bits, the rest untouched; beyond 66 or no multiple of
    3 is an argument error, not a silent full backward"""
    r = Run(synth, case_inputs(synth, 7))
    _, _, vp, ws = r.plain()
    want = n(*r.backward(vp, ws, True))
    dp, db, dt = n(*r.backward_free(vp, ws, True, n_free=3))
    assert np.array_equal(dp[:, :3], want[0][:, :3]) and (dp[:, 3:] == SENTINEL).all()
    assert np.array_equal(db, want[1]) and np.array_equal(dt, want[2])
    for bad in (0, 4, 69, 156):
        with pytest.raises(r.L.VtError):
            r.backward_free(vp, ws, True, n_free=bad)


@pytest.mark.parametrize("B", (7, 17))
def test_against_the_float64_model(synth, B):
    """the gate rule of tests/test_gpu_smplh_perjoint.py, computed for this case: every live row within 8 x the float32 oracle's worst row; the forwards --
    plain, in its new K order, and prefixed -- within the 3e-5 m of the older tests on every vertex"""
    from oracle import oracle as O
    c = case_inputs(synth, B)
    m = M.SmplhModel(synth["model"]); o = O.SmplModel(synth["model"])
    args = (c["pose"], c["betas"], c["trans"])
    fwd_ref = m.forward(*args)
    r = Run(synth, c)
    ws, pre = r.prefix()
    v, j, vp, ws = r.prefixed(ws, pre)
    for name, outs in (("plain", r.plain()[:3]), ("prefixed", (v, j, vp))):
        for what, got, ref in zip(("verts", "jtr", "v_posed"), n(*outs), fwd_ref):
            e = np.abs(got - ref).max()
            print(f"B={B} {name}: {what} max |kernel - model| = {e:.2e} m")
            assert e < 3e-5, (name, what)
    cots = [(c["dverts"], c["djtr"]), (c["dverts"], None)]
    for (dv, dj), ref in zip(cots, m.backward_many(*args, cots)):
        e32 = M.worst(M.grad_errs(o.backward(*args, dv, dj), ref))
        gate = M.GATE * e32
        dp, db, dt = n(*r.backward_free(vp, ws, dj is not None))
        errs = {"dpose": M.per_row_err(dp[:, :N_FREE], ref[0][:, :N_FREE], N_FREE // 3), "dbetas": M.per_row_err(db, ref[1], 10),
                "dtrans": M.per_row_err(dt, ref[2], 3)}
        for k, e in errs.items():
            print(f"B={B} djtr={dj is not None}: {k} worst row {int(e.argmax())} err {e.max():.2e} (fp32 oracle worst {e32:.2e}, gate {gate:.2e})")
        for k, e in errs.items():
            assert (e <= gate).all(), f"{k}: rows {np.nonzero(e > gate)[0].tolist()} exceed {gate:.2e}: {e[e > gate]}"


def test_stale_prefix_shows_and_a_rebuilt_one_is_right(synth):
    c = case_inputs(synth, 7)
    r = Run(synth, c)
    ws, pre = r.prefix()
    old = n(*r.prefixed(ws, pre)[:3])
    moved = c["pose"].copy(); moved[:, 3 * 37:3 * 37 + 3] += np.float32(0.4)          # one finger joint, every frame
    p2 = cu(moved)
    want = n(*r.plain(p2)[:3])
    assert not np.array_equal(want[0], old[0]) and not np.array_equal(want[2], old[2])
    stale = n(*r.prefixed(ws, pre, pose=p2)[:3])
    assert np.array_equal(stale[0], old[0]), "the prefixed forward read pose[:, 66:]: the prefix is supposed to stand for it"
    ws2, pre2 = r.prefix(p2)
    got = n(*r.prefixed(ws2, pre2, pose=p2)[:3])
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_a_short_fit_ends_on_the_same_bits(synth):
    """optimize_smpl, B = 4, 1/8-resolution maps, 20 Adam steps (both phases' Adam groups): FitContext.frozen_hands on and off"""
    from conftest import golden
    from vistracker_amd import ops, synthetic as syn
    from vistracker_amd.fitting import FitContext
    g = golden("smplfit")
    rng = np.random.default_rng(77)
    pose0 = np.asarray(g["pose"], np.float32).copy()
    hands = np.concatenate([synth["priors"]["lhand_mean"], synth["priors"]["rhand_mean"]]).astype(np.float32)
    pose0[:, 66:] = hands + rng.normal(0, 0.2, (pose0.shape[0], 90)).astype(np.float32)
    assert pose0.shape[0] == 4
    out = []
    for frozen in (True, False):
        ctx = FitContext(synth["model"], synth["regs"], synth["priors"], synth["decoders"], synth["labels"])
        ctx.frozen_hands = frozen
        maps = ops.FeatureMaps.from_nchw(syn.feature_maps(4, int(g["maps_seed"]), res_scale=1 / 8))
        pose, betas, trans = cu(pose0), cu(g["betas"]), cu(g["trans"])
        res = ctx.optimize_smpl(maps, pose, betas, trans, cu(g["crop_center"]), cu(g["body_center"]), cu(g["body_kpts"]), it_range=(0, 2), early_stop=False)
        assert res.steps == 20
        out.append(n(pose, betas, trans) + [res.losses])
    a, b = out
    assert not np.array_equal(a[0][:, :66], pose0[:, :66]), "the fit did not move the body pose"
    assert np.array_equal(a[0][:, 66:], pose0[:, 66:]), "a fit wrote pose[:, 66:]: the invariant the prefix rests on"
    for k, name in enumerate(("pose", "betas", "trans")):
        assert np.array_equal(a[k], b[k]), (name, float(np.abs(a[k] - b[k]).max()))
    # (the loss history is a sum of fp64 atomics over workgroups: equal to the last bits, not bit for bit, also between two runs of one path)
    assert np.isfinite(a[3]).all() and np.allclose(a[3], b[3], rtol=2e-6, atol=0)
