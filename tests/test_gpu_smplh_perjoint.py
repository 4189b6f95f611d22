"""GPU (-m gpu): the SMPL-H kernels against the float64 model (tests/smplh_model.py), every gradient row on its own scale.

Common gate: a case's gradients pass when every joint of dpose, every column of dbetas and every axis of dtrans is within ``GATE * e32`` of the model, where e32
is the largest such error of the float32 CPU oracle on the same case (tests/smplh_cases.py).  The forward is held to the absolute 3e-5 m the older tests use,
on every vertex.  The cases walk the block boundaries of the three heavy kernels, the serial reverse chain that SMPL-H's own tree never takes, trees other than
SMPL-H's on the scheduled path, poses at the edges of the axis-angle map, a gradient that enters through the joints only, and a dense-weights model."""
import numpy as np
import pytest

import smplh_cases as C
import smplh_model as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def check_case(name, mode, base):
    r = C.reference(name, base); c = r["inputs"]
    fwd, grads = C.run_kernels(C.handle_of(name, c["model"]), c, mode)
    for what, got, ref in zip(("verts", "jtr", "v_posed"), fwd, r["fwd"]):
        e = np.abs(got - ref).max()
        print(f"{name} {mode}: {what} max |kernel - model| = {e:.2e} m")
        assert e < 3e-5, what
    errs = M.grad_errs(grads, r[mode]["ref"], c["zero_joints"])
    gate = r[mode]["gate"]
    for k, e in errs.items():
        print(f"{name} {mode}: {k} worst row {int(e.argmax())} err {e.max():.2e} (fp32 oracle {r[mode]['err32'][k].max():.2e}, gate {gate:.2e})")
    for k, e in errs.items():
        assert (e <= gate).all(), f"{k}: rows {np.nonzero(e > gate)[0].tolist()} exceed {gate:.2e}: {e[e > gate]}"
    return errs


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("B", C.B_SIZES)
def test_batch_edges(synth, B, mode):
    """B on both sides of every frames-per-block constant: BWD_FB = 6 (padded frames of the tile kernel at 7), FWD_FB = 16, BL_M = 96 (at 97 the blend GEMM's
    second M block holds one frame and 95 rows of padding)"""
    check_case(f"batch{B}", mode, synth["model"])


def test_joint_only_gradient(synth):
    """dverts = 0, djtr random: dpose and dbetas come from the reverse chain alone; the joints without children get exactly zero"""
    check_case("joint_only", "djtr", synth["model"])


@pytest.mark.parametrize("mode", C.MODES)
def test_pose_edges(synth, mode):
    """rows of exactly zero, 1e-6, pi - 1e-3 and 4.0 rad, the rest pose, betas = 3"""
    check_case("pose_edges", mode, synth["model"])


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("tree", C.TREES)
def test_trees(synth, tree, mode):
    """other parents over the same arrays: the ternary heap runs the scheduled reverse chain, the chain, the star and the eleven-wide tree overflow the
    schedule (steps, steps, width) and run the serial loop; all have to agree with the model alike"""
    check_case(f"tree_{tree}", mode, synth["model"])


@pytest.mark.parametrize("mode", C.MODES)
def test_dense_weights(synth, mode):
    """100 vertices with 52 non-zero weights: the dense LBS of the forward, and the backward of such a model"""
    check_case("dense", mode, synth["model"])


def test_null_djtr_is_zero_djtr(synth):
    """autograd hands the backward a zero djtr when jtr took no part in the loss; the C ABI also takes djtr = NULL and skips the additions.  x + 0 = x: the
    two give the same values"""
    from vistracker_amd import _lib as L
    r = C.reference("batch7", synth["model"]); c = r["inputs"]; B = 7
    h = C.handle_of("batch7", c["model"])
    _, want = C.run_kernels(h, c, "none")
    p, b, t, dv = (C.cu(c[k]) for k in ("pose", "betas", "trans", "dverts"))
    verts = torch.empty(B, 6890, 3, device="cuda"); jtr = torch.empty(B, 52, 3, device="cuda"); vposed = torch.empty(B, 6890, 3, device="cuda")
    ws = torch.empty(L.lib().vt_smplh_workspace_floats(B), device="cuda")
    L.check(L.lib().vt_smplh_forward(h.h, L.dptr(p), L.dptr(b), L.dptr(t), B, L.dptr(verts), L.dptr(jtr), L.dptr(vposed), L.dptr(ws), L.stream_ptr()))
    scratch = torch.empty(L.lib().vt_smplh_bwd_scratch_floats(B), device="cuda")
    dp = torch.empty(B, 156, device="cuda"); db = torch.empty(B, 10, device="cuda"); dt = torch.empty(B, 3, device="cuda")
    L.check(L.lib().vt_smplh_backward(h.h, L.dptr(p), L.dptr(b), B, L.dptr(dv), None, L.dptr(vposed), L.dptr(ws), L.dptr(scratch),
                                      L.dptr(dp), L.dptr(db), L.dptr(dt), L.stream_ptr()))
    for got, w in zip((dp, db, dt), want):
        assert np.array_equal(got.cpu().numpy(), w)
