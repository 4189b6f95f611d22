"""CPU: the float64 SMPL-H model (tests/smplh_model.py) against the reference's recorded values and against the float64 oracle on every case the GPU tests
use (tests/smplh_cases.py); the per-row metric against a 0.1 % error on one finger joint; the soundness of the cases themselves."""
import numpy as np
import pytest

import smplh_cases as C
import smplh_model as M
from conftest import golden, GOLDEN

EPS64 = np.finfo(np.float64).eps
# The longest sums of the operator run over the 3 x 6890 vertex coordinates (dbetas, the pose-map part of dpose, the joint regressor) after the 459 pose-map terms
# of v_posed.  The worst case of a sum of n terms is n eps of the sum of magnitudes; two independent float64 evaluations of it -- this model and the oracle -- are
# 2 n eps apart at most, and a factor 2 is left for the ratio between the sum of magnitudes and the row's scale.  (Random signs make the typical distance
# ~sqrt(n) eps, two orders below the bound.)
N_TERMS = 3 * 6890 + 459
BOUND64 = 4 * EPS64 * N_TERMS          # 1.9e-11


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


@pytest.fixture(scope="module")
def base(synth):
    return synth["model"]


def test_model_vs_golden(base):
    """the reference layer's recorded forward and autograd gradients (float32), at the tolerances test_oracle_golden holds the oracle to"""
    g = golden("smplh"); vs = int(g["vsub"])
    m = M.SmplhModel(base)
    verts, jtr, vposed = m.forward(g["pose"], g["betas"], g["trans"])
    assert np.abs(verts[:, ::vs] - g["verts_sub"]).max() < 2e-5
    assert np.abs(jtr - g["jtr"]).max() < 2e-5
    assert np.abs(vposed[:, ::vs] - g["vposed_sub"]).max() < 2e-5
    gv = np.load(GOLDEN + "/smplh_gv.npy").astype(np.float32)
    dpose, dbetas, dtrans = m.backward(g["pose"], g["betas"], g["trans"], gv, g["gj"])
    assert rel(g["dpose"], dpose) < 2e-4 and rel(g["dbetas"], dbetas) < 2e-4 and rel(g["dtrans"], dtrans) < 2e-4


def test_model_rodrigues_vs_golden():
    """every recorded row, the first two included: theta = 0, where the axis is 0 / |1e-8| and the derivative (that of I + [theta]x) rests on sin(n/2) / n alone, and
    |theta| = 3.7e-4.  The recorded values ARE the shifted definition's (to float32 round-off), which is what the model restates."""
    g = golden("rodrigues")
    assert np.abs(M.rodrigues_np(g["aa"]) - g["R"]).max() < 2e-6
    d = M.rodrigues_bwd_np(g["aa"], g["gR"])
    assert rel(g["daa"], d) < 1e-4
    err = M.per_row_err(g["daa"].reshape(1, -1), d.reshape(1, -1), len(d))
    print("rodrigues golden rows 0, 1, worst:", err[0], err[1], err.max())
    assert err.max() < 1e-5            # float32 autograd of ~30 operations; rows 0 and 1 are no worse than the others
    assert np.abs(d[0] - np.array([g["gR"][0][7] - g["gR"][0][5], g["gR"][0][2] - g["gR"][0][6], g["gR"][0][3] - g["gR"][0][1]])).max() < 1e-7


@pytest.mark.parametrize("name", C.CASES)
def test_model_vs_oracle64(base, name):
    """model (autograd) == float64 oracle (hand-derived VJP in C) to float64 round-off, every case and tree; and the case is sound: finite everywhere, every row
    of every gradient has a scale (per_row_err asserts it; rows a case zeroes by construction are declared and must be exactly zero)"""
    from oracle import oracle64 as O64
    r = C.reference(name, base); c = r["inputs"]
    o = O64.SmplModel(c["model"])
    args = (c["pose"], c["betas"], c["trans"])
    for got, ref in zip(o.forward(*args), r["fwd"]):
        assert np.isfinite(ref).all() and np.isfinite(got).all()
        assert rel(got, ref) < BOUND64
    for mode in c["modes"]:
        g64 = o.backward(*args, c["dverts"], c["djtr"] if mode == "djtr" else None)
        ref = r[mode]["ref"]
        assert all(np.isfinite(a).all() for a in g64 + ref + r[mode]["o32"])
        e64 = M.grad_errs(g64, ref, c["zero_joints"])
        print(f"{name} {mode}: model vs oracle64 {M.worst(e64):.2e} (bound {BOUND64:.2e}); fp32 oracle e32 {r[mode]['e32']:.2e}")
        assert M.worst(e64) < BOUND64
        # the gate this case gives the kernels is float32 round-off class and far below the 1e-3 error the metric has to catch
        assert 1e-8 < r[mode]["e32"] < 1e-5


def test_trees_land_where_the_cases_say():
    """the four trees against the limits of the reverse-chain schedule (32 steps of 10 joints): one fits, three overflow -- each in its own way"""
    assert C.schedule_shape(C.parents_of("heap3")) == (12, 9)
    assert C.schedule_shape(C.parents_of("chain")) == (51, 1)           # too many steps (levels)
    assert C.schedule_shape(C.parents_of("star")) == (51, 1)            # too many steps (sibling ranks)
    steps, width = C.schedule_shape(C.parents_of("wide11"))
    assert steps <= 32 and width == 11                                  # too wide only
    from vistracker_amd import synthetic as syn
    steps, width = C.schedule_shape(syn.SMPLH_PARENTS)
    assert steps <= 32 and width == 10                                  # SMPL-H itself: exactly at the width limit
    for t in C.TREES:
        steps, width = C.schedule_shape(C.parents_of(t))
        assert (steps <= 32 and width <= 10) == C.SCHEDULED[t]


def _teeth_case(base):
    """the input of test_smplh_vs_oracle_ragged_batches[13] (default_rng(13), B = 13), and the float32 oracle as the stand-in for a kernel"""
    from oracle import oracle as O
    B = 13
    rng = np.random.default_rng(B)
    pose = rng.normal(0, 0.3, (B, 156)).astype(np.float32); betas = rng.normal(0, 1, (B, 10)).astype(np.float32)
    trans = rng.normal(0, 0.3, (B, 3)).astype(np.float32)
    gv = rng.normal(0, 1, (B, 6890, 3)).astype(np.float32)
    ref = M.SmplhModel(base).backward(pose, betas, trans, gv)
    o32 = O.SmplModel(base).backward(pose, betas, trans, gv)
    e32 = M.worst(M.grad_errs(o32, ref))
    return ref, o32, M.GATE * e32


def test_metric_rejects_a_finger_joint_off_by_a_thousandth(base):
    """a gradient that is right everywhere but 0.1 % too large on ONE phalanx: the per-joint gate rejects it, the whole-array rel < 3e-4 of the older
    tests accepts it (the root's gradient is ~100, a phalanx's ~1: rel sees 1e-3 * 1 / 100)"""
    ref, o32, gate = _teeth_case(base)
    assert M.worst(M.grad_errs(o32, ref)) <= gate                       # unmutated: passes
    for joint in (22, 36, 51):                                          # first left, a middle, last right phalanx
        mut = o32[0].copy().reshape(-1, 52, 3); mut[:, joint] *= 1.001
        mut = mut.reshape(-1, 156)
        err = M.per_row_err(mut, ref[0], 52)
        assert err[joint] > gate and err[joint] > 9e-4
        assert (np.delete(err, joint) <= gate).all()
        assert rel(mut, ref[0]) < 3e-4


def test_metric_rejects_a_dbetas_column_off_by_a_thousandth(base):
    """the same for dbetas.  Here the whole-array metric is NOT blind at this input: the ten columns' scales are within a factor 2.2 of each other
    (2.3 .. 4.9), so rel sees 1e-3 * scale / 4.9 >= 4.7e-4 > 3e-4 for every column.  What is asserted is what holds: the per-column gate rejects every
    column's mutation at its full 1e-3, and rel dilutes it by the column's scale over the largest."""
    ref, o32, gate = _teeth_case(base)
    scale = np.abs(ref[1]).max(0)
    for col in range(10):
        mut = o32[1].copy(); mut[:, col] *= 1.001
        err = M.per_row_err(mut, ref[1], 10)
        assert err[col] > gate and err[col] > 9e-4
        assert (np.delete(err, col) <= gate).all()
        assert abs(rel(mut, ref[1]) - 1e-3 * scale[col] / scale.max()) < 1e-5


def test_metric_refuses_a_dead_row():
    ref = np.ones((2, 6)); ref[:, 2:4] = 0
    with pytest.raises(AssertionError, match="without a scale"):
        M.per_row_err(ref, ref, 3)
    assert M.per_row_err(ref, ref, 3, zero_rows=(1,)).max() == 0
    got = ref.copy(); got[1, 3] = 1e-3                                   # a declared-zero row is held to zero, absolutely
    assert M.per_row_err(got, ref, 3, zero_rows=(1,))[1] == 1e-3
    with pytest.raises(AssertionError, match="declared zero"):
        M.per_row_err(ref, ref, 3, zero_rows=(0, 1))
    bad = np.ones((2, 6)); bad[0, 0] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        M.per_row_err(bad, np.ones((2, 6)), 3)
