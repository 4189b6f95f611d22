"""CPU: the float64 model of the fused step kernels (tests/step_model.py) checked against independent statements of the same operations --
torch autograd, torch.optim.Adam -- and the conditions its input generators promise to the GPU tests (tests/test_gpu_step_kernels.py)."""
import numpy as np
import pytest

import step_model as M

torch = pytest.importorskip("torch")


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-300)


@pytest.mark.parametrize("seed", M.SO3_SEEDS)
def test_so3_input_generator_meets_its_conditions(seed):
    """at most 25 % of the random draws rejected; every frame inside the domain min(h_i + h_j) >= 0.1 s1; the reflection has det < 0 and the
    singular values it was built from; exact rotations are rotations to float32 rounding"""
    for B in M.SO3_BATCHES:                                   # every (seed, B) pair the GPU tests may draw (they assert membership)
        M0, noise, kinds, rejected = M.so3_inputs(seed, B)
        assert rejected <= M.SO3_MAX_REJECT, rejected
        margin = M.so3_margin(M0, noise)
        assert margin.min() >= M.SO3_MIN_MARGIN, margin.min()
        k = np.array(kinds)
        p = M.project_so3(M0[k == "reflection"])
        assert (p["d"] == -1).all() and (B < 3 or np.abs(p["s"] - [3, 2, 0.5]).max() < 1e-5)
        Rm = M0[k == "rotation"].astype(np.float64)
        assert np.abs(Rm @ np.swapaxes(Rm, 1, 2) - np.eye(3)).max() < 1e-6 and np.abs(np.linalg.det(Rm) - 1).max() < 1e-6
        assert set(kinds) == set(M.SO3_KINDS[:B])


@pytest.mark.parametrize("seed", M.SO3_SEEDS[:3])
def test_so3_vjp_polar_equals_autograd(seed):
    """the polar form and torch's derivative through svd / det agree wherever autograd is defined (distinct singular values: every kind but the
    exact rotations and the near-rotations of a fit, whose 1 / (s_i^2 - s_j^2) terms it cannot take)"""
    M0, noise, kinds, _ = M.so3_inputs(seed, 48)
    keep = np.array([k not in ("rotation", "fit") for k in kinds])
    G = np.random.default_rng(seed).normal(0, 1, (48, 3, 3))
    a = M.so3_vjp_polar(M0[keep], noise[keep], G[keep]); b = M.so3_vjp_autograd(M0[keep], noise[keep], G[keep])
    for i in range(a.shape[0]):
        assert rel(a[i], b[i]) < 1e-9, (i, rel(a[i], b[i]))
    # the projection itself: a rotation
    R = M.project_so3(M0, noise)["R"]
    assert np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max() < 1e-12 and np.abs(np.linalg.det(R) - 1).max() < 1e-12
    # at exact rotations the polar form is finite and projects the gradient onto the tangent space: dM = (G - R G^T R) / 2
    rot = np.array([k == "rotation" for k in kinds])
    Rr = M.project_so3(M0[rot])["R"]
    want = 0.5 * (G[rot] - Rr @ np.swapaxes(G[rot], 1, 2) @ Rr)
    assert rel(M.so3_vjp_polar(M0[rot], None, G[rot]), want) < 1e-6


def test_rigid_and_stencil_gradients_equal_autograd():
    rng = np.random.default_rng(5)
    B, N = 5, 37
    X0, R, t, s, gX = rng.normal(0, 1, (N, 3)), rng.normal(0, 1, (B, 3, 3)), rng.normal(0, 1, (B, 3)), rng.uniform(0.5, 2, B), rng.normal(0, 1, (B, N, 3))
    Rt, tt = torch.tensor(R, requires_grad=True), torch.tensor(t, requires_grad=True)
    X = (torch.tensor(X0)[None] @ Rt + tt[:, None, :]) * torch.tensor(s)[:, None, None]
    assert rel(M.rigid(X0, R, t, s), X.detach().numpy()) < 1e-14
    (X * torch.tensor(gX)).sum().backward()
    dR, dt = M.rigid_vjp(X0, s, gX)
    assert rel(dR, Rt.grad.numpy()) < 1e-13 and rel(dt, tt.grad.numpy()) < 1e-13
    for Bv in (3, 4, 5, 9):
        v = rng.normal(0, 1, (Bv, 11)); w = rng.uniform(1, 10, 11)
        for ew in (None, w):
            vt = torch.tensor(v, requires_grad=True)
            a = vt[2:] - 2 * vt[1:-1] + vt[:-2]
            ref = ((a * a) * (1 if ew is None else torch.tensor(ew))).mean()
            (0.7 * ref).backward()
            term, dv = M.accel_term(v, 0.7, ew)
            assert abs(term - ref.item()) < 1e-13 * abs(ref.item()) and rel(dv, vt.grad.numpy()) < 1e-13
        vt = torch.tensor(v, requires_grad=True)
        d = vt[1:] - vt[:-1]
        ref = (d * d).mean(); (1.3 * ref).backward()
        term, dv = M.velocity_term(v, 1.3)
        assert abs(term - ref.item()) < 1e-13 * abs(ref.item()) and rel(dv, vt.grad.numpy()) < 1e-13


def test_regularisers_and_keypoint_chain_equal_autograd():
    rng = np.random.default_rng(6)
    B = 4
    t, t0 = rng.normal(0, 1, (B, 3)), rng.normal(0, 1, (B, 3))
    tt = torch.tensor(t, requires_grad=True)
    ref = ((tt - torch.tensor(t0)) ** 2).mean(); (2.5 * ref).backward()
    term, g = M.trans_reg(t, t0, 2.5)
    assert abs(term - ref.item()) < 1e-14 and rel(g, tt.grad.numpy()) < 1e-13
    pose, init, mean, P = rng.normal(0, 0.3, (B, 156)), rng.normal(0, 0.3, (B, 156)), rng.normal(0, 0.1, 63), np.tril(rng.normal(0, 1, (63, 63)))
    pt = torch.tensor(pose, requires_grad=True)
    y = (pt[:, 3:66] - torch.tensor(mean)) @ torch.tensor(P)
    prior = (y * y).sum(1).mean()
    pin = ((pt[:, 3:72] - torch.tensor(init)[:, 3:72]) ** 2).sum(1).mean()
    (3.0 * prior + 0.4 * pin).backward()
    tp, gp = M.body_prior(pose, mean, P, 3.0 / B); ti, gi = M.pinit_term(pose, init, 0.4)
    assert abs(tp - prior.item()) < 1e-12 * prior.item() and abs(ti - pin.item()) < 1e-12 * pin.item()
    assert rel(gp + gi, pt.grad.numpy()) < 1e-12
    K, V = 7, 50
    A = rng.uniform(0, 1, (K, V)) * (rng.uniform(0, 1, (K, V)) < 0.3)
    verts = rng.normal(0, 0.3, (B, V, 3)) + [0, 0, 2.2]
    k2 = np.concatenate([rng.uniform(0, 2000, (B, K, 2)), rng.uniform(0, 1, (B, K, 1))], -1); cc = rng.uniform(900, 1100, (B, 2))
    cam = np.array([979.7844, 979.840, 1018.952, 779.486, 1200.0])
    for mode in (0, 1):
        vt = torch.tensor(verts, requires_grad=True)
        J = torch.einsum("kv,bvc->bkc", torch.tensor(A), vt)
        px = cam[0] * J[..., 0] / J[..., 2] + cam[2]; py = cam[1] * J[..., 1] / J[..., 2] + cam[3]
        if mode == 1:
            px = (600 + px - torch.tensor(cc[:, :1])) * (512 / 1200); py = (600 + py - torch.tensor(cc[:, 1:])) * (512 / 1200)
        e = ((px - torch.tensor(k2[..., 0])) ** 2 + (py - torch.tensor(k2[..., 1])) ** 2) * torch.tensor(k2[..., 2])
        ref = e.sum() / (B * K * 2) if mode == 0 else e.mean()
        (0.7 * ref).backward()
        Jm, term, dverts = M.kpts_chain(A, verts, k2, cc, mode, cam, 512.0, 0.7)
        assert rel(Jm, J.detach().numpy()) < 1e-13 and abs(term - ref.item()) < 1e-12 * ref.item() and rel(dverts, vt.grad.numpy()) < 1e-12
    ip = np.array([0, 2, 2, 5]); ix = np.array([1, 3, 0, 3, 3]); da = np.array([.5, .5, .2, .3, .5])
    D = M.csr_dense(ip, ix, da, 3, 4)
    assert np.array_equal(D, [[0, .5, 0, .5], [0, 0, 0, 0], [.2, 0, 0, .8]])


@pytest.mark.parametrize("steps", [1, 2, 5])
def test_adam_equals_torch_optim_adam(steps):
    rng = np.random.default_rng(7)
    p0 = rng.normal(0, 1, (7, 5)); grads = rng.normal(0, 1, (steps, 7, 5)) + 0.5
    pt = torch.tensor(p0.copy(), requires_grad=True)
    opt = torch.optim.Adam([pt], lr=0.006)
    p, m, v = p0, np.zeros_like(p0), np.zeros_like(p0)
    for k in range(steps):
        pt.grad = torch.tensor(grads[k]); opt.step()
        p, m, v = M.adam(p, grads[k], m, v, k + 1, 0.006)
        assert np.abs(p - pt.detach().numpy()).max() < 1e-15
    st = opt.state[pt]
    assert rel(m, st["exp_avg"].numpy()) < 1e-15 and rel(v, st["exp_avg_sq"].numpy()) < 1e-15
    with pytest.raises(AssertionError):
        M.adam(p0, np.zeros_like(p0), np.zeros_like(p0), np.zeros_like(p0), 1, 0.006)      # sqrt(v) below the conditioning floor is refused
    mm, vv = M.adam_moments(rng, rng.normal(0, 1, (96, 9)) * 1e-4)
    assert np.sqrt(vv).min() >= 5 * M.ADAM_MIN_SQRT_V


def test_close_step_rule_and_loss_order():
    w = np.array([1.0, 0.5, 3.0, 0.25], np.float32); terms = np.array([0.3, 1e-9, 2.0, 7.0])
    fused, plain = M.weighted_loss(terms, w)
    assert fused == plain == np.float32(0.3 + 0.5e-9 + 6.0 + 1.75)
    loss, stop, ratio = M.close_step(terms, w, np.inf, 1e-3, 1)
    assert not stop and loss == plain
    prev = float(loss) * 1.00001
    assert M.close_step(terms, w, prev, 1e-3, 1)[1] and not M.close_step(terms, w, prev, 1e-3, 0)[1]
    assert not M.close_step(terms, w, float(loss) * 1.5, 1e-3, 1)[1]
    # the rule compares with prev * tol, not with tol: a loss of 100 stops at a relative change below 0.1, a loss of 0.01 only below 1e-5
    assert M.close_step([100.0], [1.0], 105.0, 1e-3, 1)[1] and not M.close_step([0.01], [1.0], 0.0100005, 1e-3, 1)[1]


def test_fp32_switch_evaluates_the_same_expression():
    rng = np.random.default_rng(8)
    v = rng.normal(0, 1, (6, 40)).astype(np.float32)
    for f in (lambda q: M.accel_term(v, 1.0, None, q), lambda q: M.velocity_term(v, 1.0, q)):
        (t64, g64), (t32, g32) = f(False), f(True)
        assert g32.dtype == np.float32 and g64.dtype == np.float64 and 0 < rel(g32, g64) < 1e-5 and abs(t32 - t64) < 1e-5 * t64
    M0, noise, _, _ = M.so3_inputs(M.SO3_SEEDS[0], 12)
    a, b = M.project_so3(M0, noise, True)["R"], M.project_so3(M0, noise)["R"]
    assert a.dtype == np.float32 and np.abs(a - b).max() < 3e-6
