"""CPU: tests/infillhead_model.py against tests/former_model.py on the whole network, against torch float64 autograd, and the conditions its cases must meet
for tests/test_gpu_infillhead.py to mean what it says: every mutant fails the GPU gates on the GPU cases, no hidden pre-activation sits on the activation's
kink, the planted zeros are exact zeros, the float32-ordered stencil does flip signs in the flip case, and the fp64 differences are the exact ones."""
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import former_cases as FC
import former_model as FM
import infillhead_model as IM
from conftest import golden

REL = 5e-15


def close(a, b, rel=REL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) <= rel * max(float(np.abs(b).max()), 1e-300)


def test_model_equals_former_model_on_the_whole_network():
    g = golden("former")
    batch = {k: g["cmf_" + k] for k in ("data_smpl", "mask_smpl", "data_obj", "mask_obj", "gt_obj")}
    opt, sd = FC.hvop_opt(0.0), FC.seeded_weights(golden("infill"), 31)
    pos = {D: FM.position_table(20, D) for D in (128, 32, 160)}
    pred, C = FM.infiller_forward(sd, opt, batch, pos)
    la, lp, d = FM.motion_losses(batch["gt_obj"], pred)
    ref = FM.infiller_backward(sd, opt, C, d)
    f = C["head"][0][0]
    P = {k: sd[k] for k in IM.HEAD_KEYS}
    mine, h = IM.head_forward(P, f)
    assert close(mine, pred) and close(h, C["head"][0][1])
    mlp, mla, md = IM.objective(pred, batch["gt_obj"])
    assert close(mlp, lp) and close(mla, la) and close(md, d)
    gh = IM.head_backward(P, f, h, md)
    for k in IM.HEAD_KEYS:
        assert close(gh[k], ref[k]), k
    # d_f through the model's encoders down to the projections' outputs, then the projection gradients
    Ps, norm = FM._enc_params(sd, "encoder_joint.", opt.num_layers_joint, opt.pre_norm_joint)
    dx = FM.stack_backward(Ps, norm, C["enc"]["joint"], gh["d_f"])["d_x"]
    for tag, dd in (("smpl", dx[..., :opt.d_model_smpl]), ("obj", dx[..., opt.d_model_smpl:])):
        Ps, norm = FM._enc_params(sd, f"encoder_{tag}.", getattr(opt, f"num_layers_{tag}"), getattr(opt, f"pre_norm_{tag}"))
        dy = FM.stack_backward(Ps, norm, C["enc"][tag], dd)["d_x"]
        dW, db = IM.proj_backward(dy, C["in"][tag])
        assert close(dW, ref[f"feat_proj_{tag}.weight"]) and close(db, ref[f"feat_proj_{tag}.bias"]), tag
        y = IM.proj_forward(C["in"][tag], sd[f"feat_proj_{tag}.weight"], sd[f"feat_proj_{tag}.bias"])
        assert close(y, C["enc"][tag][0][0]["x"]), tag


@pytest.mark.parametrize("c", IM.head_cases()[1:3] + IM.head_cases()[5:], ids=lambda c: c["id"])
def test_model_equals_torch_float64_autograd(c):
    b = IM.build_head(c)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)      # noqa: E731
    f, ps = t(b["f"]), [t(b["P"][k]) for k in IM.HEAD_KEYS]
    pred = F.linear(F.leaky_relu(F.linear(f, ps[0], ps[1])), ps[2], ps[3])
    pred.backward(torch.tensor(b["d_pred"]))
    assert close(pred.detach().numpy(), b["r64"]["pred"]) and close(f.grad.numpy(), b["r64"]["d_f"])
    for k, q in zip(IM.HEAD_KEYS, ps):
        assert close(q.grad.numpy(), b["r64"][k]), k
    # the objective: l1_loss twice, as trainer_infiller.py:33-47 composes it
    o = IM.build_objective(IM.objective_cases()[1])
    p, gt = t(o["pred"]), torch.tensor(o["gt"].astype(np.float64))
    acc = lambda a: a[:, :-2] - 2 * a[:, 1:-1] + a[:, 2:]                                   # noqa: E731
    lp, la = F.l1_loss(p, gt) * 1.0, F.l1_loss(acc(p), acc(gt)) * 0.1
    (lp + la).backward()
    assert close(float(lp.detach()), o["loss_pos"]) and close(float(la.detach()), o["loss_accel"]) and close(p.grad.numpy(), o["d_pred"])
    # a projection with a ragged Kin
    q = IM.build_proj(IM.proj_cases()[1])["p"][0]
    x, W, bb = torch.tensor(q["x"]), t(q["W"]), t(q["b"])
    y = F.linear(x, W, bb)
    y.backward(torch.tensor(q["dy"]))
    assert close(y.detach().numpy(), q["r64"]["y"]) and close(W.grad.numpy(), q["r64"]["dW"]) and close(bb.grad.numpy(), q["r64"]["db"])


def objective_gate(got_lp, got_la, got_d, b):
    """the GPU test's gate of the isolated objective: d_pred bit for bit as float32, the two terms to len x 2^-53 relative"""
    B, T, C = b["B"], b["T"], b["C"]
    bad = []
    if not np.array_equal(np.asarray(got_d).astype(np.float32), b["d_pred"].astype(np.float32)):
        bad.append("d_pred")
    if not abs(got_lp - b["loss_pos"]) <= B * T * C * 2.0 ** -53 * abs(b["loss_pos"]):
        bad.append("loss_pos")
    if not abs(got_la - b["loss_accel"]) <= B * (T - 2) * C * 2.0 ** -53 * abs(b["loss_accel"]):
        bad.append("loss_accel")
    return bad


def mutant_caught(mut):
    hit = []
    for c in IM.objective_cases():
        b = IM.build_objective(c)
        hit += [(c["id"], x) for x in objective_gate(*IM.objective(b["pred"], b["gt"], mut=mut), b)]
    for c in IM.head_cases():
        b = IM.build_head(c)
        hit += [(c["id"], k) for k in IM.failures(IM.head_run(b["P"], b["f"], b["d_pred"], mut=mut), b["r64"], b["e32"])]
    for c in IM.proj_cases():
        for q in IM.build_proj(c)["p"]:
            hit += [(c["id"], k) for k in IM.failures(IM.proj_run(q["x"], q["W"], q["b"], q["dy"], mut=mut), q["r64"], q["e32"])]
    return hit


def test_the_unmutated_model_passes_its_own_gates():
    assert IM.MUTANTS == ("sign0_is_one", "accel_mean_over_T", "stencil_crosses_clips", "leaky_ge", "bias_grad_dropped", "accel_in_fp32_order")
    assert mutant_caught(None) == []


@pytest.mark.parametrize("mut", IM.MUTANTS)
def test_every_mutant_fails_the_gpu_gates_on_the_gpu_cases(mut):
    hit = mutant_caught(mut)
    print(f"\n[{mut}] caught at {hit[:4]}", end="")
    assert hit, mut
    if mut == "accel_in_fp32_order":
        assert ("B2-T33-C9-flip", "d_pred") in hit
    if mut == "leaky_ge":
        assert all(k in (IM.HEAD_KEYS[1], "d_f", IM.HEAD_KEYS[0]) for _, k in hit)       # only through the planted zero: its frame of f is 0, so dW1 cannot see it


def test_case_conditions():
    for c in IM.head_cases():
        m = IM.kink_margin(c)
        print(f"\n[kink] {c['id']}: the nearest pre-activation is {m:.1f} e32(h) from 0", end="")
        assert m > 64, (c["id"], m)
        assert IM.build_head(c)["r64"]["h"][IM.ZERO] == 0
    assert sorted({(c["B"], c["T"]) for c in IM.head_cases()}) == sorted(IM.BT) == sorted({(c["B"], c["T"]) for c in IM.proj_cases()})
    z = IM.build_objective(IM.objective_cases()[5])
    p, g = z["pred"].astype(np.float64), z["gt"].astype(np.float64)
    assert z["kind"] == "zeros" and (p == g).sum() >= 5 and ((IM._acc(p) - IM._acc(g)) == 0).sum() >= 1
    fl = IM.build_objective(IM.objective_cases()[6])
    p, g = fl["pred"], fl["gt"]
    exact = IM._acc(p.astype(np.float64)) - IM._acc(g.astype(np.float64))
    ordered = (IM._acc(p) - IM._acc(g)).astype(np.float64)
    assert p.dtype == np.float32 and ordered.dtype == np.float64
    opposite = int((np.sign(exact) * np.sign(ordered) < 0).sum())
    print(f"\n[flip] {opposite} of {exact.size} float32-ordered second-difference errors have the opposite sign of the exact one", end="")
    assert fl["kind"] == "flip" and opposite >= 1


def test_fp64_differences_are_the_rational_values():
    """pred - gt and the six-term stencil of float32 values in float64 against fractions.Fraction, on a sample of every objective case"""
    fr = lambda v: Fraction(float(v))                                                      # noqa: E731
    for c in IM.objective_cases():
        b = IM.build_objective(c)
        p, g = b["pred"], b["gt"]
        p64, g64 = p.astype(np.float64), g.astype(np.float64)
        e, ea = p64 - g64, IM._acc(p64) - IM._acc(g64)
        r = np.random.RandomState(7)
        for _ in range(64):
            i, t, k = r.randint(c["B"]), r.randint(c["T"] - 2), r.randint(c["C"])
            assert Fraction(float(e[i, t, k])) == fr(p[i, t, k]) - fr(g[i, t, k])
            exact = (fr(p[i, t, k]) - 2 * fr(p[i, t + 1, k]) + fr(p[i, t + 2, k])) - (fr(g[i, t, k]) - 2 * fr(g[i, t + 1, k]) + fr(g[i, t + 2, k]))
            assert Fraction(float(ea[i, t, k])) == exact
