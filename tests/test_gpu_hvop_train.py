"""GPU: vistracker_amd.infill_training against the float64 model of tests/former_model.py and the reference's recorded autograd (tests/golden/former.npz,
tools/gen_golden_former.py), 4 e32 per tensor: a 2-layer TrainableTransformerV2 with its final norm, the whole TrainableConditionalMInfiller with both motion
losses and every parameter gradient, state_dict / export(), and HVOPTrainer (20 Adam steps against the float64 model stepping the same steps).
e32 = the model's float32 run against its float64 run.  Measured figures: tests/golden/former.md."""
import numpy as np
import pytest
import torch

import former_cases as FC
import former_model as FM
from conftest import golden

pytestmark = pytest.mark.gpu
WIDTHS = (128, 32, 160)


def tables(T):
    """{D: position table}: the reference builds it in float32 whatever the model's dtype (posi_embed.py:37-66), so the float64 and the float32 run of the
    model see the same table, the one infill.position_embedding_sine_1d mirrors"""
    from vistracker_amd import infill
    p = {D: infill.position_embedding_sine_1d(T, D // 2, D).numpy().astype(np.float64) for D in WIDTHS}
    return p, p


def gate(what, got, truth, e32, pick=None):
    bad, worst = [], (0.0, "")
    for k, t in truth.items():
        g = got[k].detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got[k]) else np.asarray(got[k], dtype=np.float64)
        g = g if pick is None or k not in pick else g.ravel()[pick[k]]
        err = float(np.abs(g - t).max())
        r = err / e32[k] if e32[k] > 0 else (0.0 if err == 0 else np.inf)
        worst = max(worst, (r, k))
        if not err <= 4 * e32[k]:
            bad.append((k, err, e32[k]))
    print(f"\n[{what}] worst ratio {worst[0]:.2f} ({worst[1]}) over {len(truth)} tensors", end="")
    assert not bad, bad


def test_two_layer_stack_against_the_model_and_the_reference():
    from vistracker_amd import infill, infill_training as IT
    g = golden("former")
    B, T, D, H, Fd = 2, 20, 32, 2, 64
    sd = {k[6:]: g[k] for k in g if k.startswith("tv2_w/")}
    Ps = [{k: sd[f"encoder.layers.{i}.{k}"] for k in FM.PARAM_KEYS} for i in range(2)]
    norm = (sd["encoder.norm.weight"], sd["encoder.norm.bias"])
    x, dy, m = g["tv2_x"], g["tv2_dy"], g["tv2_mask"]
    runs = {}
    for dt, pos in ((np.float64, tables(T)[0][D]), (np.float32, tables(T)[0][D])):
        y, saved = FM.stack_forward(Ps, norm, x, pos, m, H, "gelu", dt=dt)
        r = FM.stack_backward(Ps, norm, saved, dy); r["y"] = y
        runs[dt] = {k: np.asarray(v, dtype=np.float64) for k, v in r.items()}
    e32 = {k: float(np.abs(runs[np.float32][k] - runs[np.float64][k]).max()) for k in runs[np.float64]}
    net = IT.TrainableTransformerV2.from_state_dict({"enc." + k: v for k, v in sd.items()}, "enc.", 2, D, H, Fd, "gelu", True, dropout=0.05).eval()
    xt = torch.tensor(x, dtype=torch.float32, device="cuda", requires_grad=True)
    y = net(xt, torch.tensor(m, device="cuda"))
    (y * torch.tensor(dy, dtype=torch.float32, device="cuda")).sum().backward()
    got = {k: p.grad for k, p in net.named_parameters()}
    got["y"], got["d_x"] = y.detach(), xt.grad
    assert set(got) == set(e32)
    gate("stack against the model", got, runs[np.float64], e32)
    ref = {k[6:]: g[k] for k in g if k.startswith("tv2_g/")}
    ref["y"], ref["d_x"] = g["tv2_y"], g["tv2_dx"]
    assert set(ref) == set(e32)
    gate("stack against the reference's autograd", got, ref, e32)


@pytest.fixture(scope="module")
def weights():
    return FC.seeded_weights(golden("infill"), 31)


def test_infiller_gradients_against_the_model_and_the_reference(weights):
    """prediction, both motion losses and every parameter gradient of the whole network at B = 2, T = 20, per tensor"""
    from vistracker_amd import infill_training as IT
    g = golden("former")
    batch = {k: g["cmf_" + k] for k in ("data_smpl", "mask_smpl", "data_obj", "mask_obj", "gt_obj")}
    opt = FC.hvop_opt(0.0)
    p64, p32 = tables(20)
    r64, r32 = FM.infiller_run(weights, opt, batch, p64), FM.infiller_run(weights, opt, batch, p32, np.float32)
    e32 = {k: float(np.abs(r32[k] - r64[k]).max()) for k in r64}
    net = IT.TrainableConditionalMInfiller.from_state_dict(weights, opt, dropout=0.0).train()
    tb = {k: torch.tensor(v, device="cuda") for k, v in batch.items()}
    pred = net(tb["data_smpl"], tb["mask_smpl"], tb["data_obj"], tb["mask_obj"], seed=1)
    la, lp = IT.motion_losses(tb["gt_obj"], pred)
    (la + lp).backward()
    got = {k: p.grad for k, p in net.named_parameters()}
    got.update(pred=pred.detach(), loss_accel=la.detach(), loss_pos=lp.detach())
    assert set(got) == set(r64)
    gate("infiller against the model", got, r64, e32)
    # the reference's recorded autograd: prediction and losses whole, of each gradient the recorded elements, its sum and its largest magnitude
    names = [k[6:] for k in g if k.startswith("cmf_g/")]
    assert sorted(names) == sorted(k for k in r64 if k not in ("pred", "loss_accel", "loss_pos"))
    ref = {k: g["cmf_g/" + k] for k in names}
    ref.update(pred=g["cmf_pred"], loss_accel=g["cmf_loss_accel"], loss_pos=g["cmf_loss_pos"])
    gate("infiller against the reference's autograd", got, ref, e32, pick={k: g["cmf_i/" + k] for k in names})
    for k in names:
        gk = got[k].cpu().numpy().astype(np.float64)
        assert abs(np.abs(gk).max() - g["cmf_s/" + k][1]) <= 4 * e32[k], k
        assert abs(gk.sum() - g["cmf_s/" + k][0]) <= 4 * e32[k] * gk.size, k


def test_state_dict_keys_shapes_and_reload(weights):
    from vistracker_amd import infill_training as IT
    g = golden("infill")
    net = IT.TrainableConditionalMInfiller.from_state_dict({"module." + k: v for k, v in weights.items()}, FC.hvop_opt())
    sd = net.state_dict()
    assert list(sd) == [str(n) for n in g["names"]]
    assert [tuple(v.shape) for v in sd.values()] == [tuple(int(x) for x in s[:d]) for s, d in zip(g["shapes"], g["ndims"])]
    again = IT.TrainableConditionalMInfiller.from_state_dict(sd, FC.hvop_opt()).state_dict()
    assert all(torch.equal(sd[k], again[k]) and torch.equal(sd[k].cpu(), torch.tensor(weights[k])) for k in sd)


def test_export_agrees_with_the_trainable_forward(weights):
    """one clip of 180 frames: the trainable forward in eval mode, the exported inference path (library GEMMs) and the float64 model; 4 e32 of the model"""
    from vistracker_amd import infill_training as IT
    opt = FC.hvop_opt()
    batch = FC.hvop_batch(1, 180, 5)
    p64, p32 = tables(180)
    ref64 = FM.infiller_forward(weights, opt, batch, p64)[0]
    e32 = float(np.abs(FM.infiller_forward(weights, opt, batch, p32, np.float32)[0].astype(np.float64) - ref64).max())
    net = IT.TrainableConditionalMInfiller.from_state_dict(weights, opt).eval()
    b = {k: torch.tensor(v, device="cuda") for k, v in batch.items()}
    with torch.no_grad():
        mine = net(b["data_smpl"], b["mask_smpl"], b["data_obj"], b["mask_obj"])
    theirs = net.export()(b["data_smpl"], b["mask_smpl"], b["data_obj"], b["mask_obj"])
    e_mine, e_theirs = float(np.abs(mine.cpu().numpy() - ref64).max()), float(np.abs(theirs.cpu().numpy() - ref64).max())
    between = float((mine - theirs).abs().max())
    print(f"\n[export] e32 {e32:.3e} | trainable forward {e_mine:.3e} ({e_mine / e32:.2f}) | exported {e_theirs:.3e} ({e_theirs / e32:.2f}) | between them {between:.3e} "
          f"({between / e32:.2f})", end="")
    assert e_mine <= 4 * e32 and e_theirs <= 4 * e32 and between <= 4 * e32


def test_trainer_follows_the_float64_model_without_host_waits(weights, monkeypatch):
    """20 Adam steps on one fixed batch (B = 4, T = 32, p = 0, the trainer's default lr): the objective after them against the float64 model stepping the same
    steps, within 8 x the deviation of the model's own float32 run.  The widths are the configuration's: the joint encoder has one head, and a head width other
    than 16 / 32 / 160 is outside the kernels' contract."""
    from vistracker_amd import infill_training as IT
    opt = FC.hvop_opt(0.0)
    nb = FC.hvop_batch(4, 32, 11)
    p64, p32 = tables(32)
    t64, t32 = FM.adam_trajectory(weights, opt, nb, p64, 21, 1e-4), FM.adam_trajectory(weights, opt, nb, p32, 21, 1e-4, np.float32)
    batch = {k: torch.tensor(v, device="cuda") for k, v in nb.items()}
    tr = IT.HVOPTrainer(weights, opt, dropout=0.0)
    traj = [float(x) for x in [tr.train_step(batch, seed=s)[0] for s in range(21)]]
    for name, t in (("float64 model", t64), ("float32 model", t32), ("HVOPTrainer", traj)):
        print(f"\n[trainer] {name:>13}: " + " ".join(f"{v:.6f}" for v in t), end="")
    dev32, dev = abs(t32[-1] - t64[-1]), abs(traj[-1] - t64[-1])
    print(f"\n[trainer] after 20 steps: float32 model deviates {dev32:.3e}, HVOPTrainer {dev:.3e} ({dev / dev32 if dev32 > 0 else 0.0:.2f}; gate 8)", end="")
    assert np.isfinite(traj).all() and traj[-1] < traj[0]
    assert dev <= 8 * dev32, (dev, dev32)
    assert tr.set_step(0) == 1e-4 and abs(tr.set_step(35) - 1e-5) < 1e-12 and abs(tr.set_step(40) - 1e-6) < 1e-13
    tr.set_step(0)

    def barred(*a, **k):
        raise AssertionError("host wait inside train_step")
    with monkeypatch.context() as mp:
        for name in ("cpu", "numpy", "item", "tolist"):
            mp.setattr(torch.Tensor, name, barred)
        mp.setattr(torch.cuda, "synchronize", barred)
        loss, sep = tr.train_step(batch, seed=1)
    assert loss.is_cuda and sep.shape == (2,) and bool(torch.isfinite(loss))


def test_trainer_dropout_is_a_function_of_the_seed(weights):
    from vistracker_amd import infill_training as IT
    batch = {k: torch.tensor(v, device="cuda") for k, v in FC.hvop_batch(4, 32, 11).items()}
    outs = []
    for seed in (5, 5, 6):
        t2 = IT.HVOPTrainer(weights, FC.hvop_opt(), dropout=0.05)
        t2.train_step(batch, seed=seed)
        outs.append(t2.state_dict())
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0])
    assert any(not torch.equal(outs[0][k], outs[2][k]) for k in outs[0])
