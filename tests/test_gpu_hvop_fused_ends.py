"""GPU: HVOP-Net's training step with ``fused_ends=True`` -- projections, predictor and objective from csrc/infillhead.hip -- against the float64 model of
tests/former_model.py and the reference's recorded autograd (tests/golden/former.npz), 4 e32 per tensor as tests/test_gpu_hvop_train.py gates the torch-composed
step; the trainer's 20 Adam steps, seeds, epoch loop and validation; the route a configuration outside the kernels' contract takes; the option off.
e32 = the model's float32 run against its float64 run."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import clipdata_cases as CC
import former_cases as FC
import former_model as FM
from conftest import golden

pytestmark = pytest.mark.gpu
WIDTHS = (128, 32, 160)
DEV = "cuda:0"


def tables(T):
    """{D: position table}: the float32-built table of infill.position_embedding_sine_1d for both runs of the model, as tests/test_gpu_hvop_train.py takes it"""
    from vistracker_amd import infill
    return {D: infill.position_embedding_sine_1d(T, D // 2, D).numpy().astype(np.float64) for D in WIDTHS}


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


@pytest.fixture(scope="module")
def weights():
    return FC.seeded_weights(golden("infill"), 31)


LOSSES = ("loss_pos", "loss_accel")


def run_fused(weights, opt, batch, T, lw=(1.0, 0.1), want_route="hip"):
    """-> (the GPU's tensors, the float64 model's, e32) of one objective and its gradients with fused_ends=True"""
    from vistracker_amd import infill_training as IT
    p = tables(T)
    r64, r32 = FM.infiller_run(weights, opt, batch, p, lw=lw), FM.infiller_run(weights, opt, batch, p, np.float32, lw=lw)
    e32 = {k: float(np.abs(r32[k] - r64[k]).max()) for k in r64}
    net = IT.TrainableConditionalMInfiller.from_state_dict(weights, opt, dropout=0.0, fused_ends=True).train()
    assert net.ends_route == want_route if want_route == "hip" else net.ends_route.startswith("torch: "), net.ends_route
    tb = {k: torch.tensor(v, device=DEV) for k, v in batch.items()}
    loss, lp, la, pred = net.loss(tb, seed=1, lw=lw)
    assert loss.dtype == torch.float32 and lp.dtype == torch.float32 and loss.is_cuda
    loss.backward()
    got = {k: q.grad for k, q in net.named_parameters()}
    got.update(pred=pred.detach(), loss_accel=la.detach(), loss_pos=lp.detach())
    assert set(got) == set(r64)
    return got, r64, e32, net, tb


def check_away_from_the_kinks(r64, e32, gt):
    """the float64 model's L1 arguments against 64 e32[pred]: the sign of none of them is in doubt in a float32 run"""
    e = r64["pred"] - np.asarray(gt, dtype=np.float64)
    ea = e[:, :-2] - 2 * e[:, 1:-1] + e[:, 2:]
    m = min(float(np.abs(e).min()), float(np.abs(ea).min())) / e32["pred"]
    print(f"\n[kinks] the smallest |pred - gt| or |acc diff| is {m:.0f} e32[pred] from 0", end="")
    assert m > 64, m


def check_losses(got, r64, e32, lw):
    """an L1 mean is 1-Lipschitz in the max-norm of pred and the stencil has norm 4: lw_pose 4 e32[pred] and lw_accel 16 e32[pred]"""
    for k, bound in (("loss_pos", lw[0] * 4 * e32["pred"]), ("loss_accel", lw[1] * 16 * e32["pred"])):
        err = abs(float(got[k]) - float(r64[k]))
        print(f"\n[{k}] off by {err:.3e}: {err / bound:.3f} of the bound {bound:.3e}, {err / e32[k] if e32[k] > 0 else float('nan'):.2f} e32[{k}] (ungated)", end="")
        assert err <= bound, (k, err, bound)


def test_fused_ends_against_the_model_and_the_reference(weights):
    """pred and all 104 gradients at B = 2, T = 20 per tensor; the losses within the bounds derived from e32[pred]"""
    g = golden("former")
    batch = {k: g["cmf_" + k] for k in ("data_smpl", "mask_smpl", "data_obj", "mask_obj", "gt_obj")}
    got, r64, e32, _, _ = run_fused(weights, FC.hvop_opt(0.0), batch, 20)
    check_away_from_the_kinks(r64, e32, batch["gt_obj"])
    tensors = {k: v for k, v in r64.items() if k not in LOSSES}
    assert len(tensors) == 105
    gate("fused ends against the model", got, tensors, e32)
    check_losses(got, r64, e32, (1.0, 0.1))
    names = [k[6:] for k in g if k.startswith("cmf_g/")]
    assert sorted(names) == sorted(k for k in tensors if k != "pred")
    ref = {k: g["cmf_g/" + k] for k in names}
    ref["pred"] = g["cmf_pred"]
    gate("fused ends against the reference's autograd", got, ref, e32, pick={k: g["cmf_i/" + k] for k in names})
    check_losses(got, dict(loss_pos=g["cmf_loss_pos"], loss_accel=g["cmf_loss_accel"]), e32, (1.0, 0.1))
    for k in names:
        gk = got[k].cpu().numpy().astype(np.float64)
        assert abs(np.abs(gk).max() - g["cmf_s/" + k][1]) <= 4 * e32[k], k
        assert abs(gk.sum() - g["cmf_s/" + k][0]) <= 4 * e32[k] * gk.size, k


def nine_d(weights, seed=32):
    """the '9d' object representation (6D | translation: dim_obj = out_dim = 9): the three tensors whose shape depends on it are seeded anew"""
    opt = SimpleNamespace(**{**vars(FC.hvop_opt(0.0)), "obj_repre": "9d", "dim_obj": 9, "out_dim": 9})
    r = np.random.default_rng(seed)
    sd = dict(weights)
    sd["feat_proj_obj.weight"] = r.normal(0, 1 / 3.0, (32, 9)).astype(np.float32)
    sd["predictor.2.weight"] = r.normal(0, 1 / np.sqrt(32), (9, 32)).astype(np.float32)
    sd["predictor.2.bias"] = (0.02 * r.normal(size=9)).astype(np.float32)
    g = golden("former")
    batch = {k: g["cmf_" + k] for k in ("data_smpl", "mask_smpl", "mask_obj")}
    t = np.linspace(0, 1, 20)[None, :, None]
    gt = (0.5 * np.sin(2 * np.pi * (t * r.uniform(0.5, 2, (2, 1, 9)) + r.uniform(0, 1, (2, 1, 9)))) + 0.02 * r.normal(size=(2, 20, 9))).astype(np.float32)
    batch["gt_obj"] = gt
    batch["data_obj"] = np.where(np.asarray(batch["mask_obj"]).astype(bool)[..., None], np.float32(0), gt)
    return sd, opt, batch


def test_fused_ends_at_9d_against_the_model(weights):
    """dim_obj = out_dim = 9 against the float64 model only: there is no recording of the reference at '9d'"""
    sd, opt, batch = nine_d(weights)
    got, r64, e32, _, _ = run_fused(sd, opt, batch, 20)
    check_away_from_the_kinks(r64, e32, batch["gt_obj"])
    gate("fused ends, 9d", got, {k: v for k, v in r64.items() if k not in LOSSES}, e32)
    check_losses(got, r64, e32, (1.0, 0.1))


def test_two_hidden_layers_take_the_torch_route_and_still_match(weights):
    opt = SimpleNamespace(**{**vars(FC.hvop_opt(0.0)), "hidden_dims": [32, 32]})
    r = np.random.default_rng(33)
    sd = {k: v for k, v in weights.items() if not k.startswith("predictor.2.")}
    sd["predictor.2.weight"] = r.normal(0, 1 / np.sqrt(32), (32, 32)).astype(np.float32)
    sd["predictor.2.bias"] = (0.02 * r.normal(size=32)).astype(np.float32)
    sd["predictor.4.weight"], sd["predictor.4.bias"] = weights["predictor.2.weight"], weights["predictor.2.bias"]
    g = golden("former")
    batch = {k: g["cmf_" + k] for k in ("data_smpl", "mask_smpl", "data_obj", "mask_obj", "gt_obj")}
    got, r64, e32, net, _ = run_fused(sd, opt, batch, 20, want_route="torch")
    assert "hidden" in net.ends_route
    gate("two hidden layers, torch route", got, r64, e32)


def test_trainer_with_fused_ends_follows_the_float64_model_without_host_waits(weights, monkeypatch):
    """20 Adam steps at B = 4, T = 32, p = 0 within 8 x the float32 model's own deviation, as the torch-composed trainer is held to; one step with host waits barred"""
    from vistracker_amd import infill_training as IT
    opt = FC.hvop_opt(0.0)
    nb = FC.hvop_batch(4, 32, 11)
    p = tables(32)
    t64, t32 = FM.adam_trajectory(weights, opt, nb, p, 21, 1e-4), FM.adam_trajectory(weights, opt, nb, p, 21, 1e-4, np.float32)
    batch = {k: torch.tensor(v, device=DEV) for k, v in nb.items()}
    tr = IT.HVOPTrainer(weights, opt, dropout=0.0, fused_ends=True)
    assert tr.model.ends_route == "hip"
    traj = [float(x) for x in [tr.train_step(batch, seed=s)[0] for s in range(21)]]
    dev32, dev = abs(t32[-1] - t64[-1]), abs(traj[-1] - t64[-1])
    print(f"\n[trainer, fused ends] after 20 steps: float32 model deviates {dev32:.3e}, HVOPTrainer {dev:.3e} ({dev / dev32 if dev32 > 0 else 0.0:.2f}; gate 8)", end="")
    assert np.isfinite(traj).all() and traj[-1] < traj[0]
    assert dev <= 8 * dev32, (dev, dev32)

    def barred(*a, **k):
        raise AssertionError("host wait inside train_step")
    with monkeypatch.context() as mp:
        for name in ("cpu", "numpy", "item", "tolist"):
            mp.setattr(torch.Tensor, name, barred)
        mp.setattr(torch.cuda, "synchronize", barred)
        loss, sep = tr.train_step(batch, seed=1)
    assert loss.is_cuda and loss.dtype == torch.float32 and sep.shape == (2,) and sep.dtype == torch.float32 and bool(torch.isfinite(loss))


def test_fused_trainer_is_a_function_of_the_seed_and_off_is_the_old_step(weights):
    from vistracker_amd import infill_training as IT
    batch = {k: torch.tensor(v, device=DEV) for k, v in FC.hvop_batch(4, 32, 11).items()}
    outs = []
    for seed in (5, 5, 6):
        t2 = IT.HVOPTrainer(weights, FC.hvop_opt(), dropout=0.05, fused_ends=True)
        t2.train_step(batch, seed=seed)
        outs.append(t2.state_dict())
    assert all(torch.equal(outs[0][k], outs[1][k]) for k in outs[0])
    assert any(not torch.equal(outs[0][k], outs[2][k]) for k in outs[0])
    res = []
    for kw in ({}, dict(fused_ends=False)):
        t3 = IT.HVOPTrainer(weights, FC.hvop_opt(), dropout=0.05, **kw)
        assert t3.model.ends_route.startswith("torch: ")
        res.append((t3.train_step(batch, seed=5), t3.state_dict()))
    assert torch.equal(res[0][0][0], res[1][0][0]) and torch.equal(res[0][0][1], res[1][0][1]) and all(torch.equal(res[0][1][k], res[1][1][k]) for k in res[0][1])


def small_set():
    """8 clips of 20 frames"""
    from vistracker_amd.infill_data import HVOPClipData
    seqs, names = CC.sequences()
    d = HVOPClipData.from_packed(seqs, names, 20, 56, start_fr_min=2, start_fr_max=12, min_drop_len=3, max_drop_len=8, obj_repre="6d", aug_num=4, multi_kinects=True,
                                 kinect=CC.kinect(), device=DEV)
    assert d.num_clips == 8
    return d


def test_fused_train_epoch_is_the_hand_written_loop_and_validate_the_mean(weights):
    from vistracker_amd import infill_training as IT
    from vistracker_amd.training import distributed_indices
    data = small_set()
    a, b = (IT.HVOPTrainer(weights, FC.hvop_opt(), dropout=0.05, fused_ends=True) for _ in range(2))
    total, sep, n = a.train_epoch(data, 2, 9, 4)
    assert n == 2 and total.is_cuda and sep.shape == (2,)
    b.set_step(2)
    order = distributed_indices(len(data), 1, 0, 2, 9)
    losses = [b.train_step(data.batch(np.asarray(order[4 * i:4 * i + 4]), 9, 2), IT.batch_seed(9, 2, i)) for i in range(2)]
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert torch.equal(total, losses[0][0] + losses[1][0]) and torch.equal(sep, losses[0][1] + losses[1][1])
    loss, vsep = a.validate(data, 3, seed=4)
    assert all(e.training for e in a.model.enc.values())
    after = a.state_dict()
    assert all(torch.equal(sa[k], after[k]) for k in sa)
    order = distributed_indices(len(data), 1, 0, 0, 4, drop_last=False)
    a.model.eval()
    with torch.no_grad():
        each = [a._loss(data.batch(np.asarray(order[i:i + 3]), 4, 0)) for i in range(0, 8, 3)]
    a.model.train()
    want, wsep = (each[0][0] + each[1][0] + each[2][0]) / 3, (each[0][1] + each[1][1] + each[2][1]) / 3
    assert torch.equal(loss, want) and torch.equal(vsep, wsep) and bool(torch.isfinite(loss))
