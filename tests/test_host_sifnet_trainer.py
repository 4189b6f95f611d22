"""CPU: the host side of training.SIFNetTrainer -- the learning-rate schedule against torch's MultiStepLR, the key mapping of state_dict() against the reference's
parameter names (tests/golden/sifnet_state_dict_keys.txt: names only, of the shipped configuration, written by tools/gen_golden_sifnet_step.py), the refusal of
per-view triplane encoders -- and the composition of tests/sifnet_step_model.py: its objective in tests/losshead_model.py's numpy restatement, and the reference's
recorded float64 losses and gradients (tests/golden/sifnet_step.npz) held to the model."""
import os

import numpy as np
import pytest
import torch

import enctrain_model as EM
import sifnet_step_model as SM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("milestones", [(), (3,), (2, 5), (1, 2, 3), (2, 2, 6), (0,)])
@pytest.mark.parametrize("lr0,gamma", [(1e-3, 0.3), (1e-4, 0.1)])
def test_multistep_lr_is_torchs_scheduler(milestones, lr0, gamma):
    from vistracker_amd.training import multistep_lr
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=lr0)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, list(milestones), gamma)
    for epoch in range(9):                       # across and on every milestone
        assert multistep_lr(lr0, milestones, gamma, epoch) == sched.get_last_lr()[0], (epoch, milestones)
        opt.step()
        sched.step()


def shipped_state_dict(names):
    """synthetic parameters of the shipped configuration (3 stacks of depth 2) under the reference's names; an identity ConvBlock's bn4, which the reference
    registers and never uses, is added from the block's input width"""
    cin_i, tmpx_i, hg_i, _ = EM.FILTER_CASES["image"]
    cin_t, tmpx_t, hg_t, _ = EM.FILTER_CASES["triplane"]
    c = dict(P_img=EM.filter_make_params(cin_i, tmpx_i, hg_i, 3, 2, 1), P_tri=EM.filter_make_params(cin_t, tmpx_t, hg_t, 3, 2, 2), dec=SM.make_decoders(3))
    sd = SM.state_dict(c)
    for k in names:
        if k not in sd and ".bn4." in k:
            width = sd[k.split(".bn4.")[0] + ".conv1.weight"].shape[1]
            sd[k] = (np.ones if k.endswith("weight") else np.zeros)(width, np.float32)
    return sd


def test_state_dict_keys_are_the_references():
    from vistracker_amd import ops, training
    from vistracker_amd.encoder import TrainableHGFilter, state_dict_under
    from vistracker_amd.sifnet import SIFNetQuery
    with open(os.path.join(GOLDEN, "sifnet_state_dict_keys.txt")) as f:
        names = f.read().split()
    assert len(names) == len(set(names)) and any(k.startswith("image_filter.") for k in names) and any(k.startswith("triplane_encoder.") for k in names)
    sd = {"module." + k: v for k, v in shipped_state_dict(names).items()}
    assert {k[7:] for k in sd} == set(names)
    own = state_dict_under(sd, "")
    image = TrainableHGFilter.from_state_dict(own, training.IMAGE_PREFIX, num_stack=3, num_hourglass=2, device="cpu")
    tri = TrainableHGFilter.from_state_dict(own, training.TRIPLANE_PREFIX, num_stack=3, num_hourglass=2, device="cpu")
    params = ops.DecoderParams.from_decoders(SIFNetQuery.decoders_from_state_dict(own), device="cpu")
    out = training.network_state_dict(image, tri, params)
    assert set(out) == set(names), sorted(set(out) ^ set(names))
    assert all(tuple(out[k].shape) == tuple(np.shape(own[k])) and np.array_equal(out[k].detach().numpy(), own[k]) for k in names), "values in = values out"


def test_per_view_triplane_encoders_are_refused():
    from vistracker_amd import _lib
    from vistracker_amd.training import SIFNetTrainer
    sd = SM.state_dict(dict(P_img={}, P_tri={"conv1.weight": np.zeros((32, 1, 7, 7), np.float32)}, dec=SM.make_decoders(3)))
    sd = {("module." + k).replace("triplane_encoder.", "triplane_encoder_0."): v for k, v in sd.items()}
    with pytest.raises(_lib.VtError, match="per-view"):
        SIFNetTrainer(sd, None)
    with pytest.raises(_lib.VtError, match="stacks"):
        SIFNetTrainer({}, None, num_stack=3, triplane_stack=2)


def test_the_step_model_is_the_composition_and_the_references_losses():
    c = SM.case()
    r64 = SM.run(c)
    assert np.abs(SM.losshead_losses(c, r64["preds"]) - r64["losses_all"]).max() <= 1e-9 * r64["losses_all"].max()         # losshead_model's restatement of get_errors
    assert abs(r64["error"] - r64["losses_all"].sum()) <= 1e-9 * r64["error"]
    assert set(SM.gated()) <= set(r64["grads"]) and len(SM.gated()) == 40 + 2 * 10
    gold = np.load(os.path.join(GOLDEN, "sifnet_step.npz"))
    assert set(gold.files) == set(SM.gated()) | {"losses_all", "error"}
    # the reference was recorded in float64: it and the model are two float64 evaluations of one function that differ in the order of their sums, 1e-16 per
    # rounding over chains of at most a few 1e4 terms; 1e-9 of a tensor's scale leaves three digits over that and is 1e-3 of the smallest relative e32 measured
    assert np.abs(gold["losses_all"] - r64["losses_all"]).max() <= 1e-9 * r64["losses_all"].max() and abs(float(gold["error"]) - r64["error"]) <= 1e-9 * r64["error"]
    for k in SM.gated():
        want = SM.golden_sub(k)(r64["grads"][k])
        assert gold[k].dtype == np.float64 and gold[k].shape == want.shape, k
        assert np.abs(gold[k] - want).max() <= 1e-9 * max(np.abs(r64["grads"][k]).max(), 1.0), (k, np.abs(gold[k] - want).max())
