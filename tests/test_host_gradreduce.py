"""CPU: the float64 model of the rank-ordered gradient mean (tests/gradreduce_model.py) against an independent restatement, the three mutants its case set must
reject, and ``training.distributed_indices`` against ``torch.utils.data.distributed.DistributedSampler``."""
import numpy as np
import pytest

import gradreduce_model as GM


def test_model_against_the_restatement():
    for W, n, _ in GM.cases():
        v = GM.values(W, n)
        a, b = GM.mean(v), GM.mean_python(v)
        assert a.dtype == np.float32 and a.shape == (n,) and GM.same_bits(a, b), (W, n)


def test_the_values_are_what_the_cases_promise():
    v = GM.values(5, 1025)
    free = np.array([j for j in range(1025) if j % GM.PERIOD >= GM.N_SPECIAL])
    mag = np.abs(v[:, free])
    assert (np.log2(mag.max(1) / mag.min(1)) >= 30).all()                              # 30 binades inside every row
    out = GM.mean(v)
    assert out[1] == 0 and not np.signbit(out[1]) and out[2] == 0 and np.signbit(out[2])          # rows that cancel to +0, ranks that all hold -0
    assert np.isnan(out[4]) and np.isinf(out[5]) and np.isnan(out[6])
    assert GM.mean(GM.values(1, 65)).view(np.int32).tolist() == GM.values(1, 65)[0].view(np.int32).tolist()          # W = 1 is the identity


@pytest.mark.parametrize("name", sorted(GM.MUTANTS))
def test_the_cases_reject_the_mutant(name):
    differing = [(W, n) for W, n, pad in GM.cases() if pad == 0 and not GM.same_bits(GM.MUTANTS[name](GM.values(W, n)), GM.mean(GM.values(W, n)))]
    print(f"\n[{name}] differs from the model on {len(differing)} of {len(GM.cases()) // len(GM.PADS)} (W, n)", end="")
    assert differing, name


def test_power_of_two_scaling_of_the_model():
    for W in GM.WS:
        v = GM.values(W, 1025)
        v = v[:, np.isfinite(v).all(0) & (np.abs(v) < 1e30).all(0) & ((np.abs(v) > 1e-30) | (v == 0)).all(0)]
        assert GM.same_bits(GM.mean(v * np.float32(2.0 ** -7)), GM.mean(v) * np.float32(2.0 ** -7)), W


@pytest.mark.parametrize("num_items,world", [(10, 1), (10, 3), (17, 4), (64, 8)])
def test_distributed_indices_are_the_samplers(num_items, world):
    from torch.utils.data.distributed import DistributedSampler
    from vistracker_amd.training import distributed_indices
    data = list(range(num_items))
    for shuffle in (True, False):
        for drop_last in (True, False):
            for seed in (0, 7):
                for rank in range(world):
                    s = DistributedSampler(data, num_replicas=world, rank=rank, shuffle=shuffle, seed=seed, drop_last=drop_last)
                    for epoch in range(3):
                        s.set_epoch(epoch)
                        got = distributed_indices(num_items, world, rank, epoch, seed=seed, shuffle=shuffle, drop_last=drop_last)
                        assert got == list(s), (num_items, world, rank, epoch, shuffle, drop_last, seed)
    assert distributed_indices(num_items, world, 0, 0) == distributed_indices(num_items, world, 0, 0, seed=0, shuffle=True, drop_last=True)
