"""CPU: the float64 model of the stem, the stack tail and the whole HGFilter (tests/enctrain_model.py).  The manual formulas (what the kernels of
vistracker_amd/csrc/enctrain.hip evaluate) equal torch float64 autograd; evaluated on float32-rounded saved activations they meet the gate the GPU tests hold the
kernels to (4 e32 per tensor, e32 = the model's float32 run against its float64 run); and the mutants a wrong kernel would be miss it."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import convblock_model as M
import enctrain_model as EM
from conftest import ROOT

TAIL = dict(B=2, H=4, W=6, C=64, Co=32, seed=11)
STEM = dict(B=2, H=11, W=14, cin=5, cout=64, seed=13)


def _tail(last=False):
    P = EM.tail_make_params(TAIL["C"], TAIL["Co"], last, TAIL["seed"])
    return P, EM.tail_make_inputs(TAIL["B"], TAIL["H"], TAIL["W"], TAIL["C"], TAIL["Co"], TAIL["seed"] + 1)


def _r32(sv):
    r = lambda a: np.asarray(a, np.float32).astype(np.float64)      # noqa: E731
    return {k: (tuple(r(s) for s in v) if isinstance(v, tuple) else r(v)) for k, v in sv.items()}


def _worst(got, truth, e32, names=None):
    """largest error / e32 over the tensors"""
    return max(float(np.abs(got[n] - truth[n]).max()) / e32[n] for n in (names or got))


@pytest.mark.parametrize("last,use_out,use_prev", [(False, True, True), (False, False, True), (False, True, False), (True, True, False)])
def test_tail_manual_matches_autograd(last, use_out, use_prev):
    P, (ll, prev, d_out, d_prev) = _tail(last)
    d_out, d_prev = (d_out if use_out else None), (d_prev if use_prev else None)
    g64 = EM.tail_autograd_grads(P, ll, prev, d_out, d_prev)
    man = EM.tail_manual_grads(P, ll, d_out, d_prev, EM.tail_saved_from_model(P, ll, prev))
    live = {n for n in man if not (d_prev is None and n.startswith(("bl.", "al.")))}
    assert live == set(g64) - {"out", "prev"}, sorted(live ^ (set(g64) - {"out", "prev"}))
    for n in live:
        err = float(np.abs(man[n] - g64[n]).max())
        assert err <= 1e-11 * max(1.0, float(np.abs(g64[n]).max())), (n, err)


@pytest.mark.parametrize("cin,cout", [(5, 64), (1, 32)])
def test_stem_manual_matches_autograd(cin, cout):
    """cout 32: GroupNorm(32, 32) has one channel per group"""
    P = EM.stem_make_params(cin, cout, STEM["seed"])
    x, dy = EM.stem_make_inputs(STEM["B"], STEM["H"], STEM["W"], cin, cout, STEM["seed"] + 1)
    g64, man = EM.stem_autograd_grads(P, x, dy), EM.stem_manual_grads(P, x, dy)
    assert set(man) == set(g64) - {"out"}
    for n, v in man.items():
        err = float(np.abs(v - g64[n]).max())
        assert err <= 1e-11 * max(1.0, float(np.abs(g64[n]).max())), (n, err)


def test_float32_activations_meet_the_gates():
    P, (ll, prev, d_out, d_prev) = _tail()
    g64, e32 = EM.tail_reference_and_e32(P, ll, prev, d_out, d_prev)
    man = EM.tail_manual_grads(P, ll, d_out, d_prev, _r32(EM.tail_saved_from_model(P, ll, prev)))
    assert _worst(man, g64, e32) <= 4
    Ps = EM.stem_make_params(STEM["cin"], STEM["cout"], STEM["seed"])
    x, dy = EM.stem_make_inputs(STEM["B"], STEM["H"], STEM["W"], STEM["cin"], STEM["cout"], STEM["seed"] + 1)
    g64, e32 = EM.stem_reference_and_e32(Ps, x, dy)
    assert _worst(EM.stem_manual_grads(Ps, x, dy, _r32(EM.stem_saved_from_model(Ps, x))), g64, e32) <= 4


@pytest.mark.parametrize("mutant,tensors", [("bias_missing_frame", ("l.bias", "bl.bias", "al.bias", "conv_last.bias")), ("no_al_in_gout", ("l.weight", "l.bias", "d_ll")),
                                            ("no_bl_in_da", ("d_ll", "conv_last.weight", "bn_end.weight"))])
def test_tail_mutants_miss_the_gate(mutant, tensors):
    P, (ll, prev, d_out, d_prev) = _tail()
    g64, e32 = EM.tail_reference_and_e32(P, ll, prev, d_out, d_prev)
    man = EM.tail_manual_grads(P, ll, d_out, d_prev, EM.tail_saved_from_model(P, ll, prev), mutant=mutant)
    for n in tensors:
        assert float(np.abs(man[n] - g64[n]).max()) > 4 * e32[n], n


@pytest.mark.parametrize("mutant,tensors", [("bias_missing_frame", ("conv1.bias",)), ("pad2", ("conv1.weight",))])
def test_stem_mutants_miss_the_gate(mutant, tensors):
    P = EM.stem_make_params(STEM["cin"], STEM["cout"], STEM["seed"])
    x, dy = EM.stem_make_inputs(STEM["B"], STEM["H"], STEM["W"], STEM["cin"], STEM["cout"], STEM["seed"] + 1)
    g64, e32 = EM.stem_reference_and_e32(P, x, dy)
    man = EM.stem_manual_grads(P, x, dy, mutant=mutant)
    for n in tensors:
        assert float(np.abs(man[n] - g64[n]).max()) > 4 * e32[n], n


@pytest.mark.parametrize("C", [32, 64])
def test_mask_from_the_staging_expression_misses_the_gate(C):
    """on an input built so that the forward's expression and the staging expression disagree in sign on at least one element"""
    c = EM.planted_gn_case(C, 1, 8, 16, 17)
    assert c["disagree"] >= 1, "no element on which the two forward expressions disagree in sign"
    g64, g32 = EM.gn_y_grads(c), EM.gn_y_grads(c, torch.float32)
    mut = EM.gn_y_grads(c, mask=EM.staging_mask(c["y1"], *c["stats"], c["gamma"], c["beta"]))
    assert float(np.abs(mut["dbeta"] - g64["dbeta"]).max()) > 4 * float(np.abs(g32["dbeta"] - g64["dbeta"]).max())


def test_filter_manual_matches_autograd():
    """the chain over the tape (what the whole-filter GPU test compares against at the GPU forward's saved activations) IS the float64 autograd gradient"""
    P = EM.filter_make_params(1, 32, 64, 2, 1, 31)
    r = np.random.RandomState(32)
    x = r.rand(1, 1, 16, 16).astype(np.float32)
    d_outs = [r.randn(1, 64, 4, 4), r.randn(1, 64, 4, 4)]
    d_normx = r.randn(1, 128, 4, 4)
    g64 = EM.filter_autograd_grads(P, x, d_outs, d_normx)
    man = EM.filter_manual_grads(P, x, d_outs, d_normx, EM.filter_saved_from_model(P, x))
    assert set(man) == set(g64) - {"out0", "out1", "tmpx", "normx"}, sorted(set(man) ^ set(g64))
    for n, v in man.items():
        err = float(np.abs(v - g64[n]).max())
        assert err <= 1e-10 * max(1.0, float(np.abs(g64[n]).max())), (n, err)


def test_entry_points_are_declared():
    from vistracker_amd import _lib, ops
    src = open(os.path.join(ROOT, "include", "vistracker.h")).read()
    for name in ("vt_bias_grad", "vt_bias_grad_workspace_bytes", "vt_stem7x7_wgrad", "vt_stem7x7_wgrad_workspace_bytes", "vt_gn_relu_backward_y",
                 "vt_stack_tail_backward", "vt_stack_tail_backward_workspace"):
        decl = re.search(r"(?:int|long) " + name + r"\((.*?)\);", src, re.S)
        assert decl is not None and name in _lib.SIGNATURES, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    res, args = _lib.SIGNATURES["vt_stack_tail_backward"]
    decl = re.search(r"int vt_stack_tail_backward\((.*?)\);", src, re.S).group(1)
    hdr = [re.sub(r".*[ *]", "", a.strip()) for a in decl.split(",")]
    assert hdr[17:28] == list(ops.STACK_TAIL_GRADS), hdr
    for n, a in zip(hdr, args):
        assert a is (C.c_int if n in {"B", "H", "W", "C", "Co", "accumulate"} else C.c_void_p), n


@pytest.mark.parametrize("tag", list(EM.FILTER_CASES))
def test_model_matches_the_recorded_reference(tag):
    """the reference ran in float32 (tests/golden/enctrain_<tag>.npz, tools/gen_golden_enctrain.py): the float64 model differs from it by float32 rounding -- no more
    than the model's own float32 run does, times 4"""
    from conftest import golden
    gold = golden("enctrain_" + tag)
    P, x, d_outs, d_normx = EM.filter_case(tag)
    g64, e32 = EM.filter_reference_and_e32(P, x, d_outs, d_normx)
    assert set(gold) == {k for k in g64 if k not in ("tmpx", "normx") and not k.startswith("out")}
    for n, v in gold.items():
        want = g64[n].reshape(-1)[::EM.GOLDEN_WEIGHT_STEP] if g64[n].ndim == 4 else g64[n]
        err = float(np.abs(v - want).max())
        assert err <= 4 * e32[n] + 1e-30, (n, err, e32[n])


def test_state_dict_reader_strips_module_and_prefix():
    """encoder.state_dict_under / as_f32 behind the three from_state_dict: a 'module.'-prefixed state dict and a plain one give the same state_dict(), under a
    prefix and without one; a missing key raises the KeyError it always raised"""
    from vistracker_amd import encoder as E
    assert E.state_dict_under({"module.p.a": 1, "p.b": 2, "q.p.c": 3, "module.q.d": 4}, "p.") == {"a": 1, "b": 2}
    assert E.state_dict_under({"module.a": 1, "b": 2}, "") == {"a": 1, "b": 2}
    t = E.as_f32(np.arange(6, dtype=np.float64).reshape(2, 3), "cpu")
    assert t.dtype == torch.float32 and t.device.type == "cpu" and not t.requires_grad and E.as_f32(t, "cpu").data_ptr() == t.data_ptr()
    P = EM.filter_make_params(1, 32, 64, 2, 1, 31)
    block = lambda sd, p: E.TrainableConvBlock.from_state_dict(sd, p, device="cpu")            # noqa: E731
    makers = {"conv3.": block, "conv4.": block,         # an identity block and one with a projection
              "m0.": lambda sd, p: E.TrainableHourglass.from_state_dict(sd, p, depth=1, device="cpu"),
              "": lambda sd, p: E.TrainableHGFilter.from_state_dict(sd, p, num_stack=2, num_hourglass=1, device="cpu")}
    for sub, make in makers.items():
        for outer in ("", "image_filter."):
            plain = {outer + k: v for k, v in P.items()}
            a, b = make(plain, outer + sub).state_dict(), make({"module." + k: v for k, v in plain.items()}, outer + sub).state_dict()
            assert list(a) == list(b) and len(a) >= sum(k.startswith(sub) for k in P) > 0
            assert all(a[k].dtype == torch.float32 and torch.equal(a[k], b[k]) and np.array_equal(a[k].numpy(), P[sub + k]) for k in a if sub + k in P)
    for sub, make, key, text in (("conv3.", makers["conv3."], "conv3.bn2.bias", "no ConvBlock parameter 'conv3.bn2.bias'"),
                                 ("m0.", makers["m0."], "m0.b2_plus_1.conv1.weight", "no ConvBlock parameter 'm0.b2_plus_1.conv1.weight'"),
                                 ("", makers[""], "bn_end1.weight", "no encoder parameter 'bn_end1.weight'"),
                                 ("", makers[""], "top_m_0.conv3.weight", "no ConvBlock parameter 'top_m_0.conv3.weight'")):
        with pytest.raises(KeyError) as e:
            make({"module." + k: v for k, v in P.items() if k != key}, sub)
        assert e.value.args[0] == text
    with pytest.raises(KeyError) as e:
        E.HGFilterEncoder({"module.image_filter." + k: v for k, v in P.items()}, "triplane_encoder.", 2, 1, device="cpu")
    assert e.value.args[0] == "no encoder weights under prefix 'triplane_encoder.'"
    with pytest.raises(KeyError) as e:
        E.TrainableConvBlock.from_state_dict({k: v for k, v in P.items() if not k.startswith(("conv4.downsample.0", "conv4.bn4"))}, "conv4.", device="cpu")
    assert e.value.args[0] == "'conv4.downsample.2.weight' without the projection's norm"


def test_stats_hand_over_finalizes_once(monkeypatch):
    """encoder_fwd.attach_stats / stats_of with the library call stubbed: nothing attached -> None; partial sums are finalized at their first use, with the
    tensor's own sizes, and never again; an entry attached as finalized is handed over as it is"""
    from vistracker_amd import _lib, encoder_fwd as fwd
    calls = []

    class Stub:
        @staticmethod
        def vt_groupnorm_finalize(*a):
            calls.append(a)
            return 0

    monkeypatch.setattr(_lib, "lib", lambda: Stub)
    monkeypatch.setattr(_lib, "stream_ptr", lambda: 0)
    x = torch.zeros(2, 64, 8, 16)
    assert fwd.stats_of(x) is None and calls == []
    ws = fwd.partials_workspace(2, 64, 3, "cpu")
    assert ws.dtype == torch.float64 and ws.numel() == 2 * 32 + 3 * 2 * 64 * 2
    assert fwd.attach_stats(x, ws, 3) is x
    assert fwd.stats_of(x) is ws and calls == [(ws.data_ptr(), 3, 2, 8 * 16, 64, 32, 1e-5, 0)]
    assert fwd.stats_of(x) is ws and len(calls) == 1                    # already finalized: no second launch
    assert fwd.input_stats(x, True) is ws and len(calls) == 1           # the consumer's way in: the producer's statistics, no pass
    y = fwd.carry_stats(x, torch.zeros(2, 64, 8, 16))
    assert fwd.stats_of(y) is ws and len(calls) == 1                    # a copy of x shares the entry, finalized flag included
    z = fwd.attach_stats(torch.zeros(2, 64, 8, 16), ws, 3, finalized=True)
    assert fwd.stats_of(z) is ws and len(calls) == 1
    assert fwd.stats_of(torch.zeros(2, 64, 8, 16)) is None
