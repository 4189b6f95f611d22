"""CPU: the float64 ConvBlock model (tests/convblock_model.py) against the recorded reference (tests/golden/convblock.npz, tools/gen_golden_convblock.py), the
GroupNorm + ReLU backward formula of vt_gn_relu_backward against autograd, and the flat argument order of vt_conv_block_backward against _lib.SIGNATURES."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import convblock_model as M
from conftest import ROOT, golden

BLOCKS = ((64, 128, 21), (128, 128, 23))        # tools/gen_golden_convblock.py


@pytest.mark.parametrize("cin,cout,seed", BLOCKS)
def test_model_matches_the_recorded_reference(cin, cout, seed):
    """the reference ran in float32: the float64 model differs from it by float32 rounding -- no more than the model's own float32 run does, times 4"""
    gold = golden("convblock")
    P = M.make_params(cin, cout, seed)
    x, dy = M.make_inputs(1, 8, 16, cin, cout, seed + 1)
    g64, e32 = M.reference_and_e32(P, x, dy)
    tag = f"b{cin}_{cout}."
    names = [k[len(tag):] for k in gold if k.startswith(tag)]
    assert set(names) == set(g64), (sorted(names), sorted(g64))
    for n in names:
        want = g64[n].reshape(-1)[::M.GOLDEN_WEIGHT_STEP] if g64[n].ndim == 4 and n.endswith("weight") else g64[n]
        err = float(np.abs(gold[tag + n] - want).max())
        print(f"\n[{tag}{n}] e32 {e32[n]:.3e} |reference - model64| {err:.3e} of {np.abs(want).max():.3e}", end="")
        assert err <= 4 * e32[n] + 1e-30, (n, err, e32[n])


@pytest.mark.parametrize("C,B,H,W", [(32, 2, 4, 6), (256, 1, 3, 5)])
def test_gn_relu_backward_formula_matches_autograd(C, B, H, W):
    """groups of one channel (C = 32) and of eight (C = 256)"""
    r = np.random.RandomState(C)
    x = torch.tensor(r.randn(B, C, H, W) * 2 + 0.3, requires_grad=True)
    gamma = torch.tensor(1 + 0.3 * r.randn(C), requires_grad=True); beta = torch.tensor(0.3 * r.randn(C), requires_grad=True)
    g = torch.tensor(r.randn(B, C, H, W))
    torch.nn.functional.relu(torch.nn.functional.group_norm(x, 32, gamma, beta, M.EPS)).backward(g)
    mean, rstd = M.group_stats(x.detach())
    d_x, dgamma, dbeta = M.gn_relu_backward(g, x.detach(), mean, rstd, gamma.detach(), beta.detach())
    for name, got, want in (("d_x", d_x, x.grad), ("dgamma", dgamma, gamma.grad), ("dbeta", dbeta, beta.grad)):
        err = float((got - want).abs().max())
        print(f"\n[C={C}] {name}: |formula - autograd| {err:.3e} of {float(want.abs().max()):.3e}", end="")
        assert err <= 1e-12 * max(1.0, float(want.abs().max())), name


@pytest.mark.parametrize("cin,cout,seed", BLOCKS)
def test_manual_backward_matches_autograd(cin, cout, seed):
    """the explicit backward at the model's own saved activations IS the autograd gradient (what the end-to-end bound of the GPU test builds on)"""
    P = M.make_params(cin, cout, seed)
    x, dy = M.make_inputs(1, 8, 16, cin, cout, seed + 1)
    g64, man = M.autograd_grads(P, x, dy), M.manual_grads(P, x, dy)
    assert set(man) == set(g64) - {"out"}
    for n, v in man.items():
        err = float(np.abs(v - g64[n]).max())
        assert err <= 1e-11 * max(1.0, float(np.abs(g64[n]).max())), (n, err)


def test_block_entry_argument_order_matches_signatures():
    from vistracker_amd import _lib, ops
    res, args = _lib.SIGNATURES["vt_conv_block_backward"]
    names = ops.CONV_BLOCK_BACKWARD_ARGS
    assert res is C.c_int and len(args) == len(names)
    ints = {"B", "H", "W", "cin", "c1", "c2", "c3", "accumulate"}
    for n, a in zip(names, args):
        assert a is (C.c_int if n in ints else C.c_void_p), n
    # and the header declares the same names in the same order
    src = open(os.path.join(ROOT, "include", "vistracker.h")).read()
    decl = re.search(r"int vt_conv_block_backward\((.*?)\);", src, re.S).group(1)
    hdr = [re.sub(r".*[ *]", "", a.strip()) for a in decl.split(",")]
    assert hdr == list(names), hdr
    for name in ("vt_conv3x3_dgrad", "vt_conv3x3_wgrad", "vt_conv1x1_dgrad", "vt_conv1x1_wgrad", "vt_gn_relu_backward", "vt_conv_block_backward_workspace"):
        assert name in _lib.SIGNATURES
