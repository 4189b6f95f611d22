"""CPU: the float64 model of HVOP-Net's encoder layer (tests/former_model.py) against torch float64 autograd of a composition from
F.multi_head_attention_forward / F.layer_norm / the activations; the mutants the GPU gates must catch; the dropout hash; the kink condition; the C-ABI names."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import former_cases as FC
import former_model as FM


def torch_layer(P, x, pos, mask, dy, H, act):
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    P = {k: t(v).requires_grad_(True) for k, v in P.items()}
    x = t(x).requires_grad_(True); pos = t(pos)
    D = x.shape[-1]
    ln = F.layer_norm(x, (D,), P["norm1.weight"], P["norm1.bias"])
    qk = (ln + pos).transpose(0, 1)
    a, _ = F.multi_head_attention_forward(qk, qk, ln.transpose(0, 1), D, H, P["self_attn.in_proj_weight"], P["self_attn.in_proj_bias"], None, None, False, 0.0,
                                          P["self_attn.out_proj.weight"], P["self_attn.out_proj.bias"], training=True,
                                          key_padding_mask=None if mask is None else torch.tensor(mask), need_weights=False)
    y1 = x + a.transpose(0, 1)
    z = F.layer_norm(y1, (D,), P["norm2.weight"], P["norm2.bias"])
    fa = {"relu": F.relu, "gelu": F.gelu, "leaky_relu": F.leaky_relu}[act]
    y = y1 + F.linear(fa(F.linear(z, P["linear1.weight"], P["linear1.bias"])), P["linear2.weight"], P["linear2.bias"])
    (y * t(dy)).sum().backward()
    out = {k: v.grad.numpy() for k, v in P.items()}
    out["d_x"], out["y"] = x.grad.numpy(), y.detach().numpy()
    return out


@pytest.mark.parametrize("act", FM.ACTS)
@pytest.mark.parametrize("mask", ["none", "block", "all_but_one"])
def test_model_equals_torch_float64(act, mask):
    """reached: <= 9e-16 relative on every tensor (both sides float64); gate 1e-10 of the tensor's largest magnitude"""
    B, T, D, H, Fd = 2, 20, 32, 2, 64
    P = FM.make_params(D, Fd, 5)
    x, pos, dy, m = FM.make_inputs(B, T, D, 6, mask)
    got, _ = FM.run(P, x, pos, m, dy, H, act)
    ref = torch_layer(P, x, pos, m, dy, H, act)
    assert set(got) == set(ref)
    worst = 0.0
    for n in ref:
        rel = float(np.abs(got[n] - ref[n]).max() / np.abs(ref[n]).max())
        worst = max(worst, rel)
        assert rel <= 1e-10, (n, rel)
    print(f"\n[{act} {mask}] worst relative difference {worst:.2e}", end="")


def test_stack_equals_chained_torch():
    B, T, D, H, Fd = 2, 12, 32, 2, 64
    Ps = [FM.make_params(D, Fd, 40 + i) for i in range(2)]
    norm = (Ps[0]["norm1.weight"], Ps[0]["norm1.bias"])
    x, pos, dy, m = FM.make_inputs(B, T, D, 44, "block")
    y, saved = FM.stack_forward(Ps, norm, x, pos, m, H, "gelu")
    g = FM.stack_backward(Ps, norm, saved, dy)
    # torch: the same two layers chained by hand through their own input gradients
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    x1 = FM.layer_forward(Ps[0], x, pos, m, H, "gelu")[0]
    x2 = t(FM.layer_forward(Ps[1], x1, pos, m, H, "gelu")[0]).requires_grad_(True)
    yt = F.layer_norm(x2, (D,), t(norm[0]), t(norm[1]))
    (yt * t(dy)).sum().backward()
    assert np.abs(yt.detach().numpy() - y).max() <= 1e-12
    r1 = torch_layer(Ps[1], x1, pos, m, x2.grad.numpy(), H, "gelu")
    r0 = torch_layer(Ps[0], x, pos, m, r1["d_x"], H, "gelu")
    assert np.abs(g["d_x"] - r0["d_x"]).max() <= 1e-10 * np.abs(r0["d_x"]).max()
    for k in FM.PARAM_KEYS:
        for i, r in enumerate((r0, r1)):
            assert np.abs(g[f"encoder.layers.{i}.{k}"] - r[k]).max() <= 1e-10 * np.abs(r[k]).max(), (i, k)


@pytest.mark.parametrize("mut", FM.MUTANTS)
def test_gates_catch_the_mutants(mut):
    """the 4 e32 gate of the GPU tests, applied to the model's own float32 run with one defect: it must fail on y or on a gradient"""
    c = FC.build(dict(id="mut", B=3, T=17, D=32, H=2, F=64, act="gelu", mask="block", seed=77), p=0.5 if mut == "drop2_unscaled" else 0.0, seed=9)
    good, _ = FM.run(c["P"], c["x"], c["pos"], c["m"], c["dy"], c["H"], c["act"], c["p"], c["dseed"], np.float32)
    bad, _ = FM.run(c["P"], c["x"], c["pos"], c["m"], c["dy"], c["H"], c["act"], c["p"], c["dseed"], np.float32, mut=mut)
    assert all(np.abs(good[n] - c["g64"][n]).max() <= 4 * c["e32"][n] for n in good)
    assert any(np.abs(bad[n] - c["g64"][n]).max() > 4 * c["e32"][n] for n in bad), mut


@pytest.mark.parametrize("p", [0.05, 0.5])
def test_hash_keep_fraction(p):
    n = 1 << 20
    keep = FM.keep_scale(1234567891011, FM.SITE_FF, (n,), p) > 0
    sd = math.sqrt(n * p * (1 - p))
    assert abs(int(keep.sum()) - n * (1 - p)) <= 5 * sd, (int(keep.sum()), n * (1 - p), sd)


def test_hash_sites_differ_and_masks_ignore_the_shape():
    a = [FM.keep_scale(7, s, (4096,), 0.5) for s in (FM.SITE_ATTN, FM.SITE_1, FM.SITE_FF, FM.SITE_2)]
    assert all(not np.array_equal(a[i], a[j]) for i in range(4) for j in range(i))
    assert not np.array_equal(a[0], FM.keep_scale(8, FM.SITE_ATTN, (4096,), 0.5))
    flat = FM.keep_scale(7, FM.SITE_1, (4096,), 0.05)
    assert np.array_equal(flat, FM.keep_scale(7, FM.SITE_1, (4, 32, 32), 0.05).ravel()) and np.array_equal(flat[:100], FM.keep_scale(7, FM.SITE_1, (100,), 0.05))
    assert np.array_equal(FM.keep_scale(7, FM.SITE_1, (5, 3), 0.0), np.ones((5, 3)))
    # the python-integer restatement the trainer derives layer seeds with
    from vistracker_amd import infill_training as IT
    idx = np.array([0, 1, 2 ** 32 + 3, 2 ** 40 + 17], dtype=np.uint64)
    assert [IT.dropout_hash(0xfedcba9876543210, 3, int(i)) for i in idx] == [int(h) for h in FM.dropout_hash(0xfedcba9876543210, 3, idx)]


@pytest.mark.parametrize("c", [c for c in FC.layer_cases() + FC.small_cases() if c["act"] != "gelu"], ids=lambda c: c["id"])
def test_kink_condition(c):
    """relu / leaky_relu: at most 1 % of a case's feed-forward pre-activations lie within float32 reach of 0"""
    c = FC.build(c)
    near = FM.near_kink(c["P"], c["S"], c["act"])
    assert near.mean() <= 0.01, float(near.mean())


def test_former_entry_points_resolve():
    from vistracker_amd import _lib
    l = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(l, n) and n in _lib.SIGNATURES for n in ("vt_former_layer_forward", "vt_former_layer_backward", "vt_layernorm_forward", "vt_layernorm_backward"))


def test_model_matches_the_recorded_reference():
    """tests/golden/former.npz (tools/gen_golden_former.py): the reference's TransformerV2 and ConditionalMInfiller in train mode with dropout 0, float64 autograd.
    Gate 1e-10 of the tensor's largest magnitude; reached: printed."""
    from conftest import golden
    from vistracker_amd import infill
    # the reference builds its position table in float32 whatever the model's dtype (posi_embed.py:37-66): infill.position_embedding_sine_1d is that table
    table = lambda T, D: infill.position_embedding_sine_1d(T, D // 2, D).numpy().astype(np.float64)          # noqa: E731
    g = golden("former")
    sd = {k[6:]: g[k] for k in g if k.startswith("tv2_w/")}
    Ps = [{k: sd[f"encoder.layers.{i}.{k}"] for k in FM.PARAM_KEYS} for i in range(2)]
    norm = (sd["encoder.norm.weight"], sd["encoder.norm.bias"])
    y, saved = FM.stack_forward(Ps, norm, g["tv2_x"], table(20, 32), g["tv2_mask"], 2, "gelu")
    got = FM.stack_backward(Ps, norm, saved, g["tv2_dy"]); got["y"] = y
    ref = {k[6:]: g[k] for k in g if k.startswith("tv2_g/")}
    ref["y"], ref["d_x"] = g["tv2_y"], g["tv2_dx"]
    assert set(got) == set(ref)
    worst = max(float(np.abs(got[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in ref)
    batch = {k: g["cmf_" + k] for k in ("data_smpl", "mask_smpl", "data_obj", "mask_obj", "gt_obj")}
    r = FM.infiller_run(FC.seeded_weights(golden("infill"), 31), FC.hvop_opt(0.0), batch, {D: table(20, D) for D in (128, 32, 160)})
    names = [k[6:] for k in g if k.startswith("cmf_g/")]
    assert sorted(names) == sorted(k for k in r if k not in ("pred", "loss_accel", "loss_pos"))
    worst2 = max(float(np.abs(r[k] - g["cmf_" + k]).max() / np.abs(g["cmf_" + k]).max()) for k in ("pred", "loss_accel", "loss_pos"))
    for k in names:
        scale = g["cmf_s/" + k][1]
        worst2 = max(worst2, float(np.abs(r[k].ravel()[g["cmf_i/" + k]] - g["cmf_g/" + k]).max() / scale), abs(np.abs(r[k]).max() - scale) / scale,
                     abs(r[k].sum() - g["cmf_s/" + k][0]) / (scale * r[k].size))
    print(f"\n[former.npz] stack {worst:.2e}, infiller {worst2:.2e} of the largest magnitude", end="")
    assert worst <= 1e-10 and worst2 <= 1e-10, (worst, worst2)
