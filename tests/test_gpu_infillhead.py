"""GPU: csrc/infillhead.hip through vistracker_amd.ops against the float64 model of tests/infillhead_model.py.  The isolated objective: d_pred bit for bit, the
two fp64 terms to len x 2^-53.  The isolated projections and predictor: 4 e32 per tensor, e32 = the model's float32 run against its float64 run.  Bitwise
properties, refusals, and the autograd wrappers against the raw functions.  Measured ratios: tests/golden/infillhead.md."""
import numpy as np
import pytest
import torch

import infillhead_model as IM

pytestmark = pytest.mark.gpu


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda").contiguous()


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def gate(what, got, truth, e32):
    r = IM.ratios({k: host(v) for k, v in got.items()}, truth, e32)
    print(f"\n[{what}] " + " ".join(f"{k} {v:.2f}" for k, v in r.items()), end="")
    bad = {k: v for k, v in r.items() if not v <= IM.GATE}
    assert not bad, bad


def head_params(P):
    return [dev(P[k]) for k in IM.HEAD_KEYS]


def dummy_head(B, T, C, seed=1):
    """a small predictor around a given pred: the objective reads pred and gt only"""
    r = np.random.RandomState(seed)
    params = [dev(r.randn(16, 16) / 4), dev(0.1 * r.randn(16)), dev(r.randn(C, 16) / 4), dev(0.1 * r.randn(C))]
    return dev(r.randn(B, T, 16)), dev(r.randn(B, T, 16)), params


@pytest.mark.parametrize("c", IM.objective_cases(), ids=lambda c: c["id"])
def test_objective_bit_for_bit(c):
    from vistracker_amd import ops
    b = IM.build_objective(c)
    B, T, C = c["B"], c["T"], c["C"]
    f, h, params = dummy_head(B, T, C)
    d_pred, _, _, terms = ops.infill_head_backward(f, h, params, gt=dev(b["gt"]), pred=dev(b["pred"]), want_terms=True)
    want = b["d_pred"].astype(np.float32)
    got = d_pred.cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    lp, la = (float(x) for x in terms.cpu())
    rp, ra = abs(lp - b["loss_pos"]) / b["loss_pos"], abs(la - b["loss_accel"]) / b["loss_accel"]
    print(f"\n[objective {c['id']}] loss_pos off by {rp / 2.0 ** -53:.1f} x 2^-53 (gate {B * T * C}), loss_accel by {ra / 2.0 ** -53:.1f} (gate {B * (T - 2) * C})", end="")
    assert rp <= B * T * C * 2.0 ** -53 and ra <= B * (T - 2) * C * 2.0 ** -53
    if c["kind"] == "zeros":
        p64, g64 = b["pred"].astype(np.float64), b["gt"].astype(np.float64)
        assert (p64 == g64).sum() >= 5 and ((IM._acc(p64) - IM._acc(g64)) == 0).sum() >= 1  # the planted zeros are there: sign(0) = 0 is part of the bitwise check
    if c["kind"] == "flip":
        _, _, dm = IM.objective(b["pred"], b["gt"], mut="accel_in_fp32_order")
        assert not np.array_equal(dm.astype(np.float32), got)


@pytest.mark.parametrize("c", IM.proj_cases(), ids=lambda c: c["id"])
def test_projections_against_the_model(c):
    from vistracker_amd import ops
    b = IM.build_proj(c)
    xs, Ws, bs, dys = ([dev(q[k]) for q in b["p"]] for k in ("x", "W", "b", "dy"))
    ys = ops.infill_proj_forward(xs, Ws, bs)
    dWs, dbs = ops.infill_proj_backward(dys, xs, Ws, bs)
    for i, q in enumerate(b["p"]):
        gate(f"proj {c['id']} #{i}", dict(y=ys[i], dW=dWs[i], db=dbs[i]), q["r64"], q["e32"])
    one = ops.infill_proj_forward(xs[1:], Ws[1:], bs[1:])[0]                              # a problem alone gives the bits it gives in a table
    assert torch.equal(one, ys[1])


def run_head(ops, b, d_pred=None, **kw):
    params = head_params(b["P"])
    f = dev(b["f"])
    pred, h, _ = ops.infill_head_forward(f, params)
    _, d_f, grads, _ = ops.infill_head_backward(f, h, params, d_pred=dev(b["d_pred"]) if d_pred is None else d_pred, **kw)
    out = dict(pred=pred, h=h, d_f=d_f)
    out.update(zip(IM.HEAD_KEYS, grads))
    return out


@pytest.mark.parametrize("c", IM.head_cases(), ids=lambda c: c["id"])
def test_head_against_the_model(c):
    from vistracker_amd import ops
    m = IM.kink_margin(c)
    assert m > 64, (c["id"], m)                                                            # no pre-activation on the kink but the planted one, whose slope is defined
    b = IM.build_head(c)
    got = run_head(ops, b)
    assert float(got["h"][IM.ZERO]) == 0.0
    gate(f"head {c['id']}", got, b["r64"], b["e32"])


@pytest.fixture(scope="module")
def case():
    return IM.build_head(IM.head_cases()[1])                                                # B 3, T 17, C 9: three tiles and a ragged fourth, two clips in a tile


def objective_run(ops, b, gt, f=None, upstream=1.0, **kw):
    params = head_params(b["P"])
    f = dev(b["f"]) if f is None else f
    pred, h, _ = ops.infill_head_forward(f, params)
    d_pred, d_f, grads, terms = ops.infill_head_backward(f, h, params, gt=gt, pred=pred, upstream=upstream, want_terms=True, **kw)
    out = dict(pred=pred, d_pred=d_pred, d_f=d_f, terms=terms)
    out.update(zip(IM.HEAD_KEYS, grads))
    return out


def test_two_calls_give_equal_bits(case):
    from vistracker_amd import ops
    gt = dev(np.random.RandomState(3).randn(case["B"], case["T"], case["C"]))
    a, b = objective_run(ops, case, gt), objective_run(ops, case, gt)
    assert all(torch.equal(a[k], b[k]) for k in a)
    a, b = run_head(ops, case), run_head(ops, case)
    assert all(torch.equal(a[k], b[k]) for k in a)
    q = IM.build_proj(IM.proj_cases()[4])
    args = [[dev(p[k]) for p in q["p"]] for k in ("dy", "x", "W", "b")]
    r1, r2 = ops.infill_proj_backward(*args), ops.infill_proj_backward(*args)
    assert all(torch.equal(x, y) for x, y in zip(r1[0] + r1[1], r2[0] + r2[1]))
    values = ops.infill_head_forward(dev(case["f"]), head_params(case["P"]), gt, save_h=False)      # the forward-only mode: the same prediction and terms
    full = objective_run(ops, case, gt)
    assert values[1] is None and torch.equal(values[0], full["pred"]) and torch.equal(values[2], full["terms"])


@pytest.mark.parametrize("k", (-20, 20))
def test_power_of_two_upstream_scales_every_gradient_bit_for_bit(case, k):
    from vistracker_amd import ops
    s = 2.0 ** k
    grads = ("d_f",) + IM.HEAD_KEYS
    a, b = run_head(ops, case), run_head(ops, case, d_pred=dev(case["d_pred"]) * s)
    assert all(torch.equal(a[n] * s, b[n]) for n in grads)
    gt = dev(np.random.RandomState(3).randn(case["B"], case["T"], case["C"]))
    a, b = objective_run(ops, case, gt), objective_run(ops, case, gt, upstream=s)
    assert all(torch.equal(a[n] * s, b[n]) for n in grads + ("d_pred",)) and torch.equal(a["terms"], b["terms"])
    q = IM.build_proj(IM.proj_cases()[1])
    dy, x, W, bb = ([dev(p[n]) for p in q["p"]] for n in ("dy", "x", "W", "b"))
    r1, r2 = ops.infill_proj_backward(dy, x, W, bb), ops.infill_proj_backward([d * s for d in dy], x, W, bb)
    assert all(torch.equal(u * s, v) for u, v in zip(r1[0] + r1[1], r2[0] + r2[1]))


def test_a_clip_does_not_see_the_other_clips(case):
    from vistracker_amd import ops
    r = np.random.RandomState(4)
    gt, f = r.randn(case["B"], case["T"], case["C"]), case["f"].copy()
    a = objective_run(ops, case, dev(gt))
    gt2 = gt.copy(); gt2[1] = r.randn(case["T"], case["C"]); f[1] = r.randn(case["T"], case["D"])
    b = objective_run(ops, case, dev(gt2), f=dev(f))
    for n in ("pred", "d_pred", "d_f"):
        assert torch.equal(a[n][0], b[n][0]) and torch.equal(a[n][2], b[n][2]) and not torch.equal(a[n][1], b[n][1]), n


def test_accumulate_equals_write_plus_add_and_null_outputs_are_skipped(case):
    from vistracker_amd import ops
    a = run_head(ops, case)
    r = np.random.RandomState(5)
    base = {n: dev(r.randn(*a[n].shape)) for n in ("d_f",) + IM.HEAD_KEYS}
    out = (base["d_f"].clone(), [base[n].clone() for n in IM.HEAD_KEYS])
    run_head(ops, case, out=out, accumulate=True)
    assert torch.equal(out[0], base["d_f"] + a["d_f"]) and all(torch.equal(o, base[n] + a[n]) for o, n in zip(out[1], IM.HEAD_KEYS))
    part = run_head(ops, case, want_df=False, want=(True, False, False, True))
    assert part["d_f"] is None and part[IM.HEAD_KEYS[1]] is None and part[IM.HEAD_KEYS[2]] is None
    assert torch.equal(part[IM.HEAD_KEYS[0]], a[IM.HEAD_KEYS[0]]) and torch.equal(part[IM.HEAD_KEYS[3]], a[IM.HEAD_KEYS[3]])
    keep = base[IM.HEAD_KEYS[1]].clone()
    run_head(ops, case, out=(None, [None, keep, None, None]))                              # only the named buffer is written
    assert torch.equal(keep, a[IM.HEAD_KEYS[1]])
    q = IM.build_proj(IM.proj_cases()[1])
    dy, x, W, bb = ([dev(p[n]) for p in q["p"]] for n in ("dy", "x", "W", "b"))
    dWs, dbs = ops.infill_proj_backward(dy, x, W, bb)
    bw, bb0 = [dev(r.randn(*w.shape)) for w in W], [dev(r.randn(*v.shape)) for v in bb]
    ow, ob = [t.clone() for t in bw], [t.clone() for t in bb0]
    ops.infill_proj_backward(dy, x, W, bb, out=(ow, ob), accumulate=True)
    assert all(torch.equal(o, s + g) for o, s, g in zip(ow + ob, bw + bb0, dWs + dbs))
    pw, pb = ops.infill_proj_backward(dy, x, W, bb, want=((False, True), (True, False)))
    assert pw[0] is None and pb[1] is None and torch.equal(pw[1], dWs[1]) and torch.equal(pb[0], dbs[0])


def test_autograd_wrappers_equal_the_raw_functions(case):
    """infill_head_train forms its gradients with the values and multiplies them by the upstream scalar; infill_proj_train gives gradients to weights and biases only"""
    from vistracker_amd import ops
    gt = dev(np.random.RandomState(3).randn(case["B"], case["T"], case["C"]))
    raw = objective_run(ops, case, gt, lw_pose=1.0, lw_accel=0.1)
    f = dev(case["f"]).requires_grad_(True)
    params = [q.requires_grad_(True) for q in head_params(case["P"])]
    loss, lp, la, pred = ops.infill_head_train(f, gt, params, 1.0, 0.1)
    assert loss.dtype == torch.float64 and not lp.requires_grad and not pred.requires_grad and torch.equal(pred, raw["pred"])
    assert torch.equal(torch.stack([lp, la]), raw["terms"]) and torch.equal(loss.detach(), raw["terms"].sum())
    (loss * 0.5).backward()
    assert torch.equal(f.grad, raw["d_f"] * 0.5) and all(torch.equal(q.grad, raw[n] * 0.5) for q, n in zip(params, IM.HEAD_KEYS))
    with torch.no_grad():
        v = ops.infill_head_train(f, gt, params, 1.0, 0.1)
    assert torch.equal(v[0], loss.detach()) and torch.equal(v[3], pred)
    q = IM.build_proj(IM.proj_cases()[1])
    dy, x, W, bb = ([dev(p[n]) for p in q["p"]] for n in ("dy", "x", "W", "b"))
    dWs, dbs = ops.infill_proj_backward(dy, x, W, bb)
    W, bb = [w.requires_grad_(True) for w in W], [v.requires_grad_(True) for v in bb]
    ys = ops.infill_proj_train(x, W, bb)
    sum((y * d).sum() for y, d in zip(ys, dy)).backward()
    assert all(torch.equal(p.grad, g) for p, g in zip(W + bb, dWs + dbs))


def test_refusals(case):
    from vistracker_amd import ops
    from vistracker_amd._lib import VtError
    r = np.random.RandomState(6)

    def head(B=2, T=5, D=32, Hd=16, C=6):
        return (dev(r.randn(B, T, D)), [dev(r.randn(Hd, D)), dev(r.randn(Hd)), dev(r.randn(C, Hd)), dev(r.randn(C))], dev(r.randn(B, T, C)))
    for kw in (dict(T=2), dict(D=24), dict(Hd=80), dict(C=17)):
        f, params, gt = head(**kw)
        with pytest.raises(VtError, match="unsupported shape"):
            ops.infill_head_forward(f, params)
        with pytest.raises(VtError, match="unsupported shape"):
            ops.infill_head_train(f, gt, params)
    f, params, gt = head()
    with pytest.raises(VtError, match="float32"):
        ops.infill_head_train(f.half(), gt, params)
    with pytest.raises(VtError, match="float32"):
        ops.infill_head_train(f, gt.half(), params)
    with pytest.raises(VtError, match="device tensor"):
        ops.infill_head_train(f, gt.cpu(), params)
    with pytest.raises(VtError, match="device tensor"):
        ops.infill_head_forward(f.cpu(), params)
    with pytest.raises(VtError, match="contiguous"):
        ops.infill_head_train(f, dev(r.randn(2, 6, 5)).transpose(1, 2), params)
    with pytest.raises(VtError, match="four parameters"):
        ops.infill_head_forward(f, params[:3])
    pred, h, _ = ops.infill_head_forward(f, params)
    with pytest.raises(VtError, match="gt"):
        ops.infill_head_backward(f, h, params, pred=pred)
    x, W, b = dev(r.randn(2, 5, 9)), dev(r.randn(32, 9)), dev(r.randn(32))
    for bad in (([x.half()], [W], [b]), ([x.cpu()], [W], [b]), ([x], [dev(r.randn(24, 9))], [dev(r.randn(24))]), ([x], [dev(r.randn(32, 8))], [b]),
                ([dev(r.randn(2, 5, 161))], [dev(r.randn(32, 161))], [b]), ([x.transpose(0, 1)], [W], [b]), ([x] * 5, [W] * 5, [b] * 5)):
        with pytest.raises(VtError):
            ops.infill_proj_forward(*bad)
        with pytest.raises(VtError):
            ops.infill_proj_train(*bad)
