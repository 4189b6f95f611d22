"""GPU: vt_former_layer_forward / vt_former_layer_backward (csrc/formertrain.hip) through ops, against the float64 model of tests/former_model.py, per tensor.
Gate: 4 e32 as tests/test_gpu_convblock.py and test_gpu_hourglass.py define it (e32 = the model's own float32 run against its float64 run on the test's inputs).
The backward is checked against the model's gradient AT the GPU forward's tape, and against pure float64 with the forward's error (e_fwd) added.  relu / leaky_relu:
at the tape the model takes the sign of every pre-activation from the kernel's own h, so no element has to be left out; tests/test_host_former_model.py checks that
at most 1 % of a case's pre-activations are within float32 reach of 0.  Measured ratios: tests/golden/former.md."""
import ctypes as C

import numpy as np
import pytest
import torch

import former_cases as FC
import former_model as FM

pytestmark = pytest.mark.gpu


def dv(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype).contiguous()


def gpu_run(c, dy=None, want_dx=True, want=None, out=None, accumulate=False):
    from vistracker_amd import ops
    params = [dv(c["P"][k]) for k in FM.PARAM_KEYS]
    x, pos, m = dv(c["x"]), dv(c["pos"]), (None if c["m"] is None else dv(c["m"], torch.uint8))
    y, tape = ops.former_layer_forward(x, pos, m, params, c["H"], c["act"], c["p"], c["dseed"])
    d_x, grads = ops.former_layer_backward(dv(c["dy"]) if dy is None else dy, tape, x, pos, m, params, c["H"], c["act"], c["p"], c["dseed"], want_dx=want_dx, want=want,
                                           out=out, accumulate=accumulate)
    res = {"y": y, "d_x": d_x}
    res.update(dict(zip(FM.PARAM_KEYS, grads)))
    views = ops.former_tape_views(tape, c["B"], c["T"], c["D"], c["H"], c["F"])
    return res, {k: v.cpu().numpy().astype(np.float64) for k, v in views.items()}


def check(what, got, truth, e32, e_extra=None):
    """per tensor: error <= 4 e32 (+ e_extra, outside the factor)"""
    bad = []
    for n, t in truth.items():
        e, x = e32[n], (e_extra[n] if e_extra else 0.0)
        g = got[n]
        err = float(np.abs((g.detach().cpu().numpy() if torch.is_tensor(g) else g).astype(np.float64) - t).max())
        print(f"\n[{what}] {n:>28}: e32 {e:.3e} | kernel error {err:.3e} ({(err - x) / e if e > 0 else 0.0:.2f})", end="")
        if not (np.isfinite(err) and err <= 4 * e + x):
            bad.append((n, err, e, x))
    assert not bad, bad


def check_tape(c, tape):
    """what the forward saved, so that a wrongly saved tensor cannot move the truth it is later judged by.
    q|k|v, O, y1, h: against the float64 forward at 4 e32.  The row statistics are fp64 functions of a tensor that is exact (x) or gated (y1): 1e-12 relative
    against float64 statistics of that tensor -- tighter than e32, which over the one or four elements these tensors have at T = 1 is a draw, not a scale (the
    first run measured lse at 4.2 e32 and mean2 at 24 e32 there, with y1 and q|k|v inside their gates).  The log-sum-exp is a float32 function of the saved q|k:
    against float64 from those, within the float32 reach of a score -- (hd + 2) 2^-24 sum_d |q_d k_d| scale, the bound of a float32 dot product of hd terms and
    its scaling -- plus 4 x 2^-24 |lse| for expf, the sum, logf and the final addition."""
    S, D, H = c["S"], c["D"], c["H"]
    big = ("qkv", "O", "y1", "h")
    check(c["id"] + " tape", {"tape/" + k: tape[k] for k in big}, {"tape/" + k: np.asarray(S[k], dtype=np.float64) for k in big}, c["e32"])
    _, _, m1, r1 = FM._ln(c["x"], 1.0, 0.0)
    _, _, m2, r2 = FM._ln(tape["y1"], 1.0, 0.0)
    for k, t in (("mean1", m1), ("rstd1", r1), ("mean2", m2), ("rstd2", r2)):
        err = float(np.abs(tape[k] - t).max())
        assert err <= 1e-12 * max(1.0, float(np.abs(t).max())), (k, err)
    hd = D // H
    q, k = FM._heads(tape["qkv"][..., :D], H), FM._heads(tape["qkv"][..., D:2 * D], H)
    scale = 1 / np.sqrt(hd)
    s = np.einsum("bhid,bhjd->bhij", q, k) * scale
    reach = np.einsum("bhid,bhjd->bhij", np.abs(q), np.abs(k)) * scale * (hd + 2) * 2.0 ** -24
    if c["m"] is not None:
        s = np.where(c["m"][:, None, None, :], -np.inf, s); reach = np.where(c["m"][:, None, None, :], 0.0, reach)
    mx = s.max(-1, keepdims=True)
    lse = (mx + np.log(np.exp(s - mx).sum(-1, keepdims=True)))[..., 0]
    bound = reach.max(-1) + 4 * 2.0 ** -24 * np.abs(lse)
    err = np.abs(tape["lse"] - lse)
    print(f"\n[{c['id']} tape] lse: largest error / bound {float((err / bound).max()):.3f}", end="")
    assert (err <= bound).all(), float((err / bound).max())


def against_model(c):
    got, tape = gpu_run(c)
    check(c["id"] + " forward", got, {"y": c["g64"]["y"]}, c["e32"])
    # what the forward saved, against the float64 forward: a wrongly saved tensor must not move the truth it is later judged by
    check_tape(c, tape)
    at_tape, _ = FM.run(c["P"], c["x"], c["pos"], c["m"], c["dy"], c["H"], c["act"], c["p"], c["dseed"], tape=tape)
    at_tape.pop("y")
    check(c["id"] + " at the tape", got, at_tape, c["e32"])
    e_fwd = {n: float(np.abs(at_tape[n] - c["g64"][n]).max()) for n in at_tape}
    check(c["id"] + " against float64", got, {n: c["g64"][n] for n in at_tape}, c["e32"], e_extra=e_fwd)


@pytest.mark.parametrize("c", FC.layer_cases(), ids=lambda c: c["id"])
def test_layer_every_tiling_edge(c):
    against_model(FC.build(c))


@pytest.mark.parametrize("c", FC.small_cases(), ids=lambda c: c["id"])
def test_layer_masks_and_activations(c):
    against_model(FC.build(c))


@pytest.mark.parametrize("c", FC.dropout_cases(), ids=lambda c: c["id"])
def test_layer_dropout_equals_the_hashed_model(c):
    against_model(FC.build(c, c["p"], c["dseed"]))


def _bits(c):
    return FC.build(dict(id="bits", B=3, T=33, D=32, H=2, F=64, act="gelu", mask="block", seed=61))


def test_layer_bitwise_properties():
    c = _bits(None)
    a, _ = gpu_run(c)
    b, _ = gpu_run(c)
    assert all(torch.equal(a[k], b[k]) for k in a)
    for k in (-20, 20):
        s, _ = gpu_run(c, dy=dv(c["dy"]) * 2.0 ** k)
        assert all(torch.equal(s[n], a[n] * 2.0 ** k) for n in a if n != "y"), k
    # NULL outputs are skipped and leave the others' bits
    want = [i % 3 == 0 for i in range(12)]
    part, _ = gpu_run(c, want_dx=False, want=want)
    assert part["d_x"] is None
    for k, w in zip(FM.PARAM_KEYS, want):
        assert (part[k] is None) if not w else torch.equal(part[k], a[k]), k
    # accumulate adds onto every output
    r = np.random.RandomState(2)
    start = {k: dv(r.randn(*a[k].shape)) for k in a if k != "y"}
    acc, _ = gpu_run(c, out=(start["d_x"].clone(), [start[k].clone() for k in FM.PARAM_KEYS]), accumulate=True)
    assert all(torch.equal(acc[k], start[k] + a[k]) for k in start)


def test_layer_clip_alone_equals_clip_in_batch():
    c = _bits(None)
    full, _ = gpu_run(c)
    for b in range(c["B"]):
        one = dict(c, B=1, x=c["x"][b:b + 1], dy=c["dy"][b:b + 1], m=c["m"][b:b + 1])
        alone, _ = gpu_run(one)
        assert torch.equal(alone["y"][0], full["y"][b]) and torch.equal(alone["d_x"][0], full["d_x"][b]), b


def test_unsupported_shapes_are_refused_and_write_nothing():
    from vistracker_amd import _lib as L, ops
    lib = L.lib()
    for (B, T, D, H, F) in ((1, 193, 32, 2, 64), (1, 16, 48, 1, 64), (1, 16, 40, 1, 64), (1, 16, 32, 2, 272), (1, 16, 32, 2, 72), (1, 0, 32, 2, 64), (1, 16, 176, 1, 64)):
        assert lib.vt_former_layer_tape_floats(B, T, D, H, F) == -1 and lib.vt_former_layer_workspace_floats(B, T, D, H, F) == -1
        n = max(1, B * T * D)
        x = torch.zeros(4 * n + 4096, device="cuda"); y = torch.full((n,), 7.0, device="cuda")
        ptrs = (C.c_void_p * 12)(*[x.data_ptr()] * 12)
        rc = lib.vt_former_layer_forward(x.data_ptr(), x.data_ptr(), None, ptrs, B, T, D, H, F, 1, 0.0, 0, y.data_ptr(), None, x.data_ptr(), L.stream_ptr())
        assert rc == L.VT_ERR_ARG and bool((y == 7.0).all())
    with pytest.raises(L.VtError):
        ops.former_layer_forward(torch.zeros(1, 193, 32, device="cuda"), torch.zeros(193, 32, device="cuda"), None, [torch.zeros(1, device="cuda")] * 4 +
                                 [torch.zeros(64, 32, device="cuda")] + [torch.zeros(1, device="cuda")] * 7, 2, "gelu")


def test_inference_forward_without_a_tape_equals_the_taped_one():
    from vistracker_amd import ops
    c = _bits(None)
    params = [dv(c["P"][k]) for k in FM.PARAM_KEYS]
    x, pos, m = dv(c["x"]), dv(c["pos"]), dv(c["m"], torch.uint8)
    y0, _ = ops.former_layer_forward(x, pos, m, params, c["H"], c["act"])
    y1, t = ops.former_layer_forward(x, pos, m, params, c["H"], c["act"], tape=False)
    assert t is None and torch.equal(y0, y1)


def test_layernorm_entry_points():
    """vt_layernorm_forward / _backward through the C ABI at a ragged M with more than one chunk: against the model, NULL outputs, accumulate"""
    from vistracker_amd import _lib as L
    lib = L.lib()
    M, D = 1301, 160
    r = np.random.RandomState(4)
    f = lambda a: a.astype(np.float32).astype(np.float64)                     # noqa: E731
    x, dy, w, b = f(r.randn(1, M, D) * 2 + 0.5), f(r.randn(1, M, D)), f(1 + 0.2 * r.randn(D)), f(0.1 * r.randn(D))
    res = {}
    for dt in (np.float64, np.float32):
        y, xh, _, rstd = FM._ln(x.astype(dt), w.astype(dt), b.astype(dt))
        dx, dw, db = FM._ln_bwd(dy.astype(dt), xh, rstd, w.astype(dt))
        res[dt] = {k: np.asarray(v, dtype=np.float64) for k, v in dict(y=y, d_x=dx, d_w=dw, d_b=db).items()}
    e32 = {k: float(np.abs(res[np.float32][k] - res[np.float64][k]).max()) for k in res[np.float64]}
    X, DY, W, Bb = dv(x), dv(dy), dv(w), dv(b)
    ws = torch.empty(int(lib.vt_layernorm_backward_workspace_floats(M, D)), device="cuda")

    def run(want=(True, True, True), start=None, accumulate=0):
        y = torch.empty_like(X); st = torch.empty(M, 2, dtype=torch.float64, device="cuda")
        L.check(lib.vt_layernorm_forward(X.data_ptr(), W.data_ptr(), Bb.data_ptr(), M, D, y.data_ptr(), st.data_ptr(), L.stream_ptr()))
        o = [t.clone() for t in start] if start else [torch.empty_like(X), torch.empty_like(W), torch.empty_like(W)]
        o = [t if k else None for t, k in zip(o, want)]
        L.check(lib.vt_layernorm_backward(DY.data_ptr(), X.data_ptr(), st.data_ptr(), W.data_ptr(), M, D, *[None if t is None else t.data_ptr() for t in o], accumulate,
                                          ws.data_ptr(), L.stream_ptr()))
        return dict(y=y, d_x=o[0], d_w=o[1], d_b=o[2])

    full = run()
    check("layernorm", full, res[np.float64], e32)
    part = run(want=(False, True, False))
    assert part["d_x"] is None and part["d_b"] is None and torch.equal(part["d_w"], full["d_w"])
    part = run(want=(True, False, True))
    assert part["d_w"] is None and torch.equal(part["d_x"], full["d_x"]) and torch.equal(part["d_b"], full["d_b"])
    start = [dv(r.randn(1, M, D)), dv(r.randn(D)), dv(r.randn(D))]
    acc = run(start=start, accumulate=1)
    assert all(torch.equal(acc[k], s0 + full[k]) for k, s0 in zip(("d_x", "d_w", "d_b"), start))
    assert lib.vt_layernorm_backward_workspace_floats(M, 24) == -1
    assert lib.vt_layernorm_forward(X.data_ptr(), W.data_ptr(), Bb.data_ptr(), M, 24, X.data_ptr(), None, L.stream_ptr()) == L.VT_ERR_ARG


def test_wrong_dtypes_and_shapes_are_refused():
    from vistracker_amd import _lib as L, ops
    c = _bits(None)
    params = [dv(c["P"][k]) for k in FM.PARAM_KEYS]
    x, pos = dv(c["x"]), dv(c["pos"])
    with pytest.raises(L.VtError):
        ops.former_layer_forward(x.double(), pos, None, params, c["H"], c["act"])
    with pytest.raises(L.VtError):
        ops.former_layer_forward(x, pos[:-1].contiguous(), None, params, c["H"], c["act"])
    with pytest.raises(L.VtError):
        ops.former_layer_forward(x, pos, None, params[:4] + [params[4][:, :-16].contiguous()] + params[5:], c["H"], c["act"])
    with pytest.raises(L.VtError):
        ops.former_layer_forward(x, pos, torch.zeros(c["B"], c["T"] + 1, dtype=torch.bool, device="cuda"), params, c["H"], c["act"])
    with pytest.raises(L.VtError):
        ops.layernorm_train(x.double(), params[8], params[9])
    with pytest.raises(L.VtError):
        ops.layernorm_train(x, params[8][:-1], params[9])
