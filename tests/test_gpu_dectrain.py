"""GPU: vt_decoder_train_forward / vt_decoder_weight_grads (csrc/dectrain.hip), ops.DecoderParams, ops.sifnet_query_train, SIFNetQuery.query_train and
training.DecoderTrainer against the float64 model of tests/dectrain_model.py and the reference's recorded values (tests/golden/dectrain.npz).

Every bound is MEASURED, not chosen (the convention of tests/test_gpu_losshead.py and tests/test_gpu_boundary.py): e32 = the float32 run of the model against
its float64 run on the inputs of the test, and the kernel gets 4 e32 -- per head for the predictions, and per PARAMETER TENSOR for the gradients: 40 bounds, each
on its tensor's own scale (a whole-array metric hid a 7 % error in one joint of the SMPL-H backward once).  For the recorded case the float32 run is the
reference's own.  Inputs: B = 2, N = 150 (two full 64-point tiles and one of 22) with points outside the image, outside each orthographic plane and on exact
texel coordinates among the bulk (dectrain_model.make_inputs; the classes are asserted non-empty below)."""
import ctypes as C

import numpy as np
import pytest
import torch

import dectrain_model as M
from conftest import golden

pytestmark = pytest.mark.gpu
B, N = 2, 150


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def split(flat):
    """flat gradient (device or host tensor) -> {(head, layer, kind): float64 array} through the library's offsets"""
    from vistracker_amd import ops
    p = ops.DecoderParams(flat.detach().cpu().clone())
    return {k: v.numpy().astype(np.float64) for k, v in p.views.items()}


def check_grads(got, ref, e32, what, keys=M.TENSORS):
    bad = []
    print(f"\n[{what}] per tensor: e32 | kernel error | largest element")
    for k in keys:
        assert np.isfinite(got[k]).all(), (what, k)
        err = np.abs(got[k] - ref["grads"][k]).max()
        print(f"  {k[0]:>7}.{k[1]}.{k[2]:<6} {e32['grads'][k]:.3e} {err:.3e} {np.abs(ref['grads'][k]).max():.3e}")
        if not err <= 4 * e32["grads"][k]:
            bad.append((k, err, e32["grads"][k]))
    assert not bad, (what, bad)


def check_preds(got, ref, e32, what, s=0):
    for i, h in enumerate(M.HEADS):
        g = got[i].detach().cpu().numpy().reshape(ref["preds"][s][i].shape).astype(np.float64)
        err = np.abs(g - ref["preds"][s][i]).max()
        print(f"\n[{what}] {h}: e32 {e32['preds'][s][i]:.3e} kernel {err:.3e}", end="")
        assert np.isfinite(g).all() and err <= 4 * e32["preds"][s][i], (what, h, err, e32["preds"][s][i])


@pytest.fixture(scope="module")
def env():
    """decoders, two map sets that share their tmpx tensors (chore_triplane.py:139-149), the points -- on the host and on the device"""
    from vistracker_amd import ops, synthetic as syn
    dec = syn.sifnet_decoders(3)
    maps = syn.feature_maps(B, res_scale=0.125)
    other = syn.feature_maps(B, seed=9, res_scale=0.125)
    maps2 = {k: (maps[k] if "tmpx" in k else other[k]) for k in maps}
    pts, cc, bc = M.make_inputs(B, N, seed=11)
    e = {"dec": dec, "maps": [maps, maps2], "pts": pts, "cc": cc, "bc": bc, "fm": [ops.FeatureMaps.from_nchw(maps), ops.FeatureMaps.from_nchw(maps2)],
         "d": tuple(dev(a) for a in (pts, cc, bc)), "up": [M.make_upstream(B, N, seed=12), M.make_upstream(B, N, seed=13)]}
    e["ref1"] = M.reference_and_e32(dec, [maps], pts, cc, bc, upstream=[e["up"][0]])
    return e


def params_of(env):
    from vistracker_amd import ops
    return ops.DecoderParams.from_decoders(env["dec"])


def raw_grads(env, params, fm, up, chunk=0, accumulate=0, dflat=None, ws=None, pts=None, cc=None, bc=None):
    """one vt_decoder_weight_grads call -> the flat gradient (device tensor); ``up``: head -> array, a missing head = NULL"""
    from vistracker_amd import _lib as L
    pts, cc, bc = env["d"] if pts is None else (pts, cc, bc)
    b, n = pts.shape[:2]
    g = [dev(up[h]) if h in up else None for h in M.HEADS]
    dflat = torch.empty_like(params.flat.detach()) if dflat is None else dflat
    nbytes = L.lib().vt_decoder_weight_grads_ws_bytes(b, n, chunk)
    assert nbytes > 0
    ws = torch.empty(nbytes // 4 + 4, device="cuda") if ws is None else ws
    assert ws.numel() * 4 >= nbytes
    L.check(L.lib().vt_decoder_weight_grads(L.dptr(params.flat.detach()), params.cam.ctypes.data, C.byref(fm.c), L.dptr(pts), L.dptr(cc), L.dptr(bc), b, n,
                                            *[L.dptr(t) for t in g], L.dptr(dflat), accumulate, chunk, L.dptr(ws), L.stream_ptr()))
    return dflat


# ---- a: forward ----------------------------------------------------------------------------------------------------------------------------------------------
def test_a_forward_every_head(env):
    from vistracker_amd import ops
    cls = M.point_classes(env["maps"][0], env["pts"], env["cc"], env["bc"])
    for k in ("outside_image", "outside_right", "outside_back", "outside_top", "exact_texel", "bulk"):
        assert cls[k].any(), k
    ref, e32 = env["ref1"]
    preds = ops.sifnet_query_train(params_of(env), env["fm"][0], *env["d"])
    assert len(preds) == 1 and tuple(preds[0][1].shape) == (B, 3, 3, N)
    check_preds(preds[0], ref, e32, "a forward")
    df = preds[0][0].detach().cpu().numpy().transpose(0, 2, 1)
    assert (df[cls["outside_image"]] == M.OUT_DIST).all()


# ---- b: weight gradients -------------------------------------------------------------------------------------------------------------------------------------
def test_b_weight_gradients_random_upstream(env):
    from vistracker_amd import ops
    ref, e32 = env["ref1"]
    p = params_of(env)
    preds = ops.sifnet_query_train(p, env["fm"][0], *env["d"])
    sum((t.reshape(B, k, N) * dev(env["up"][0][h])).sum() for t, h, k in zip(preds[0], M.HEADS, M.DIMS)).backward()
    check_grads(split(p.flat.grad), ref, e32, "b(i) random upstream, five heads")


def test_b_weight_gradients_through_get_errors(env, synth):
    from vistracker_amd.sifnet import SIFNetQuery
    lab = M.make_labels(B, N, seed=14)
    ref, e32 = M.reference_and_e32(env["dec"], [env["maps"][0]], env["pts"], env["cc"], env["bc"], labels=lab)
    net = SIFNetQuery(env["dec"])
    net.set_feature_maps(env["fm"][0])
    p = params_of(env)
    net.query_train(p, env["d"][0], crop_center=env["d"][1], body_center=env["d"][2])
    assert len(net.intermediate_preds_list) == 1 and net.preds is net.intermediate_preds_list[0]
    error, losses_all = net.get_errors(dev(lab["df_h"]), dev(lab["df_o"]), dev(lab["labels"], torch.int32), dev(lab["pca_axis"]), 5.0, env["d"][2],
                                       dev(lab["obj_center"]), visibility=dev(lab["visibility"]))
    error.backward()
    err = np.abs(losses_all.cpu().numpy() - ref["losses_all"])
    print(f"\nlosses_all (the loss head has its own test; a mean's float32 error cancels to almost nothing, so it is no bound): e32 {e32['losses_all'].tolist()} "
          f"kernel {err.tolist()}")
    assert np.isfinite(err).all()
    check_grads(split(p.flat.grad), ref, e32, "b(ii) get_errors, S = 1")


# ---- c: chunks, determinism, the smallest call ---------------------------------------------------------------------------------------------------------------
def test_c_chunks_determinism_single_point(env):
    ref, e32 = env["ref1"]
    p = params_of(env)
    g_def = raw_grads(env, p, env["fm"][0], env["up"][0])
    g_64 = raw_grads(env, p, env["fm"][0], env["up"][0], chunk=64)              # three chunks a frame, the last of 22 points
    check_grads(split(g_def), ref, e32, "c default chunk")
    check_grads(split(g_64), ref, e32, "c chunk_points = 64")
    assert torch.equal(raw_grads(env, p, env["fm"][0], env["up"][0]), g_def) and torch.equal(raw_grads(env, p, env["fm"][0], env["up"][0], chunk=64), g_64)
    # B = 1, N = 1
    pts, cc, bc = env["pts"][:1, 5:6], env["cc"][:1], env["bc"][:1]
    up = {h: a[:1, :, 5:6] for h, a in env["up"][0].items()}
    maps1 = {k: v[:1] for k, v in env["maps"][0].items()}
    r1, e1 = M.reference_and_e32(env["dec"], [maps1], pts, cc, bc, upstream=[up])
    g1 = raw_grads(env, p, env["fm"][0].slice(0, 1), up, pts=dev(pts), cc=dev(cc), bc=dev(bc))
    check_grads(split(g1), r1, e1, "c B = 1, N = 1")
    from vistracker_amd import _lib as L
    fm = env["fm"][0]
    for bad in (dict(chunk=100), dict(chunk=-64), dict(chunk=32768)):
        assert L.lib().vt_decoder_weight_grads_ws_bytes(B, N, bad["chunk"]) == -1
        rc = L.lib().vt_decoder_weight_grads(L.dptr(p.flat.detach()), p.cam.ctypes.data, C.byref(fm.c), *[L.dptr(t) for t in env["d"]], B, N, None, None, None, None,
                                             None, L.dptr(g_def), 0, bad["chunk"], L.dptr(g_def), L.stream_ptr())
        assert rc == L.VT_ERR_ARG


# ---- d: stacks and accumulate --------------------------------------------------------------------------------------------------------------------------------
def test_d_two_stacks_and_accumulate(env):
    from vistracker_amd import ops
    ref, e32 = M.reference_and_e32(env["dec"], env["maps"], env["pts"], env["cc"], env["bc"], upstream=env["up"])
    p = params_of(env)
    preds = ops.sifnet_query_train(p, env["fm"], *env["d"])
    assert len(preds) == 2
    for s in range(2):
        check_preds(preds[s], ref, e32, f"d stack {s}", s)
    sum((t.reshape(B, k, N) * dev(env["up"][s][h])).sum() for s in range(2) for t, h, k in zip(preds[s], M.HEADS, M.DIMS)).backward()
    joint = split(p.flat.grad)
    check_grads(joint, ref, e32, "d two stacks, one backward")
    sep = [split(raw_grads(env, p, env["fm"][s], env["up"][s])) for s in range(2)]
    for k in M.TENSORS:
        assert np.abs(joint[k] - (sep[0][k] + sep[1][k])).max() <= 4 * e32["grads"][k], k
    one = raw_grads(env, p, env["fm"][0], env["up"][0])
    two = raw_grads(env, p, env["fm"][0], env["up"][0], accumulate=1, dflat=one.clone())
    a, b = two.double().cpu().numpy(), 2 * one.double().cpu().numpy()
    assert (np.abs(a - b) <= np.abs(b) * 2.0 ** -23).all()


# ---- e: zeros, poison ----------------------------------------------------------------------------------------------------------------------------------------
def test_e_null_heads_zero_upstream_poisoned_buffers(env):
    from vistracker_amd import _lib as L
    p = params_of(env)
    full = raw_grads(env, p, env["fm"][0], env["up"][0])
    for drop in M.HEADS:
        g = split(raw_grads(env, p, env["fm"][0], {h: a for h, a in env["up"][0].items() if h != drop}))
        f = split(full)
        for k in M.TENSORS:
            if k[0] == drop:
                assert (g[k] == 0).all(), k
            else:
                assert np.array_equal(g[k], f[k]), k                                 # the heads do not see each other
    assert (raw_grads(env, p, env["fm"][0], {}) == 0).all()
    assert (raw_grads(env, p, env["fm"][0], {h: np.zeros_like(a) for h, a in env["up"][0].items()}) == 0).all()
    for chunk in (0, 64):
        want = raw_grads(env, p, env["fm"][0], env["up"][0], chunk=chunk)
        ws = torch.full((L.lib().vt_decoder_weight_grads_ws_bytes(B, N, chunk) // 4 + 4,), float("nan"), device="cuda")
        got = raw_grads(env, p, env["fm"][0], env["up"][0], chunk=chunk, ws=ws, dflat=torch.full_like(want, float("nan")))
        assert torch.equal(got, want), chunk


# ---- f: the train step ---------------------------------------------------------------------------------------------------------------------------------------
F_N, F_STEPS = 512, 20


def test_f_decoder_trainer(env):
    """DecoderTrainer, 20 steps of lr 1e-3 on one fixed labelled batch (B = 2, N = 512, 1/8-resolution maps, labels of dectrain_model.make_labels).  The float64
    model with torch.optim.Adam on the CPU (dectrain_model.train_model, run by this test first) takes the total error of this batch from 1405.157 to 187.725: a
    drop of 1217.432.  The trainer must reach at least half of the model's drop, with every intermediate error finite.  No parameter trajectories are compared:
    Adam's first steps are +- lr whatever the gradient's size, so rounding decides the signs near zero."""
    from vistracker_amd import training
    from vistracker_amd.sifnet import SIFNetQuery
    pts, cc, bc = M.make_inputs(B, F_N, seed=21)
    lab = M.make_labels(B, F_N, seed=22)
    model = M.train_model(env["dec"], env["maps"][0], pts, cc, bc, lab, F_STEPS + 1)
    drop = model[0] - model[-1]
    print(f"\nfloat64 model: error {model[0]:.4f} -> {model[-1]:.4f} after {F_STEPS} steps, drop {drop:.4f}")
    assert drop > 0
    net = SIFNetQuery(env["dec"])
    net.set_feature_maps(env["fm"][0])
    tr = training.DecoderTrainer(net, lr=1e-3)
    batch = {"points": dev(pts), "body_center": dev(bc), **{k: dev(v, torch.int32 if k == "labels" else torch.float32) for k, v in lab.items()}}
    errors = []
    for _ in range(F_STEPS + 1):
        error, losses_all = tr.train_step(batch, dev(cc))
        assert error.is_cuda and error.dtype == torch.float64 and tuple(losses_all.shape) == (6,)
        errors.append(error)
    errors = torch.stack(errors).cpu().numpy()
    print(f"DecoderTrainer: error {errors[0]:.4f} -> {errors[-1]:.4f}, drop {errors[0] - errors[-1]:.4f}")
    assert np.isfinite(errors).all()
    assert errors[0] - errors[-1] >= 0.5 * drop
    # the trained decoders validate at the last error's level through the packed kernels
    val = training.validate(tr.export(), batch, dev(cc))
    assert np.isfinite(val["total"]) and val["total"] < errors[0] - 0.5 * drop


# ---- g: export, state_dict -----------------------------------------------------------------------------------------------------------------------------------
def test_g_export_pins_the_flat_layout(env):
    from vistracker_amd import ops, training
    from vistracker_amd.sifnet import SIFNetQuery
    ref, e32 = env["ref1"]
    net = SIFNetQuery(env["dec"])
    net.set_feature_maps(env["fm"][0])
    tr = training.DecoderTrainer(net)
    with torch.no_grad():
        tr.params.flat.mul_(1.03125)                                                # not the weights `net` was built with (exact in float32)
    dec2 = tr.params.to_decoders()
    r2, e2 = M.reference_and_e32(dec2, [env["maps"][0]], env["pts"], env["cc"], env["bc"])
    plain = ops.sifnet_query_train(tr.params, env["fm"][0], *env["d"])[0]
    check_preds(plain, r2, e2, "g plain weights")
    out = tr.export()
    out.handle.set_precision("fp32")
    out.query(env["d"][0], crop_center=env["d"][1], body_center=env["d"][2])
    check_preds(out.get_preds(), r2, e2, "g export -> strict-fp32 query")
    for i, h in enumerate(M.HEADS):
        d = float((out.get_preds()[i].reshape(B, -1, N) - plain[i].reshape(B, -1, N)).abs().max())
        assert d <= 4 * e2["preds"][0][i], (h, d)
    before = tr.params.flat.detach().clone()
    sd = tr.state_dict()
    assert all(v.is_cuda for v in sd.values()) and tuple(sd["df.0.weight"].shape) == (128, 611, 1)
    tr.params.load_state_dict(sd)
    assert torch.equal(tr.params.flat.detach(), before)
    from vistracker_amd import _lib as L
    with pytest.raises(L.VtError):                                                  # the points are data here: one that requires grad raises, loudly
        ops.sifnet_query_train(tr.params, env["fm"][0], env["d"][0].clone().requires_grad_(True), env["d"][1], env["d"][2])


# ---- h: the reference's recorded values ----------------------------------------------------------------------------------------------------------------------
def test_h_recorded_reference(env):
    """|kernel - golden| <= 4 |golden - float64 model|, per prediction head and per recorded gradient tensor: the reference's own float32 error on these inputs"""
    from vistracker_amd import ops
    g = golden("dectrain")
    assert np.array_equal(g["pts"], env["pts"]) and all(np.array_equal(g["up_" + h], env["up"][0][h]) for h in M.HEADS)
    r64 = env["ref1"][0]
    p = params_of(env)
    preds = ops.sifnet_query_train(p, env["fm"][0], *env["d"])[0]
    sum((t.reshape(B, k, N) * dev(env["up"][0][h])).sum() for t, h, k in zip(preds, M.HEADS, M.DIMS)).backward()
    got = split(p.flat.grad)
    rows = list(g["rows"])
    bad = []
    for i, h in enumerate(M.HEADS):
        e = np.abs(g["pred_" + h] - r64["preds"][0][i]).max()
        err = np.abs(preds[i].detach().cpu().numpy().reshape(B, -1, N) - g["pred_" + h]).max()
        print(f"\n[h] {h}: e32 {e:.3e} |kernel - golden| {err:.3e}", end="")
        if not err <= 4 * e:
            bad.append((h, err, e))
        for l in range(4):
            for kind in ("weight", "bias"):
                sub = (lambda a: a[rows] if kind == "weight" and l < 3 else a)      # noqa: E731
                want = g[f"g_{h}_{l}_{kind}"].astype(np.float64)
                e = np.abs(want - sub(r64["grads"][(h, l, kind)])).max()
                err = np.abs(sub(got[(h, l, kind)]) - want).max()
                print(f"\n    {l}.{kind}: e32 {e:.3e} |kernel - golden| {err:.3e}", end="")
                if not err <= 4 * e:
                    bad.append((h, l, kind, err, e))
    assert not bad, bad
