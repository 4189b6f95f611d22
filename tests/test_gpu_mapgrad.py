"""GPU: vt_decoder_grads (csrc/dectrain.hip, section 5) -- the gradient of the decoder training step to the eight feature maps -- through the C ABI,
ops.sifnet_query_train, SIFNetQuery.query_train and training.DecoderTrainer, against the float64 model of tests/mapgrad_model.py and the reference's recorded
autograd gradients (tests/golden/mapgrad.npz).

Every bound is MEASURED (the convention of tests/test_gpu_dectrain.py): e32 = the float32 run of the model against its float64 run on the inputs of the test,
per MAP TENSOR, and the kernel gets 4 e32.  Maps at res_scale = 0.125 (16^2 and 32^2 texels): 150 points collide on texels everywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import dectrain_model as M
import mapgrad_model as G
from conftest import golden

pytestmark = pytest.mark.gpu
B, N = 2, 150


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def nchw(t):
    return t.detach().permute(0, 3, 1, 2).cpu().numpy().astype(np.float64)


def check_maps(got, ref, e32, what, s=0):
    """got: the eight NHWC device gradients in map order"""
    bad = []
    print(f"\n[{what}] per map: e32 | kernel error | largest element")
    for n, t in zip(G.MAPS, got):
        g, want, e = nchw(t), ref["dmaps"][s][n], e32["dmaps"][s][n]
        assert g.shape == want.shape and np.isfinite(g).all(), (what, n)
        err = np.abs(g - want).max()
        print(f"  {n:>10} {e:.3e} {err:.3e} {np.abs(want).max():.3e}")
        if not err <= 4 * e:
            bad.append((n, err, e))
    assert not bad, (what, bad)


@pytest.fixture(scope="module")
def env():
    from vistracker_amd import ops, synthetic as syn
    dec = syn.sifnet_decoders(3)
    maps = syn.feature_maps(B, res_scale=0.125)
    other = syn.feature_maps(B, seed=9, res_scale=0.125)
    maps2 = {k: (maps[k] if "tmpx" in k else other[k]) for k in maps}
    pts, cc, bc = M.make_inputs(B, N, seed=11)
    e = {"dec": dec, "maps": [maps, maps2], "pts": pts, "cc": cc, "bc": bc, "fm": [ops.FeatureMaps.from_nchw(maps), ops.FeatureMaps.from_nchw(maps2)],
         "d": tuple(dev(a) for a in (pts, cc, bc)), "up": [M.make_upstream(B, N, seed=12), M.make_upstream(B, N, seed=13)]}
    e["ref1"] = G.reference_and_e32(dec, [maps], pts, cc, bc, upstream=[e["up"][0]])
    return e


def params_of(env):
    from vistracker_amd import ops
    return ops.DecoderParams.from_decoders(env["dec"])


def raw(env, params, fm, up, chunk=0, want=(1,) * 8, weights=True, acc_maps=0, dmaps=None, ws=None, pts=None, cc=None, bc=None, fill=None, rc_only=False, dres=None):
    """one vt_decoder_grads call -> (flat gradient or None, the eight map gradients (None where not requested))"""
    from vistracker_amd import _lib as L
    pts, cc, bc = env["d"] if pts is None else (pts, cc, bc)
    b, n = pts.shape[:2]
    g = [dev(up[h]) if h in up else None for h in M.HEADS]
    dflat = torch.empty_like(params.flat.detach()) if weights else None
    if dmaps is None:
        dmaps = [(torch.empty_like(t) if fill is None else torch.full_like(t, fill)) if w else None for t, w in zip(fm.t, want)]
    dm = L.VtMaps()
    for i, t in enumerate(fm.t):
        dm.res[i] = t.shape[1] if dres is None else dres[i]
        dm.maps[i] = None if dmaps[i] is None else dmaps[i].data_ptr()
    nbytes = L.lib().vt_decoder_grads_ws_bytes(b, n, chunk, 1)
    assert nbytes > 0
    ws = (torch.empty(nbytes // 4 + 4, device="cuda") if fill is None else torch.full((nbytes // 4 + 4,), fill, device="cuda")) if ws is None else ws
    rc = L.lib().vt_decoder_grads(L.dptr(params.flat.detach()), params.cam.ctypes.data, C.byref(fm.c), L.dptr(pts), L.dptr(cc), L.dptr(bc), b, n,
                                  *[L.dptr(t) for t in g], L.dptr(dflat), 0, C.byref(dm), acc_maps, chunk, L.dptr(ws), L.stream_ptr())
    if rc_only:
        return rc
    L.check(rc)
    return dflat, dmaps


def weight_grads(env, params, fm, up, chunk=0, pts=None, cc=None, bc=None):
    from vistracker_amd import _lib as L
    pts, cc, bc = env["d"] if pts is None else (pts, cc, bc)
    b, n = pts.shape[:2]
    g = [dev(up[h]) if h in up else None for h in M.HEADS]
    dflat = torch.empty_like(params.flat.detach())
    ws = torch.empty(L.lib().vt_decoder_weight_grads_ws_bytes(b, n, chunk) // 4 + 4, device="cuda")
    L.check(L.lib().vt_decoder_weight_grads(L.dptr(params.flat.detach()), params.cam.ctypes.data, C.byref(fm.c), L.dptr(pts), L.dptr(cc), L.dptr(bc), b, n,
                                            *[L.dptr(t) for t in g], L.dptr(dflat), 0, chunk, L.dptr(ws), L.stream_ptr()))
    return dflat


def leaf_maps(fm, share=None):
    """a FeatureMaps of fresh leaves that require grad (``share``: another one whose tmpx tensors are taken over, as the stacks of the reference share them)"""
    from vistracker_amd import ops
    d = {}
    for k, t in zip(ops.MAP_ORDER, fm.t):
        d[k] = share.t[ops.MAP_ORDER.index(k)] if share is not None and "tmpx" in k else t.detach().clone().requires_grad_(True)
    return ops.FeatureMaps(d)


# ---- a: random upstream, five heads --------------------------------------------------------------------------------------------------------------------------
def test_a_random_upstream_all_maps(env):
    from vistracker_amd import ops
    assert tuple(ops.MAP_ORDER) == G.MAPS
    ref, e32 = env["ref1"]
    p = params_of(env)
    dflat, dmaps = raw(env, p, env["fm"][0], env["up"][0])
    check_maps(dmaps, ref, e32, "a random upstream, five heads")
    assert torch.equal(dflat, weight_grads(env, p, env["fm"][0], env["up"][0]))


# ---- b: get_errors and error.backward() ----------------------------------------------------------------------------------------------------------------------
def test_b_through_get_errors(env):
    from vistracker_amd.sifnet import SIFNetQuery
    lab = M.make_labels(B, N, seed=14)
    ref, e32 = G.reference_and_e32(env["dec"], [env["maps"][0]], env["pts"], env["cc"], env["bc"], labels=lab)
    net = SIFNetQuery(env["dec"])
    flats = []
    for fm in (env["fm"][0], leaf_maps(env["fm"][0])):
        p = params_of(env)
        net.query_train(p, env["d"][0], crop_center=env["d"][1], body_center=env["d"][2], maps=fm)
        error, _ = net.get_errors(dev(lab["df_h"]), dev(lab["df_o"]), dev(lab["labels"], torch.int32), dev(lab["pca_axis"]), 5.0, env["d"][2],
                                  dev(lab["obj_center"]), visibility=dev(lab["visibility"]))
        error.backward()
        flats.append(p.flat.grad.clone())
    assert all(t.grad is not None and t.is_leaf for t in fm.t)
    check_maps([t.grad for t in fm.t], ref, e32, "b get_errors, S = 1")
    assert torch.equal(flats[0], flats[1])                                          # the weight gradient does not see whether the maps are leaves


# ---- c: slabs, chunks, determinism, the smallest call --------------------------------------------------------------------------------------------------------
def test_c_slab_and_chunk_edges(env):
    """chunk_points = 64 at N = 1100: 18 chunks a frame, 36 in all, two slabs of 32 and 4 -- the second starts inside frame 1, so frame 1's texels are fed from both"""
    n = 1100
    pts, cc, bc = M.make_inputs(B, n, seed=31)
    up = M.make_upstream(B, n, seed=32)
    ref, e32 = G.reference_and_e32(env["dec"], [env["maps"][0]], pts, cc, bc, upstream=[up])
    p, d = params_of(env), dict(pts=dev(pts), cc=dev(cc), bc=dev(bc))
    w64, m64 = raw(env, p, env["fm"][0], up, chunk=64, **d)
    wdef, mdef = raw(env, p, env["fm"][0], up, **d)
    check_maps(m64, ref, e32, "c chunk_points = 64, two slabs")
    check_maps(mdef, ref, e32, "c default chunk")
    for name, a, b_ in zip(G.MAPS, m64, mdef):
        assert float((a - b_).abs().max()) <= 4 * e32["dmaps"][0][name], name
    w2, m2 = raw(env, p, env["fm"][0], up, chunk=64, **d)
    assert torch.equal(w2, w64) and all(torch.equal(a, b_) for a, b_ in zip(m2, m64))
    print("\n[c] two calls, chunk_points = 64: identical bits; checksums", [float(t.double().sum()) for t in m64])
    assert torch.equal(w64, weight_grads(env, p, env["fm"][0], up, chunk=64, **d))
    # B = 1, N = 1
    pts1, cc1, bc1 = env["pts"][:1, 5:6], env["cc"][:1], env["bc"][:1]
    up1 = {h: a[:1, :, 5:6] for h, a in env["up"][0].items()}
    maps1 = {k: v[:1] for k, v in env["maps"][0].items()}
    r1, e1 = G.reference_and_e32(env["dec"], [maps1], pts1, cc1, bc1, upstream=[up1])
    _, m1 = raw(env, p, env["fm"][0].slice(0, 1), up1, pts=dev(pts1), cc=dev(cc1), bc=dev(bc1))
    check_maps(m1, r1, e1, "c B = 1, N = 1")


# ---- d: pile-up, boundaries, nothing inside ------------------------------------------------------------------------------------------------------------------
def test_d_pile_up_and_boundary(env):
    bc = env["bc"]
    boundary = np.array([[1, 0.3, 0.1], [-1, -0.2, 0.3], [0.1, 1, -0.2], [0.3, -1, 0.2], [0.2, 0.1, 1], [-0.3, 0.2, -1], [1, -1, 1], [-1, 1, -1]], np.float32)
    pts = np.empty((B, N, 3), np.float32)
    pts[0] = bc[0] + np.array([0.0625, -0.125, 0.03125], np.float32)               # every point of frame 0 is the same point: one cell per map gets everything
    pts[1] = bc[1] + boundary[np.arange(N) % len(boundary)]                          # plane coordinates of exactly -1 / +1: texel 0 / R - 1, each hit ~19 times
    up = M.make_upstream(B, N, seed=41)
    ref, e32 = G.reference_and_e32(env["dec"], [env["maps"][0]], pts, env["cc"], bc, upstream=[up])
    p = params_of(env)
    _, dm = raw(env, p, env["fm"][0], up, pts=dev(pts), cc=env["d"][1], bc=env["d"][2])
    check_maps(dm, ref, e32, "d pile-up (frame 0) and exact boundary texels (frame 1)")
    for t in dm:
        assert int((t[0].abs().sum(-1) != 0).sum()) <= 4                             # frame 0: the four texels of one cell, nothing else
    # frame 0 wholly outside the image and every plane: exact zeros there, frame 1 as ever
    pts2 = env["pts"].copy()
    pts2[0] = bc[0] + np.array([2.5, 2.0, 0.0], np.float32) + 0.01 * (env["pts"][0] - bc[0])
    ref2, e2 = G.reference_and_e32(env["dec"], [env["maps"][0]], pts2, env["cc"], bc, upstream=[env["up"][0]])
    assert all((ref2["dmaps"][0][n][0] == 0).all() for n in G.MAPS)
    _, dm2 = raw(env, p, env["fm"][0], env["up"][0], pts=dev(pts2), cc=env["d"][1], bc=env["d"][2], fill=float("nan"))
    check_maps(dm2, ref2, e2, "d frame 0 outside every map")
    assert all(bool((t[0] == 0).all()) for t in dm2)


# ---- e: two stacks that share their tmpx tensors -------------------------------------------------------------------------------------------------------------
def test_e_two_stacks_sharing_tmpx(env):
    from vistracker_amd import ops
    ref, e32 = G.reference_and_e32(env["dec"], env["maps"], env["pts"], env["cc"], env["bc"], upstream=env["up"])
    for n in G.MAPS:
        assert ("tmpx" in n) == np.array_equal(ref["dmaps"][0][n], ref["dmaps"][1][n]), n      # a shared tensor has ONE gradient, the sum over its stacks
    p = params_of(env)
    fm0 = leaf_maps(env["fm"][0]); fm1 = leaf_maps(env["fm"][1], share=fm0)
    preds = ops.sifnet_query_train(p, [fm0, fm1], *env["d"])
    sum((t.reshape(B, k, N) * dev(env["up"][s][h])).sum() for s in range(2) for t, h, k in zip(preds[s], M.HEADS, M.DIMS)).backward()
    check_maps([t.grad for t in fm0.t], ref, e32, "e stack 0 (tmpx: the sum of both stacks)", 0)
    check_maps([t.grad for t in fm1.t], ref, e32, "e stack 1", 1)
    # the same through two calls of the C entry, the second accumulating onto the shared tensors' buffers
    _, d0 = raw(env, p, env["fm"][0], env["up"][0])
    shared = [d0[i] if "tmpx" in n else torch.empty_like(d0[i]) for i, n in enumerate(G.MAPS)]
    raw(env, p, env["fm"][1], env["up"][1], want=[int("tmpx" not in n) for n in G.MAPS], dmaps=[None if "tmpx" in n else shared[i] for i, n in enumerate(G.MAPS)])
    raw(env, p, env["fm"][1], env["up"][1], want=[int("tmpx" in n) for n in G.MAPS], dmaps=[shared[i] if "tmpx" in n else None for i, n in enumerate(G.MAPS)], acc_maps=1)
    check_maps(shared, ref, e32, "e two calls, accumulate_maps on the shared tensors", 1)
    for i, n in enumerate(G.MAPS):
        assert float((shared[i] - fm1.t[i].grad).abs().max()) <= 4 * e32["dmaps"][1][n], n
    # weights from the joint backward: what test_gpu_dectrain's case d checks, here only that the maps did not disturb them
    q = params_of(env)
    preds = ops.sifnet_query_train(q, env["fm"], *env["d"])
    sum((t.reshape(B, k, N) * dev(env["up"][s][h])).sum() for s in range(2) for t, h, k in zip(preds[s], M.HEADS, M.DIMS)).backward()
    assert torch.equal(p.flat.grad, q.flat.grad)


# ---- f: calling conventions ----------------------------------------------------------------------------------------------------------------------------------
def test_f_calling_conventions(env):
    from vistracker_amd import _lib as L
    p, fm, up = params_of(env), env["fm"][0], env["up"][0]
    w, full = raw(env, p, fm, up)
    # poisoned outputs and workspace
    w_nan, m_nan = raw(env, p, fm, up, fill=float("nan"))
    assert torch.equal(w_nan, w) and all(bool(torch.isfinite(a).all()) and torch.equal(a, b_) for a, b_ in zip(m_nan, full))
    # a NULL map pointer leaves the other seven alone
    for skip in (0, 3, 7):
        _, m = raw(env, p, fm, up, want=[int(i != skip) for i in range(8)])
        assert m[skip] is None and all(torch.equal(a, b_) for i, (a, b_) in enumerate(zip(m, full)) if i != skip), skip
    # NULL heads: the heads add, so dropping one changes the maps by that head's share; dropping all gives exact zeros / leaves an accumulating call's buffers alone
    ref4, e4 = G.reference_and_e32(env["dec"], [env["maps"][0]], env["pts"], env["cc"], env["bc"], upstream=[{h: a for h, a in up.items() if h != "parts"}])
    check_maps(raw(env, p, fm, {h: a for h, a in up.items() if h != "parts"})[1], ref4, e4, "f parts NULL")
    wz, mz = raw(env, p, fm, {}, fill=float("nan"))
    assert bool((wz == 0).all()) and all(bool((t == 0).all()) for t in mz)
    keep = [t.clone() for t in full]
    raw(env, p, fm, {}, dmaps=keep, acc_maps=1)
    assert all(torch.equal(a, b_) for a, b_ in zip(keep, full))
    # dparams NULL: the maps' bits do not change
    wn, mn = raw(env, p, fm, up, weights=False)
    assert wn is None and all(torch.equal(a, b_) for a, b_ in zip(mn, full))
    # errors: a resolution that is not the map's, nothing requested
    res = [t.shape[1] for t in fm.t]; res[2] += 1
    assert raw(env, p, fm, up, dres=res, rc_only=True) == L.VT_ERR_ARG
    assert raw(env, p, fm, up, weights=False, want=(0,) * 8, rc_only=True) == L.VT_ERR_ARG
    nb = L.lib().vt_decoder_grads_ws_bytes(B, N, 0, 1)
    ws = torch.empty(nb // 4 + 4, device="cuda")
    rc = L.lib().vt_decoder_grads(L.dptr(p.flat.detach()), p.cam.ctypes.data, C.byref(fm.c), *[L.dptr(t) for t in env["d"]], B, N, None, None, None, None, None,
                                  None, 0, None, 0, 0, L.dptr(ws), L.stream_ptr())
    assert rc == L.VT_ERR_ARG


# ---- g: the reference's recorded gradients -------------------------------------------------------------------------------------------------------------------
def test_g_recorded_reference(env):
    """|kernel - golden| <= 4 |golden - float64 model| per map tensor, on the recorded channels of the recorded texel rows; every other row is an exact zero in the
    reference, and there the kernel gets 4 x the float32 model's own error on those rows (the reference's is zero by construction)"""
    g = golden("mapgrad")
    assert np.array_equal(g["pts"], env["pts"]) and np.array_equal(g["cc"], env["cc"]) and np.array_equal(g["bc"], env["bc"])
    ref, e32 = env["ref1"]
    _, dm = raw(env, params_of(env), env["fm"][0], env["up"][0])
    bad = []
    for n, t in zip(G.MAPS, dm):
        Cn = t.shape[-1]
        got = t.cpu().numpy().reshape(-1, Cn).astype(np.float64)
        model = ref["dmaps"][0][n].transpose(0, 2, 3, 1).reshape(-1, Cn)
        idx, val = g["idx_" + n], g["val_" + n].astype(np.float64)
        st = G.GOLDEN_CHANNEL_STEP
        e = np.abs(val - model[idx][:, ::st]).max()
        err = np.abs(got[idx][:, ::st] - val).max()
        rest = np.ones(len(got), bool); rest[idx] = False
        err0 = np.abs(got[rest]).max(initial=0.0)
        print(f"\n[g] {n:>10}: e32 {e:.3e} |kernel - golden| {err:.3e}; rows the reference left zero: kernel {err0:.3e}", end="")
        if not (err <= 4 * e and err0 <= 4 * e32["dmaps"][0][n]):
            bad.append((n, err, e, err0))
    assert not bad, bad


# ---- h: the train step, maps only ----------------------------------------------------------------------------------------------------------------------------
H_N, H_STEPS, H_LR = 512, 5, 1e-2


def test_h_trainer_maps_only(env):
    """DecoderTrainer.train_step(train_decoders=False) with the eight maps as the only leaves and torch.optim.Adam(lr = 1e-2) on them, five steps on one fixed
    labelled batch.  mapgrad_model.train_maps_model runs the same loop in float64 on the CPU; as in test_gpu_dectrain's case f the trainer must reach at least
    half of the model's drop with every error finite (Adam's first steps are +- lr whatever the gradient's size, so no trajectories are compared), and here
    also start from the model's first error, which no update has touched yet, within float32 round-off of the objective."""
    from vistracker_amd import training
    from vistracker_amd.sifnet import SIFNetQuery
    pts, cc, bc = M.make_inputs(B, H_N, seed=21)
    lab = M.make_labels(B, H_N, seed=22)
    model = G.train_maps_model(env["dec"], env["maps"][0], pts, cc, bc, lab, H_STEPS + 1, H_LR)
    drop = model[0] - model[-1]
    print(f"\nfloat64 model: error before each step {[round(e, 4) for e in model]}, drop {drop:.4f}")
    assert drop > 0
    net = SIFNetQuery(env["dec"])
    fm = leaf_maps(env["fm"][0])
    net.set_feature_maps(fm)
    tr = training.DecoderTrainer(net)
    before = tr.params.flat.detach().clone()
    opt = torch.optim.Adam(fm.t, lr=H_LR)
    batch = {"points": dev(pts), "body_center": dev(bc), **{k: dev(v, torch.int32 if k == "labels" else torch.float32) for k, v in lab.items()}}
    errors = []
    for _ in range(H_STEPS + 1):
        opt.zero_grad()
        error, _ = tr.train_step(batch, dev(cc), train_decoders=False)
        assert all(t.grad is not None for t in fm.t) and tr.params.flat.grad is None
        opt.step()
        errors.append(error)
    errors = torch.stack(errors).cpu().numpy()
    print(f"trainer, maps only: error before each step {[round(float(e), 4) for e in errors]}, drop {errors[0] - errors[-1]:.4f}")
    assert np.isfinite(errors).all() and torch.equal(tr.params.flat.detach(), before)
    assert abs(errors[0] - model[0]) <= 1e-4 * abs(model[0])
    assert errors[0] - errors[-1] >= 0.5 * drop
