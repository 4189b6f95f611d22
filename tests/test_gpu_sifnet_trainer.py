"""GPU: training.SIFNetTrainer, the trainer that joins the two TrainableHGFilter encoders to the decoders.  It adds no kernel, so the tests are compositional: a
step is the merged parts composed by hand, bit for bit; its losses and gradients are those of the float64 model tests/sifnet_step_model.py (the existing models
composed) evaluated at the GPU forward's saved activations; it trains; it does not wait on the host; it round-trips through state_dict() and export(); its schedule
is the learning rate set directly.  Shape: B = 2, two stacks of depth 1, a 128 x 128 input, N = 150 points (sifnet_step_model.case).

The bound of the model test is MEASURED in the test: e32 = the float32 CPU run of the model against its float64 run, per tensor; the gate is 8 e32.  Figures
measured on an MI355X: tests/golden/sifnet_step.md."""
import concurrent.futures
import os

import numpy as np
import pytest
import torch

import sifnet_step_model as SM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sifnet_step.npz")


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def host(t):
    return t.detach().double().cpu().numpy()


@pytest.fixture(scope="module")
def env():
    c = SM.case()
    lab = c["labels"]
    batch = {"points": dev(c["pts"]), "df_h": dev(lab["df_h"]), "df_o": dev(lab["df_o"]), "labels": dev(lab["labels"], torch.int32), "pca_axis": dev(lab["pca_axis"]),
             "body_center": dev(c["bc"]), "obj_center": dev(lab["obj_center"]), "visibility": dev(lab["visibility"])}
    # the model's float64 and float32 runs (CPU, about 5 s) are computed ONCE, on a thread that runs beside the tests before the one that reads them (the last)
    pool = concurrent.futures.ThreadPoolExecutor(1)
    model = pool.submit(SM.reference_and_e32, c)
    pool.shutdown(wait=False)
    return dict(c=c, sd=SM.state_dict(c), batch=batch, images=dev(c["images"]), cc=dev(c["cc"]), model=model)


def make(env, sd=None, **kw):
    from vistracker_amd.training import SIFNetTrainer
    return SIFNetTrainer(env["sd"] if sd is None else sd, None, num_stack=SM.NUM_STACK, num_hourglass=SM.DEPTH, triplane_stack=SM.NUM_STACK, device=DEV, **kw)


def state(tr):
    """every parameter and Adam moment of the trainer, as clones"""
    out = []
    for o in (tr.image_optimizer, tr.tri_optimizer):
        out += [o.flat.clone(), o.m.clone(), o.v.clone()]
    return out + [tr.params.flat.detach().clone(), tr.optimizer.m[0].clone(), tr.optimizer.v[0].clone()]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def hand_step(tr, batch, images, cc):
    """train_step written out from the merged parts: the encoder forwards, the map tensors as detached leaves that require grad, a DecoderTrainer-style
    query_train + get_errors + backward, the maps' .grad fed to the backward of the encoder outputs, the three optimiser steps"""
    from vistracker_amd import ops
    tr.image_optimizer.zero_grad(); tr.tri_optimizer.zero_grad(); tr.optimizer.zero_grad()
    b = images.shape[0]
    feats, tmpx, _ = tr.image(images[:, :5])
    tfeats, ttmpx, _ = tr.tri(images[:, 5:8].transpose(0, 1).reshape(3 * b, 1, *images.shape[2:]))
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1)            # noqa: E731
    shared = {"tmpx": nhwc(tmpx)}
    shared.update({f"tri_tmpx{v}": nhwc(ttmpx[v * b:(v + 1) * b]) for v in range(3)})
    maps = []
    for s in range(len(feats)):
        d = dict(shared)
        d["im_feat"] = nhwc(feats[s]).requires_grad_(True)
        d.update({f"tri_feat{v}": nhwc(tfeats[s][v * b:(v + 1) * b]).requires_grad_(True) for v in range(3)})
        maps.append(ops.FeatureMaps(d))
    tr.net.query_train(tr.params, batch["points"], crop_center=cc, body_center=batch["body_center"], maps=maps)
    error, losses_all = tr.net.get_errors(batch["df_h"], batch["df_o"], batch["labels"], batch["pca_axis"], tr.max_dist, batch["body_center"], batch["obj_center"],
                                          visibility=batch["visibility"])
    error.backward()
    i0, t0 = ops.MAP_ORDER.index("im_feat"), ops.MAP_ORDER.index("tri_feat0")
    assert all(m.t[ops.MAP_ORDER.index(k)].grad is None for m in maps for k in shared)
    torch.autograd.backward(feats, [m.t[i0].grad.permute(0, 3, 1, 2) for m in maps])
    torch.autograd.backward(tfeats, [torch.cat([m.t[t0 + v].grad for v in range(3)], 0).permute(0, 3, 1, 2) for m in maps])
    tr.image_optimizer.step(); tr.tri_optimizer.step(); tr.optimizer.step()
    return error.detach(), losses_all


# ---- 1: a step is the merged parts, bit for bit ------------------------------------------------------------------------------------------------------------------
def test_step_is_the_composition_bit_for_bit(env):
    a, b = make(env), make(env)
    assert same(state(a), state(b))
    for step in range(2):
        ea, la = a.train_step(env["batch"], env["images"], env["cc"])
        eb, lb = hand_step(b, env["batch"], env["images"], env["cc"])
        assert ea.dtype == la.dtype == torch.float64 and ea.shape == () and la.shape == (6,)
        assert torch.equal(ea, eb) and torch.equal(la, lb), step
        sa, sb = state(a), state(b)
        assert same(sa, sb), (step, [i for i, (x, y) in enumerate(zip(sa, sb)) if not torch.equal(x, y)])
    assert not same(state(a), state(make(env)))            # and the two steps moved the parameters


def gradients(tr):
    """{reference checkpoint key: gradient} of the trainer's last backward"""
    from vistracker_amd import ops
    g = {SM.IMAGE + k: v.grad for k, v in tr.image.named_parameters()}
    g.update({SM.TRIPLANE + k: v.grad for k, v in tr.tri.named_parameters()})
    views = ops.DecoderParams(tr.params.flat.grad.detach().clone(), tr.params.cam).views
    g.update({f"{SM.MODULES[name]}.{2 * l}.{kind}": v for (name, l, kind), v in views.items()})
    return g


# ---- 3: it trains ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_it_trains(env):
    """20 steps on the fixed batch at lr 1e-3.  The float64 model (sifnet_step_model.train, run on a CPU) falls from a mean of 1532.6 over its first three steps to
    203.3 over its last three; the figures of this run: tests/golden/sifnet_step.md"""
    tr = make(env, lr=1e-3)
    errors = [tr.train_step(env["batch"], env["images"], env["cc"])[0] for _ in range(20)]
    errors = torch.stack(errors).cpu().numpy()
    first, last = errors[:3].mean(), errors[-3:].mean()
    print(f"\n[trains] first three {first:.4f}, last three {last:.4f}; all: {np.array2string(errors, precision=2)}", end="")
    assert np.isfinite(errors).all() and last < first


# ---- 4: no host wait -------------------------------------------------------------------------------------------------------------------------------------------------
def test_train_step_does_not_wait_on_the_host(env, monkeypatch):
    tr = make(env)
    tr.train_step(env["batch"], env["images"], env["cc"])              # the first step may allocate and pack; the barred one is a step of the loop

    def barred(*a, **k):
        raise AssertionError("train_step went to the host")

    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", barred)
        mp.setattr(torch.Tensor, "numpy", barred)
        mp.setattr(torch.Tensor, "item", barred)
        mp.setattr(torch.cuda, "synchronize", barred)
        error, losses_all = tr.train_step(env["batch"], env["images"], env["cc"])
    assert error.is_cuda and losses_all.is_cuda and bool(torch.isfinite(error))


# ---- 5: round trips --------------------------------------------------------------------------------------------------------------------------------------------------
def test_round_trips(env):
    from vistracker_amd import ops
    from vistracker_amd.training import validate
    tr = make(env)
    sd = tr.state_dict()
    assert set(sd) >= set(env["sd"]) and all(np.array_equal(sd[k].cpu().numpy(), env["sd"][k]) for k in env["sd"])           # what went in, no step taken
    again = make(env, sd={"module." + k: v for k, v in sd.items()})
    e0, l0 = tr.train_step(env["batch"], env["images"], env["cc"])
    e1, l1 = again.train_step(env["batch"], env["images"], env["cc"])
    assert torch.equal(e0, e1) and torch.equal(l0, l1)
    tr.train_step(env["batch"], env["images"], env["cc"])
    assert tr.export().maps is None
    net = tr.export(env["images"])
    with torch.no_grad():
        own = tr.forward(env["images"])[-1]
    fresh = net.encoder(env["images"])
    assert all(torch.equal(a, b) for a, b in zip(fresh.t, own.t)), [k for k, a, b in zip(ops.MAP_ORDER, fresh.t, own.t) if not torch.equal(a, b)]
    val = validate(net, env["batch"], env["cc"])
    assert list(val) == list(ops.LOSS_SLOTS) + ["total"] and len(val) == 7 and all(np.isfinite(v) for v in val.values()), val
    trained = tr.state_dict()
    assert all(torch.equal(trained[k].reshape(-1), torch.as_tensor(np.asarray(w if kind == "weight" else b), device=DEV).reshape(-1))
               for name, mod in SM.MODULES.items() for i, (w, b) in zip((0, 2, 4, 6), net.decoders[name]) for kind, k in (("weight", f"{mod}.{i}.weight"), ("bias", f"{mod}.{i}.bias")))


def test_export_packs_nothing_on_the_host(env, monkeypatch):
    """export(images) encodes with handles packed on the device; its eight maps are those of a SIFNetEncoder built from state_dict() that packs on the host"""
    from vistracker_amd import _lib, encoder as E, ops
    tr = make(env)
    tr.train_step(env["batch"], env["images"], env["cc"])
    calls = []

    def counted(name):
        real = getattr(_lib.lib(), name)

        def f(*a):
            calls.append(name)
            return real(*a)
        return f

    with monkeypatch.context() as mp:
        for name in ("vt_conv3x3_create", "vt_conv1x1_create", "vt_stem7x7_create"):
            mp.setattr(_lib.lib(), name, counted(name))
        net = tr.export(env["images"])
        assert calls == [] and net.encoder.image._handles and not any(ent.on_host for e in (net.encoder.image, net.encoder.tri[0]) for ent in e._handles.values())
        mp.setattr(E._PackedHandles, "host_repack", True)
        ref = E.SIFNetEncoder(tr.state_dict(), num_stack=SM.NUM_STACK, num_hourglass=SM.DEPTH, triplane_stack=SM.NUM_STACK, device=DEV)
        want = ref(env["images"])
        assert len(calls) == len(ref.image._handles) + len(ref.tri[0]._handles) > 0           # the reference did pack on the host
    assert len(want.t) == len(net.maps.t) == len(ops.MAP_ORDER) == 8
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(net.maps.t, want.t)), [k for k, a, b in zip(ops.MAP_ORDER, net.maps.t, want.t) if not torch.equal(a, b)]


# ---- 6: the schedule ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_schedule_is_the_learning_rate_set_directly(env):
    lr0 = 1e-3
    a = make(env, lr=lr0, milestones=(3,), gamma=0.3)
    a.set_step(2)
    assert a.lr == lr0
    a.train_step(env["batch"], env["images"], env["cc"])
    # b: built with lr0 * 0.3 directly and brought to a's state: parameters through state_dict(), moments and step counts copied
    b = make(env, sd=a.state_dict(), lr=lr0 * 0.3)
    for oa, ob in ((a.image_optimizer, b.image_optimizer), (a.tri_optimizer, b.tri_optimizer)):
        ob.m.copy_(oa.m); ob.v.copy_(oa.v); ob.t = oa.t
    b.optimizer.m[0].copy_(a.optimizer.m[0]); b.optimizer.v[0].copy_(a.optimizer.v[0]); b.optimizer.t = a.optimizer.t
    assert same(state(a), state(b))
    assert a.set_step(3) == lr0 * 0.3 == a.lr == b.lr and a.optimizer.lrs == b.optimizer.lrs
    ea = a.train_step(env["batch"], env["images"], env["cc"])
    eb = b.train_step(env["batch"], env["images"], env["cc"])
    assert torch.equal(ea[0], eb[0]) and torch.equal(ea[1], eb[1]) and same(state(a), state(b))


# ---- 2 (placed last: its CPU reference runs on the fixture's thread meanwhile): against the float64 model ----------------------------------------------------------------------------------------------------------------------------------
def gpu_forward(tr, images):
    """both encoder forwards block by block (tests/test_gpu_enctrain.py walk: the same launches) -> (the S map sets as NCHW float64 arrays in
    sifnet_step_model.stack_maps' form, the two tapes of saved activations)"""
    import test_gpu_enctrain as TE
    b = images.shape[0]
    xi = images[:, :5].contiguous(memory_format=torch.channels_last)
    xt = images[:, 5:8].transpose(0, 1).reshape(3 * b, 1, *images.shape[2:]).contiguous(memory_format=torch.channels_last)
    oi, tmpx, _, nodes_i = TE.walk(tr.image, xi)
    ot, ttmpx, _, nodes_t = TE.walk(tr.tri, xt)
    saved = TE.model_saved(nodes_i, b), TE.model_saved(nodes_t, 3 * b)
    return (oi, tmpx, ot, ttmpx), SM.stack_maps([host(o) for o in oi], host(tmpx), [host(o) for o in ot], host(ttmpx), b), saved


def test_losses_and_gradients_against_the_float64_model(env):
    """Measured on an MI355X: tests/golden/sifnet_step.md"""
    c = env["c"]
    tr = make(env)
    walked, gpu_maps, (saved_i, saved_t) = gpu_forward(tr, env["images"])
    with torch.no_grad():
        own = tr.forward(env["images"])
    from vistracker_amd import ops
    assert all(np.array_equal(host(t.permute(0, 3, 1, 2)), gpu_maps[s][k]) for s in range(SM.NUM_STACK) for k, t in zip(ops.MAP_ORDER, own[s].t))        # the walk is the trainer's forward: all eight maps of every stack
    truth = SM.at_saved(c, gpu_maps, saved_i, saved_t)
    del walked
    r64, e32 = env["model"].result()
    error, losses_all = tr.train_step(env["batch"], env["images"], env["cc"])
    got = gradients(tr)
    bad = []
    la = host(losses_all)
    for i, name in enumerate(("df_h", "df_o", "parts", "pca", "vis", "obj_center")):
        err, e = abs(la[i] - truth["losses_all"][i]), e32["losses_all"][i]
        print(f"\n[loss {name:>10}] float64 {r64['losses_all'][i]:.6e} | e32 {e:.3e} | GPU error at the saved activations {err:.3e} ({err / e if e else 0:.2f})", end="")
        if not err <= 8 * e:
            bad.append((name, err, e))
    assert abs(float(error) - la.sum()) <= 1e-9 * la.sum()
    for k in SM.gated():
        err, e = float(np.abs(host(got[k]).reshape(truth["grads"][k].shape) - truth["grads"][k]).max()), e32["grads"][k]
        print(f"\n[grad {k:>34}] largest element {np.abs(r64['grads'][k]).max():.3e} | e32 {e:.3e} | GPU error at the saved activations {err:.3e} ({err / e if e else 0:.2f})", end="")
        if not (np.isfinite(err) and err <= 8 * e):
            bad.append((k, err, e))
    # the reference's own run, recorded in float64 (tests/golden/sifnet_step.npz, tools/gen_golden_sifnet_step.py; held to the model at 1e-9 of each tensor's scale
    # by tests/test_host_sifnet_trainer.py): the GPU's values against the recorded ones, gated the same way, 8 e32 per tensor
    gold = np.load(GOLDEN)
    for i, name in enumerate(("df_h", "df_o", "parts", "pca", "vis", "obj_center")):
        err, e = abs(la[i] - float(gold["losses_all"][i])), e32["losses_all"][i]
        print(f"\n[recorded loss {name:>10}] e32 {e:.3e} | GPU against the reference {err:.3e} ({err / e if e else 0:.2f})", end="")
        if not err <= 8 * e:
            bad.append(("recorded loss " + name, err, e))
    for k in SM.gated():
        err, e = float(np.abs(SM.golden_sub(k)(host(got[k]).reshape(truth["grads"][k].shape)) - gold[k]).max()), e32["grads"][k]
        print(f"\n[recorded {k:>34}] e32 {e:.3e} | GPU against the reference {err:.3e} ({err / e if e else 0:.2f})", end="")
        if not (np.isfinite(err) and err <= 8 * e):
            bad.append(("recorded " + k, err, e))
    assert not bad, bad
