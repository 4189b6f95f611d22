"""GPU: training.SIFNetTrainer(guard=True): the step guard and the gradient record between the gradient mean and the optimiser steps.  With finite gradients the
guarded trainer is the plain one, bit for bit; clipping is the float64 model's (tests/gradstat_model.py); a NaN or Inf in any of the three gradient buffers skips the
step on the device, is reported under the name of the leaf that owns it and costs one step of bias correction; the record's names are the checkpoint's; nothing
waits on the host; two ranks take the same decision (tests/guard_ranks_script.py).  Shape: B = 2, two stacks of depth 1, a 128 x 128 input, N = 150 points
(sifnet_step_model.case), as tests/test_gpu_sifnet_trainer.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gradstat_model as GS
import sifnet_step_model as SM
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCRIPT = os.path.join(ROOT, "tests", "guard_ranks_script.py")


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


@pytest.fixture(scope="module")
def env():
    c = SM.case()
    lab = c["labels"]
    batch = {"points": dev(c["pts"]), "df_h": dev(lab["df_h"]), "df_o": dev(lab["df_o"]), "labels": dev(lab["labels"], torch.int32), "pca_axis": dev(lab["pca_axis"]),
             "body_center": dev(c["bc"]), "obj_center": dev(lab["obj_center"]), "visibility": dev(lab["visibility"])}
    return dict(c=c, sd=SM.state_dict(c), batch=batch, images=dev(c["images"]), cc=dev(c["cc"]))


def make(env, **kw):
    from vistracker_amd.training import SIFNetTrainer
    return SIFNetTrainer(env["sd"], None, num_stack=SM.NUM_STACK, num_hourglass=SM.DEPTH, triplane_stack=SM.NUM_STACK, device=DEV, **kw)


def micro(env):
    from vistracker_amd.training import slice_batch
    return [(slice_batch(env["batch"], slice(k, k + 1)), env["images"][k:k + 1], env["cc"][k:k + 1]) for k in range(SM.B)]


def state(tr):
    """every parameter and Adam moment of the trainer, as clones"""
    out = []
    for o in (tr.image_optimizer, tr.tri_optimizer):
        out += [o.flat.clone(), o.m.clone(), o.v.clone()]
    return out + [tr.params.flat.detach().clone(), tr.optimizer.m[0].clone(), tr.optimizer.v[0].clone()]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def step(tr, env):
    return tr.train_step(env["batch"], env["images"], env["cc"])


def layout(tr):
    """[(name, offset, numel)] per gradient buffer, from the leaves' own addresses and the library's decoder table: independent of the guard's bookkeeping"""
    from vistracker_amd import _lib as L, ops
    out = []
    for prefix, enc, opt in ((SM.IMAGE, tr.image, tr.image_optimizer), (SM.TRIPLANE, tr.tri, tr.tri_optimizer)):
        out.append([(prefix + k, (p.data_ptr() - opt.flat.data_ptr()) // 4, p.numel()) for k, p in enc.named_parameters()])
    dec = []
    for h, head in enumerate(ops.HEADS):
        for l in range(4):
            for is_bias, kind in enumerate(("weight", "bias")):
                dec.append((f"{SM.MODULES[head]}.{2 * l}.{kind}", int(L.lib().vt_decoder_param_offset(h, l, is_bias)), tr.params.views[(head, l, kind)].numel()))
    return out + [dec]


# ---- 1: finite gradients: the guard changes nothing ------------------------------------------------------------------------------------------------------------
def test_finite_gradients_leave_the_step_bit_for_bit(env):
    plain, guarded, clipped = make(env), make(env, guard=True, record=2), make(env, guard=True, clip_norm=1e30)
    assert plain.guard is None and same(state(plain), state(guarded))
    for k in range(3):
        e0, l0 = step(plain, env)
        for tr in (guarded, clipped):
            e, l = step(tr, env)
            assert torch.equal(e, e0) and torch.equal(l, l0), k
    assert same(state(plain), state(guarded)) and same(state(plain), state(clipped)) and not same(state(plain), state(make(env)))
    rec, recc = guarded.guard.read(), clipped.guard.read()
    assert rec["steps"] == 3 and rec["skipped"] == 0 and not rec["skip"] and rec["coef"] == 1.0 and rec["norm"] > 0 and rec["error"] == float(e0)
    assert [r["step"] for r in rec["ring"]] == [1, 2] and rec["ring"][1]["sumsq"] == rec["sumsq"] and sum(rec["nonfinite"].values()) == 0
    assert recc["coef"] == 1.0 and recc["norm"] == rec["norm"] and recc["ring"] == []          # 1e30 never bites: the multiplication by 1 is exact (and not made)


# ---- 2: the record's names ---------------------------------------------------------------------------------------------------------------------------------------
def test_record_names_are_the_checkpoint_keys_of_the_stepped_leaves(env):
    """in the order of state_dict().  state_dict() holds two kinds of keys beside them that no optimiser steps and that therefore have no gradient to record: the
    reference's ``downsample.0.*`` aliases of a projection block's bn4, and the bn4 of an identity block, which its forward never uses"""
    tr = make(env, guard=True)
    names = tr.guard.names
    keys = list(tr.state_dict())
    assert [k for k in keys if k in set(names)] == names and len(set(names)) == len(names)
    assert all(".downsample.0." in k or ".bn4." in k for k in keys if k not in set(names))
    assert names == [n for buf in layout(tr) for n, _, _ in buf]
    rec = tr.guard.read()
    assert list(rec["sumsq"]) == list(rec["maxabs"]) == list(rec["nonfinite"]) == names


# ---- 3: clipping -------------------------------------------------------------------------------------------------------------------------------------------------
def test_clipping_is_the_models(env):
    probe = make(env, guard=True)
    step(probe, env)
    norm0 = probe.guard.read()["norm"]
    tr = make(env, guard=True, clip_norm=0.5 * norm0)
    error, _ = tr.backward(env["batch"], env["images"], env["cc"])
    before = [g.detach().clone() for g in tr.flat_grads()]
    skip = tr.guard.close(tr.flat_grads(), error)
    after = tr.flat_grads()
    segs = [[(o, o + n) for _, o, n in buf] for buf in layout(tr)]
    hosts = [b.cpu().numpy() for b in before]
    st = [GS.seg_stats(h, s) for h, s in zip(hosts, segs)]
    want = GS.close([x[0] for x in st], [x[2] for x in st], float(error), 0.5 * norm0)
    rec = tr.guard.read()
    n_el = sum(e - b for s in segs for b, e in s)
    print(f"\n[clip] norm {rec['norm']:.9e} (model {want['norm']:.9e}), coef {rec['coef']:.9f} (model {float(want['coef']):.9f})", end="")
    assert not bool(skip.item()) and not want["skip"] and abs(rec["norm"] - norm0) <= n_el * GS.EPS * norm0
    assert not GS.close_failures(rec, want, GS.coef_of(rec["norm"], 0.5 * norm0), n_el)
    assert np.float32(rec["coef"]).view(np.uint32) == want["coef"].view(np.uint32) and 0.49 < rec["coef"] < 0.51
    for k, (a, h) in enumerate(zip(after, hosts)):
        assert np.array_equal(a.detach().cpu().numpy().view(np.int32), GS.scaled(h, want["coef"], False).view(np.int32)), k


# ---- 4: poisoned steps -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("buffer", [0, 1, 2], ids=["image", "triplane", "decoders"])
def test_a_poisoned_step_is_skipped_and_named(env, buffer, value):
    """ordinary NaN arithmetic: one element of one gradient buffer is overwritten after the backward"""
    tr, twin = make(env, guard=True, record=2), make(env)
    start = state(tr)
    error, _ = tr.backward(env["batch"], env["images"], env["cc"])
    grads = tr.flat_grads()
    buf = layout(tr)[buffer]
    name, off, numel = buf[len(buf) // 2]
    grads[buffer].detach()[off + numel - 1] = value                        # the leaf's last element: the next float is padding or the next leaf
    host = grads[buffer].detach().cpu().numpy()
    tr.apply(error)
    assert same(state(tr), start) and same(state(tr), state(twin))            # parameters and both moments of all three optimisers untouched
    rec = tr.guard.read()
    assert rec["steps"] == 1 and rec["skipped"] == 1 and rec["skip"] is True
    assert {k: v for k, v in rec["nonfinite"].items() if v} == {name: 1}
    want = GS.seg_stats(host, [(off, off + numel)])
    assert abs(rec["sumsq"][name] - want[0][0]) <= numel * GS.EPS * want[0][0] and want[0][0] > 0 and np.isfinite(rec["norm"])
    assert np.float32(rec["maxabs"][name]) == want[1][0]
    # the next clean step: a plain trainer at the same state whose optimisers' t was advanced without a step takes the same one
    for o in (twin.image_optimizer, twin.tri_optimizer, twin.optimizer):
        o.t += 1
    assert (tr.image_optimizer.t, tr.tri_optimizer.t, tr.optimizer.t) == (1, 1, 1)
    e1, l1 = step(tr, env)
    e2, l2 = step(twin, env)
    assert torch.equal(e1, e2) and torch.equal(l1, l2) and same(state(tr), state(twin)) and not same(state(tr), start)
    rec = tr.guard.read()
    assert rec["steps"] == 2 and rec["skipped"] == 1 and not rec["skip"] and [r["skip"] for r in rec["ring"]] == [True, False]


def test_a_non_finite_objective_alone_skips(env):
    tr = make(env, guard=True)
    start = state(tr)
    tr.backward(env["batch"], env["images"], env["cc"])
    tr.apply(torch.tensor(float("inf"), dtype=torch.float64, device=DEV))
    rec = tr.guard.read()
    assert same(state(tr), start) and rec["skipped"] == 1 and sum(rec["nonfinite"].values()) == 0 and rec["error"] == float("inf")


# ---- 5: no host wait -----------------------------------------------------------------------------------------------------------------------------------------------
def test_guarded_steps_do_not_wait_on_the_host(env, monkeypatch):
    tr = make(env, guard=True, clip_norm=1e-3, record=2)
    step(tr, env); tr.train_step_micro(micro(env))                           # the first steps may allocate and pack

    def barred(*a, **k):
        raise AssertionError("a guarded step went to the host")

    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", barred)
        mp.setattr(torch.Tensor, "numpy", barred)
        mp.setattr(torch.Tensor, "item", barred)
        mp.setattr(torch.Tensor, "tolist", barred)
        mp.setattr(torch.cuda, "synchronize", barred)
        error, _ = step(tr, env)
        errors, _ = tr.train_step_micro(micro(env))
    rec = tr.guard.read()
    assert error.is_cuda and errors.shape == (SM.B,) and rec["steps"] == 4 and rec["skipped"] == 0 and rec["coef"] < 1
    assert rec["error"] == float(errors.sum())                                # micro-batches: the sum of the micro errors


# ---- 6: two ranks take the same decision -----------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_skip_together(env, tmp_path):
    e = dict(os.environ, MASTER_ADDR="127.0.0.1", MIOPEN_FIND_MODE="FAST")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29621", SCRIPT,
           str(tmp_path / "guard")]
    out = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.count("RANK_OK") == 2, out.stdout[-2000:] + out.stderr[-4000:]
    r0, r1 = (dict(np.load(str(tmp_path / f"guard.rank{r}.npz"))) for r in range(2))
    assert GS.same_records(r0, r1)                                            # state and record, every array, as bits
    # one process, two micro-batches, the same poison in the second one's row before the mean
    tr = make(env, guard=True, record=3)
    name, off, numel = layout(tr)[0][len(layout(tr)[0]) // 2]
    for k in range(3):
        rows = tr.reducer.rows(SM.B)
        errors = []
        for m, (batch, images, cc) in enumerate(micro(env)):
            error, _ = tr.backward(batch, images, cc)
            for ws, g in zip(rows, tr.flat_grads()):
                ws[m].copy_(g)
            errors.append(error)
        if k == 1:
            rows[0][1, off + numel - 1] = float("nan")
        tr.reducer.reduce_local(rows, tr.flat_grads())
        tr.apply(torch.stack(errors).sum())
    mine = GS.record_arrays(tr.guard.read())
    mine.update({f"state{i}": t.cpu().numpy().view(np.int32).astype(np.int64) for i, t in enumerate(state(tr))})
    assert int(mine["head"][1]) == 1 and GS.same_records(r0, mine), [k for k in mine if k not in r0 or not np.array_equal(r0[k], mine[k])]
