"""GPU: data-parallel steps of training.SIFNetTrainer.  ``train_step`` is ``backward`` + ``apply``, unchanged; the mean over micro-batches is the gradient of the
whole batch (the float64 model tests/sifnet_step_model.py at the GPU forward's saved activations, gated at 8 e32 per tensor, e32 measured here); two ranks with one
frame each end where one rank with two micro-batches ends, bit for bit (two gloo ranks on the one GPU of the test box, tests/ddp_ranks_script.py); the RCCL route
with a group of one is the plain step and does not wait on the host; ranks built from different weights are caught by the constructor.
Shape: B = 2, two stacks of depth 1, a 128 x 128 input, N = 150 points (sifnet_step_model.case).  Figures measured on an MI355X: tests/golden/sifnet_step_micro.md."""
import concurrent.futures
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sifnet_step_model as SM
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCRIPT = os.path.join(ROOT, "tests", "ddp_ranks_script.py")
STATE_KEYS = ("image_p", "image_m", "image_v", "tri_p", "tri_m", "tri_v", "dec_p", "dec_m", "dec_v")


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
    # the model's float64 and float32 runs (CPU, about 5 s) are computed ONCE, on a thread that runs beside the tests before the one that reads them
    pool = concurrent.futures.ThreadPoolExecutor(1)
    model = pool.submit(SM.reference_and_e32, c)
    pool.shutdown(wait=False)
    return dict(c=c, sd=SM.state_dict(c), batch=batch, images=dev(c["images"]), cc=dev(c["cc"]), model=model)


def make(env, **kw):
    from vistracker_amd.training import SIFNetTrainer
    return SIFNetTrainer(env["sd"], None, num_stack=SM.NUM_STACK, num_hourglass=SM.DEPTH, triplane_stack=SM.NUM_STACK, device=DEV, **kw)


def micro(env):
    """the case as two single-frame micro-batches"""
    from vistracker_amd.training import slice_batch
    return [(slice_batch(env["batch"], slice(k, k + 1)), env["images"][k:k + 1], env["cc"][k:k + 1]) for k in range(SM.B)]


def state(tr):
    """every parameter and Adam moment of the trainer, as clones"""
    out = []
    for o in (tr.image_optimizer, tr.tri_optimizer):
        out += [o.flat.clone(), o.m.clone(), o.v.clone()]
    return out + [tr.params.flat.detach().clone(), tr.optimizer.m[0].clone(), tr.optimizer.v[0].clone()]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def launch(nproc, port, args, extra_env=None):
    e = dict(os.environ, MASTER_ADDR="127.0.0.1", MIOPEN_FIND_MODE="FAST", **(extra_env or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1", "--master-port", str(port), SCRIPT] + args
    return subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=600, cwd=ROOT)


# ---- 1: train_step is unchanged ----------------------------------------------------------------------------------------------------------------------------------------
def test_train_step_is_backward_then_apply(env):
    a, b = make(env, group=None), make(env)
    assert a.group is None and same(state(a), state(b))
    for step in range(3):
        ea, la = a.train_step(env["batch"], env["images"], env["cc"])
        eb, lb = b.backward(env["batch"], env["images"], env["cc"])
        b.apply()
        assert torch.equal(ea, eb) and torch.equal(la, lb), step
    assert same(state(a), state(b)) and not same(state(a), state(make(env)))
    assert a.in_sync() is True


def test_unequal_micro_batches_raise(env):
    from vistracker_amd import _lib as L
    from vistracker_amd.training import slice_batch
    tr = make(env)
    with pytest.raises(L.VtError):
        tr.train_step_micro([micro(env)[0], (env["batch"], env["images"], env["cc"])])
    with pytest.raises(L.VtError):
        tr.train_step_micro([])
    assert slice_batch(env["batch"], slice(1, 2))["points"].shape == (1,) + tuple(env["batch"]["points"].shape[1:])


def test_micro_step_does_not_wait_on_the_host(env, monkeypatch):
    tr = make(env)
    tr.train_step_micro(micro(env))              # the first step may allocate and pack

    def barred(*a, **k):
        raise AssertionError("train_step_micro went to the host")

    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", barred)
        mp.setattr(torch.Tensor, "numpy", barred)
        mp.setattr(torch.Tensor, "item", barred)
        mp.setattr(torch.cuda, "synchronize", barred)
        errors, losses_all = tr.train_step_micro(micro(env))
    assert errors.shape == (SM.B,) and losses_all.shape == (SM.B, 6) and errors.is_cuda and bool(torch.isfinite(errors).all())


# ---- 3: two ranks equal two micro-batches, bit for bit -----------------------------------------------------------------------------------------------------------------
def test_two_ranks_equal_two_micro_batches(env, tmp_path):
    out = launch(2, 29611, [str(tmp_path / "ddp"), "gloo", "train"])
    assert out.returncode == 0 and out.stdout.count("RANK_OK") == 2, out.stdout[-2000:] + out.stderr[-4000:]
    r0, r1 = (dict(np.load(str(tmp_path / f"ddp.rank{r}.npz"))) for r in range(2))
    tr = make(env)
    steps = [tr.train_step_micro(micro(env)) for _ in range(3)]
    errors, losses = torch.stack([e for e, _ in steps]).cpu().numpy(), torch.stack([l for _, l in steps]).cpu().numpy()          # (3, 2), (3, 2, 6)
    mine = dict(zip(STATE_KEYS, (t.cpu().numpy() for t in state(tr))))
    for k in STATE_KEYS:
        assert np.array_equal(r0[k].view(np.int32), r1[k].view(np.int32)), ("the ranks differ", k)
        assert np.array_equal(r0[k].view(np.int32), mine[k].view(np.int32)), ("ranks against micro-batches", k, float(np.abs(r0[k].astype(np.float64) - mine[k]).max()))
    assert np.array_equal(r0["grad_dec"].view(np.int32), tr.params.flat.grad.cpu().numpy().view(np.int32))          # every rank's .grad holds the mean, as DDP leaves it
    for r, rec in enumerate((r0, r1)):                                                                            # the returned errors stay the rank's own
        assert np.array_equal(rec["errors"], errors[:, r]) and np.array_equal(rec["losses"], losses[:, r]), r


# ---- 4: RCCL with a group of one ---------------------------------------------------------------------------------------------------------------------------------------
def test_rccl_group_of_one_is_the_plain_step(env, tmp_path):
    out = launch(1, 29612, [str(tmp_path / "one"), "nccl", "train"], dict(VT_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0 and "RANK_OK" in out.stdout and "NO_HOST_WAIT_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    rec = dict(np.load(str(tmp_path / "one.rank0.npz")))
    tr = make(env)
    errors = torch.stack([tr.train_step(env["batch"], env["images"], env["cc"])[0] for _ in range(3)]).cpu().numpy()
    mine = dict(zip(STATE_KEYS, (t.cpu().numpy() for t in state(tr))))
    for k in STATE_KEYS:
        assert np.array_equal(rec[k].view(np.int32), mine[k].view(np.int32)), k
    assert np.array_equal(rec["errors"], errors)


# ---- 5: a mismatch is caught -------------------------------------------------------------------------------------------------------------------------------------------
def test_ranks_built_from_different_weights_are_caught(tmp_path):
    out = launch(2, 29613, [str(tmp_path / "bad"), "gloo", "mismatch"])
    assert out.returncode != 0 and out.stdout.count("MISMATCH_CAUGHT") == 2 and "RANK_OK" not in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 2 (placed last: its CPU reference runs on the fixture's thread meanwhile): micro-batches against the whole batch --------------------------------------------------
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
    return SM.stack_maps([host(o) for o in oi], host(tmpx), [host(o) for o in ot], host(ttmpx), b), saved


def gradients(tr):
    """{reference checkpoint key: gradient} of the trainer's gradient buffers"""
    from vistracker_amd import ops
    g = {SM.IMAGE + k: v.grad for k, v in tr.image.named_parameters()}
    g.update({SM.TRIPLANE + k: v.grad for k, v in tr.tri.named_parameters()})
    views = ops.DecoderParams(tr.params.flat.grad.detach().clone(), tr.params.cam).views
    g.update({f"{SM.MODULES[name]}.{2 * l}.{kind}": v for (name, l, kind), v in views.items()})
    return g


def test_micro_batch_mean_against_the_float64_model(env):
    """Measured on an MI355X: tests/golden/sifnet_step_micro.md"""
    from vistracker_amd import ops
    c = env["c"]
    tr = make(env)
    # the forward kernels treat frames independently: a micro-batch's maps are the rows of the whole batch's, bit for bit
    with torch.no_grad():
        whole = tr.forward(env["images"])
        for k in range(SM.B):
            part = tr.forward(env["images"][k:k + 1])
            for s in range(SM.NUM_STACK):
                for name, a, b in zip(ops.MAP_ORDER, part[s].t, whole[s].t):
                    assert torch.equal(a.view(torch.int32), b[k:k + 1].view(torch.int32)), ("frame", k, "stack", s, name)
    gpu_maps, (saved_i, saved_t) = gpu_forward(tr, env["images"])
    truth = SM.at_saved(c, gpu_maps, saved_i, saved_t)
    r64, e32 = env["model"].result()
    errors, losses_all = tr.train_step_micro(micro(env))
    got = gradients(tr)
    bad = []
    la = host(losses_all).mean(0)                       # every term is a mean over frames: the mean of the micro-batches' losses is the batch's
    for i, name in enumerate(("df_h", "df_o", "parts", "pca", "vis", "obj_center")):
        err, e = abs(la[i] - truth["losses_all"][i]), e32["losses_all"][i]
        print(f"\n[micro loss {name:>10}] float64 {r64['losses_all'][i]:.6e} | e32 {e:.3e} | mean over micro-batches against the model at the saved activations {err:.3e} ({err / e if e else 0:.2f})", end="")
        if not err <= 8 * e:
            bad.append((name, err, e))
    for k in SM.gated():
        err, e = float(np.abs(host(got[k]).reshape(truth["grads"][k].shape) - truth["grads"][k]).max()), e32["grads"][k]
        print(f"\n[micro grad {k:>34}] largest element {np.abs(r64['grads'][k]).max():.3e} | e32 {e:.3e} | GPU error at the saved activations {err:.3e} ({err / e if e else 0:.2f})", end="")
        if not (np.isfinite(err) and err <= 8 * e):
            bad.append((k, err, e))
    assert not bad, bad
