"""GPU: csrc/clipdata.hip through vistracker_amd.infill_data.HVOPClipData against the numpy model of tests/clipdata_model.py (float64 the reference, float32 the
error scale) and the reference's recorded ``get_item`` (tests/golden/clipdata.npz).  Gate per column group (body 6D, body translation, object 6D, object
translation): |gpu - f64| <= 8 e32, e32 the float32 model's largest error on the case; a group whose e32 is 0 (copies, masks) must match exactly.  No frame is
left out of a case: tests/test_host_clipdata.py shows that no un-masked augmented frame of these cases lies near the angle pi.  Measured ratios:
tests/golden/clipdata.md."""
import numpy as np
import pytest
import torch

import clipdata_cases as CC
import clipdata_model as M
import former_cases as FC
from conftest import golden
from test_host_clipdata import golden_setting

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dataset(T, window, obj_repre, aug_num, **kw):
    from vistracker_amd.infill_data import HVOPClipData
    seqs, names = CC.sequences()
    args = dict(start_fr_min=2, start_fr_max=12, min_drop_len=3, max_drop_len=8, obj_repre=obj_repre, aug_num=aug_num, multi_kinects=True, kinect=CC.kinect(), device=DEV)
    args.update(kw)
    return HVOPClipData.from_packed(seqs, names, T, window, **args)


def dev_dec(dec):
    return {k: torch.tensor(np.ascontiguousarray(v), dtype=torch.int32, device=DEV) for k, v in dec.items() if k in ("kid", "drop_len", "start_fr", "aug_start")}


def host(batch):
    return {k: v.cpu().numpy() for k, v in batch.items()}


def report(tag, res):
    for (t, grp), (err, e32) in res.items():
        print(f"\n[clipdata] {tag} {t}/{grp}: err {err:.3e} e32 {e32:.3e} ratio {err / e32 if e32 > 0 else 0.0:.2f}", end="")


@pytest.mark.parametrize("c", CC.build_cases(), ids=lambda c: c["id"])
def test_build_against_the_float64_model(c):
    b = CC.build(c)
    kw = dict(start_fr_min=0, start_fr_max=1, min_drop_len=0, max_drop_len=0) if c["T"] == 1 else {}
    data = dataset(c["T"], c["window"], c["obj_repre"], c["aug_num"], **kw)
    tab, starts, dates, n_seq = CC.model_data(c["T"], c["window"])
    assert np.array_equal(data.clip_start_host, starts) and np.array_equal(data.clip_date_host, dates) and data.n_seq == n_seq and len(data) == len(starts)
    noise = torch.tensor(b["noise"], dtype=torch.float32, device=DEV) if c["aug_num"] else None
    got = host(data.build(b["idx"], dev_dec(b["dec"]), noise=noise))
    res, bad = M.gate(got, b["ref64"], b["ref32"], c["obj_dim"])
    report(c["id"], res)
    assert not bad, bad
    assert got["mask_obj"].dtype == np.bool_ and got["data_smpl"].shape == (c["B"], c["T"], 147) and got["data_obj"].shape == (c["B"], c["T"], c["obj_dim"])
    assert np.array_equal(got["drop_start"], b["dec"]["start_fr"]) and np.array_equal(got["drop_len"], b["dec"]["drop_len"])
    # bit for bit: gt_smpl is data_smpl; gt_obj is data_obj on frames neither masked nor augmented; a masked, un-augmented row is zero; kid == 1 copies translations
    assert np.array_equal(got["gt_smpl"], got["data_smpl"])
    free = ~b["ref64"]["mask_obj"] & ~b["ref64"]["aug"]
    assert np.array_equal(got["gt_obj"][free], got["data_obj"][free])
    assert (got["data_obj"][b["ref64"]["mask_obj"] & ~b["ref64"]["aug"]] == 0).all()
    for i in np.nonzero(b["dec"]["kid"] == 1)[0]:
        s = int(starts[b["idx"][i]])
        assert np.array_equal(got["data_smpl"][i, :, 144:], tab["trans"][s:s + c["T"]].astype(np.float32))
        if c["obj_dim"] == 9:
            assert np.array_equal(got["gt_obj"][i, :, 6:], tab["obj_trans"][s:s + c["T"]].astype(np.float32))


@pytest.mark.parametrize("s", range(4))
def test_build_against_the_recording(s):
    g = golden("clipdata")
    tab, starts, dates, rec, T, od, _ = golden_setting(g, s)
    aug = rec["aug_start"].shape[1]
    data = dataset(T, int(g["window"]), "6d" if od == 6 else "9d", aug)
    idx = rec["clip"]
    ref32 = M.build(tab, starts[idx], dates[idx], rec, T, od, rec["noise"], np.float32)
    noise = torch.tensor(rec["noise"], dtype=torch.float32, device=DEV) if aug else None
    got = host(data.build(idx, dev_dec(rec), noise=noise))
    res, bad = M.gate(got, rec, ref32, od)
    report(f"recording s{s}", res)
    assert not bad, bad


def test_bitwise_properties_and_draws():
    data = dataset(20, 7, "9d", 4)
    idx = np.asarray([5, 0, 33, 12, 56], np.int32)
    a, b = data.batch(idx, 77, 3), data.batch(idx, 77, 3)
    assert all(torch.equal(a[k], b[k]) for k in a)
    # a clip's rows depend on (seed, epoch, clip) only: alone, in another position, among other clips
    for pos, i in enumerate(idx):
        alone = data.batch(np.asarray([i]), 77, 3)
        assert all(torch.equal(alone[k][0], a[k][pos]) for k in a), int(i)
    r = data.batch(idx[::-1].copy(), 77, 3)
    assert all(torch.equal(r[k].flip(0), a[k]) for k in a)
    assert not torch.equal(data.batch(idx, 77, 4)["data_obj"], a["data_obj"]) and not torch.equal(data.batch(idx, 78, 3)["data_obj"], a["data_obj"])
    # the draws are the model's integers
    every = np.arange(data.num_clips, dtype=np.int32)
    for seed, epoch in ((77, 3), (0x9abcdef012345678, 2 ** 32 - 1)):
        d = host(data.draw(every, seed, epoch))
        m = M.draw(every, seed, epoch, 20, True, 3, 8, 2, 12, 4)
        for k in m:
            assert d[k].dtype == np.int32 and np.array_equal(d[k], m[k]), k
    assert (host(dataset(20, 7, "6d", 0, multi_kinects=False, kinect=None).draw(every, 1, 0))["kid"] == 1).all()
    # the hashed noise: batch() equals build() with the model's float32 Box-Muller values to the gate of the explicit-noise cases
    dec = data.draw(idx, 77, 3)
    z = M.hashed_noise(idx, 77, 3, 4, np.float32)
    tab, starts, dates, _ = CC.model_data(20, 7)
    hd = {k: v.cpu().numpy() for k, v in dec.items()}
    ref64 = M.build(tab, starts[idx], dates[idx], hd, 20, 9, M.hashed_noise(idx, 77, 3, 4, np.float64), np.float64)
    ref32 = M.build(tab, starts[idx], dates[idx], hd, 20, 9, z, np.float32)
    assert CC.min_aug_w(ref64) >= CC.W_MIN
    res, bad = M.gate(host(a), ref64, ref32, 9)
    report("hashed noise", res)
    assert not bad, bad


def test_refusals():
    from vistracker_amd import ops
    from vistracker_amd._lib import VtError
    from vistracker_amd.infill_data import HVOPClipData
    data = dataset(20, 7, "6d", 4)
    idx = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    dec = data.draw(idx, 1, 0)
    start, date = data.clip_start[:2].contiguous(), data.clip_date[:2].contiguous()
    build = lambda tables=data.tables, R=data.w2c_R, st=start, dc=dec, od=6: ops.clip_build(tables, R, data.w2c_t, st, date, dc, 20, od, None, idx, 1, 0)          # noqa: E731
    build()
    with pytest.raises(VtError, match="dtype"):
        build(tables=dict(data.tables, poses=data.tables["poses"].double()))
    with pytest.raises(VtError, match="dtype"):
        build(dc=dict(dec, kid=dec["kid"].long()))
    with pytest.raises(VtError, match="contiguous"):
        build(tables=dict(data.tables, trans=torch.zeros((3, data.tables["trans"].shape[0]), device=DEV).t()))
    with pytest.raises(VtError, match="contiguous"):
        build(st=torch.zeros(4, dtype=torch.int32, device=DEV)[::2])
    with pytest.raises(VtError, match="shape"):
        build(dc=dict(dec, drop_len=dec["drop_len"][:1]))
    with pytest.raises(VtError, match="device"):
        build(st=start.cpu())
    with pytest.raises(VtError, match="obj_dim"):
        build(od=7)
    with pytest.raises(VtError, match="dtype"):
        ops.clip_draw(idx.long(), 1, 0, 20, True, 3, 8, 2, 12, 4)
    with pytest.raises(VtError, match="out of range"):
        data.batch([0, data.num_clips], 1, 0)
    with pytest.raises(VtError, match="out of range"):
        data.draw([-1], 1, 0)
    seqs, names = CC.sequences()
    with pytest.raises(VtError, match="no sequence"):
        HVOPClipData.from_packed(seqs, names, 231, 7, kinect=CC.kinect(), device=DEV)
    for kw in (dict(start_fr_min=12, start_fr_max=12), dict(max_drop_len=18, start_fr_min=2), dict(min_drop_len=9, max_drop_len=8), dict(aug_num=20)):
        with pytest.raises(VtError):
            dataset(20, 7, "6d", kw.pop("aug_num", 0), **kw)
    with pytest.raises(VtError, match="empty"):
        ops.clip_draw(idx, 1, 0, 20, True, 3, 18, 2, 12, 0)
    with pytest.raises(VtError, match="smpl_repre"):
        dataset(20, 7, "6d", 0, smpl_repre="joints-smpl")
    with pytest.raises(VtError, match="transforms"):
        dataset(20, 7, "6d", 0, kinect={"Date01": CC.kinect()["Date01"]})
    # the phase rule of __len__
    assert len(dataset(20, 7, "6d", 0, phase="val")) == 2 and len(data) == data.num_clips == 57


@pytest.fixture(scope="module")
def weights():
    return FC.seeded_weights(golden("infill"), 31)


def small_set():
    """8 clips of 20 frames"""
    d = dataset(20, 56, "6d", 4)
    assert d.num_clips == 8
    return d


def test_train_epoch_is_the_hand_written_loop_without_a_host_wait(weights, monkeypatch):
    from vistracker_amd import infill_training as IT
    from vistracker_amd.training import distributed_indices
    data = small_set()
    a, b = IT.HVOPTrainer(weights, FC.hvop_opt(), dropout=0.05), IT.HVOPTrainer(weights, FC.hvop_opt(), dropout=0.05)

    def barred(*a_, **k_):
        raise AssertionError("train_epoch went to the host")

    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", barred)
        mp.setattr(torch.Tensor, "numpy", barred)
        mp.setattr(torch.cuda, "synchronize", barred)
        total, sep, n = a.train_epoch(data, 2, 9, 4)
    assert n == 2 and total.is_cuda and sep.shape == (2,)
    b.set_step(2)
    order = distributed_indices(len(data), 1, 0, 2, 9)
    losses = []
    for i in range(2):
        losses.append(b.train_step(data.batch(np.asarray(order[4 * i:4 * i + 4]), 9, 2), IT.batch_seed(9, 2, i)))
    sa, sb = a.state_dict(), b.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert torch.equal(total, losses[0][0] + losses[1][0]) and torch.equal(sep, losses[0][1] + losses[1][1])
    assert any(not torch.equal(sa[k], torch.as_tensor(weights[k], device=DEV)) for k in sa)
    # two ranks split the order
    assert a.train_epoch(data, 3, 9, 4, world=2, rank=1)[2] == 1


def test_validate_is_the_mean_of_the_batch_losses(weights):
    from vistracker_amd import infill_training as IT
    from vistracker_amd.training import distributed_indices
    data = small_set()
    tr = IT.HVOPTrainer(weights, FC.hvop_opt(), dropout=0.05)
    before = tr.state_dict()
    loss, sep = tr.validate(data, 3, seed=4)
    assert all(e.training for e in tr.model.enc.values())
    after = tr.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)
    order = distributed_indices(len(data), 1, 0, 0, 4, drop_last=False)
    tr.model.eval()
    with torch.no_grad():
        each = [tr._loss(data.batch(np.asarray(order[i:i + 3]), 4, 0)) for i in range(0, 8, 3)]
    tr.model.train()
    assert len(each) == 3
    want, wsep = (each[0][0] + each[1][0] + each[2][0]) / 3, (each[0][1] + each[1][1] + each[2][1]) / 3
    assert torch.equal(loss, want) and torch.equal(sep, wsep) and bool(torch.isfinite(loss))
    assert torch.equal(tr.validate(data, 3, max_batches=1, seed=4)[0], each[0][0])
