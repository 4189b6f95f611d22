"""GPU (-m gpu): the three bookkeeping kernels of a generator round (vt_gen_round_compact, vt_gen_scatter_heads, vt_gen_resample; vistracker_amd/csrc/gen.hip)
against the exact model (tests/gen_model.py) on the cases of tests/gen_cases.py, and the fused driver of Generator.gen_pc_batch against the torch driver with a
stubbed network.

Every operation of the kernels is exact (integer indices, copies, one float32 multiply and one float32 add, no contraction), so every comparison here is bit for
bit on the raw arrays: the whole allocation of every output -- guard bands, rows behind the capacity and entries the contract leaves unwritten included.
tests/test_host_gen_model.py shows that the model is the torch formulation the kernels replaced and that these cases tell seventeen wrong variants from it."""
import ast
import functools
import types

import numpy as np
import pytest

import gen_cases as GC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FAMILIES = sorted(GC.FAMILIES)


def _shape(case, k):
    return case[k].shape


def _mismatch(case, k, got, want):
    """None, or a message naming the case, the frame, the first differing index, and the got and want values"""
    gb, wb = GC.bits(got), GC.bits(want)
    if np.array_equal(gb, wb):
        return None
    i = int(np.flatnonzero(gb != wb)[0]); shape = _shape(case, k); n = int(np.prod(shape))
    if i < GC.GUARD or i >= GC.GUARD + n:
        return f"{case['name']} {k}: guard band element {i - GC.GUARD if i < GC.GUARD else i - GC.GUARD - n:+d} of the array: got {got[i]!r}, want {want[i]!r}"
    idx = tuple(int(x) for x in np.unravel_index(i - GC.GUARD, shape))
    return f"{case['name']} {k}: frame {idx[0]}, index {idx}: got {got[i]!r}, want {want[i]!r} ({int((gb != wb).sum())} elements differ)"


@functools.lru_cache(maxsize=None)
def _first_run(family):
    """every case of a family through its kernel, once per session (do not modify)"""
    cases, _, run = GC.FAMILIES[family]
    return [run(c) for c in cases()]


@pytest.mark.parametrize("family", FAMILIES)
def test_every_element_equals_the_model(family):
    cases, expected, _ = GC.FAMILIES[family]
    n_cases = n_elems = 0
    for c, got in zip(cases(), _first_run(family)):
        want = expected(c)
        for k in want:
            assert (got[k] is None) == (want[k] is None), (c["name"], k)
            if want[k] is not None:
                msg = _mismatch(c, k, got[k], want[k])
                assert msg is None, msg
                n_elems += want[k].size
        n_cases += 1
    print(f"{family}: {n_cases} cases, {n_elems} elements compared bit for bit (guard bands and unwritten entries included)")


@pytest.mark.parametrize("family", FAMILIES)
def test_two_calls_give_equal_bits(family):
    cases, _, run = GC.FAMILIES[family]
    for c, first in zip(cases(), _first_run(family)):
        again = run(c)
        for k, a in first.items():
            msg = None if a is None else _mismatch(c, k, again[k], a)
            assert msg is None, "second call: " + msg


@pytest.mark.parametrize("family", FAMILIES)
def test_a_frame_alone_equals_the_frame_in_its_batch(family):
    cases, _, run = GC.FAMILIES[family]
    for c, batch in zip(cases(), _first_run(family)):
        if c["B"] == 1:
            continue
        for b in range(c["B"]):
            f = GC.frame_of(c, b); alone = run(f)
            for k, a in alone.items():
                if a is None:
                    continue
                want = GC.guarded(np.ascontiguousarray(GC.inner(batch[k], c[k].shape)[b:b + 1]), GC.guard_of(a.dtype))
                msg = _mismatch(f, k, a, want)
                assert msg is None, f"alone against frame {b} of the batch: " + msg


# ---- bad arguments: an error code, VtError through L.check (asserted by the runners), nothing written --------------------------------------------------------
def _by_name(family, name):
    return next(c for c in GC.FAMILIES[family][0]() if c["name"].startswith(name))


BAD = {
    "compact": ("compact-S65-write_pre-b0", [dict(surface=None), dict(df=None), dict(active=None), dict(fill=None), dict(order=None), dict(cnt=None), dict(fill_out=None),
                                              dict(B=0), dict(B=-1), dict(S=0), dict(S=-1), dict(cap=0), dict(cap=-1), dict(write=1, buf_points=None), dict(pre=None)]),
    "scatter": ("scatter-C3-kmax65-cap70", [dict(pred=None), dict(fill_old=None), dict(cnt=None), dict(buf=None), dict(B=0), dict(B=-1), dict(C=0), dict(C=-1), dict(kmax=0),
                                            dict(kmax=-1), dict(cap=0), dict(cap=-1)]),
    "resample": ("resample-M257-S0_7-S65", [dict(samples=None), dict(order=None), dict(cnt=None), dict(init=None), dict(u=None), dict(pert=None), dict(out=None), dict(B=0),
                                            dict(B=-1), dict(S=0), dict(S=-1), dict(S0=0), dict(S0=-1), dict(M=0), dict(M=-1)]),
}


@pytest.mark.parametrize("family", FAMILIES)
def test_bad_arguments_are_refused_and_nothing_is_written(family):
    name, overrides = BAD[family]; c = _by_name(family, name); run = GC.FAMILIES[family][2]
    assert family != "compact" or (c["write"] == 1 and c["pre"] is not None and c["kept_pre"] is not None)       # dict(pre=None): kept_pre without pre
    for o in overrides:
        out = run(c, override=o, expect_error=True)
        for k, a in out.items():
            msg = None if a is None else _mismatch(c, k, a, GC.guarded(np.ascontiguousarray(c[k]), GC.guard_of(a.dtype)))
            assert msg is None, f"refused call {o} wrote: " + msg
    run(c)                                                                                                      # and the unmodified call is accepted


# ---- the fused driver against the torch driver, the network stubbed -----------------------------------------------------------------------------------------------
class _StubNet:
    """ops.sifnet_project_step / ops.sifnet_query as small deterministic torch functions of the points and a round counter.  The projection leaves the points
    where they are; a sample is near the surface when a hash of its position is below the rate of its frame in this round (the frame's number travels in
    crop_center[:, 0]).  Records what a correct driver must return: per frame, the points it showed that pass the filter, in sample order, from round 1 on."""
    def __init__(self, rate):
        self.rate, self.round, self.kept, self.seen, self.counts = rate, 0, {}, [], []

    def project_step(self, net, maps, pts, crop_center, body_center, df_idx, threshold=1.0, out=None, want_target=True):
        assert want_target and net is None and maps is None
        frames = [int(round(v)) for v in crop_center[:, 0].tolist()]
        h = torch.frac(torch.sin(pts.sum(-1) * 37.0 + self.round).abs() * 1000.0)
        near = h < torch.tensor([self.rate(f, self.round) for f in frames], device=pts.device)[:, None]
        df = torch.full(near.shape, 0.5, device=pts.device); df[near] = 0.01
        mask = near & (pts[:, :, 2] > 1.0)
        for j, f in enumerate(frames):
            if self.round > 0:
                self.kept.setdefault(f, []).append(pts[j][mask[j]].clone())
        self.seen.append(tuple(frames)); self.counts.append({f: int(mask[j].sum()) for j, f in enumerate(frames)})
        self.round += 1
        if out is not None and out is not pts:
            out.copy_(pts)
        return (pts if out is None else out), df

    def query(self, net, maps, pts, crop_center, body_center, head_mask=31):
        x = pts.transpose(1, 2)
        parts = torch.sin(pts.sum(-1)[:, None, :] * torch.arange(1, 15, device=pts.device, dtype=pts.dtype)[None, :, None])
        return None, torch.cat([x, x * 2.0, x * 0.5], 1).contiguous(), parts, (x + 1.0).contiguous(), torch.sigmoid(pts[:, :, 2])[:, None, :]


NUM_POINTS, S0 = 300, 3000
SCENARIOS = {
    # (a) frame 2 keeps nothing in rounds 0 and 1: it restarts from the grid twice
    "restart": dict(B=4, skip=True, rate=lambda f, r: 0.0 if f == 2 and r < 2 else 0.003),
    # (b) every frame in every round; frame 0 keeps everything and reaches the capacity while frame 1 keeps about 0.1 %
    "capacity": dict(B=3, skip=False, rate=lambda f, r: (1.0, 0.001, 0.3)[f]),
    # (c) default sit-out: frame 0 is ahead and sits out; from round 5 on the slow frames' yield rises thirty-fold, the common count overtakes frame 0
    "reactivation": dict(B=3, skip=True, rate=lambda f, r: 0.005 if f == 0 else (0.001 if r < 5 else 0.03)),
}


def run_driver(setattr_, scenario, fused, device="cuda:0"):
    from vistracker_amd import ops
    from vistracker_amd.generator import GeneratorTriplaneVis
    sc = SCENARIOS[scenario]; B = sc["B"]; stub = _StubNet(sc["rate"])
    setattr_(ops, "sifnet_project_step", stub.project_step); setattr_(ops, "sifnet_query", stub.query)
    model = types.SimpleNamespace(handle=None, maps=None)
    gen = GeneratorTriplaneVis(model, "x", seed=5, device=device); gen.use_projection = False; gen.fused_rounds = fused; gen.skip_done_frames = sc["skip"]
    gen.reseed(0)
    bc = torch.tensor([[0.0, 0.0, 2.2]] * B, device=device)
    cc = torch.zeros(B, 2, device=device); cc[:, 0] = torch.arange(B, device=device)
    init = gen.get_grid_samples(S0, B, bc)
    out = gen.gen_pc_batch(model, "object", init, NUM_POINTS, {"crop_center": cc, "body_center": bc, "path": ["x"] * B}, num_steps=1)
    return {k: v.cpu().numpy() for k, v in out.items()}, stub


def _stats(text):
    line = [l for l in text.splitlines() if l.startswith("[VT_GEN_STATS]")]
    assert len(line) == 1, text
    return ast.literal_eval(line[0].split("max):", 1)[1].strip())


@pytest.mark.parametrize("scenario", sorted(SCENARIOS))
def test_fused_driver_equals_the_torch_driver(scenario, monkeypatch, capsys):
    monkeypatch.setenv("VT_GEN_STATS", "1")
    capsys.readouterr()
    sorts = []; argsort = torch.argsort                                    # the torch driver sorts the mask once a round, the fused driver never
    monkeypatch.setattr(torch, "argsort", lambda *x, **kw: (sorts.append(1), argsort(*x, **kw))[1])
    a, stub_a = run_driver(monkeypatch.setattr, scenario, True); stats_a = _stats(capsys.readouterr().out); sorts_a = len(sorts)
    b, stub_b = run_driver(monkeypatch.setattr, scenario, False); stats_b = _stats(capsys.readouterr().out)
    assert sorts_a == 0 and len(sorts) == len(stub_b.seen), (sorts_a, len(sorts))
    B = SCENARIOS[scenario]["B"]; n = a["points"].shape[1]; cap = NUM_POINTS + 20000
    # both drivers showed the network the same frames in the same rounds and kept the same numbers of points
    assert stub_a.seen == stub_b.seen and stub_a.counts == stub_b.counts and stats_a == stats_b
    assert set(a) == set(b) == {"points", "pca_axis", "parts", "centers", "visibility"} and n >= NUM_POINTS
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(GC.bits(a[k]), GC.bits(b[k])), (scenario, k)
    for i in range(B):                                                      # the points are the kept points the stub recorded, in order, cut to the common count
        ref = torch.cat(stub_a.kept[i], 0).cpu().numpy()
        assert ref.shape[0] >= n and np.array_equal(GC.bits(a["points"][i]), GC.bits(np.ascontiguousarray(ref[:n]))), (scenario, i)
    assert np.isfinite(a["points"]).all() and np.isfinite(a["pca_axis"]).all() and np.isfinite(a["visibility"]).all()
    # each scenario took its branch.  stats: (round, active frames, round minimum, common count, fill min, fill median, fill max)
    if scenario == "restart":
        assert stub_a.counts[0][2] == 0 and stub_a.counts[1][2] == 0 and stub_a.counts[2][2] > 1                # cnt <= 1 after rounds 0 and 1: two restarts
        assert min(stub_a.counts[0][f] for f in (0, 1, 3)) > 1 and stats_a[0][2] == 0
    if scenario == "capacity":
        assert max(s[6] for s in stats_a) == cap and all(s[1] == B for s in stats_a)
        assert sum(c[0] for c in stub_a.counts[1:]) > cap                                                       # frame 0 kept more than fits: rows were cut off
    if scenario == "reactivation":
        out_rounds = [r for r, seen in enumerate(stub_a.seen) if 0 not in seen]
        assert out_rounds and 0 in stub_a.seen[-1] and len(stub_a.seen) - 1 > out_rounds[-1]                   # frame 0 sat out and came back
        assert stub_a.seen[-1] == (0,) and stats_a[-1][1] == 1                                                  # alone: the refill rounds
        assert stats_a[-1][3] == n and stats_a[-1][4] >= n
