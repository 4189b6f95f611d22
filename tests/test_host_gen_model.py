"""CPU: the exact model of the generator's round kernels (tests/gen_model.py) against the torch formulation those kernels replaced (the non-fused branch of
Generator.gen_pc_batch, restated below expression by expression), the conditions the case set of tests/gen_cases.py promises, and the mutants of the model that
the cases must tell from it.  Every comparison is bit for bit."""
import numpy as np
import pytest

import gen_cases as GC
import gen_model as GM

torch = pytest.importorskip("torch")

same = lambda a, b: a.shape == b.shape and np.array_equal(GC.bits(np.ascontiguousarray(a)), GC.bits(np.ascontiguousarray(b)))


# ---- the torch expressions of vistracker_amd/generator.py (the branch below ``if fused:``) ---------------------------------------------------------------------
def torch_round(c):
    """mask, stable argsort, scatter with the trash row -> buf_points, order, kept_pre (the gather the kept-points head query reads), cnt, fill"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    samples_surface, df_target, fill = t(c["surface"]), t(c["df"]), t(c["fill"]); B, S, cap = c["B"], c["S"], c["cap"]
    act = t(c["active"]).bool()
    mask = (df_target < GC.FILTER_VAL) & (samples_surface[:, :, 2] > GC.ZMIN) & act[:, None]
    cnt = mask.sum(1)
    order = torch.argsort((~mask).to(torch.uint8), dim=1, stable=True)
    ar = torch.arange(S)[None]
    buf = t(c["buf_points"]).clone()
    if c["write"]:
        dest = fill[:, None] + ar
        valid = (ar < cnt[:, None]) & (dest < cap)
        dest = torch.where(valid, dest, torch.full_like(dest, cap))
        buf.scatter_(1, dest[..., None].expand(B, S, 3), samples_surface.gather(1, order[..., None].expand(B, S, 3)))
        fill = torch.minimum(fill + cnt, torch.full_like(fill, cap))
    else:
        fill = torch.minimum(fill, torch.full_like(fill, cap))          # (the driver leaves fill alone in round 0, and fill <= cap always)
    kept_pre = None if c["pre"] is None else t(c["pre"]).gather(1, order[..., None].expand(B, S, 3))
    return buf.numpy(), order.numpy(), None if kept_pre is None else kept_pre.numpy(), cnt.numpy(), fill.numpy()


def torch_scatter(c):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    B, kmax, cap = c["B"], c["kmax"], c["cap"]; fill, cnt = t(c["fill_old"]), t(c["cnt"])
    ar = torch.arange(kmax)[None]
    dest = fill[:, None] + ar
    valid = (ar < cnt[:, None]) & (dest < cap)
    dest = torch.where(valid, dest, torch.full_like(dest, cap))
    pr = t(c["pred"]).reshape(B, -1, kmax).transpose(1, 2)
    Cc = pr.shape[2]
    buf = t(c["buf"]).clone()
    buf.scatter_(1, dest[:, :kmax, None].expand(B, kmax, Cc), pr)
    return buf.numpy()


def torch_resample(c, threshold=1.0):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    B, S0, sample_num = c["B"], c["S0"], c["M"]
    samples, order, cnt, samples_init, u, pert = t(c["samples"]), t(c["order"]).long(), t(c["cnt"]), t(c["init"]), t(c["u"]), t(c["pert"])
    k = torch.minimum((u * cnt[:, None]).long(), (cnt[:, None] - 1).clamp(min=0))
    near = samples.gather(1, order.gather(1, k)[..., None].expand(B, sample_num, 3)) + (threshold / 3) * pert
    k0 = (u * S0).long().clamp(max=S0 - 1)
    restart = samples_init.gather(1, k0[..., None].expand(B, sample_num, 3)) + 0.5 * pert
    return torch.where((cnt > 1)[:, None, None], near, restart).numpy()


# ---- 1. the model is what the kernels replaced ---------------------------------------------------------------------------------------------------------------
def test_compaction_model_equals_the_torch_formulation():
    for c in GC.compact_cases():
        e = GC.expected_compact(c)
        buf, order, kept_pre, cnt, fill = torch_round(c); B, S, cap = c["B"], c["S"], c["cap"]
        m_buf, m_order, m_cnt, m_fill = GC.inner(e["buf_points"], (B, cap + 1, 3)), GC.inner(e["order"], (B, S)), GC.inner(e["cnt"], (B,)), GC.inner(e["fill_out"], (B,))
        assert np.array_equal(m_cnt, cnt) and np.array_equal(m_fill, fill), c["name"]
        assert same(m_buf[:, :cap], buf[:, :cap]), c["name"]                                    # everything but the trash row
        assert same(m_buf[:, cap], c["buf_points"][:, cap]), c["name"]                          # which the model leaves alone
        for b in range(B):
            assert np.array_equal(m_order[b, :cnt[b]], order[b, :cnt[b]]) and (m_order[b, cnt[b]:] == GC.PRE_I).all(), (c["name"], b)
        if c["kept_pre"] is not None:
            assert same(GC.inner(e["kept_pre"], (B, S, 3)), kept_pre), c["name"]
        else:
            assert e["kept_pre"] is None


def test_scatter_model_equals_the_torch_formulation():
    for c in GC.scatter_cases():
        m = GC.inner(GC.expected_scatter(c)["buf"], c["buf"].shape); cap = c["cap"]
        assert same(m[:, :cap], torch_scatter(c)[:, :cap]) and same(m[:, cap], c["buf"][:, cap]), c["name"]


def test_resample_model_equals_the_torch_formulation():
    assert GC.NEAR_SCALE == float(np.float32(1.0 / 3))                                          # what generator.py passes for threshold = 1
    for c in GC.resample_cases():
        assert same(GC.inner(GC.expected_resample(c)["out"], c["out"].shape), torch_resample(c)), c["name"]


# ---- 2. the cases are what they promise ----------------------------------------------------------------------------------------------------------------------
def test_sentinels_are_finite_nonzero_and_no_input_value():
    for s in (GC.GUARD_F, GC.PRE_F, GC.GUARD_I, GC.PRE_I):
        assert np.isfinite(s) and s != 0
    assert GC.GUARD_F != GC.PRE_F and GC.GUARD_I != GC.PRE_I
    for fam, (cases, _, _) in GC.FAMILIES.items():
        for c in cases():
            for k, v in c.items():
                if isinstance(v, np.ndarray) and k not in ("buf_points", "order", "kept_pre", "cnt", "fill_out", "buf", "out", "keep") or (fam == "resample" and k in ("order", "cnt")):
                    assert not np.isin(v, [GC.GUARD_F, GC.PRE_F, GC.GUARD_I, GC.PRE_I]).any(), (c["name"], k)


def test_compaction_cases_cover_what_they_promise():
    cases = GC.compact_cases(); seen_kinds, seen_rungs, seen_edges, seen_cfg, counts = set(), set(), set(), set(), {}
    assert {c["B"] for c in cases} == {1, 3, 5} and {c["S"] for c in cases} == set(GC.COMPACT_S) and {c["cap"] for c in cases} == set(GC.CAPS)
    fv, zm = np.float32(GC.FILTER_VAL), np.float32(GC.ZMIN)
    for c in cases:
        B, S, cap = c["B"], c["S"], c["cap"]; e = GC.expected_compact(c); cnt = GC.inner(e["cnt"], (B,))
        form = GC.COMPACT_FORMS[c["form"]]
        assert (c["pre"] is not None) == form["has_pre"] and (c["kept_pre"] is not None) == form["has_kept_pre"] and c["write"] == form["write"]
        seen_cfg |= {("S-form", S, c["form"]), ("cap-form", cap, c["form"]), ("S-cap", S, cap)}
        assert np.array_equal(cnt, c["keep"].sum(1) * c["active"]), c["name"]                # the frames keep what they were built to keep
        for b, kind in enumerate(c["kinds"]):
            seen_kinds.add((S, c["form"], kind)); counts.setdefault(S, set()).add(int(cnt[b]))
            k = np.flatnonzero(c["keep"][b])
            if kind == "inactive":
                assert not c["active"][b] and c["keep"][b].all() and cnt[b] == 0
            if kind == "two" and S > 64:
                assert list(k) == [63, 64]
            if kind == "wave_last":
                assert list(k) == list(range(63, S, 64))
            if kind == "random30" and S >= 255:
                assert 0.2 * S < len(k) < 0.4 * S
            f, n = int(c["fill"][b]), int(cnt[b])
            assert 0 <= f <= cap
            if c["write"] and n > 0:
                seen_rungs |= {r for r, hit in (("empty", f == 0), ("exact_fit", f + n == cap and f > 0), ("one_cut", f + n == cap + 1 and f > 0), ("one_left", f == cap - 1 and n > 1 and cap > 1),
                                                ("full", f == cap), ("overflow_from_empty", f == 0 and n > cap)) if hit}
        for b, name, i in c["edges"]:
            df, z = c["df"][b, i], c["surface"][b, i, 2]
            assert dict(df_eq=df == fv, df_below=df == np.nextafter(fv, np.float32(-1)) and df < fv, z_eq=z == zm, z_above=z == np.nextafter(zm, np.float32(2)) and z > zm,
                        df_nan=np.isnan(df), z_nan=np.isnan(z), df_ninf=df == -np.inf, z_pinf=z == np.inf)[name], (c["name"], name)
            assert c["keep"][b, i] == GC.EDGE_KEPT[name] and c["kinds"][b] == "edges"
            seen_edges.add((name, S >= 8))
        if S >= 8:
            for b, kind in enumerate(c["kinds"]):
                assert kind != "edges" or {n for bb, n, _ in c["edges"] if bb == b} == set(GC.EDGES), c["name"]
    kinds = {k for batch in GC.COMPACT_BATCHES for k in batch}
    assert kinds == {"none", "all", "first", "last", "two", "every_second", "wave_last", "random30", "inactive", "edges"}
    assert seen_kinds == {(S, f, k) for S in GC.COMPACT_S for f in GC.COMPACT_FORMS for k in kinds}
    assert seen_cfg >= {("S-form", S, f) for S in GC.COMPACT_S for f in GC.COMPACT_FORMS} | {("cap-form", cap, f) for cap in GC.CAPS for f in GC.COMPACT_FORMS} \
        | {("S-cap", S, cap) for S in GC.COMPACT_S for cap in GC.CAPS}
    assert seen_rungs == set(GC.RUNGS) | {"overflow_from_empty"}
    assert {n for n, _ in seen_edges} == set(GC.EDGES) and {n for n, big in seen_edges if not big} == set(GC.EDGES)          # also among the S = 1 frames
    for S, got in counts.items():
        assert {0, 1, S} <= got and (S < 2 or 2 in got), (S, sorted(got))                       # the kept counts 0, 1, 2 and S occur at every S


def test_scatter_cases_cover_what_they_promise():
    cases = GC.scatter_cases(); combos, blocks = set(), set()
    assert {(c["C"], c["kmax"], c["cap"]) for c in cases} == {(C, k, cap) for C in GC.SCATTER_C for k in GC.SCATTER_KMAX for cap in GC.CAPS}
    for c in cases:
        blocks.add(c["kmax"] * c["C"] > 256)
        for b in range(c["B"]):
            n, f, cap = int(c["cnt"][b]), int(c["fill_old"][b]), c["cap"]
            assert 0 <= n <= c["kmax"] and 0 <= f <= cap
            assert n == dict(zero=0, one=1, kmax_less_one=c["kmax"] - 1, kmax=c["kmax"]).get(c["cnt_kinds"][b], n)
            combos.add((c["cnt_kinds"][b], c["rungs"][b]))
            if n > 0:
                combos |= {r for r, hit in (("empty", f == 0), ("exact_fit", f + n == cap and f > 0), ("one_cut", f + n == cap + 1 and f > 0), ("one_left", f == cap - 1 and n > 1 and cap > 1),
                                            ("full", f == cap)) if hit}
    assert blocks == {False, True}
    assert combos >= {(k, r) for k in GC.SCATTER_CNT for r in GC.RUNGS} | set(GC.RUNGS)


def test_resample_cases_cover_what_they_promise():
    cases = GC.resample_cases()
    assert {(c["M"], c["S0"], c["S"]) for c in cases} == {(M, S0, S) for M in GC.RESAMPLE_M for S0 in GC.RESAMPLE_S0 for S in GC.RESAMPLE_S}
    for S in GC.RESAMPLE_S:
        assert {int(n) for c in cases if c["S"] == S for n in c["cnt"]} == {0, 1, S} | {n for n in (2, 3) if n <= S}
    for M in GC.RESAMPLE_M:
        planted = set().union(*[c["u_kinds"] for c in cases if c["M"] == M])
        assert planted == set(GC.U_KINDS), (M, planted)
    one = np.float32(1)
    for c in cases:
        assert c["u"].dtype == np.float32 and (c["u"] >= 0).all() and (c["u"] <= one).all()
        if c["M"] > 1:
            assert c["u_kinds"] >= {"zero", "below_one", "one"} and (c["u"] == one).any() and (c["u"] == 0).any() and (c["u"] == np.nextafter(one, np.float32(0))).any()
        for b in range(c["B"]):
            assert sorted(c["order"][b]) == list(range(c["S"]))
        assert c["S"] == 1 or not np.array_equal(c["order"][0], np.arange(c["S"]))
    # the value of near_scale tells the rounded product plus the point from a fused multiply-add somewhere in every case that has a frame with cnt > 1
    for c in cases:
        if (c["cnt"] > 1).any() and c["M"] > 1:
            assert not same(GC.expected_resample(c)["out"], GC.expected_resample(c, "resample_fma")["out"]), c["name"]


def test_guard_bands_survive_the_model_and_inputs_are_not_modified():
    for fam, (cases, expected, _) in GC.FAMILIES.items():
        for c in cases():
            before = {k: v.copy() for k, v in c.items() if isinstance(v, np.ndarray)}
            for k, full in expected(c).items():
                if full is None:
                    continue
                g = GC.GUARD_F if full.dtype == np.float32 else GC.GUARD_I
                assert (full[:GC.GUARD] == g).all() and (full[-GC.GUARD:] == g).all() and full.size == c[k].size + 2 * GC.GUARD, (c["name"], k)
            for k, v in before.items():
                assert same(v, c[k]), (c["name"], k)


def test_frame_of_a_case_is_that_frame():
    c = GC.compact_cases()[1]; f = GC.frame_of(c, 3)
    assert f["B"] == 1 and same(f["surface"][0], c["surface"][3]) and f["cap"] == c["cap"] and f["fill"].shape == (1,)
    whole = GC.inner(GC.expected_compact(c)["order"], (c["B"], c["S"])); alone = GC.inner(GC.expected_compact(f)["order"], (1, c["S"]))
    assert same(whole[3], alone[0])


# ---- 3. the cases tell a subtly wrong kernel from a right one ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", sorted(set(GM.MUTANTS) - GM.HARMLESS))
def test_every_mutant_changes_an_output(mutant):
    for fam in GM.MUTANTS[mutant]:
        cases, expected, _ = GC.FAMILIES[fam]
        hit = None
        for c in cases():
            a, b = expected(c), expected(c, mutant)
            if any(a[k] is not None and not same(a[k], b[k]) for k in a):
                hit = c["name"]; break
        assert hit is not None, (mutant, fam, "no case of the family notices")


def test_every_family_is_hit_by_at_least_two_mutants():
    assert not GM.HARMLESS - set(GM.MUTANTS)
    for fam in GC.FAMILIES:
        assert len([m for m, fams in GM.MUTANTS.items() if fam in fams and m not in GM.HARMLESS]) >= 2, fam
    with pytest.raises(KeyError):
        GM.scatter_heads(*[None] * 5, mutant="df_le")                    # a mutant of another family is refused, not silently ignored
