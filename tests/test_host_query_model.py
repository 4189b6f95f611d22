"""The float64 model of the SIF-Net point query (tests/query_model.py) and the gates of tests/test_gpu_query_perpoint.py, checked on the CPU: the model against the
float64 oracle and the reference's recorded values, the float32 oracle against every gate (correct float32 arithmetic passes; this is where E32 comes from), the
split-operand emulation (where E_SPLIT and KINK_RELU come from), the cap on kink exclusions, and mutants of the model that the per-point gates must catch."""
import numpy as np
import pytest

import query_cases as QC
import query_model as Q
from conftest import golden


@pytest.fixture(scope="module")
def cases():
    return {c.name: c for c in QC.all_cases()}


HOST_OPTS = [dict(order="identity", proj=False, step=True), dict(order="random", proj=False), dict(order="reversed", proj=False)]


def _opts(c):
    return HOST_OPTS if c.family in ("fused", "gain") else None


def test_model_agrees_with_the_float64_oracle(cases):
    """values and query_bwd of oracle.oracle64.SifNet on a random case: float64 round-off (1e-6 of ONE float32 unit of the own scale)"""
    from oracle import oracle64 as O64
    recs, _, exact = QC.evaluate(cases["tiles-N150"], QC.OracleBackend(O64))
    assert all(ok for _, ok in exact)
    for r in recs:
        assert r.units.max() < 1e-6, (r.op, r.units.max())


def test_model_agrees_with_the_reference_values():
    """tests/golden/query.npz (the reference's own float32 run): within the float32 gate of the random family"""
    from vistracker_amd import synthetic as syn
    g = golden("query")
    M = Q.QueryModel(syn.sifnet_decoders(3), syn.feature_maps(4, 4, res_scale=float(g["res_scale"])))
    fw = M.forward(g["pts"], g["crop_center"], g["body_center"])
    for h, name in enumerate(Q.HEADS):
        assert Q.units(g[name], fw[name], fw["S_" + name]).max() <= QC.gate("tiles", "value", "fp32"), name
        fh = M.forward(g["pts"], g["crop_center"], g["body_center"], heads=(h,)); ok = ~Q.excluded(fh["margins"])
        d, S = M.backward(fh, {h: g["g_" + name]})
        assert ok.mean() >= 1 - QC.MAX_EXCLUDED
        assert Q.units(g["dpts_" + name], d, S)[ok].max() <= QC.gate("tiles", "dpts", "fp32"), name


def test_kink_exclusions_stay_under_the_cap(cases):
    """a condition on the seeds, not a tolerance: at most 2 % of a case's points within float32 reach of a kink, none of the placed ones"""
    for c in cases.values():
        frac, placed = QC.excluded_fraction(c)
        assert frac <= QC.MAX_EXCLUDED and not placed, (c.name, frac, placed)


def test_every_clamp_class_is_populated(cases):
    """below, past and far beyond (outside the image) both clamps: a change of seed may not empty a class unnoticed"""
    for name in ("fused", "gain"):
        n = QC.clamp_classes(cases[name])
        assert min(n["human_below"], n["human_past"], n["object_below"], n["object_past"]) >= 20 and n["outside"] >= 3, (name, n)


def test_gain_case_needs_range_level_1(cases):
    """|activation| of the last hidden layer beyond 1023 (level 0 of vt_maps::act_level) and below 16 368 (level 1)"""
    c = cases["gain"]; fw = c.model().forward(c.pts, c.cc, c.bc, heads=(0, 2))
    top = max(float(np.maximum(fw["mlp"][h]["pre"][l], 0).max()) for h in (0, 2) for l in range(3))
    last = max(float(np.maximum(fw["mlp"][h]["pre"][2], 0).max()) for h in (0, 2))
    assert last > 1023 and top < 16368, (last, top)
    c = cases["fused"]; fw = c.model().forward(c.pts, c.cc, c.bc, heads=(0, 2))
    assert max(float(np.maximum(fw["mlp"][h]["pre"][l], 0).max()) for h in (0, 2) for l in range(3)) < 1023 / 4


def test_oracle32_meets_every_gate(cases, capsys):
    """correct float32 arithmetic passes: every output of every point of every case, the terms and the bit-exact facts.  Prints the measured e32 table."""
    from oracle import oracle as O32
    be = QC.OracleBackend(O32); worst = {}
    for c in cases.values():
        recs, terms, exact = QC.evaluate(c, be, route="fp32", fused_opts=_opts(c))
        assert all(ok for _, ok in exact), (c.name, [w for w, ok in exact if not ok])
        for name, err, g in terms:
            assert err <= g, (c.name, name, err, g)
        for r in recs:
            k = (c.family, r.kind); worst[k] = max(worst.get(k, 0.0), r.worst())
    with capsys.disabled():
        print("\ne32, worst |oracle32 - model| / (u S):")
        for (fam, kind), v in sorted(worst.items()):
            print("  %-8s %-6s measured %.4g   recorded E32 %.4g (x %.2f)   GPU gate %.4g" % (fam, kind, v, QC.E32[fam][kind], QC.E32[fam][kind] / max(v, 1e-300), Q.GATE * QC.E32[fam][kind]))
    for (fam, kind), v in worst.items():
        assert v <= QC.E32[fam][kind], (fam, kind, v, QC.E32[fam][kind])     # the recorded figure is this measurement rounded up by 20 %; the slack is printed, not asserted


def _emulate(c, h, g, split):
    """the decoders of head h in the emulated number format, the rest of the chain in float64 -> value units, dpts units, per-layer pre-activation units"""
    M = c.model(); fw = M.forward(c.pts, c.cc, c.bc, heads=(h,)); m = fw["mlp"][h]; B, N = c.B, c.N; k = Q.HEAD_DIMS[h]
    go = np.asarray(g, np.float64).transpose(0, 2, 1).copy()
    if h == 0:
        go[~fw["in_img"]] = 0
    if h == 4:
        sg = Q.sigmoid(m["out"]); go = go * sg * (1 - sg)
    out, pre, dfeat = Q.emu_decoder(M.W[h], M.b[h], fw["ft"]["feat"].reshape(-1, 611).astype(np.float32), go.reshape(-1, k).astype(np.float32), split)
    d = M.to_points(fw, dfeat.reshape(B, N, 611).astype(np.float64), np.zeros((B, N, 611)))[0]
    ref, S = M.backward(fw, {h: g}); ok = ~Q.excluded(QC.exact_coords(c, fw["margins"]))
    uv = Q.units(out.reshape(B, N, k), m["out"], m["S"][3]).max()
    ul = [float(Q.units(pre[l].reshape(B, N, 128), m["pre"][l], m["S"][l]).max()) for l in range(3)]
    return float(uv), float(Q.units(d, ref, S)[ok].max()), ul


def test_split_emulation(cases, capsys):
    """the split-f16 format's term: the decoders with every GEMM operand carried to 22 bits (emu_decoder), against the model.  Where E_SPLIT comes from; the derived
    worst case (1 + 3 2^-22)^4 - 1 = 48 u of the own scale is the per-element backstop above it.  Also: what float32 / split arithmetic moves a hidden
    pre-activation by, per layer -- the basis of KINK_RELU."""
    ev, ed, el = {}, {}, {False: [0, 0, 0], True: [0, 0, 0]}
    for c in (cases["tiles-N150"], cases["goexp"], cases["gain"]):
        for h in range(5):
            g = c.g[h] if hasattr(c, "g") else np.random.default_rng(h).normal(0, 1, (c.B, Q.HEAD_DIMS[h], c.N)).astype(np.float32)
            for split in (False, True):
                v, d, l = _emulate(c, h, g, split)
                ev[split] = max(ev.get(split, 0), v); ed[split] = max(ed.get(split, 0), d); el[split] = [max(a, b) for a, b in zip(el[split], l)]
    with capsys.disabled():
        print("\nemulated number formats, worst |emulation - model| / (u S):   value   dpts   pre-activation of layers 1, 2, 3")
        for split in (False, True):
            print("  %-8s %.4g  %.4g  %s" % ("split22" if split else "float32", ev[split], ed[split], " ".join("%.4g" % x for x in el[split])))
    assert ev[True] <= QC.E_SPLIT[0]["value"] and ed[True] <= QC.E_SPLIT[0]["dpts"]    # numpy's float32 matmul sums in its BLAS's order: only the upper side is asserted
    # the range levels: real float16 halves at the kernel's operand scales (the lo half of an ordinary operand is a float16 subnormal at level 2)
    lvl = {}
    for level in (0, 1, 2):
        for c in (cases["tiles-N150"], cases["goexp"], cases["borders"], cases["fused"], cases["gain"]):
            if c.name == "gain" and level == 0:
                continue                                    # beyond level 0's range: the emulation overflows float16 there as the kernel does
            M = c.model(); fw = M.forward(c.pts, c.cc, c.bc); feat = fw["ft"]["feat"].reshape(-1, 611).astype(np.float32)
            for h in range(5):
                out = Q.emu_decoder(M.W[h], M.b[h], feat, None, True, Q.operand_scales(c.decoders(), Q.HEADS[h], level))[0]
                lvl[level] = max(lvl.get(level, 0.0), float(Q.units(out.reshape(c.B, c.N, -1), fw["mlp"][h]["out"], fw["mlp"][h]["S"][3]).max()))
    with capsys.disabled():
        print("  float16 halves at the operand scales of range level 0 / 1 / 2, value: " + " / ".join("%.4g (recorded %.4g)" % (lvl[k], QC.E_SPLIT[k]["value"]) for k in (0, 1, 2)))
    for k in (0, 1, 2):
        assert lvl[k] <= QC.E_SPLIT[k]["value"] and QC.E_SPLIT[k]["dpts"] == QC.E_SPLIT[0]["dpts"]
        assert abs(QC.E_SPLIT[k]["point"] - QC.E_SPLIT[k]["value"] - QC.E_SPLIT[k]["dpts"]) < 1e-12
    backstop = Q.split_backstop(1.0) / Q.U
    assert all(Q.GATE * v <= backstop for v in QC.E_SPLIT[0].values()), "the measured split term may not exceed the derived worst case (22-bit operands: level 0)"
    for split in (False, True):
        assert all(Q.GATE * x <= kr for x, kr in zip(el[split], Q.KINK_RELU)), (el[split], Q.KINK_RELU)


MUTANT_CASES = dict(swap_wx="tiles-N150", chan_shift="tiles-N150", relu_other_head="tiles-N150", tile_63_64="tiles-N150", flush_small_go="goexp",
                    df_mask_leak="borders", no_sigmoid_deriv="tiles-N65", order_write="fused")
"""the clamp mask with < instead of <= is not among them: the thresholds are float32(0.1) and float32(0.8), and a distance the network computes cannot be placed
exactly on either (the issue's condition for that mutant)"""


def test_mutants_fail_the_per_point_gates(cases, capsys):
    """one deliberate defect each; the per-point gates (the wider, split-f16 ones) must catch every one.  Prints whether the whole-array `rel` gates of
    tests/test_gpu_parity.py would have."""
    rows = []
    for mut in Q.MUTANTS:
        c = cases[MUTANT_CASES[mut]]
        recs, _, exact = QC.evaluate(c, None, route="split-f16", mutant=mut, fused_opts=[dict(order="random", proj=False)] if c.family == "fused" else None)
        fails = [r for r in recs if r.worst() > QC.gate(c.family, r.kind, "split-f16")] + [w for w, ok in exact if not ok]
        olds = [r.old_rel for r in recs if r.old_rel is not None]
        old_pass = all(e < bar for e, bar in olds)
        worst = max((r.worst() / max(QC.gate(c.family, r.kind, "split-f16"), 1e-300) for r in recs), default=0.0)
        rows.append((mut, c.name, len(fails), worst, old_pass, max(e / bar for e, bar in olds)))
    with capsys.disabled():
        print("\nmutant                case         gates failed   worst / gate   whole-array rel gate passes it   (worst rel / its bar)")
        for r in rows:
            print("  %-18s %-12s %4d        %10.3g        %-5s                        %.3g" % r)
    for r in rows:
        assert r[2] > 0, r
