"""Named, seeded inputs of the generator-round tests (tests/test_host_gen_model.py, tests/test_gpu_gen_kernels.py), built on the CPU, and the runners that
put them through vt_gen_round_compact / vt_gen_scatter_heads / vt_gen_resample (vistracker_amd/csrc/gen.hip).

Every output array lies inside a larger allocation: GUARD elements of a guard sentinel before and after it.  Arrays a kernel only partly writes start filled
with a second sentinel.  Both sentinels are finite, non-zero and equal to no input value (asserted in tests/test_host_gen_model.py), so "unchanged" is checked
element by element: the tests compare the WHOLE allocations, guard bands included, bit for bit with ``expected_*`` (tests/gen_model.py on the same arrays).

The sizes are the edges of the kernels: one partial wave, a wave seam (64), one 256-sample pass, a pass seam, three passes; kmax * C below and above one
256-thread block; M around one block.  The fill levels are the edges of the capacity: empty, exact fit, one row cut off, one row left, full.
"""
import functools

import numpy as np

import gen_model as GM

F32 = np.float32
GUARD = 64
GUARD_F, PRE_F = F32(-7.5), F32(1234.5)          # float guard band / prefill
GUARD_I, PRE_I = -7777, -5555                    # the same for the int32 and int64 arrays
FILTER_VAL, ZMIN = float(F32(0.03)), 1.0
NEAR_SCALE = float(F32(1.0 / 3.0))               # 1/3: the rounded product plus the point differs from a fused multiply-add for many perturbations
CAPS = [1, 70, 300]
RUNGS = ["empty", "exact_fit", "one_cut", "one_left", "full"]


def guarded(a, guard):
    full = np.full(a.size + 2 * GUARD, guard, a.dtype)
    full[GUARD:GUARD + a.size] = a.ravel()
    return full


def inner(full, shape):
    return full[GUARD:GUARD + int(np.prod(shape))].reshape(shape)


def bits(a):
    return a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.itemsize])


def guard_of(dtype):
    return GUARD_F if dtype == F32 else 0xA5 if dtype in (np.uint8, np.bool_) else GUARD_I


def _fill_rung(rung, cap, cnt):
    """the fill level of a frame that keeps cnt points: never negative, never above the capacity"""
    return {"empty": 0, "exact_fit": max(cap - cnt, 0), "one_cut": min(max(cap - cnt + 1, 0), cap), "one_left": cap - 1, "full": cap}[rung]


# ---- compaction ---------------------------------------------------------------------------------------------------------------------------------------------
COMPACT_S = [1, 63, 64, 65, 255, 256, 257, 513, 1000]
# write = 1 with kept_pre; the round-0 call: write = 0, kept_pre = NULL, pre = NULL; write = 1 with kept_pre = NULL
COMPACT_FORMS = {"write_pre": dict(write=1, has_pre=True, has_kept_pre=True), "round0": dict(write=0, has_pre=False, has_kept_pre=False),
                 "write_nopre": dict(write=1, has_pre=True, has_kept_pre=False)}
# the frames of the four batches of every (S, form): B = 5, 5, 3, 1
COMPACT_BATCHES = [["none", "all", "first", "last", "two"], ["every_second", "wave_last", "random30", "inactive", "edges"], ["edges", "inactive", "all"], ["edges"]]
EDGES = ["df_eq", "df_below", "z_eq", "z_above", "df_nan", "z_nan", "df_ninf", "z_pinf"]
EDGE_KEPT = dict(df_eq=False, df_below=True, z_eq=False, z_above=True, df_nan=False, z_nan=False, df_ninf=True, z_pinf=True)


def _keep_pattern(rng, S, kind):
    i = np.arange(S)
    if kind == "none": return np.zeros(S, bool)
    if kind in ("all", "inactive"): return np.ones(S, bool)
    if kind == "first": return i == 0
    if kind == "last": return i == S - 1
    if kind == "two": return ((i == 63) | (i == 64)) if S > 64 else ((i == 0) | (i == S - 1))      # (S = 1 has no two samples: one kept)
    if kind == "every_second": return i % 2 == 0
    if kind == "wave_last": return i % 64 == 63
    if kind in ("random30", "edges"): return rng.random(S) < 0.3
    raise KeyError(kind)


def _compact_frame(rng, S, kind, rot):
    """-> surface (S,3), df (S), keep (S) bool (what an active frame must keep), edges {name: sample index}"""
    keep = _keep_pattern(rng, S, kind)
    why = rng.integers(0, 3, S)                                             # a dropped sample fails the distance test, the depth test, or both
    df = np.where(keep | (why == 1), rng.uniform(0.001, 0.02, S), rng.uniform(0.04, 1.0, S)).astype(F32)
    z = np.where(keep | (why == 0), rng.uniform(1.5, 3.0, S), rng.uniform(0.2, 0.9, S)).astype(F32)
    edges = {}
    if kind == "edges":
        fv, zm = F32(FILTER_VAL), F32(ZMIN)
        value = dict(df_eq=("df", fv), df_below=("df", np.nextafter(fv, F32(-np.inf))), z_eq=("z", zm), z_above=("z", np.nextafter(zm, F32(np.inf))),
                     df_nan=("df", F32(np.nan)), z_nan=("z", F32(np.nan)), df_ninf=("df", F32(-np.inf)), z_pinf=("z", F32(np.inf)))
        where = rng.permutation(S)[:len(EDGES)]
        for t, i in enumerate(where):                                       # (S < 8: as many edges as fit, another selection in every case)
            name = EDGES[(rot + t) % len(EDGES)]; arr, v = value[name]
            df[i], z[i] = F32(0.01), F32(2.0)                               # the other test passes clearly: the edge value alone decides
            if arr == "df": df[i] = v
            else: z[i] = v
            keep[i] = EDGE_KEPT[name]; edges[name] = int(i)
    surface = np.stack([rng.normal(0, 1, S).astype(F32), rng.normal(0, 1, S).astype(F32), z], 1)
    return surface, df, keep, edges


@functools.lru_cache(maxsize=None)
def compact_cases():
    """-> list of dicts: name, form, B, S, cap, write, surface, df, pre (or None), active, fill, keep (B,S) bool, kinds, rungs, edges [(frame, name, index)],
    and the output arrays before the call: buf_points, order, kept_pre (or None), cnt, fill_out (inner arrays, sentinel-filled)"""
    out = []; n_edge_frames = 0
    for si, S in enumerate(COMPACT_S):
        for fi, (form, f) in enumerate(COMPACT_FORMS.items()):
            for bi, kinds in enumerate(COMPACT_BATCHES):
                n = len(out); rng = np.random.default_rng(7000 + n)
                B, cap = len(kinds), CAPS[(si + fi + bi) % 3]
                fr = []
                for kind in kinds:                                          # the n-th frame with edges starts its selection at edge n
                    fr.append(_compact_frame(rng, S, kind, n_edge_frames)); n_edge_frames += kind == "edges"
                keep = np.stack([x[2] for x in fr])
                active = np.array([kind != "inactive" for kind in kinds], np.uint8)
                rungs = [RUNGS[(n + j) % 5] for j in range(B)]
                fill = np.array([_fill_rung(r, cap, int(keep[j].sum()) * int(active[j])) for j, r in enumerate(rungs)], np.int64)
                out.append(dict(name=f"compact-S{S}-{form}-b{bi}-cap{cap}", form=form, B=B, S=S, cap=cap, write=f["write"],
                                surface=np.stack([x[0] for x in fr]), df=np.stack([x[1] for x in fr]),
                                pre=rng.normal(0, 1, (B, S, 3)).astype(F32) if f["has_pre"] else None, active=active, fill=fill, keep=keep, kinds=kinds, rungs=rungs,
                                edges=[(j, name, i) for j, x in enumerate(fr) for name, i in x[3].items()],
                                buf_points=np.full((B, cap + 1, 3), PRE_F, F32), order=np.full((B, S), PRE_I, np.int32),
                                kept_pre=np.full((B, S, 3), PRE_F, F32) if f["has_kept_pre"] else None,
                                cnt=np.full(B, PRE_I, np.int64), fill_out=np.full(B, PRE_I, np.int64)))
    return out


def frame_of(case, b):
    """frame b of a compaction, scatter or resample case as a case of its own with B = 1"""
    return {k: (v[b:b + 1] if isinstance(v, np.ndarray) and v.shape[:1] == (case["B"],) else v) for k, v in case.items()} | dict(B=1, name=f"{case['name']}-frame{b}")


def _full(case, names, arrays):
    return {k: (None if a is None else guarded(a, guard_of(a.dtype))) for k, a in zip(names, arrays)}


COMPACT_OUT = ("buf_points", "order", "kept_pre", "cnt", "fill_out")


def expected_compact(case, mutant=None):
    """-> the whole allocations (guard bands included) after the call, by the model"""
    c = case
    res = GM.round_compact(c["surface"], c["df"], c["pre"], c["active"], FILTER_VAL, ZMIN, c["fill"], c["cap"], c["write"], c["buf_points"], c["order"], c["kept_pre"],
                           mutant=mutant)
    return _full(c, COMPACT_OUT, res)


# ---- scatter ------------------------------------------------------------------------------------------------------------------------------------------------
SCATTER_C = [1, 3, 9, 14]
SCATTER_KMAX = [64, 128, 192, 65]                # 65: what min(S, ...) gives for S = 65
SCATTER_CNT = ["zero", "one", "kmax_less_one", "kmax", "random"]


@functools.lru_cache(maxsize=None)
def scatter_cases():
    """-> list of dicts: name, B = 5, C, kmax, cap, pred (B,C,kmax), fill_old, cnt (B) int64, cnt_kinds, rungs, buf (B,cap+1,C) before the call"""
    out = []
    for C in SCATTER_C:
        for kmax in SCATTER_KMAX:
            for cap in CAPS:
                n = len(out); rng = np.random.default_rng(8000 + n); B = 5
                kinds = [SCATTER_CNT[(j + n) % 5] for j in range(B)]
                cnt = np.array([dict(zero=0, one=1, kmax_less_one=kmax - 1, kmax=kmax, random=int(rng.integers(2, kmax - 1)))[k] for k in kinds], np.int64)
                rungs = [RUNGS[(2 * j + n) % 5] for j in range(B)]
                fill_old = np.array([_fill_rung(r, cap, int(c)) for r, c in zip(rungs, cnt)], np.int64)
                out.append(dict(name=f"scatter-C{C}-kmax{kmax}-cap{cap}", B=B, C=C, kmax=kmax, cap=cap, pred=rng.normal(0, 1, (B, C, kmax)).astype(F32), fill_old=fill_old,
                                cnt=cnt, cnt_kinds=kinds, rungs=rungs, buf=np.full((B, cap + 1, C), PRE_F, F32)))
    return out


def expected_scatter(case, mutant=None):
    c = case
    return _full(c, ("buf",), (GM.scatter_heads(c["pred"], c["fill_old"], c["cnt"], c["cap"], c["buf"], mutant=mutant),))


# ---- resample -----------------------------------------------------------------------------------------------------------------------------------------------
RESAMPLE_M = [1, 255, 256, 257]
RESAMPLE_S0 = [1, 7, 3000]
RESAMPLE_S = [1, 65, 1000]
RESAMPLE_CNT = ["zero", "one", "two", "three", "all"]
U_KINDS = ["zero", "below_one", "one", "j_over_c", "below_j_over_c"]


def _special_u(c):
    """(kind, value) list for a frame that draws among c entries (c = cnt where cnt > 1, else S0)"""
    one = F32(1.0)
    # 1.0 itself: torch.rand draws from [0, 1) and never returns it; the clamp of the contract is a guard only, pinned here all the same
    sp = [("zero", F32(0.0)), ("below_one", np.nextafter(one, F32(0.0))), ("one", one)]
    for j in sorted({1, c // 2, c - 1} - {0}):
        if 0 < j < c:
            q = F32(j) / F32(c)                                              # j / c as float32 rounds it: u * c lands on j or just below it
            sp += [("j_over_c", q), ("below_j_over_c", np.nextafter(q, F32(0.0)))]
    return sp


@functools.lru_cache(maxsize=None)
def resample_cases():
    """-> list of dicts: name, B = 5, S, S0, M, samples (B,S,3), order (B,S) int32 (a random permutation: its first cnt entries are the kept list), cnt (B) int64,
    cnt_kinds, init (B,S0,3), u (B,M), u_kinds (set of the special values planted), pert (B,M,3), out (B,M,3) before the call"""
    out = []
    for M in RESAMPLE_M:
        for S0 in RESAMPLE_S0:
            for S in RESAMPLE_S:
                n = len(out); rng = np.random.default_rng(9000 + n); B = 5
                kinds = [RESAMPLE_CNT[(j + n) % 5] for j in range(B)]
                cnt = np.array([min(dict(zero=0, one=1, two=2, three=3, all=S)[k], S) for k in kinds], np.int64)
                u = rng.random((B, M)).astype(F32); u = np.minimum(u, np.nextafter(F32(1.0), F32(0.0))); planted = set()
                for b in range(B):
                    sp = _special_u(int(cnt[b]) if cnt[b] > 1 else S0)
                    if M < len(sp):
                        sp = [sp[(n + b + t) % len(sp)] for t in range(M)]
                    for (kind, v), m in zip(sp, rng.permutation(M)):
                        u[b, m] = v; planted.add(kind)
                out.append(dict(name=f"resample-M{M}-S0_{S0}-S{S}", B=B, S=S, S0=S0, M=M, samples=rng.normal(0, 1, (B, S, 3)).astype(F32),
                                order=np.stack([rng.permutation(S) for _ in range(B)]).astype(np.int32), cnt=cnt, cnt_kinds=kinds,
                                init=rng.normal(0, 1, (B, S0, 3)).astype(F32), u=u, u_kinds=planted, pert=rng.normal(0, 1, (B, M, 3)).astype(F32),
                                out=np.full((B, M, 3), PRE_F, F32)))
    return out


def expected_resample(case, mutant=None):
    c = case
    return _full(c, ("out",), (GM.resample(c["samples"], c["order"], c["cnt"], c["init"], c["u"], c["pert"], NEAR_SCALE, mutant=mutant),))


# ---- running the kernels (GPU) --------------------------------------------------------------------------------------------------------------------------------
class _Dev:
    """an array inside a guarded device allocation; ``ptr`` is the address of the array itself"""
    def __init__(self, torch, a):
        self.t = torch.from_numpy(guarded(a, guard_of(a.dtype))).cuda()
        self.ptr = self.t.data_ptr() + GUARD * a.itemsize

    def full(self):
        return self.t.cpu().numpy()


def _run(fn, names, args, case, inputs, outputs, override, expect_error):
    """upload, call, download.  ``override`` replaces arguments by name (None: a NULL pointer).  -> {output name: whole allocation or None}"""
    import torch
    from vistracker_amd import _lib as L
    dev = {k: (None if case[k] is None else _Dev(torch, np.ascontiguousarray(case[k]))) for k in inputs + outputs}
    a = dict(args)
    a.update({k: (None if d is None else d.ptr) for k, d in dev.items()})
    a.update(override or {})
    rc = getattr(L.lib(), fn)(*[a[k] for k in names], L.stream_ptr())
    torch.cuda.synchronize()
    if expect_error:
        assert rc != 0, (fn, override, "was accepted")
        try:
            L.check(rc)
        except L.VtError:
            pass
        else:
            raise AssertionError("L.check did not raise")
    else:
        L.check(rc)
    for k in inputs:
        assert dev[k] is None or np.array_equal(bits(dev[k].full()), bits(guarded(np.ascontiguousarray(case[k]), guard_of(case[k].dtype)))), (case["name"], k, "input changed")
    return {k: (None if dev[k] is None else dev[k].full()) for k in outputs}


def run_compact(case, override=None, expect_error=False):
    c = case
    names = ("surface", "df", "pre", "active", "B", "S", "filter_val", "zmin", "fill", "cap", "write", "buf_points", "order", "kept_pre", "cnt", "fill_out")
    return _run("vt_gen_round_compact", names, dict(B=c["B"], S=c["S"], filter_val=FILTER_VAL, zmin=ZMIN, cap=c["cap"], write=c["write"]), c,
                ("surface", "df", "pre", "active", "fill"), COMPACT_OUT, override, expect_error)


def run_scatter(case, override=None, expect_error=False):
    c = case
    return _run("vt_gen_scatter_heads", ("pred", "B", "C", "kmax", "fill_old", "cnt", "cap", "buf"), dict(B=c["B"], C=c["C"], kmax=c["kmax"], cap=c["cap"]), c,
                ("pred", "fill_old", "cnt"), ("buf",), override, expect_error)


def run_resample(case, override=None, expect_error=False):
    c = case
    names = ("samples", "order", "cnt", "init", "B", "S", "S0", "u", "pert", "M", "near_scale", "out")
    return _run("vt_gen_resample", names, dict(B=c["B"], S=c["S"], S0=c["S0"], M=c["M"], near_scale=NEAR_SCALE), c,
                ("samples", "order", "cnt", "init", "u", "pert"), ("out",), override, expect_error)


FAMILIES = {"compact": (compact_cases, expected_compact, run_compact), "scatter": (scatter_cases, expected_scatter, run_scatter),
            "resample": (resample_cases, expected_resample, run_resample)}
