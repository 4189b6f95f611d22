"""Exact model of the three bookkeeping kernels of a generator round (vistracker_amd/csrc/gen.hip: vt_gen_round_compact, vt_gen_scatter_heads, vt_gen_resample),
written from the contract in include/vistracker.h and the header comment of gen.hip: plain numpy, one explicit loop over the frames, no sort of any kind.

Every operation is exact -- integer indices, copies, one float32 multiply and one float32 add (the library is built with -ffp-contract=off) -- so the tests that
use this model compare bit for bit and need no tolerance.

``mutant`` (a name of MUTANTS) exists for tests/test_host_gen_model.py only: it selects a wrong variant that the case set of tests/gen_cases.py must tell from
the model, as in tests/query_model.py.
"""
import numpy as np

F32 = np.float32

# name -> the kernel families whose model it breaks
MUTANTS = {
    "df_le": ("compact",),                       # <= for the distance test
    "z_ge": ("compact",),                        # >= for the depth test
    "active_ignored": ("compact",),
    "wave_reversed": ("compact",),               # kept order reversed within each 64-sample wave
    "pass_reversed": ("compact",),               # kept order reversed within each 256-sample pass
    "pass_base_lost": ("compact",),              # a pass's base not carried over: each pass starts at k = 0 again
    "kept_pre_tail_unwritten": ("compact",),
    "dest_le_cap": ("compact", "scatter"),       # dest <= cap admitted: the row behind the capacity is written
    "fill_out_unclamped": ("compact",),
    "fill_out_advanced_without_write": ("compact",),
    "scatter_transposed": ("scatter",),          # pred read in a (B, kmax, C) layout
    "scatter_fill_new": ("scatter",),            # rows counted from the fill level AFTER the round
    "resample_cnt_gt0": ("resample",),           # cnt > 0 as the branch condition
    "resample_no_clamp": ("resample",),
    "resample_fma": ("resample",),               # product and sum as one fused multiply-add
    "resample_no_order": ("resample",),          # samples[k] instead of samples[order[k]]
    "resample_near_scale_in_restart": ("resample",),
}
# A mutant is harmless for a kernel when the kernel can never see the branch it breaks.  None is: tests/gen_cases.py reaches every branch above
# (tests/test_host_gen_model.py::test_every_mutant_changes_an_output).
HARMLESS = frozenset()


def _check(mutant, family):
    if mutant is not None and (mutant not in MUTANTS or family not in MUTANTS[mutant]):
        raise KeyError((mutant, family))


def _grouped_reversed(idx, width):
    """idx ascending -> the same indices, reversed inside every group of ``width`` consecutive SAMPLE positions"""
    out = []
    for g in np.unique(idx // width):
        out.append(idx[idx // width == g][::-1])
    return np.concatenate(out) if out else idx


def round_compact(surface, df_target, pre, active, filter_val, zmin, fill, cap, write, buf_points, order, kept_pre, mutant=None):
    """surface (B,S,3), df_target (B,S), pre (B,S,3) or None float32; active (B) bytes; fill (B) int64; buf_points (B,cap+1,3) or None, order (B,S) int32,
    kept_pre (B,S,3) or None: the arrays' contents BEFORE the call.  -> new copies (buf_points, order, kept_pre) and cnt, fill_out (B) int64."""
    _check(mutant, "compact")
    B, S = df_target.shape
    fv, zm = F32(filter_val), F32(zmin)
    buf_points = None if buf_points is None else buf_points.copy()
    order = order.copy()
    kept_pre = None if kept_pre is None else kept_pre.copy()
    cnt = np.zeros(B, np.int64); fill_out = np.zeros(B, np.int64)
    for b in range(B):
        df = df_target[b].astype(F32); z = surface[b, :, 2].astype(F32)
        near = (df <= fv) if mutant == "df_le" else (df < fv)               # NaN compares false either way
        front = (z >= zm) if mutant == "z_ge" else (z > zm)
        mask = near & front
        if not active[b] and mutant != "active_ignored":
            mask = np.zeros(S, bool)
        kept = np.nonzero(mask)[0]; dropped = np.nonzero(~mask)[0]
        c = len(kept); f0 = int(fill[b])
        if mutant == "wave_reversed":
            kept = _grouped_reversed(kept, 64)
        if mutant == "pass_reversed":
            kept = _grouped_reversed(kept, 256)
        slot = np.arange(c)                                                 # kept sample k goes to slot k ...
        tail = c + np.arange(len(dropped))
        if mutant == "pass_base_lost":                                      # ... or to its rank inside its own 256-sample pass
            slot = np.array([np.count_nonzero(kept[:k] // 256 == kept[k] // 256) for k in range(c)], np.int64)
            tail = c + np.array([np.count_nonzero(dropped[:k] // 256 == dropped[k] // 256) for k in range(len(dropped))], np.int64)
        for k in range(c):                                                  # in sample order: a later pass overwrites an earlier one where slots collide
            i = kept[k]; s = int(slot[k])
            order[b, s] = i
            if kept_pre is not None:
                kept_pre[b, s] = pre[b, i]
            dest = f0 + s
            if write and (dest <= cap if mutant == "dest_le_cap" else dest < cap):
                buf_points[b, dest] = surface[b, i]
        if kept_pre is not None and mutant != "kept_pre_tail_unwritten":
            for k in range(len(dropped)):
                if tail[k] < S:
                    kept_pre[b, tail[k]] = pre[b, dropped[k]]
        cnt[b] = c
        f1 = f0 + c if (write or mutant == "fill_out_advanced_without_write") else f0
        fill_out[b] = f1 if mutant == "fill_out_unclamped" else min(f1, cap)
    return buf_points, order, kept_pre, cnt, fill_out


def scatter_heads(pred, fill_old, cnt, cap, buf, mutant=None):
    """pred (B,C,kmax) float32, fill_old, cnt (B) int64, buf (B,cap+1,C): its contents before the call -> a new copy of buf"""
    _check(mutant, "scatter")
    B, C, kmax = pred.shape
    buf = buf.copy()
    src = pred.reshape(B, kmax, C).transpose(0, 2, 1) if mutant == "scatter_transposed" else pred
    for b in range(B):
        f0 = int(fill_old[b])
        if mutant == "scatter_fill_new":
            f0 = min(f0 + int(cnt[b]), cap)
        for k in range(min(int(cnt[b]), kmax)):
            dest = f0 + k
            if dest <= cap if mutant == "dest_le_cap" else dest < cap:
                for c in range(C):
                    buf[b, dest, c] = src[b, c, k]
    return buf


def resample(samples, order, cnt, init, u, pert, near_scale, mutant=None):
    """samples (B,S,3), order (B,S) int32, cnt (B) int64, init (B,S0,3), u (B,M), pert (B,M,3) -> (B,M,3) float32.
    A mutant that reads behind an array (no clamp) gets NaN there."""
    _check(mutant, "resample")
    B, M = u.shape; S, S0 = samples.shape[1], init.shape[1]
    ns = F32(near_scale)
    out = np.zeros((B, M, 3), F32)

    def move(p, scale, n):
        if mutant == "resample_fma":
            return (p.astype(np.float64) + np.float64(scale) * n.astype(np.float64)).astype(F32)
        prod = (F32(scale) * n.astype(F32)).astype(F32)                     # the product is rounded to float32 ...
        return (p.astype(F32) + prod).astype(F32)                           # ... then the sum

    for b in range(B):
        c = int(cnt[b])
        for m in range(M):
            uu = F32(u[b, m]); n = pert[b, m]
            if c > (0 if mutant == "resample_cnt_gt0" else 1):
                k = int(F32(uu * F32(c)))
                if mutant != "resample_no_clamp":
                    k = min(k, c - 1)
                if k >= S:
                    out[b, m] = np.nan; continue
                out[b, m] = move(samples[b, k if mutant == "resample_no_order" else int(order[b, k])], ns, n)
            else:
                k0 = int(F32(uu * F32(S0)))
                if mutant != "resample_no_clamp":
                    k0 = min(k0, S0 - 1)
                if k0 >= S0:
                    out[b, m] = np.nan; continue
                out[b, m] = move(init[b, k0], ns if mutant == "resample_near_scale_in_restart" else F32(0.5), n)
    return out
