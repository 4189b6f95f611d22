"""The definition of the gradient record and the step guard (vt_grad_stats, vt_grad_guard_close, vt_grad_scale) in numpy float64, sums by ``math.fsum`` (the
correctly rounded sum: no order of additions enters the definition), the gates the kernels are held to, and the cases both the host and the GPU tests use.

A segment is a (begin, end) pair of offsets into the flat float32 gradient; what lies between two segments belongs to none."""
import math

import numpy as np

CHUNK = 4096                          # VT_GRAD_STATS_CHUNK: the kernel cuts a segment into chunks of this many elements, from the segment's start
EPS = 2.0 ** -53


# ---- the definition --------------------------------------------------------------------------------------------------------------------------------------------
def seg_stats(g, segs):
    """-> (sumsq float64 (n_seg,), maxabs float32 (n_seg,), nonfinite int32 (n_seg,)): over the FINITE elements of every segment the sum of squares (each float32
    squared in float64, which is exact) and the largest magnitude, and the number of NaN / Inf elements"""
    g = np.asarray(g, dtype=np.float32)
    sumsq, maxabs, nonfinite = np.zeros(len(segs)), np.zeros(len(segs), np.float32), np.zeros(len(segs), np.int32)
    for s, (b, e) in enumerate(segs):
        x = g[b:e].astype(np.float64)
        fin = np.isfinite(x)
        nonfinite[s] = int((~fin).sum())
        xf = x[fin]
        sumsq[s] = math.fsum((xf * xf).tolist())
        maxabs[s] = np.float32(np.abs(xf).max()) if xf.size else np.float32(0)
    return sumsq, maxabs, nonfinite


def coef_of(norm, max_norm):
    """torch's clip_grad_norm_ coefficient, evaluated in float64 and rounded to float32 once; 1 without clipping"""
    if max_norm is None or not max_norm > 0:
        return np.float32(1)
    return np.float32(min(1.0, float(max_norm) / (float(norm) + 1e-6)))


def close(sumsqs, nonfinites, error, max_norm):
    """the step's decision from the per-buffer results -> dict(norm, coef, skip)"""
    total = math.fsum([float(x) for a in sumsqs for x in a])
    norm = math.sqrt(total)
    skip = any(int(x) > 0 for a in nonfinites for x in a) or not math.isfinite(float(error))
    return {"norm": norm, "coef": coef_of(norm, max_norm), "skip": bool(skip)}


def scaled(g, coef, skip):
    """the gradient after vt_grad_scale: one float32 multiplication per element, nothing on a skipped step"""
    g = np.asarray(g, dtype=np.float32)
    return g.copy() if skip else (g * np.float32(coef)).astype(np.float32)


# ---- the gates -------------------------------------------------------------------------------------------------------------------------------------------------
def stats_failures(got, want, segs):
    """nonfinite and maxabs exact (maxabs as bits); sumsq within len . 2^-53 relative of the fsum value: n - 1 float64 additions of non-negative terms, each exact
    product rounded once per addition, are within (n - 1) . 2^-53 (1 + O(2^-53)) of the true sum in ANY order, so the bound is derived, not measured"""
    bad = []
    gs, gm, gn = (np.asarray(a) for a in got)
    ws, wm, wn = want
    for s, (b, e) in enumerate(segs):
        if int(gn[s]) != int(wn[s]):
            bad.append((s, "nonfinite", int(gn[s]), int(wn[s])))
        if np.float32(gm[s]).view(np.uint32) != np.float32(wm[s]).view(np.uint32):
            bad.append((s, "maxabs", float(gm[s]), float(wm[s])))
        if not abs(float(gs[s]) - float(ws[s])) <= (e - b) * EPS * float(ws[s]):
            bad.append((s, "sumsq", float(gs[s]), float(ws[s])))
    return bad


def close_failures(got, want, got_norm_coef, n_elements):
    """``got`` / ``want``: dict(norm, coef, skip); norm within n_elements . 2^-53 relative (the sums' bound; the square root halves a relative error and adds half
    an ulp, which the bound of a sum over at least two elements covers), skip exact, coef the bits of ``got_norm_coef`` = coef_of(the kernel's own norm)"""
    bad = []
    if not abs(got["norm"] - want["norm"]) <= max(n_elements, 2) * EPS * want["norm"]:
        bad.append(("norm", got["norm"], want["norm"]))
    if bool(got["skip"]) != bool(want["skip"]):
        bad.append(("skip", got["skip"], want["skip"]))
    if np.float32(got["coef"]).view(np.uint32) != np.float32(got_norm_coef).view(np.uint32):
        bad.append(("coef", float(got["coef"]), float(got_norm_coef)))
    return bad


# ---- the cases -------------------------------------------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7, 600001)
GAPS = (0, 1, 64)
NAN, PINF, NINF = np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)


def values(rng, n, huge=True):
    """float32 values over 30 binades with denormals and, with ``huge``, +-3e38 among them (next to 9e76 a sum of squares no longer shows a missing small term)"""
    x = (rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-15, 16, n)).astype(np.float32)
    if n >= 5:
        x[rng.integers(0, n)] = np.float32(1e-40)             # denormals
        x[rng.integers(0, n)] = np.float32(-1.4e-45)
    if huge and n >= 63:
        x[rng.integers(0, n)] = np.float32(3e38)
        x[rng.integers(0, n)] = np.float32(-3e38)
    return x


def case(seed=0):
    """-> (g float32 (n,), segs [(begin, end)]): the lengths of LENGTHS, then a segment of non-finite
    values only, one of zeros only, and three of length 1 that hold a NaN, a +Inf and a -Inf; packed with gaps of 0, 1 and 64 elements in turn (and 2 in front),
    every gap filled with NaN.  NaN / Inf sit at the first and last element of a segment and at both sides of a chunk edge."""
    rng = np.random.default_rng(seed)
    parts, segs, at = [np.full(2, NAN)], [], 2
    bodies = [values(rng, n, huge=n in (64, CHUNK, 3 * CHUNK + 7)) for n in LENGTHS]
    bodies[6][0], bodies[6][-1] = NAN, NINF                                    # 65: first and last element
    bodies[9][CHUNK - 1], bodies[9][CHUNK] = PINF, NAN                         # CHUNK + 1: both sides of the chunk edge
    bodies[10][2 * CHUNK - 1], bodies[10][2 * CHUNK] = NAN, NINF               # 3 CHUNK + 7: both sides of its second edge
    bodies[11][0], bodies[11][-1] = PINF, NAN                                  # 600 001: first and last
    bodies.append(np.array([NAN, PINF, NINF] * 23 + [NAN], np.float32))       # 70 values, none finite
    bodies.append(np.zeros(130, np.float32))
    bodies += [np.array([v], np.float32) for v in (NAN, PINF, NINF)]
    for k, b in enumerate(bodies):
        segs.append((at, at + b.size))
        gap = GAPS[k % 3]
        parts += [b, np.full(gap, NAN)]
        at += b.size + gap
    parts.append(np.full(3, NAN))
    return np.concatenate(parts).astype(np.float32), segs


def record_arrays(rec, prefix=""):
    """``ops.StepGuard.read()`` as flat arrays (for npz files and bitwise comparison); the ring's entries under ``ring<i>.``"""
    out = {prefix + "head": np.array([rec.get("steps", 0), rec.get("skipped", 0), rec["step"], int(rec["skip"])], np.int64),
           prefix + "f64": np.array([rec["norm"], rec["error"], rec["coef"]] + list(rec["sumsq"].values()) + list(rec["maxabs"].values()), np.float64),
           prefix + "nonfinite": np.array(list(rec["nonfinite"].values()), np.int64)}
    for i, r in enumerate(rec.get("ring", [])):
        out.update(record_arrays(r, f"{prefix}ring{i}."))
    return out


def same_records(a, b):
    """two ``record_arrays`` results hold the same keys and the same bits"""
    return sorted(a) == sorted(b) and all(np.array_equal(np.asarray(a[k]).view(np.int64), np.asarray(b[k]).view(np.int64)) for k in a)
