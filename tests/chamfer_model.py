"""A plain numpy model of the ragged contact Chamfer term (vt_chamfer_ragged, vt_chamfer_ragged_ws, vt_chamfer_ragged_idx) and of the evaluation metric's
nearest-neighbour distance (vt_nn_distance).  It shares no code with the product or with oracle/: the formulas are restated from the header.

    term = 1/P  sum_p [ 1/nx_p sum_i min_j |x_i - y_j|^2  +  1/ny_p sum_j min_i |y_j - x_i|^2 ]        over ALL P pairs, an empty pair adds nothing
    near-side term of point a_i with nearest far point b_j:   t = 2 (a_i - b_j) gscale / (na P);   the row of a_i receives +t, the row of b_j receives -t

The nearest neighbour is the winner of an ascending scan with a strict compare: the smallest index among equal distances.

Next to the values the model returns what a per-row error bound needs, per gradient row: ``n``, the number of terms added into it (its own near-side term plus
every far-side record that names it), and ``S``, the per-component sum of the absolute values of those terms.  Per near point it returns the TIE SET
{j : d(i, j) <= dmin(i) (1 + 12 u)}, u = 2^-24, on the squared distances: a float32 ``d0 d0 + d1 d1 + d2 d2`` of exact float32 inputs carries at most 5 roundings
(three differences feed three products -- 2 per summand -- and two additions follow: (1 + u)^5 at the most, with or without contraction), so a float32 scan can
prefer j to the true winner j* only if d_j <= d_j* (1 + 5u) / (1 - 5u) < d_j* (1 + 12u).  A near point whose tie set has one member has ONE admissible winner.

``dtype=np.float32`` evaluates the same formulas in float32 (the term is still summed in float64, as a check of the lattice cases, where every operation is exact).
"""
import numpy as np

U = 2.0 ** -24
TIE = 12 * U


def _sqdist(a, b):
    """(na, nb) squared distances in the dtype of a / b: d0 d0 + d1 d1 + d2 d2, summed in this order"""
    d0 = a[:, None, 0] - b[None, :, 0]; d = d0 * d0
    d1 = a[:, None, 1] - b[None, :, 1]; d += d1 * d1
    d2 = a[:, None, 2] - b[None, :, 2]; d += d2 * d2
    return d


def _tie_sets(d, dmin):
    """per near point the ascending indices j with d[i, j] <= dmin[i] (1 + 12u)"""
    m = d.astype(np.float64) <= dmin.astype(np.float64)[:, None] * (1.0 + TIE)
    return [np.flatnonzero(r) for r in m]


def _direction(a, b, k, ga, gb, na_, nb_, Sa, Sb):
    """near cloud a against far cloud b; k = gscale / (na P) as the dtype's number, 2 (a - b) gs / na spelled as one factor.  Adds into the rows in place."""
    d = _sqdist(a, b)
    nn = np.argmin(d, axis=1)                                   # numpy's argmin returns the FIRST minimum: ascending scan, strict compare
    dmin = d[np.arange(len(a)), nn]
    t = (a - b[nn]) * a.dtype.type(2) * k
    ga += t; na_ += 1; Sa += np.abs(t)
    np.subtract.at(gb, nn, t); np.add.at(nb_, nn, 1); np.add.at(Sb, nn, np.abs(t))          # unbuffered: far rows named more than once collect every record, in record order
    return nn, dmin, _tie_sets(d, dmin)


def chamfer(xs, ys, gscale=1.0, dtype=np.float64):
    """xs, ys: lists of (n, 3) arrays (n may be 0), one per pair.  -> dict:
    term (float), dx / dy (total, 3) in ``dtype``, nn_x / nn_y (lists of int arrays, -1-free; empty for a dead pair), n_x / n_y (total,) int, S_x / S_y (total, 3)
    float64, ties_x / ties_y (lists over pairs of lists over near points of index arrays), offx / offy (P + 1) int32."""
    P = len(xs); assert P == len(ys) and P > 0
    f = np.dtype(dtype).type
    offx = np.concatenate([[0], np.cumsum([len(a) for a in xs])]).astype(np.int32); offy = np.concatenate([[0], np.cumsum([len(b) for b in ys])]).astype(np.int32)
    dx = np.zeros((offx[-1], 3), dtype); dy = np.zeros((offy[-1], 3), dtype)
    n_x = np.zeros(offx[-1], np.int64); n_y = np.zeros(offy[-1], np.int64)
    S_x = np.zeros((offx[-1], 3), dtype); S_y = np.zeros((offy[-1], 3), dtype)
    term = 0.0; out = dict(nn_x=[], nn_y=[], ties_x=[], ties_y=[])
    for p in range(P):
        a = np.asarray(xs[p], dtype).reshape(-1, 3); b = np.asarray(ys[p], dtype).reshape(-1, 3)
        if len(a) == 0 or len(b) == 0:
            for k in out:
                out[k].append([] if k.startswith("ties") else np.zeros(0, np.int64))
            continue
        sx, sy = slice(offx[p], offx[p + 1]), slice(offy[p], offy[p + 1])
        nn1, m1, t1 = _direction(a, b, f(gscale) / f(len(a) * P), dx[sx], dy[sy], n_x[sx], n_y[sy], S_x[sx], S_y[sy])
        nn2, m2, t2 = _direction(b, a, f(gscale) / f(len(b) * P), dy[sy], dx[sx], n_y[sy], n_x[sx], S_y[sy], S_x[sx])
        term += float(m1.astype(np.float64).sum()) / len(a) + float(m2.astype(np.float64).sum()) / len(b)
        out["nn_x"].append(nn1); out["nn_y"].append(nn2); out["ties_x"].append(t1); out["ties_y"].append(t2)
    out.update(term=term / P, dx=dx, dy=dy, n_x=n_x, n_y=n_y, S_x=S_x.astype(np.float64), S_y=S_y.astype(np.float64), offx=offx, offy=offy)
    return out


def ambiguous(ref):
    """number of near points (both directions, all pairs) whose tie set has more than one member"""
    return sum(len(t) > 1 for k in ("ties_x", "ties_y") for pair in ref[k] for t in pair)


def nn_distance(query, search):
    """query (P, nq, 3), search (P, ns, 3) -> (P, nq) float64: the Euclidean distance from every query point to the nearest search point"""
    q = np.asarray(query, np.float64); s = np.asarray(search, np.float64)
    return np.stack([np.sqrt(_sqdist(a, b).min(1)) for a, b in zip(q, s)])


# ---- the gates of tests/test_gpu_chamfer.py (derived, see that file's docstring), shared with tools/chamfer_perpoint_report.py ---------------------------------------
def term_gate(ref):
    return 8 * U * ref["term"]


def row_gate(n, S, initial=None):
    """(n + 8) u S per row and component; with a nonzero start value of the row (n + 9) u (S + |initial|)"""
    n = np.asarray(n, np.float64)[:, None]
    return (n + 8) * U * S if initial is None else (n + 9) * U * (S + np.abs(np.asarray(initial, np.float64)))
