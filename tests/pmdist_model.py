"""Brute-force model of the point-to-mesh labels (vt_point_mesh_distance, vt_nearest_vertex): the yardstick of tests/test_gpu_boundary.py.

numpy only, float64 by default, no code shared with the product.  ``dtype=np.float32`` runs the SAME formulas in single precision: the difference between
the two runs on a given input is the error the number format itself causes (e32 in the tests), which bounds what may be asked of an fp32 kernel.

Closest point of a triangle (a, b, c) to p by Voronoi region (Ericson, Real-Time Collision Detection, 5.1.5): the three vertex regions, the three edge
regions, the interior.  A triangle without area (|ab x ac|^2 <= 1e-12 |ab|^2 |ac|^2) is its longest edge -- a segment or a point.
"""
import numpy as np


def _dot(u, v):
    return (u * v).sum(-1)


def _safe_div(num, den):
    ok = den > 0
    return np.where(ok, num / np.where(ok, den, 1), 0)


def closest_on_segment(p, s0, s1):
    """closest point of the segments s0 -> s1 (T,3) to the points p (P,3): (P,T,3)"""
    e = s1 - s0
    t = np.clip(_safe_div(_dot(p[:, None] - s0[None], e[None]), _dot(e, e)[None]), 0, 1)
    return s0[None] + t[..., None] * e[None]


def closest_on_triangles(p, a, b, c):
    """p (P,3), a, b, c (T,3) in one dtype -> the closest point of every triangle to every point (P,T,3), and the region code (P,T):
    0 a, 1 b, 2 c, 3 edge ab, 4 edge ac, 5 edge bc, 6 interior, 7 a triangle without area (answered as its longest edge)"""
    dt = p.dtype
    ab, ac = b - a, c - a
    ap, bp, cp = p[:, None] - a[None], p[:, None] - b[None], p[:, None] - c[None]
    d1, d2 = _dot(ab[None], ap), _dot(ac[None], ap)
    d3, d4 = _dot(ab[None], bp), _dot(ac[None], bp)
    d5, d6 = _dot(ab[None], cp), _dot(ac[None], cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    r_a = (d1 <= 0) & (d2 <= 0)
    r_b = (d3 >= 0) & (d4 <= d3)
    r_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    r_c = (d6 >= 0) & (d5 <= d6)
    r_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    r_bc = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
    region = np.select([r_a, r_b, r_ab, r_c, r_ac, r_bc], [0, 1, 3, 2, 4, 5], 6)
    den = va + vb + vc
    zero, one = np.zeros((), dt), np.ones((), dt)
    w_bc = _safe_div(d4 - d3, (d4 - d3) + (d5 - d6))
    v = np.select([region == 0, region == 1, region == 3, region == 2, region == 4, region == 5],
                  [zero, one, _safe_div(d1, d1 - d3), zero, zero, 1 - w_bc], np.clip(_safe_div(vb, den), 0, 1))
    w = np.select([region == 0, region == 1, region == 3, region == 2, region == 4, region == 5],
                  [zero, zero, zero, one, _safe_div(d2, d2 - d6), w_bc], np.clip(_safe_div(vc, den), 0, 1))
    q = a[None] + v[..., None] * ab[None] + w[..., None] * ac[None]
    # triangles without area: the longest edge
    n = np.cross(ab, ac)
    flat = _dot(n, n) <= dt.type(1e-12) * (_dot(ab, ab) * _dot(ac, ac))
    if flat.any():
        i = np.nonzero(flat)[0]
        corners = np.stack([a[i], b[i], c[i]], 1)                                   # (F,3,3)
        pairs = np.array([[0, 1], [0, 2], [1, 2]])
        ln = ((corners[:, pairs[:, 1]] - corners[:, pairs[:, 0]]) ** 2).sum(-1)     # (F,3)
        k = ln.argmax(1)
        s0 = corners[np.arange(len(i)), pairs[k, 0]]; s1 = corners[np.arange(len(i)), pairs[k, 1]]
        q[:, i] = closest_on_segment(p, s0, s1)
        region[:, i] = 7
    return q.astype(dt), region


def point_mesh(points, verts, faces, dtype=np.float64, chunk=64, second=False, workers=8):
    """points (N,3), verts (NV,3), faces (NF,3) -> dict: dist (N,), closest (N,3), face (N,) of the minimum over all triangles.  With ``second``: also
    dist2 (N,), the smallest distance among the faces that share no vertex with the best one (inf when there is none).  Chunked over the points so that
    512 points x 13776 faces stay within ~1 GB of temporaries; the chunks are independent and run on ``workers`` threads (numpy releases the GIL)."""
    from concurrent.futures import ThreadPoolExecutor
    dt = np.dtype(dtype)
    p_all = np.asarray(points).astype(dt); v = np.asarray(verts).astype(dt); f = np.asarray(faces).astype(np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    N = len(p_all)
    out = {"dist": np.empty(N, dt), "closest": np.empty((N, 3), dt), "face": np.empty(N, np.int64)}
    if second:
        out["dist2"] = np.empty(N, dt)

    def one(s):
        p = p_all[s:s + chunk]
        q, _ = closest_on_triangles(p, a, b, c)
        d = np.sqrt(((p[:, None] - q) ** 2).sum(-1))                                # (P,T)
        j = d.argmin(1); r = np.arange(len(p))
        out["dist"][s:s + chunk] = d[r, j]; out["closest"][s:s + chunk] = q[r, j]; out["face"][s:s + chunk] = j
        if second:
            fb = f[j]                                                               # (P,3) corners of the best face
            share = (f[None, :, :, None] == fb[:, None, None, :]).any((-1, -2))     # (P,T)
            out["dist2"][s:s + chunk] = np.where(share, np.inf, d).min(1)

    with ThreadPoolExecutor(max(1, int(workers))) as ex:
        list(ex.map(one, range(0, N, chunk)))
    return out


def nearest_vertex(points, verts, dtype=np.float64, chunk=256, second_labels=None):
    """points (N,3), verts (NV,3) -> (index (N,), distance (N,)) of the nearest vertex, ties to the smaller index.  With ``second_labels`` (NV,) also the
    distance (N,) to the nearest vertex whose label differs from the nearest one's (inf when there is none)."""
    dt = np.dtype(dtype)
    p_all = np.asarray(points).astype(dt); v = np.asarray(verts).astype(dt)
    idx = np.empty(len(p_all), np.int64); dist = np.empty(len(p_all), dt); other = np.empty(len(p_all), dt)
    for s in range(0, len(p_all), chunk):
        p = p_all[s:s + chunk]
        d = np.sqrt(((p[:, None] - v[None]) ** 2).sum(-1))
        j = d.argmin(1)
        idx[s:s + chunk] = j; dist[s:s + chunk] = d[np.arange(len(p)), j]
        if second_labels is not None:
            lab = np.asarray(second_labels)
            other[s:s + chunk] = np.where(lab[None, :] != lab[j][:, None], d, np.inf).min(1)
    return (idx, dist, other) if second_labels is not None else (idx, dist)
