"""Test helper (not a test file): the silhouette term of csrc/sil.hip restated in numpy, independent of the kernels and of oracle/vt_oracle.c.

Rule (sil.hip's header; Kato et al. 2018): projection u = K x/z, v <- 1 - v, NDC = 2 (. - 1/2); faces doubled with reversed winding, back faces skipped; pixel (xi, yi) is
covered when its centre ((2 xi + 1 - is)/is, (2 yi + 1 - is)/is) is inside and near < z < far; nearest face owns, the smaller id on equal depth; image row r = yi = is-1-r.

forward():  per face over its pixel box.  Edge tests and depths in float64 from the float32 projected corners (edge='f64'), with the float32 reach of every decision
            kept, so that a pixel whose owner float32 arithmetic cannot decide is CONTESTED; edge='f32' takes the edge tests in float32, operation by operation.
backward(): the edge sweeps.  Every discrete decision (d0 range, floor / ceil of d1_cross and d0_cross2, the != guards, the sign that eps takes) in numpy float32,
            operation by operation (IEEE float32 in numpy = the un-contracted C / HIP code); every magnitude in float64.  Returns per vertex component the gradient
            after un-projection, its scale S (sum of |terms|, carried through the un-projection with absolute values) and Q, the rounding of the fixed-point
            accumulators (2^-35 per face that contributed, carried the same way)."""
import numpy as np

F = np.float32
NEAR, FAR = float(F(0.1)), float(F(100.0))
U = 2.0 ** -24
FIXQ = 2.0 ** -35
TIE = 1e-5              # relative depth difference below which float32 cannot be trusted to order two faces
REACH = 8 * U           # float32 reach of an edge function, relative to the sum of its two products' magnitudes


def project32(verts, K):
    """sil_project_kernel in float32, operation by operation -> (B, NV, 3)"""
    v = np.asarray(verts, F); K = np.asarray(K, F).reshape(-1, 9)
    z = v[..., 2]; zz = z + F(1e-9)
    x_ = v[..., 0] / zz; y_ = v[..., 1] / zz
    k = [K[:, i][:, None] for i in range(9)]
    u = k[0] * x_ + k[1] * y_ + k[2]
    w = F(1) - (k[3] * x_ + k[4] * y_ + k[5])
    return np.stack([F(2) * (u - F(0.5)), F(2) * (w - F(0.5)), z], -1).astype(F)


def doubled(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f, f[:, [0, 2, 1]]], 0)


def forward(pv, faces, size, edge="f64", tie_larger=False):
    """pv (NV,3) float32 projected vertices of ONE frame -> dict: owner (is,is) image orientation (-1 background), contested (is,is) bool,
    z1 / z2 the two nearest float64 depths (inf where none), clipped (per doubled face: pixels inside the triangle refused by near / far), inside (same: accepted)"""
    is_ = int(size); f2s = doubled(faces); n2 = len(f2s)
    best = np.full((is_, is_), np.inf); own = np.full((is_, is_), -1, np.int64); second = np.full((is_, is_), np.inf); unc = np.full((is_, is_), np.inf)
    clipped = np.zeros(n2, np.int64); accepted = np.zeros(n2, np.int64)
    rec = {}
    for f2 in range(n2):
        fc32 = pv[f2s[f2]].reshape(9).astype(F); c = fc32
        if (c[7] - c[1]) * (c[3] - c[0]) < (c[4] - c[1]) * (c[6] - c[0]):            # back side (float32: a discrete decision of the rule)
            continue
        den32 = c[0] * (c[4] - c[7]) + c[3] * (c[7] - c[1]) + c[6] * (c[1] - c[4])
        if den32 == 0:
            continue
        d = fc32.astype(np.float64)
        x0 = max(int(np.floor((d[[0, 3, 6]].min() * is_ + is_ - 1) / 2)) - 1, 0); x1 = min(int(np.ceil((d[[0, 3, 6]].max() * is_ + is_ - 1) / 2)) + 1, is_ - 1)
        y0 = max(int(np.floor((d[[1, 4, 7]].min() * is_ + is_ - 1) / 2)) - 1, 0); y1 = min(int(np.ceil((d[[1, 4, 7]].max() * is_ + is_ - 1) / 2)) + 1, is_ - 1)
        if x0 > x1 or y0 > y1:
            continue
        xi, yi = np.meshgrid(np.arange(x0, x1 + 1), np.arange(y0, y1 + 1))
        if edge == "f32":
            xp32 = (F(2) * xi.astype(F) + F(1) - F(is_)) / F(is_); yp32 = (F(2) * yi.astype(F) + F(1) - F(is_)) / F(is_)
            out = np.zeros(xi.shape, bool)
            for a, b in ((0, 3), (3, 6), (6, 0)):
                out |= (yp32 - c[a + 1]) * (c[b] - c[a]) < (xp32 - c[a]) * (c[b + 1] - c[a + 1])
            sure_in = ~out; maybe = np.zeros_like(out)
            xp = xp32.astype(np.float64); yp = yp32.astype(np.float64)
        else:
            xp = (2.0 * xi + 1 - is_) / is_; yp = (2.0 * yi + 1 - is_) / is_
            sure_in = np.ones(xi.shape, bool); sure_out = np.zeros(xi.shape, bool)
            for a, b in ((0, 3), (3, 6), (6, 0)):
                t1 = (yp - d[a + 1]) * (d[b] - d[a]); t2 = (xp - d[a]) * (d[b + 1] - d[a + 1])
                r = REACH * (np.abs(t1) + np.abs(t2)) + 2 * U * (np.abs(d[b] - d[a]) + np.abs(d[b + 1] - d[a + 1]))        # (the float32 centre itself is u off)
                sure_in &= t1 - t2 >= r; sure_out |= t1 - t2 < -r
            maybe = ~sure_in & ~sure_out
        cand = sure_in | maybe
        if not cand.any():
            continue
        den = d[0] * (d[4] - d[7]) + d[3] * (d[7] - d[1]) + d[6] * (d[1] - d[4])
        w0 = ((d[4] - d[7]) * xp + (d[6] - d[3]) * yp + (d[3] * d[7] - d[6] * d[4])) / den
        w1 = ((d[7] - d[1]) * xp + (d[0] - d[6]) * yp + (d[6] * d[1] - d[0] * d[7])) / den
        w2 = ((d[1] - d[4]) * xp + (d[3] - d[0]) * yp + (d[0] * d[4] - d[3] * d[1])) / den
        w0, w1, w2 = (np.clip(w, 0.0, 1.0) for w in (w0, w1, w2))
        ws = w0 + w1 + w2
        with np.errstate(divide="ignore", invalid="ignore"):
            zp = 1.0 / (w0 / ws / d[2] + w1 / ws / d[5] + w2 / ws / d[8])
        zp = np.where(np.isfinite(zp), zp, np.inf)
        in_rng = (zp > NEAR * (1 + TIE)) & (zp < FAR * (1 - TIE)); off_rng = (zp <= NEAR * (1 - TIE)) | (zp >= FAR * (1 + TIE))
        plane = ~in_rng & ~off_rng
        clipped[f2] = int((sure_in & off_rng).sum()); accepted[f2] = int((sure_in & in_rng).sum())
        sure = sure_in & in_rng; doubt = cand & ~off_rng & ~sure
        sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        b_, o_, s_, u_ = best[sl], own[sl], second[sl], unc[sl]
        u_[doubt] = np.minimum(u_[doubt], zp[doubt])
        # a face with the same projected corners as the current owner has the same float32 depth, bit for bit: the earlier (smaller) id keeps the pixel
        same = np.zeros(xi.shape, bool)
        for g2 in np.unique(o_[sure & (zp == b_)]):
            if g2 >= 0 and np.array_equal(rec[int(g2)], fc32):
                same |= (o_ == g2)
        twin = sure & same & (zp == b_)
        if tie_larger:
            o_[twin] = f2
        sure = sure & ~twin
        nearer = sure & ((zp <= b_) if tie_larger else (zp < b_))
        s_[nearer] = b_[nearer]; b_[nearer] = zp[nearer]; o_[nearer] = f2
        later = sure & ~nearer
        s_[later] = np.minimum(s_[later], zp[later])
        rec[f2] = fc32
    with np.errstate(invalid="ignore"):
        contested = (unc <= best * (1 + TIE)) | (np.isfinite(second) & (second - best <= TIE * best))
    contested &= np.isfinite(unc) | np.isfinite(best)
    return dict(owner=own[::-1].copy(), contested=contested[::-1].copy(), z1=best[::-1].copy(), z2=second[::-1].copy(), clipped=clipped, accepted=accepted)


def sweep_masks(owner, d_image):
    """(is,is) image orientation -> rowmask[yi, xi], colmask[xi, yi] booleans in the kernels' y-up coordinates: uncovered pixel with d_image < 0"""
    m = ((np.asarray(owner) < 0) & (np.asarray(d_image, F) < 0))[::-1]
    return m.copy(), m.T.copy()


def pack_words(m):
    """(n, is) booleans -> (n, is/64) uint64, bit k of word w = column 64 w + k"""
    n, is_ = m.shape
    b = m.reshape(n, is_ // 64, 64).astype(np.uint64)
    return (b << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def backward(pv, faces, K, verts, owner, d_image, size, eps=1e-4, fault=None, decide=F):
    """ONE frame.  pv (NV,3) float32 projected vertices, owner / d_image (is,is) image orientation.  -> grad (NV,3) float64, S (NV,3), Q (NV,3), stats.
    fault: None | 'drop_word' | 'swap_round' | 'border_empty' (sensitivity variants).  decide: the number format of the discrete decisions --
    float32 is the rule of the kernels and of the float32 oracle; float64 only serves the comparison with the float64 oracle, which decides in float64."""
    D = decide
    is_ = int(size); isf = D(is_); f2s = doubled(faces); NV = len(pv)
    fim = np.asarray(owner)[::-1]; gal = np.asarray(d_image, F)[::-1].astype(np.float64)
    flag_out = (fim < 0) & (gal < 0)
    eps64 = float(D(eps))
    g = np.zeros((NV, 2)); S = np.zeros((NV, 2)); nq = np.zeros((NV, 2))
    stats = dict(walks=0, max_words=0, out_terms=0, in_terms=0, breaks=0, d0_clamped=0, d1_clamped=0, on_corner=0, int_cross=0)
    for f2 in np.unique(fim[fim >= 0]):
        vi = f2s[int(f2)]
        P = (D(0.5) * (pv[vi, :2].astype(D) * isf + isf - D(1))).astype(D)            # (3,2) corners in pixel units as the decisions see them (float32: rounded)
        P64 = 0.5 * (pv[vi, :2].astype(np.float64) * is_ + is_ - 1)                   # ... and their exact values, from which every magnitude is taken
        gf = np.zeros((3, 2)); sf = np.zeros((3, 2))
        for edge in range(3):
            pp = P[[(edge + k) % 3 for k in range(3)]]; pp64 = P64[[(edge + k) % 3 for k in range(3)]]
            for axis in range(2):
                p = pp if axis == 0 else pp[:, ::-1]
                p64 = pp64 if axis == 0 else pp64[:, ::-1]
                lo32, hi32 = min(p[0, 0], p[1, 0]), max(p[0, 0], p[1, 0])
                direction = (-1 if p[0, 0] < p[1, 0] else 1) if axis == 0 else (1 if p[0, 0] < p[1, 0] else -1)
                d0_from = int(max(np.ceil(lo32), D(0))); d0_to = int(min(hi32, D(is_ - 1)))
                if np.ceil(lo32) < 0 or hi32 > is_ - 1:
                    stats["d0_clamped"] += 1
                if d0_to < d0_from:
                    continue
                with np.errstate(all="ignore"):
                    slope32 = (p[1, 1] - p[0, 1]) / (p[1, 0] - p[0, 0]); slope64 = (p64[1, 1] - p64[0, 1]) / (p64[1, 0] - p64[0, 0])
                for d0 in range(d0_from, d0_to + 1):
                    d0f = D(d0)
                    with np.errstate(all="ignore"):
                        x32 = ((p[2, 1] - p[0, 1]) / (p[2, 0] - p[0, 0]) * (d0f - p[0, 0]) + p[0, 1]) if (d0f - p[0, 0]) * (d0f - p[2, 0]) < 0 else \
                              ((p[1, 1] - p[2, 1]) / (p[1, 0] - p[2, 0]) * (d0f - p[2, 0]) + p[2, 1])
                        c32 = slope32 * (d0f - p[0, 0]) + p[0, 1]; c64 = slope64 * (d0 - p64[0, 0]) + p64[0, 1]
                    if not np.isfinite(c32):
                        # an edge along the other axis through d0 (p[0][0] == p[1][0] == d0): 0 x inf.  Both != guards are then false, so whichever pixel the
                        # conversion of a NaN names, no term is formed -- the position contributes nothing
                        stats["on_corner"] += 1
                        continue
                    up = direction > 0
                    if fault == "swap_round" and axis == 0:
                        up = not up
                    d1_in = int(np.floor(c32)) if up else int(np.ceil(c32))
                    d1_out = d1_in + direction
                    stats["int_cross"] += int(np.floor(c32) == np.ceil(c32))
                    if d1_in < 0 or d1_in >= is_ or d1_out < 0 or d1_out >= is_:
                        stats["breaks"] += 1
                        if not (fault == "border_empty" and 0 <= d1_in < is_):
                            continue
                    stats["walks"] += 1
                    px = (lambda d1: (d1, d0)) if axis == 0 else (lambda d1: (d0, d1))          # (yi, xi)
                    if 0 <= d1_out < is_:
                        own_in = fim[px(d1_in)]; a_out = fim[px(d1_out)] >= 0
                    else:                  # ('border_empty': the second break dropped -- a d1_out beyond the image counts as an empty pixel, the inward sweep runs)
                        own_in = -2; a_out = False
                    useA = p[1, 0] != d0f; useB = p[0, 0] != d0f
                    stats["on_corner"] += int(not (useA and useB))

                    def terms(d1s, dg):
                        """the contributions of pixels d1s (int array) with diff_grad dg (float64 array) to corners 0 and 1"""
                        out = []
                        d1f = d1s.astype(D)
                        for use, num32, den32, num64, den64 in ((useA, p[1, 0] - p[0, 0], p[1, 0] - d0f, p64[1, 0] - p64[0, 0], p64[1, 0] - d0),
                                                                (useB, p[1, 0] - p[0, 0], d0f - p[0, 0], p64[1, 0] - p64[0, 0], d0 - p64[0, 0])):
                            if not use or len(d1s) == 0:
                                out.append((0.0, 0.0)); continue
                            dist32 = num32 / den32 * (d1f - c32) * D(2) / isf
                            pos = dist32 > 0
                            mag = np.abs(num64 / den64 * (d1s - c64) * 2.0 / is_) + eps64
                            t = -dg / np.where(pos, mag, -mag)
                            out.append((float(t.sum()), float(np.abs(t).sum())))
                        return out

                    ga = gb = sa = sb = 0.0
                    if own_in == f2:
                        lim = is_ - 1 if direction > 0 else 0
                        a, b = max(min(d1_out, lim), 0), min(max(d1_out, lim), is_ - 1)
                        stats["d1_clamped"] += int(min(d1_out, lim) < 0 or max(d1_out, lim) > is_ - 1)
                        line = flag_out[a:b + 1, d0] if axis == 0 else flag_out[d0, a:b + 1]
                        d1s = a + np.nonzero(line)[0]
                        if fault == "drop_word":
                            d1s = d1s[(d1s >> 6) != 1]
                        if len(d1s):
                            stats["max_words"] = max(stats["max_words"], int(d1s[-1] >> 6) - int(d1s[0] >> 6) + 1)
                            stats["out_terms"] += len(d1s)
                            gl = gal[d1s, d0] if axis == 0 else gal[d0, d1s]
                            (ta, xa), (tb, xb) = terms(d1s, -gl)
                            ga += ta; sa += xa; gb += tb; sb += xb
                    if not a_out:
                        # a third edge parallel to the sweep gives +-inf (NaN where d0 lies on it): it bounds nothing.  The conversion saturates (NaN -> 0), the
                        # clamps below keep the sweep in the image; only this face's own pixels of the line contribute, whichever way the limit points
                        lim = (int(np.ceil(x32)) if direction > 0 else int(np.floor(x32))) if np.isfinite(x32) else (0 if np.isnan(x32) or x32 < 0 else is_)
                        a, b = max(min(d1_in, lim), 0), min(max(d1_in, lim), is_ - 1)
                        if a <= b:
                            stats["d1_clamped"] += int(min(d1_in, lim) < 0 or max(d1_in, lim) > is_ - 1)
                            ol = fim[a:b + 1, d0] if axis == 0 else fim[d0, a:b + 1]
                            gl = gal[a:b + 1, d0] if axis == 0 else gal[d0, a:b + 1]
                            sel = (ol == f2) & (gl > 0)
                            d1s = a + np.nonzero(sel)[0]
                            if len(d1s):
                                stats["in_terms"] += len(d1s)
                                (ta, xa), (tb, xb) = terms(d1s, gl[sel])
                                ga += ta; sa += xa; gb += tb; sb += xb
                    c = 1 - axis
                    gf[edge, c] += ga; sf[edge, c] += sa
                    gf[(edge + 1) % 3, c] += gb; sf[(edge + 1) % 3, c] += sb
        for k in range(3):
            g[vi[k]] += gf[k]; S[vi[k]] += sf[k]; nq[vi[k]] += sf[k] > 0
    return (*unproject(g, S, nq * FIXQ, K, verts), stats)


def unproject(g, S, Qp, K, verts):
    """(u_n, v_n) gradients -> camera-space vertices; S and Q carried with absolute values"""
    K = np.asarray(K, np.float64).reshape(9); v = np.asarray(verts, np.float64)
    z = v[:, 2] + 1e-9
    gx = 2 * g[:, 0] * K[0] - 2 * g[:, 1] * K[3]; gy = 2 * g[:, 0] * K[1] - 2 * g[:, 1] * K[4]
    grad = np.stack([gx / z, gy / z, -(gx * v[:, 0] + gy * v[:, 1]) / (z * z)], -1)

    def carry(a):
        ax = 2 * a[:, 0] * abs(K[0]) + 2 * a[:, 1] * abs(K[3]); ay = 2 * a[:, 0] * abs(K[1]) + 2 * a[:, 1] * abs(K[4])
        return np.stack([ax / z, ay / z, (ax * np.abs(v[:, 0]) + ay * np.abs(v[:, 1])) / (z * z)], -1)
    return grad, carry(S), carry(Qp)


def mask_term(image, keep, ref, occ, gscale):
    """(B,is,is) float32 each -> d_image float32 (2 d keep occ gs, left to right, gs = gscale / B in float32) and the term mean_b(occ_b sum d^2) in float64"""
    image, keep, ref, occ = (np.asarray(a, F) for a in (image, keep, ref, occ))
    B = image.shape[0]
    gs = F(gscale) / F(B)
    d = keep * image - ref
    ob = occ[:, None, None]
    d_image = (((F(2) * d) * keep) * ob) * gs
    per = (d * d).astype(np.float64).reshape(B, -1).sum(1)
    return d_image.astype(F), float((per * occ.astype(np.float64)).sum() / B), per


def units(got, want, S, Q=0.0):
    """|got - want| in units of u S after the fixed-point allowance Q; inf where the scale is 0 and the value is not"""
    err = np.maximum(np.abs(np.asarray(got, np.float64) - want) - Q, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = err / (U * S)
    return np.where(S > 0, r, np.where(err > 0, np.inf, 0.0))
