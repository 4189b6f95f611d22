"""Test helper (not a test file): the cases of tests/test_host_sil_model.py and tests/test_gpu_sil_perpixel.py -- small meshes at every size class of csrc/sil.hip
(words per sweep-mask line wpl = size / 64 = 1, 2, 3, 4, 5, 8; power-of-two sizes multiply by 1 / size, the others divide), the geometry the 256-pixel tests never
show (image border, depth planes, close layers, pixel centres on edges and vertices, slivers, face counts around a lane group) and an upstream gradient whose
negative part fills whole rows.  numpy only.  The preconditions each family claims are asserted by tests/test_host_sil_model.py."""
import numpy as np

from vistracker_amd import synthetic as syn

F = np.float32
EPS = 1e-4
GATE = 8                    # as tests/test_gpu_smplh_perjoint.py and the query tests
MAX_CONTESTED = 0.005       # share of a case's covered pixels whose owner float32 arithmetic cannot decide
SIZES = (64, 128, 192, 256, 320, 512)
LAYER_GAPS = (1e-2, 1e-3, 1e-4)
NARROW_GAPS = (1e-5, 1e-6, 1e-6)

# worst |float32 CPU oracle - model| per case in units of u S (u = 2^-24), measured by tests/test_host_sil_model.py, which holds these figures to a fresh
# measurement within a factor of 2 (tests/golden/sil_perpixel.md).  The terms are diff_grad / (sA (d1 - d1_cross) + eps): the difference d1 - d1_cross
# cancels, so correct float32 arithmetic is hundreds of u away from the exact value wherever a sweep pixel lies close to the edge.
E32 = {
    "inside-64": 620.0,
    "inside-128": 3900.0,
    "inside-192": 14000.0,
    "inside-256": 7500.0,
    "inside-320": 4000.0,
    "inside-512": 27000.0,
    "inside-256-rand": 11000.0,
    "cut-64": 2300.0,
    "near-64": 1300.0,
    "far-64": 6100.0,
    "layers-64": 570.0,
    "layers-narrow-64": 570.0,
    "slivers-64": 310.0,
    "counts-64-nf1": 71.0,
    "counts-64-nf15": 480.0,
    "counts-64-nf16": 480.0,
    "counts-64-nf17": 480.0,
    "cut-192": 14000.0,
    "near-192": 6500.0,
    "far-192": 7900.0,
    "layers-192": 520.0,
    "layers-narrow-192": 520.0,
    "slivers-192": 500.0,
    "counts-192-nf1": 150.0,
    "counts-192-nf15": 11000.0,
    "counts-192-nf16": 11000.0,
    "counts-192-nf17": 11000.0,
    "cut-320": 5500.0,
    "near-320": 8300.0,
    "far-320": 6600.0,
    "layers-320": 150.0,
    "layers-narrow-320": 150.0,
    "slivers-320": 51000.0,
    "counts-320-nf1": 2500.0,
    "counts-320-nf15": 2100.0,
    "counts-320-nf16": 2100.0,
    "counts-320-nf17": 2100.0,
    "lattice-64": 1.5,
    "lattice-192": 17000.0,
    "lattice-256": 1.2,
    "lattice-320": 14000.0,
}


def gate(case):
    """allowed |kernel - model| in units of u S: GATE x the float32 oracle's own error on this case, never less than GATE float32 roundings"""
    return GATE * max(E32[case.name], 1.0)


def family_e32():
    out = {}
    for k, v in E32.items():
        f = k.split("-")[0]; out[f] = max(out.get(f, 0.0), v)
    return out


_TV, _TF = syn.object_template(n_lat=7, n_lon=12)          # 86 vertices, 168 faces


def _K(B, f=1.6, cx=0.5, cy=0.5):
    K = np.zeros((B, 9), F); K[:, 0] = K[:, 4] = f; K[:, 2] = cx; K[:, 5] = cy; K[:, 8] = 1
    return K


def _posed(seed, B, scale=1.0, tz=2.3, jitter=0.05):
    rng = np.random.default_rng(seed)
    R = syn.random_rotations(B, rng)
    t = rng.normal(0, jitter, (B, 3)) * scale + [0, 0, tz]
    return (np.einsum("nc,bcd->bnd", _TV.astype(np.float64) * scale, R) + t[:, None]).astype(F)


class Case:
    def __init__(self, name, family, size, verts, faces, K, exact=False, asserted=True, gscale=0.75, d_image=None, f32edges=False):
        # exact: no pixel may be left out of an owner comparison; f32edges: the model's forward takes its edge tests in float32 (every exact case does)
        self.name, self.family, self.size, self.exact, self.asserted, self.eps = name, family, int(size), exact, asserted, EPS
        self.f32edges = bool(f32edges or exact)
        self.verts = np.ascontiguousarray(verts, F); self.faces = np.ascontiguousarray(faces, np.int32); self.K = np.ascontiguousarray(K, F)
        self.B, self.NV, self.NF = self.verts.shape[0], self.verts.shape[1], self.faces.shape[0]
        self.gscale = float(gscale); self.d_image = d_image
        B, s = self.B, self.size
        # reference silhouette: much larger than the object and shifted from it -- everything right of a column that moves with the frame, up to the last pixel and
        # the top row; keep: a rectangular hole.  Uncovered pixels with d < 0 then fill whole rows across every 64-bit word boundary and reach the last word.
        self.ref = np.zeros((B, s, s), F); self.keep = np.ones((B, s, s), F)
        for b in range(B):
            self.ref[b, : s - s // 8, int((0.45 - 0.15 * b) * s):] = 1
        self.keep[:, s // 3: s // 3 + s // 6, s // 2: s // 2 + s // 5] = 0
        self.occ = np.array([1.0, 0.6, 0.35], F)[:B]

    def __repr__(self):
        return self.name


def _lattice(size):
    """a flat sheet at z = 1 whose vertices project onto pixel centres (exactly at the power-of-two sizes): cells of 8 and 16 pixels, so that barycentric weights and
    depths are exact there too and every shared edge is an exact tie; the left column and the top row of vertices lie on border pixels, the right and bottom rims
    run through centres inside the image"""
    ix = [0, 8, 16, 24, 40, 56]; iy = [size - 1 - k for k in (0, 16, 32, 40, 48, 56)]
    n = len(ix)
    verts = np.array([[(2 * i + 1 - size) / (2.0 * size), -(2 * j + 1 - size) / (2.0 * size), 1.0] for j in iy for i in ix])
    faces = []
    for j in range(n - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i, (j + 1) * n + i + 1
            faces += [[a, b, d], [a, d, c]] if (i + j) % 2 == 0 else [[a, b, c], [b, d, c]]
    return verts[None], np.array(faces), _K(1, 1.0)


def _layers(gaps):
    gx, gy = np.array([-0.8, 0.05, 0.8]), np.array([-0.8, -0.1, 0.8])
    hx, hy = np.array([-0.75, -0.1, 0.7]), np.array([-0.8, 0.15, 0.78])
    tri = []
    for j in range(2):
        for i in range(2):
            a, b, c, d = j * 3 + i, j * 3 + i + 1, (j + 1) * 3 + i, (j + 1) * 3 + i + 1
            tri += [[a, b, d], [a, d, c]]
    tri = np.array(tri)
    verts = []
    for g in gaps:
        XA, YA = np.meshgrid(gx, gy); XB, YB = np.meshgrid(hx, hy)
        # two PLANES of camera space, (X / 2, Y / 2, 1) z being the ray of image point (X, Y): A is z = 2 + 0.3 x; B is A scaled by 1 + g about the eye, then
        # tilted away by 5e-4 per unit of Y -- along every ray B lies behind A by the relative gap g + 5e-4 (Y + 0.8) / (1 - 0.15 X) >= g
        zA = 2 / (1 - 0.15 * XA)
        zB = 2 * (1 + g) / (1 - 0.15 * XB - 0.0005 * (YB + 0.8))
        A = np.stack([XA * zA / 2, YA * zA / 2, zA], -1).reshape(-1, 3); Bs = np.stack([XB * zB / 2, YB * zB / 2, zB], -1).reshape(-1, 3)
        verts.append(np.concatenate([Bs, A], 0))                    # the FAR sheet takes the smaller face ids: a wrong order or a tie rule shows as its ids
    return np.array(verts), np.concatenate([tri, tri + 9], 0), _K(len(gaps), 1.0)


def _slivers(size):
    px = 2.0 / size
    P = [(-0.9, -0.9), (0.9, 0.88), (0.9, 0.9)]                                       # long and thin: a box of the whole image, a line of centres
    for cx, cy in ((-0.5, 0.5), (0.25, -0.75), (0.0, 0.0)):                           # smaller than a pixel, around a pixel CORNER: no centre inside
        P += [(cx + 0.3 * px, cy), (cx - 0.2 * px, cy + 0.25 * px), (cx - 0.2 * px, cy - 0.25 * px)]
    P += [(-0.5, -0.25), (0.0, 0.0), (0.5, 0.25)]                                    # collinear: den == 0 exactly
    P += [(0.1, -0.8), (0.7, -0.7), (0.3, -0.2)]                                     # listed twice: the smaller id owns
    P += [(-0.8, 0.2), (-0.2, 0.3), (-0.6, 0.9)]
    ndc = np.array(P)
    verts = np.stack([ndc[:, 0] / 2, -ndc[:, 1] / 2, np.ones(len(P))], -1)
    faces = [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(5)] + [[15, 16, 17], [15, 16, 17], [18, 19, 20]]
    return verts[None], np.array(faces), _K(1, 1.0)


def all_cases():
    out = []
    for s in SIZES:
        out.append(Case(f"inside-{s}", "inside", s, _posed(40 + s, 3), _TF, _K(3), gscale=0.0003 if s == 256 else 0.75))
    rng = np.random.default_rng(7)
    out.append(Case("inside-256-rand", "inside", 256, _posed(41, 3), _TF, _K(3), d_image=rng.normal(0, 1, (3, 256, 256)).astype(F)))
    for s in (64, 192, 320):
        K = _K(3); K[0, 2], K[0, 5] = 0.05, 0.06; K[1, 2] = -0.08; K[2, 2], K[2, 5] = 0.95, 0.96          # two borders and a corner; centre outside; the opposite corner
        out.append(Case(f"cut-{s}", "cut", s, _posed(50 + s, 3), _TF, K))
        out.append(Case(f"near-{s}", "near", s, _posed(60 + s, 3, scale=0.1, tz=0.1), _TF, _K(3, 0.8)))
        out.append(Case(f"far-{s}", "far", s, _posed(70 + s, 3, scale=100.0, tz=100.0), _TF, _K(3, 0.8)))
        out.append(Case(f"layers-{s}", "layers", s, *_layers(LAYER_GAPS), exact=True))
        out.append(Case(f"layers-narrow-{s}", "layers", s, *_layers(NARROW_GAPS), asserted=False))
        out.append(Case(f"slivers-{s}", "slivers", s, *_slivers(s), exact=True))
        v1 = _posed(80 + s, 1)
        for nf in (1, 15, 16, 17):
            out.append(Case(f"counts-{s}-nf{nf}", "counts", s, v1, _TF[:nf], _K(1)))
    for s in (64, 192, 256, 320):
        # every lattice case is compared with float32 edge tests.  At 320 the vertices are within float32 rounding of the centres, not on them, and the float32 oracle
        # breaks two of the depth ties on shared edges by its own rounding: those pixels alone are left out (tests/test_host_sil_model.py proves them contested)
        out.append(Case(f"lattice-{s}", "lattice", s, *_lattice(s), exact=s != 320, f32edges=True))
    return out


_REF = {}


def reference(case):
    """computed once per case and shared: the float32 oracle's image, owner map and gradient, the upstream gradient, the model's forward per frame and the model's
    backward on the ORACLE's owner map.  Nothing in it is modified by the tests."""
    if case.name in _REF:
        return _REF[case.name]
    import sil_model as M
    from oracle import oracle as O
    c = case
    img = O.sil_forward(c.verts, c.faces, c.K, c.size); fi = O.sil_face_index(c.verts, c.faces, c.K, c.size)
    pv = M.project32(c.verts, c.K)
    if c.d_image is not None:
        dimg, term = c.d_image, None
    else:
        dimg, term, _ = M.mask_term(img, c.keep, c.ref, c.occ, c.gscale)
    fw = [M.forward(pv[b], c.faces, c.size, edge="f32" if c.f32edges else "f64") for b in range(c.B)]
    f64 = fw if not c.f32edges else ([M.forward(pv[b], c.faces, c.size) for b in range(c.B)] if not c.exact else None)
    bw = [M.backward(pv[b], c.faces, c.K[b], c.verts[b], fi[b], dimg[b], c.size, c.eps) for b in range(c.B)]
    r = dict(img=img, fi=fi, pv=pv, dimg=dimg, term=term, fw=fw, grad=np.stack([x[0] for x in bw]), S=np.stack([x[1] for x in bw]), Q=np.stack([x[2] for x in bw]),
             stats=[x[3] for x in bw], owner=np.stack([x["owner"] for x in fw]))
    # contested: what the float64 model cannot decide (None in an exact case, where it plays no part).  skip: the pixels left out of the kernel's comparison with the
    # oracle -- ONLY those where oracle and model were found to differ; tests/test_host_sil_model.py shows each of them contested and caps their number
    r["contested"] = None if f64 is None else np.stack([x["contested"] for x in f64])
    r["skip"] = (r["owner"] != fi) | ((r["owner"] >= 0) != (img > 0))
    _REF[case.name] = r
    return r
