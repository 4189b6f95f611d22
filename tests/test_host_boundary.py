"""CPU: the float64 point-to-mesh model against closed forms, and the host side of vistracker_amd.boundary_sampler (no GPU call)."""
import numpy as np
import pytest

import pmdist_model as M
from vistracker_amd.boundary_sampler import BoundarySampler

# the hand-made triangle of the closed forms: a right angle at a, in the plane z = 0
A, B_, C_ = np.array([0.0, 0, 0]), np.array([2.0, 0, 0]), np.array([0.0, 1, 0])
# (query in the plane, closest point, region code of pmdist_model.closest_on_triangles); each query is lifted to z = +0.5 and z = -0.7 as well
REGION_CASES = [
    ((-1.0, -1.0), (0.0, 0.0), 0),      # vertex a
    ((3.0, -0.5), (2.0, 0.0), 1),       # vertex b
    ((-0.5, 2.0), (0.0, 1.0), 2),       # vertex c
    ((1.0, -1.0), (1.0, 0.0), 3),       # edge ab
    ((-1.0, 0.5), (0.0, 0.5), 4),       # edge ac
    ((2.0, 2.0), (1.2, 0.4), 5),        # edge bc: b + 0.4 (c - b)
    ((0.5, 0.25), (0.5, 0.25), 6),      # interior
]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_model_seven_regions_closed_form(dtype):
    tol = 1e-12 if dtype == np.float64 else 1e-6
    tri = [x[None].astype(dtype) for x in (A, B_, C_)]
    for (qx, qy), (cx, cy), code in REGION_CASES:
        for z in (0.5, -0.7, 0.0):
            p = np.array([[qx, qy, z]], dtype)
            q, region = M.closest_on_triangles(p, *tri)
            assert region[0, 0] == code, ((qx, qy, z), region)
            assert q.dtype == dtype
            np.testing.assert_allclose(q[0, 0], [cx, cy, 0.0], atol=tol)
            r = M.point_mesh(p, np.stack([A, B_, C_]), [[0, 1, 2]], dtype=dtype)
            np.testing.assert_allclose(r["dist"][0], np.sqrt((qx - cx) ** 2 + (qy - cy) ** 2 + z * z), atol=tol)
            assert r["face"][0] == 0


def test_model_on_the_surface_and_at_a_corner():
    v = np.stack([A, B_, C_])
    r = M.point_mesh(np.array([[0.5, 0.25, 0.0], [2.0, 0, 0], [1.0, 0.5, 0.0]]), v, [[0, 1, 2]])      # interior, corner b, on the edge bc
    np.testing.assert_allclose(r["dist"], 0, atol=1e-15)
    np.testing.assert_allclose(r["closest"], [[0.5, 0.25, 0], [2, 0, 0], [1, 0.5, 0]], atol=1e-15)


def test_model_zero_area_triangles():
    """collinear corners (in any order), two equal corners, three equal corners: the distance to the segment or the point, never NaN"""
    p = np.array([[1.0, 1, 0], [-1.0, 0, 2], [5.0, 0, 0], [1.5, 0, 0]])
    seg = np.sqrt([1.0, 5.0, 4.0, 0.0])                                   # to the segment (0,0,0) -> (3,0,0)
    for v in ([[0, 0, 0], [1.0, 0, 0], [3.0, 0, 0]], [[3.0, 0, 0], [0, 0, 0], [1.0, 0, 0]], [[1.0, 0, 0], [3.0, 0, 0], [0, 0, 0]],
              [[0, 0, 0], [3.0, 0, 0], [3.0, 0, 0]], [[0, 0, 0], [0, 0, 0], [3.0, 0, 0]]):
        for dt in (np.float64, np.float32):
            r = M.point_mesh(p, np.array(v), [[0, 1, 2]], dtype=dt)
            assert np.isfinite(r["dist"]).all() and np.isfinite(r["closest"]).all()
            np.testing.assert_allclose(r["dist"], seg, atol=1e-6)
    r = M.point_mesh(p, np.array([[1.0, 2, 3]] * 3), [[0, 1, 2]])
    np.testing.assert_allclose(r["dist"], np.linalg.norm(p - [1.0, 2, 3], axis=1), atol=1e-14)


def test_model_minimum_second_best_and_nearest_vertex():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0.0, 0, 5], [1, 0, 5], [0, 1, 5], [1.0, 1, 0]])
    f = [[0, 1, 2], [3, 4, 5], [1, 6, 2]]                                  # face 2 shares an edge with face 0, face 1 floats 5 above
    p = np.array([[0.2, 0.2, 1.0], [0.2, 0.2, 4.5], [0.9, 0.9, -2.0]])
    r = M.point_mesh(p, v, f, second=True)
    np.testing.assert_array_equal(r["face"], [0, 1, 2])
    np.testing.assert_allclose(r["dist"], [1.0, 0.5, 2.0], atol=1e-14)
    np.testing.assert_allclose(r["dist2"], [4.0, 4.5, np.sqrt(49 + 0.32)], atol=1e-14)   # the best face that shares no vertex with the winner
    idx, d, other = M.nearest_vertex(p, v, second_labels=np.array([0, 0, 0, 1, 1, 1, 0]))
    np.testing.assert_array_equal(idx, [0, 3, 6])
    np.testing.assert_allclose(d, np.linalg.norm(p - v[idx], axis=1), atol=1e-14)
    np.testing.assert_allclose(other[0], np.linalg.norm(p[0] - v[3]), atol=1e-14)


def test_flip_part_labels():
    bs = BoundarySampler(np.zeros(6890, np.int32))
    left_right = {1: 6, 2: 7, 3: 8, 4: 9, 5: 10, 12: 13}
    full = {**left_right, **{v: k for k, v in left_right.items()}, 0: 0, 11: 11}
    parts = np.arange(14).astype(np.int32)
    out = bs.flip_part_labels(parts)
    assert out.dtype == parts.dtype and out is not parts
    np.testing.assert_array_equal(out, [full[p] for p in range(14)])
    np.testing.assert_array_equal(parts, np.arange(14))                     # the input is left alone
    np.testing.assert_array_equal(bs.flip_part_labels(out), parts)         # an involution
    import torch
    t = bs.flip_part_labels(torch.arange(14, dtype=torch.int32))
    np.testing.assert_array_equal(t.numpy(), out)


def test_part_labels_from_the_asset_layout(tmp_path):
    import pickle
    asset = {"head": np.array([0, 5]), "torso": np.array([1, 2, 6889]), "arm": np.array([3])}
    want = np.zeros(6890, np.int32); want[[1, 2, 6889]] = 1; want[3] = 2
    np.testing.assert_array_equal(BoundarySampler(asset).part_labels, want)
    path = tmp_path / "parts.pkl"
    with open(path, "wb") as fh:
        pickle.dump(asset, fh)
    np.testing.assert_array_equal(BoundarySampler(str(path)).part_labels, want)
    lab = (np.arange(6890) % 14).astype(np.int64)
    bs = BoundarySampler(lab)
    assert bs.part_labels.dtype == np.int32
    np.testing.assert_array_equal(bs.part_labels, lab)


def test_get_sample_num():
    bs = BoundarySampler(np.zeros(6890, np.int32))
    assert bs.get_sample_num(0.5, 100000) == 50000
    assert bs.get_sample_num(0.01, 100000) == 10000                         # the floor: thres = 10000 by default
    assert bs.get_sample_num(0.01, 100000, thres=500) == 1000
    assert bs.get_sample_num(0.1, 100000, thres=10000) == 10000            # int(ratio * total) == thres is not below it
    assert bs.get_sample_num(0.99, 2048, thres=1024) == 2027               # int(2027.52)
    assert bs.get_sample_num(0.01, 2048, thres=1024) == 1024
    assert isinstance(bs.get_sample_num(0.3, 7), int)


def test_bounds_and_grid_samples():
    import torch
    bmin, bmax = BoundarySampler.get_bounds()
    np.testing.assert_array_equal(bmin, [-3.0, -0.9, 0.2])
    np.testing.assert_array_equal(bmax, [3.0, 1.8, 4.0])
    g = torch.Generator(device="cpu"); g.manual_seed(3)
    pts = BoundarySampler.get_grid_samples(bmin, bmax, 5000, generator=g, device="cpu")
    assert tuple(pts.shape) == (5000, 3) and pts.dtype == torch.float32
    p = pts.numpy().astype(np.float64)
    assert (p >= bmin.astype(np.float32)).all() and (p <= bmax.astype(np.float32)).all()
    # uniform: every axis fills its range (5000 draws leave less than 1 % at either end with probability 1 - 2 e^-50) and its mean is central
    span = bmax - bmin
    assert ((p.min(0) - bmin) < 0.01 * span).all() and ((bmax - p.max(0)) < 0.01 * span).all()
    assert (np.abs(p.mean(0) - 0.5 * (bmin + bmax)) < 4 * span / np.sqrt(12 * 5000)).all()
    g.manual_seed(3)
    again = BoundarySampler.get_grid_samples(bmin, bmax, 5000, generator=g, device="cpu")
    assert torch.equal(pts, again)
    assert tuple(BoundarySampler.get_grid_samples(bmin, bmax, 0, generator=g, device="cpu").shape) == (0, 3)


def _cloud(seed=0, n=400):
    rng = np.random.default_rng(seed)
    R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return (rng.normal(size=(n, 3)) * [0.5, 0.2, 0.05]) @ R.T + [0.3, -1.0, 2.5]


def test_compute_pca_against_numpy():
    x = _cloud()
    ax = BoundarySampler.compute_pca(x)
    assert ax.shape == (3, 3) and ax.dtype == np.float64
    np.testing.assert_allclose(ax @ ax.T, np.eye(3), atol=1e-12)            # orthonormal rows
    xc = x - x.mean(0)
    var = ((xc @ ax.T) ** 2).sum(0) / (len(x) - 1)
    assert var[0] > var[1] > var[2]                                         # by descending variance
    w, v = np.linalg.eigh(np.cov(x.T))
    np.testing.assert_allclose(var, w[::-1], rtol=1e-10)
    np.testing.assert_allclose(np.abs(ax @ v[:, ::-1]), np.eye(3), atol=1e-8)    # the eigenvectors of the covariance, up to sign
    # the documented sign: the entry of largest magnitude of every row is positive
    assert (ax[np.arange(3), np.abs(ax).argmax(1)] > 0).all()
    # a batch is answered per frame, a (verts, faces) pair is accepted, tensors too
    import torch
    y = _cloud(1)
    both = BoundarySampler.compute_pca((torch.tensor(np.stack([x, y]), dtype=torch.float64), None))
    np.testing.assert_allclose(both[0], ax, atol=1e-12)
    np.testing.assert_allclose(both[1], BoundarySampler.compute_pca(y), atol=1e-12)


def test_compute_pca_sign_matches_installed_sklearn():
    decomposition = pytest.importorskip("sklearn.decomposition")
    for seed in range(4):
        x = _cloud(seed)
        pca = decomposition.PCA(n_components=3)
        pca.fit(x)
        np.testing.assert_allclose(BoundarySampler.compute_pca(x), pca.components_, atol=1e-9)
