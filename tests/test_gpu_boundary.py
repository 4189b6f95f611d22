"""GPU: vt_point_mesh_distance / vt_nearest_vertex (csrc/pmdist.hip) and vistracker_amd.boundary_sampler against the float64 brute force of
tests/pmdist_model.py.

The bound of every comparison with the model is MEASURED, not guessed: e32 = the largest difference between the model run in float32 and in float64 on the
inputs of the test -- what the number format alone costs -- and the kernel, which evaluates the same formulas in another, equally valid order, gets 4 e32.
"""
import numpy as np
import pytest
import torch

import pmdist_model as M

pytestmark = pytest.mark.gpu

# the hand-made triangle of tests/test_host_boundary.py and its seven region queries (in-plane query, closest point)
TRI = np.array([[0.0, 0, 0], [2.0, 0, 0], [0.0, 1, 0]], np.float32)
SEVEN = [((-1.0, -1.0), (0.0, 0.0)), ((3.0, -0.5), (2.0, 0.0)), ((-0.5, 2.0), (0.0, 1.0)), ((1.0, -1.0), (1.0, 0.0)), ((-1.0, 0.5), (0.0, 0.5)),
         ((2.0, 2.0), (1.2, 0.4)), ((0.5, 0.25), (0.5, 0.25))]


def seven_queries():
    q = np.array([[x, y, z] for (x, y), _ in SEVEN for z in (0.5, -0.7)] + [[0.5, 0.25, 0.0], [2.0, 0.0, 0.0]], np.float32)    # + on the surface, at a corner
    c = np.array([[x, y, 0.0] for _, (x, y) in SEVEN for _ in (0, 1)] + [[0.5, 0.25, 0.0], [2.0, 0.0, 0.0]], np.float64)
    return q, c


from pmdist_cases import body_object_case, dev, model_reference  # noqa: E402


@pytest.fixture(scope="module")
def case():
    from vistracker_amd import ops
    c = body_object_case()
    c["ref_h"], c["e32_h"] = model_reference(c["points"], c["body"], c["body_faces"])          # each mesh is held to 4 x ITS OWN e32
    c["ref_o"], c["e32_o"] = model_reference(c["points"], c["obj"], c["obj_faces"])
    p = dev(c["points"])
    c["gpu_h"] = ops.point_mesh_distance(p, dev(c["body"]), dev(c["body_faces"], torch.int32))
    c["gpu_o"] = ops.point_mesh_distance(p, dev(c["obj"]), dev(c["obj_faces"], torch.int32))
    return c


def on_face_error(closest, verts, faces, face_id):
    """largest float64 distance from closest[i] to the triangle faces[face_id[i]] of verts"""
    worst = 0.0
    for i, f in enumerate(face_id):
        worst = max(worst, float(M.point_mesh(closest[i:i + 1], verts, faces[f:f + 1], workers=1)["dist"][0]))
    return worst


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_hand_made_mesh():
    """two triangles sharing an edge (together the rectangle [0,2] x [0,1] in z = 0: its closest point is a clamp) and triangles without area; the seven
    region queries of the first triangle, above and below the plane, on the surface and at a corner.  The seven regions against the triangle alone are
    test_shapes_at_the_edges' NF = 1 case.  The triangles without area, 20 m apart in y: collinear corners with the longest edge a->b, a->c and b->c (the
    three branches of the set-up kernel), two equal corners (a == b, b == c), three equal corners."""
    from vistracker_amd import ops
    verts = [[0.0, 0, 0], [2.0, 0, 0], [0.0, 1, 0], [2.0, 1, 0]]
    faces = [[0, 1, 2], [1, 3, 2]]
    q, _ = seven_queries()
    q = np.concatenate([q, [[1.6, 0.7, 0.3]]]).tolist()
    want = np.stack([np.clip(np.array(q)[:, 0], 0, 2), np.clip(np.array(q)[:, 1], 0, 1), np.zeros(len(q))], 1).tolist()
    want_face = [None] * len(q)                                                 # either triangle of the rectangle may own a query on the shared edge ...
    want_face[-1] = 1                                                            # ... but (1.6, 0.7) lies over the second one only
    xs = {"a->b": (8.0, 5.0, 6.0), "a->c": (5.0, 6.0, 8.0), "b->c": (6.0, 5.0, 8.0), "a == b": (5.0, 5.0, 8.0), "b == c": (5.0, 8.0, 8.0)}
    for k, (name, x3) in enumerate(xs.items()):                                  # each the segment x in [5, 8] at y = 20 (k + 1), z = 5
        y = 20.0 * (k + 1); base = len(verts)
        verts += [[x, y, 5.0] for x in x3]; faces.append([base, base + 1, base + 2])
        q += [[7.0, y + 1, 5.0], [9.0, y, 5.0], [4.0, y, 6.0], [5.5, y, 5.0]]
        want += [[7.0, y, 5.0], [8.0, y, 5.0], [5.0, y, 5.0], [5.5, y, 5.0]]
        want_face += [len(faces) - 1] * 4
    base = len(verts); verts.append([5.0, 140.0, 5.0]); faces.append([base, base, base])        # three equal corners: a point
    q += [[7.0, 141.0, 5.0], [5.0, 140.0, 5.0]]; want += [[5.0, 140.0, 5.0]] * 2; want_face += [len(faces) - 1] * 2
    verts, faces, q, want = np.array(verts, np.float32), np.array(faces, np.int32), np.array(q, np.float32), np.array(want, np.float64)
    dist, closest, face = (t.cpu().numpy() for t in ops.point_mesh_distance(dev(q), dev(verts), dev(faces, torch.int32)))
    assert np.isfinite(dist).all() and np.isfinite(closest).all()
    np.testing.assert_allclose(closest, want, atol=1e-6)
    np.testing.assert_allclose(dist, np.linalg.norm(q - want, axis=1), atol=1e-6)
    for i, f in enumerate(want_face):
        assert face[i] == f if f is not None else face[i] < 2, (i, face[i], f)
    assert on_face_error(closest.astype(np.float64), verts, faces, face) < 1e-6
    ref = M.point_mesh(q, verts, faces)
    np.testing.assert_allclose(dist, ref["dist"], atol=1e-6)
    np.testing.assert_array_equal(face[[f is not None for f in want_face]], ref["face"][[f is not None for f in want_face]])
    # culling off: the same bits (the set-up's segment records and their spheres)
    for x, y in zip(ops.point_mesh_distance(dev(q), dev(verts), dev(faces, torch.int32), culling=False), (dist, closest, face)):
        np.testing.assert_array_equal(x.cpu().numpy(), y)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["h", "o"])
def test_body_and_object_distance(case, mesh):
    pts = case["points"].astype(np.float64)
    ref, (dist, closest, face) = case["ref_" + mesh], [t.cpu().numpy() for t in case["gpu_" + mesh]]
    bound = 4 * case["e32_" + mesh]
    err = np.abs(dist - ref["dist"])
    print(f"\n[{mesh}] e32 = {case['e32_' + mesh]:.3e}  bound 4 e32 = {bound:.3e}  kernel |dist - model| max = {err.max():.3e}")
    assert np.isfinite(dist).all() and np.isfinite(closest).all()
    assert err.max() <= bound
    own = np.abs(np.linalg.norm(closest.astype(np.float64) - pts, axis=-1) - dist)
    assert own.max() <= bound                                                    # the distance IS |p - closest| of the point written out
    nf = len(case["body_faces" if mesh == "h" else "obj_faces"])
    assert face.min() >= 0 and face.max() < nf


@pytest.mark.parametrize("mesh", ["h", "o"])
def test_body_and_object_closest_point(case, mesh):
    """|closest - model closest| <= 4 e32 outside the queries equidistant from two separate patches (best and second-best faces WITHOUT a common vertex
    within the bound).  Faces that share an edge are NOT excluded: a query on the bisector of a concave edge of the object has two closest points 0.2 mm
    apart whose distances differ by 1e-9 .. 1e-8 m, which fp32 alone cannot order (the float32 run of the model names the other face for 2 .. 4 of 512
    queries per frame); the kernel's fp64 arbiter among the near-minimal triangles does."""
    ref, (dist, closest, face) = case["ref_" + mesh], [t.cpu().numpy() for t in case["gpu_" + mesh]]
    bound = 4 * case["e32_" + mesh]
    tie = (ref["dist2"] - ref["dist"]) < bound
    dq = np.linalg.norm(closest - ref["closest"], axis=-1)
    print(f"\n[{mesh}] equidistant from two patches: {int(tie.sum())} of {tie.size} excluded; |closest - model closest| max over the rest = {dq[~tie].max():.3e}, "
          f"{int((dq[~tie] > bound).sum())} beyond the bound {bound:.3e}")
    assert tie.mean() <= 0.01
    assert dq[~tie].max() <= bound


def test_culling_changes_nothing(case):
    from vistracker_amd import ops
    p, v, f = dev(case["points"]), dev(case["body"]), dev(case["body_faces"], torch.int32)
    B, N = case["points"].shape[:2]; NF = len(case["body_faces"])
    n_all = torch.zeros(1, dtype=torch.int64, device="cuda"); n_cull = torch.zeros(1, dtype=torch.int64, device="cuda")
    full = ops.point_mesh_distance(p, v, f, culling=False, n_tests=n_all)
    cull = ops.point_mesh_distance(p, v, f, n_tests=n_cull)
    for a, b, c in zip(full, cull, case["gpu_h"]):
        assert torch.equal(a, b) and torch.equal(a, c)
    print(f"\npoint-triangle tests: {int(n_cull)} of {int(n_all)} executed with culling ({100 * (1 - int(n_cull) / int(n_all)):.1f} % skipped)")
    assert int(n_all) == B * N * NF
    assert 0 < int(n_cull) < int(n_all)
    d_only, none_c, none_f = ops.point_mesh_distance(p, v, f, want_closest=False, want_face=False)
    assert none_c is None and none_f is None and torch.equal(d_only, full[0])


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_nearest_vertex_and_part_labels(case):
    from vistracker_amd import ops
    from vistracker_amd.boundary_sampler import BoundarySampler
    p, v = dev(case["points"]), dev(case["body"])
    vid, vd = (t.cpu().numpy() for t in ops.nearest_vertex(p, v))
    bs = BoundarySampler(case["labels"])
    _, _, _, _, parts = bs.compute_labels((dev(case["obj"]), dev(case["obj_faces"], torch.int32)), p, (v, dev(case["body_faces"], torch.int32)))
    parts = parts.cpu().numpy()
    near = 0
    for b in range(len(case["points"])):
        idx, d, other = M.nearest_vertex(case["points"][b], case["body"][b], second_labels=case["labels"])
        _, d32 = M.nearest_vertex(case["points"][b], case["body"][b], dtype=np.float32)
        e32 = float(np.abs(d32.astype(np.float64) - d).max())
        err = float(np.abs(vd[b] - d).max())
        print(f"\nframe {b}: nearest vertex e32 = {e32:.3e}, kernel |vert_dist - model| max = {err:.3e}")
        assert err <= 4 * e32
        np.testing.assert_allclose(np.linalg.norm(case["points"][b].astype(np.float64) - case["body"][b][vid[b]], axis=1), vd[b], atol=4 * e32)
        margin = (other - d) <= 1e-4 * d                                         # a vertex of another part as near as the nearest, within 1e-4 relative
        near += int(margin.sum())
        assert (parts[b][~margin] == case["labels"][idx][~margin]).all()
        assert (parts[b] == case["labels"][vid[b]]).all()
    print(f"points within 1e-4 relative of a part border: {near} of {parts.size}")
    assert near <= 0.01 * parts.size
    assert parts.dtype == np.int32


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_shapes_at_the_edges(case):
    from vistracker_amd import ops
    # NF = 1: the seven regions of one triangle, closed form
    q, want = seven_queries()
    dist, closest, face = (t.cpu().numpy() for t in ops.point_mesh_distance(dev(q), dev(TRI), dev([[0, 1, 2]], torch.int32)))
    np.testing.assert_allclose(closest, want, atol=1e-6)
    np.testing.assert_allclose(dist, np.linalg.norm(q - want, axis=1), atol=1e-6)
    assert (face == 0).all() and np.isfinite(dist).all()
    # N = 257 (one lane into a second workgroup) on B = 3 poses of the object, frame 1 moved by 1 m: frame b must use mesh b
    of = case["obj_faces"]; f = dev(of, torch.int32)
    verts = np.stack([case["obj"][0], case["obj"][0] + np.float32([1, 0, 0]), case["obj"][0]])
    pts = np.repeat(case["points"][:1, :257], 3, 0)
    ref, e32 = model_reference(pts, verts, of)
    d3, c3, f3 = ops.point_mesh_distance(dev(pts), dev(verts), f)
    err = np.abs(d3.cpu().numpy() - ref["dist"])
    print(f"\nN = 257, B = 3: e32 = {e32:.3e}, kernel max error {err.max():.3e}")
    assert err.max() <= 4 * e32
    assert torch.equal(d3[0], d3[2]) and torch.equal(c3[0], c3[2]) and torch.equal(f3[0], f3[2])
    assert np.abs(ref["dist"][1] - ref["dist"][0]).max() > 0.5                    # the distances moved with the mesh ...
    assert not torch.equal(d3[0], d3[1])
    vid3, vd3 = ops.nearest_vertex(dev(pts), dev(verts))
    # ... and a frame computed alone (B = 1, with and without the frame axis) is bit-identical to the same frame inside the batch
    for b in range(3):
        d1, c1, f1 = ops.point_mesh_distance(dev(pts[b:b + 1]), dev(verts[b:b + 1]), f)
        assert torch.equal(d1[0], d3[b]) and torch.equal(c1[0], c3[b]) and torch.equal(f1[0], f3[b])
        vid1, vd1 = ops.nearest_vertex(dev(pts[b]), dev(verts[b]))
        assert vid1.shape == (257,) and torch.equal(vid1, vid3[b]) and torch.equal(vd1, vd3[b])
    d0, c0, f0 = ops.point_mesh_distance(dev(pts[1]), dev(verts[1]), f)
    assert d0.shape == (257,) and c0.shape == (257, 3) and f0.shape == (257,)
    assert torch.equal(d0, d3[1]) and torch.equal(c0, c3[1])
    # N = 1
    d, c, fi = ops.point_mesh_distance(dev(pts[:, :1]), dev(verts), f)
    assert d.shape == (3, 1) and torch.equal(d[:, 0], d3[:, 0]) and torch.equal(c[:, 0], c3[:, 0]) and torch.equal(fi[:, 0], f3[:, 0])
    vid, vd = ops.nearest_vertex(dev(pts[:, :1]), dev(verts))
    assert torch.equal(vid[:, 0], vid3[:, 0]) and torch.equal(vd[:, 0], vd3[:, 0])


def test_bad_arguments_are_errors():
    from vistracker_amd import _lib as L, ops
    v = dev(TRI); q = dev(np.zeros((4, 3)))
    with pytest.raises(L.VtError):
        ops.point_mesh_distance(q, v, dev([[0, 1, 3]], torch.int32))             # a vertex index past the end
    with pytest.raises(L.VtError):
        ops.point_mesh_distance(q, v, dev([[0, -1, 2]], torch.int32))
    with pytest.raises(L.VtError):
        ops.point_mesh_distance(q[None], v, dev([[0, 1, 2]], torch.int32))       # a frame axis on one side only
    with pytest.raises(L.VtError):
        ops.point_mesh_distance(torch.zeros(4, 3), torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))     # host tensors: no CPU path
    assert L.lib().vt_point_mesh_workspace_bytes(0, 5) == -1 and L.lib().vt_point_mesh_workspace_bytes(2, 5) == 2 * 5 * 64


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------------------------
def mesh_area(v, f):
    t = v[f].astype(np.float64)
    return 0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1).sum()


def test_sampler(case, synth):
    from vistracker_amd import ops
    from vistracker_amd.boundary_sampler import BoundarySampler
    bs = BoundarySampler(case["labels"], seed=5)
    smpl = (dev(case["body"]), dev(case["body_faces"], torch.int32)); obj = (dev(case["obj"]), dev(case["obj_faces"], torch.int32))
    n, ratio = 2000, 0.01
    a = bs.boundary_sampling(smpl, obj, sigma=1e-5, sample_num=n, grid_ratio=ratio)
    again = bs.boundary_sampling(smpl, obj, sigma=1e-5, sample_num=n, grid_ratio=ratio)
    samples, d_h, d_o, parts, n_h, n_o = a
    n_grid = int(ratio * n)
    assert tuple(samples.shape) == (3, n + n_grid, 3) and tuple(d_h.shape) == (3, n + n_grid) and tuple(n_o.shape) == (3, n + n_grid, 3)
    assert parts.dtype == torch.int32 and d_o.dtype == torch.float32
    for x, y in zip(a, again):
        assert torch.equal(x, y)                                                 # the same seed: the same bits
    other = bs.boundary_sampling(smpl, obj, sigma=1e-5, sample_num=n, grid_ratio=ratio, generator=6)
    assert not torch.equal(other[0], samples)
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    with_g = bs.boundary_sampling(smpl, obj, sigma=1e-5, sample_num=n, grid_ratio=ratio, generator=g)
    assert torch.equal(with_g[0], samples)
    # a frame's samples and labels do not depend on the batch it sits in
    one = bs.boundary_sampling((smpl[0][1], smpl[1]), (obj[0][1], obj[1]), sigma=1e-5, sample_num=n, grid_ratio=ratio, keys=[1])
    pair = bs.boundary_sampling((smpl[0][1:], smpl[1]), (obj[0][1:], obj[1]), sigma=1e-5, sample_num=n, grid_ratio=ratio, keys=[1, 2])
    for x, y, z in zip(a, one, pair):
        assert x.shape[1:] == y.shape and torch.equal(x[1], y) and torch.equal(x[1:], z)
    # the box points
    bmin, bmax = (torch.as_tensor(x, dtype=torch.float32, device="cuda") for x in bs.get_bounds())
    grid = samples[:, n:]
    assert grid.shape[1] == n_grid and bool((grid >= bmin).all()) and bool((grid <= bmax).all())
    # area-weighted over both meshes: the share of surface samples on the object (nearer to it than to the body) is its share of the area
    for b in range(3):
        p_obj = mesh_area(case["obj"][b], case["obj_faces"]) / (mesh_area(case["obj"][b], case["obj_faces"]) + mesh_area(case["body"][b], case["body_faces"]))
        k = int((d_o[b, :n] < d_h[b, :n]).sum())
        sd = np.sqrt(n * p_obj * (1 - p_obj))
        print(f"\nframe {b}: {k} of {n} surface samples on the object, expected {n * p_obj:.1f} +- {sd:.1f}")
        assert abs(k - n * p_obj) <= 4 * sd
        assert float(torch.minimum(d_o[b, :n], d_h[b, :n]).max()) < 1e-3          # sigma = 1e-5: every surface sample is on a surface
    # equal_sample: exactly n // 2 on each mesh, the body first
    eq = bs.boundary_sampling(smpl, obj, sigma=1e-6, sample_num=n + 1, grid_ratio=ratio, equal_sample=True)
    assert eq[0].shape[1] == 2 * ((n + 1) // 2) + int(ratio * (n + 1))
    assert float(eq[1][:, :n // 2].max()) < 1e-4 and float(eq[2][:, n // 2:n].max()) < 1e-4
    assert int((eq[1][:, n // 2:n] < 1e-4).sum()) < 0.05 * n and int((eq[2][:, :n // 2] < 1e-4).sum()) < 0.05 * n
    # boundary_sample_all: the reference's keys, shapes and dtypes
    lm = ops.LandmarkHandle(synth["regs"]["body25"])
    out = bs.boundary_sample_all(lm, smpl, obj, sigmas=[0.08, 0.02], ratios=[0.01, 0.99], sample_num=2048)
    assert set(out) == {"points", "dist_h", "dist_o", "parts", "pca_axis", "smpl_center", "body_kpts", "obj_center"}
    counts = {"sigma0.08": 1024 + 64, "sigma0.02": 2027 + 126}                   # get_sample_num(r, 2048, thres=1024) + int(n / 16)
    for key, dt, tail in (("points", np.float32, (3,)), ("dist_h", np.float32, ()), ("dist_o", np.float32, ()), ("parts", np.uint8, ())):
        assert set(out[key]) == set(counts)
        for s, cnt in counts.items():
            assert out[key][s].dtype == dt and out[key][s].shape == (3, cnt) + tail
    assert out["pca_axis"].shape == (3, 3, 3) and out["pca_axis"].dtype == np.float32
    assert out["smpl_center"].shape == (3, 3) and out["body_kpts"].shape == (3, 25, 3) and out["body_kpts"].dtype == np.float32
    assert out["obj_center"].shape == (3, 3) and out["obj_center"].dtype == np.float32
    np.testing.assert_allclose(out["obj_center"], case["obj"].mean(1), atol=1e-5)
    np.testing.assert_array_equal(out["smpl_center"], out["body_kpts"][:, 8])
    assert out["parts"]["sigma0.02"].max() < 14
    single = bs.boundary_sample_all(lm, (smpl[0][0], smpl[1]), (obj[0][0], obj[1]), sigmas=[0.08, 0.02], ratios=[0.01, 0.99], sample_num=2048, flip=True,
                                    add_neighbours=True)
    assert set(single) == set(out) | {"neighbours_h", "neighbours_o"}
    assert single["points"]["sigma0.02"].shape == (2153, 3) and single["neighbours_h"]["sigma0.02"].shape == (2153, 3)
    assert single["pca_axis"].shape == (3, 3) and single["smpl_center"].shape == (3,) and single["body_kpts"].shape == (25, 3)
    np.testing.assert_array_equal(single["points"]["sigma0.02"], out["points"]["sigma0.02"][0])
    np.testing.assert_array_equal(single["parts"]["sigma0.02"], bs.flip_part_labels(out["parts"]["sigma0.02"][0]))


def test_sampler_generator_object_is_only_read(case, synth):
    """a torch.Generator passed in is read for its seed and never reseeded: with two sigmas, frame k alone (keys=[k]) and inside a batch (keys=[k, k+1]) gets
    the same bits for EVERY sigma, and a second call with the same object repeats the first"""
    from vistracker_amd import ops
    from vistracker_amd.boundary_sampler import BoundarySampler
    bs = BoundarySampler(case["labels"], seed=1)
    sv, sf = dev(case["body"]), dev(case["body_faces"], torch.int32); ov, of = dev(case["obj"]), dev(case["obj_faces"], torch.int32)
    lm = ops.LandmarkHandle(synth["regs"]["body25"])
    g = torch.Generator(device="cuda"); g.manual_seed(1234)
    state = g.get_state().clone()
    kw = dict(sigmas=[0.08, 0.02], ratios=[0.5, 0.5], sample_num=512, add_neighbours=True, generator=g)
    k = 7
    alone = bs.boundary_sample_all(lm, (sv[1:2], sf), (ov[1:2], of), keys=[k], **kw)
    batch = bs.boundary_sample_all(lm, (sv[1:3], sf), (ov[1:3], of), keys=[k, k + 1], **kw)
    again = bs.boundary_sample_all(lm, (sv[1:3], sf), (ov[1:3], of), keys=[k, k + 1], **kw)
    assert g.initial_seed() == 1234 and torch.equal(g.get_state(), state)
    for name in ("points", "dist_h", "dist_o", "parts", "neighbours_h", "neighbours_o"):
        for s in ("sigma0.08", "sigma0.02"):
            np.testing.assert_array_equal(alone[name][s][0], batch[name][s][0], err_msg=f"{name} {s}")
            np.testing.assert_array_equal(again[name][s], batch[name][s], err_msg=f"{name} {s}")
    assert not np.array_equal(batch["points"]["sigma0.02"][0], batch["points"]["sigma0.02"][1])
    assert not np.array_equal(batch["points"]["sigma0.08"][0][:256], batch["points"]["sigma0.02"][0][:256])      # each sigma its own stream
    # the int seed and the Generator with that seed are the same base; another seed is another stream
    by_int = bs.boundary_sample_all(lm, (sv[1:2], sf), (ov[1:2], of), keys=[k], **{**kw, "generator": 1234})
    np.testing.assert_array_equal(by_int["points"]["sigma0.02"], alone["points"]["sigma0.02"])
    other = bs.boundary_sample_all(lm, (sv[1:2], sf), (ov[1:2], of), keys=[k], **{**kw, "generator": 1235})
    assert not np.array_equal(other["points"]["sigma0.02"], alone["points"]["sigma0.02"])
    # boundary_sampling twice with one Generator: the same base both times
    a = bs.boundary_sampling((sv[:1], sf), (ov[:1], of), sample_num=300, generator=g)
    b = bs.boundary_sampling((sv[:1], sf), (ov[:1], of), sample_num=300, generator=g)
    assert torch.equal(a[0], b[0])
