"""Host: the float64 contact model (tests/contact_model.py) against the reference's own ContactVisualizer.get_contact_spheres recorded in
tests/golden/contact.npz (tools/gen_golden_contact.py), the shares of vertices the GPU tests may exclude, and the two pieces of geometry the
feature restates on the host: the look-at transform of the top view and the icosphere of the contact spheres."""
import os

import numpy as np
import pytest

import contact_model as M
from vistracker_amd import visualize as V

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contact.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def test_model_matches_reference_fixture(gold):
    B = gold["smpl"].shape[0]
    touching = 0
    for b in range(B):
        r = M.regions(gold["smpl"][b], gold["labels"], gold["obj"][b], float(gold["thres"]))
        clear = ~r["near_tie"]
        np.testing.assert_array_equal(r["idx"][clear], gold["idx"][b][clear])          # the kd-tree's tie order is not pinned
        np.testing.assert_allclose(r["dist"], gold["dist"][b], rtol=0, atol=1e-12)
        np.testing.assert_array_equal(r["dist"] < float(gold["thres"]), gold["mask"][b])
        np.testing.assert_array_equal(r["part"][clear], gold["part"][b][clear])
        if not r["near_tie"].any():
            np.testing.assert_array_equal(r["count"], gold["count"][b])
            np.testing.assert_allclose(r["centre"], gold["centre"][b], rtol=0, atol=1e-12)
        touching += int(2 <= (gold["count"][b] > 0).sum() <= 4)
    assert touching == 3 and (gold["count"] > 0).any(1).sum() == 3                    # 2-4 parts in three frames, none in the fourth


def _shares(smpl, labels, obj, thres):
    tie = thr = 0
    for b in range(len(smpl)):
        r = M.regions(smpl[b], labels, obj[b], thres)
        tie += int(r["near_tie"].sum()); thr += int(r["near_thres"].sum())
    n = obj.shape[0] * obj.shape[1]
    return tie / n, thr / n


def test_near_case_shares_of_the_fixture(gold):
    tie, thr = _shares(gold["smpl"], gold["labels"], gold["obj"], float(gold["thres"]))
    print(f"fixture: near-tie share {tie:.5f}, near-threshold share {thr:.5f}")
    assert tie <= M.MAX_NEAR_SHARE and thr <= M.MAX_NEAR_SHARE


def test_near_case_shares_of_the_gpu_inputs(gold):
    sc = M.scene(M.BATCH_N, M.BATCH_TOUCH)
    tie, thr = _shares(sc["smpl"], sc["labels"], sc["obj"], 0.04)
    print(f"{M.BATCH_N}-frame case: near-tie share {tie:.5f}, near-threshold share {thr:.5f}")
    assert tie <= M.MAX_NEAR_SHARE and thr <= M.MAX_NEAR_SHARE
    # the fixture's inputs are this builder's too
    fx = M.scene(4, M.FIXTURE_TOUCH, M.FIXTURE_SEED)
    np.testing.assert_array_equal(fx["smpl"], gold["smpl"]); np.testing.assert_array_equal(fx["obj"], gold["obj"])


def test_model_ties_go_to_the_smaller_index():
    s = np.array([[1.0, 0, 0], [0, 1.0, 0], [-1.0, 0, 0], [0, 1.0, 0]])
    idx, d1, d2 = M.nearest(s, np.array([[0.0, 0, 0], [0, 2.0, 0]]))
    assert idx.tolist() == [0, 1] and d1.tolist() == [1.0, 1.0] and d2.tolist() == [1.0, 1.0]


def test_look_at_properties():
    for eye, at, up in [(V.TOP_EYE, V.TOP_AT, V.TOP_UP), ((1.0, 2.0, -3.0), (0.5, -1.0, 2.0), (0.0, 1.0, 0.2))]:
        R, T = V.look_at_view_transform(eye, at, up)
        assert R.dtype == np.float64 and T.dtype == np.float64
        np.testing.assert_allclose(R.T @ R, np.eye(3), atol=1e-14)
        assert abs(np.linalg.det(R) - 1.0) < 1e-14
        np.testing.assert_allclose(np.asarray(eye) @ R + T, 0, atol=1e-14)
        d = np.linalg.norm(np.asarray(at) - np.asarray(eye))
        np.testing.assert_allclose(np.asarray(at) @ R + T, [0, 0, d], atol=1e-14)
        Rm, Tm = M.look_at(eye, at, up)
        np.testing.assert_allclose(R, Rm, atol=1e-15); np.testing.assert_allclose(T, Tm, atol=1e-15)
    with pytest.raises(ValueError):
        V.look_at_view_transform((0, 0, 0), (0, 0, 1), (0, 0, 2))


def test_icosphere_properties():
    v, f = V.icosphere(2)
    assert v.shape == (162, 3) and f.shape == (320, 3) and v.dtype == np.float64
    assert np.abs(np.linalg.norm(v, axis=1) - 1).max() <= 1e-12
    edges = {tuple(sorted(e)) for t in f for e in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0]))}
    assert len(v) - len(edges) + len(f) == 2
    assert sorted(np.unique(f).tolist()) == list(range(162))
    tri = v[f]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    assert (np.einsum("ij,ij->i", n, tri.mean(1)) > 0).all()
    assert np.linalg.norm(n, axis=1).min() > 1e-3                                       # no sliver faces


def test_default_palette_is_distinct():
    c = V.PART_COLORS
    assert c.shape == (14, 3) and c.min() >= 0 and c.max() <= 1
    d = np.linalg.norm(c[:, None] - c[None], axis=-1) + 10 * np.eye(14)
    assert d.min() > 0.25
    for other in V.SMPL_OBJ_COLOR_LIST:
        assert np.linalg.norm(c - np.asarray(other), axis=1).min() > 0.2
