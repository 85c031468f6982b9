"""CPU: the numpy restatement of prepare_clouds (tests/prepare_reference.py) pinned independently -- its stage-2 counts
against scipy's kd-tree on the real clouds, its stage 1 against an np.unique grouping, its edge semantics on hand-made
points -- and the real clouds shown to exercise both stages."""
import os

import numpy as np
import pytest

import prepare_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REAL = ("local_268", "local_642", "dso_9000", "global_a", "global_b", "global_c")
EXPECTED = {"local_268": (16384, 14698, 14614), "dso_9000": (9000, 7687, 7201), "global_c": (8192, 7145, 7121)}


@pytest.fixture(scope="module")
def clouds():
    d = np.load(os.path.join(GOLDEN, "demo_clouds.npz"))
    return {k: np.ascontiguousarray(d[k], np.float32) for k in REAL}


def _unique_voxels(pts, voxel):
    """Stage 1 a second way: np.unique on the cell triples, np.add.at (unbuffered, in index order) for the sums."""
    cell = R.voxel_cells(pts, voxel).astype(np.int64)
    _, first, inv, cnt = np.unique(cell, axis=0, return_index=True, return_inverse=True, return_counts=True)
    sums = np.zeros((first.size, 3), np.float64)
    np.add.at(sums, inv.reshape(-1), pts.astype(np.float64))
    return (sums / cnt[:, None]).astype(np.float32)[np.argsort(first, kind="stable")]


@pytest.mark.parametrize("name", REAL)
def test_real_clouds_both_stages(clouds, name):
    from scipy.spatial import cKDTree
    pts = clouds[name]
    s1 = R.voxel_grid(pts, 0.2)
    assert np.array_equal(s1.view(np.int32), _unique_voxels(pts, 0.2).view(np.int32))
    tree = cKDTree(s1.astype(np.float64))
    inner = tree.query_ball_point(s1.astype(np.float64), 1.0 - 1e-9, return_length=True)
    outer = tree.query_ball_point(s1.astype(np.float64), 1.0 + 1e-9, return_length=True)
    assert np.array_equal(inner, outer), "a point within 1e-9 of a shell: the kd-tree cannot arbitrate"
    counts = R.radius_counts(s1, 1.0)
    assert np.array_equal(counts, tree.query_ball_point(s1.astype(np.float64), 1.0, return_length=True))
    keep = counts > 4
    n, v, m = pts.shape[0], s1.shape[0], int(keep.sum())
    assert n - v >= 0.05 * n, "stage 1 merges too little to be exercised"
    assert v - m >= 5, "stage 2 finds too few outliers to be exercised"
    if name in EXPECTED:
        assert (n, v, m) == EXPECTED[name]
    r = R.prepare_cloud(pts, 8192)
    assert tuple(r["counts"]) == (n, v, m) and r["num_valid"] == min(m, 8192)
    assert np.array_equal(r["stage2"], s1[keep])


def test_street_scene_and_random_cloud_against_the_kdtree():
    from scipy.spatial import cKDTree
    for pts in (R.street_scene(), np.random.default_rng(3).random((20000, 3), dtype=np.float32) * np.float32(12.0)):
        s1 = R.voxel_grid(pts, 0.2)
        assert np.array_equal(s1.view(np.int32), _unique_voxels(pts, 0.2).view(np.int32))
        tree = cKDTree(s1.astype(np.float64))
        q = s1.astype(np.float64)
        if np.array_equal(tree.query_ball_point(q, 1.0 - 1e-9, return_length=True),
                          tree.query_ball_point(q, 1.0 + 1e-9, return_length=True)):
            assert np.array_equal(R.radius_counts(s1, 1.0), tree.query_ball_point(q, 1.0, return_length=True))
    r = R.prepare_cloud(R.street_scene(), 16384)
    assert r["counts"][0] == 60300 and 16384 < r["counts"][2] < 65536 and r["counts"][1] - r["counts"][2] >= 100


def test_voxel_faces_origin_and_order():
    pts, kw = R.tie_cases()["voxel_faces"]
    cell = R.voxel_cells(pts, 0.25)
    # origin -0.125: 0.125 sits on the face between cells 0 and 1 and belongs to cell 1; one float below it, to cell 0
    assert cell[:, 0].tolist() == [0, 1, 0, 2, 1, 1, 0, 3, 2]
    assert cell[:, 1].tolist() == [0, 0, 0, 1, 0, 1, 0, 0, 2]
    s1 = R.voxel_grid(pts, 0.25)
    assert s1.shape == (7, 3)
    # voxel of points 0, 2 and 6 first (lowest member 0), then that of point 1, of point 3, ...
    p = pts.astype(np.float64)
    assert np.array_equal(s1[0], (((p[0] + p[2]) + p[6]) / 3.0).astype(np.float32))
    assert np.array_equal(s1[1], pts[1]) and np.array_equal(s1[2], pts[3])
    r = R.prepare_cloud(pts, **kw)
    assert r["num_valid"] == 7 and np.array_equal(r["points"][:7], s1) and (r["points"][7:] == R.PAD).all()


def test_strict_shell_and_more_than_nb_points():
    pts, kw = R.tie_cases()["shell_unit_lattice"]
    assert (R.radius_counts(pts, 1.0) == 1).all()              # neighbours at d2 == r2 exactly are outside
    r = R.prepare_cloud(pts, **kw)
    assert r["num_valid"] == 0 and tuple(r["counts"]) == (125, 125, 0) and (r["points"] == R.PAD).all()
    assert (r["centroid"] == 0).all()
    pts, kw = R.tie_cases()["shell_half_lattice"]
    c = R.radius_counts(pts, 1.0).reshape(6, 6, 6)
    assert c[0, 0, 0] == 8 and c[2, 2, 2] == 27 and c[0, 2, 2] == 18
    r = R.prepare_cloud(pts, **kw)                             # nb_points = 8: "more than", so the 8 corners go
    assert tuple(r["counts"]) == (216, 216, 208)
    assert R.prepare_cloud(pts, **dict(kw, nb_points=7))["counts"][2] == 216


def test_duplicates_and_crowded_voxels():
    pts, kw = R.tie_cases()["duplicates"]
    s1 = R.voxel_grid(pts, 0.2)
    assert np.array_equal(s1.view(np.int32), _unique_voxels(pts, 0.2).view(np.int32))
    assert (s1 == np.array([1.5, 2.5, -0.5], np.float32)).all(axis=1).sum() == 1    # 40 copies -> the point itself
    pts, kw = R.tie_cases()["duplicates_no_voxel"]
    assert R.radius_counts(pts, 1.0).min() >= 5                                     # a copy is a neighbour at d2 = 0
    pts, kw = R.tie_cases()["crowded_voxels"]
    cell = R.voxel_cells(pts, 0.2).astype(np.int64)
    sizes = np.unique(cell, axis=0, return_counts=True)[1]
    assert sizes.max() > 4096 and ((sizes > 16) & (sizes <= 4096)).any()
    assert np.array_equal(R.voxel_grid(pts, 0.2).view(np.int32), _unique_voxels(pts, 0.2).view(np.int32))


def test_fixed_size_branches():
    pts, kw = R.tie_cases()["m_equals_targetnum"]
    r = R.prepare_cloud(pts, **kw)
    assert r["num_valid"] == 216 and np.array_equal(r["points"], pts)               # m == targetnum: no pad, no crop
    pts, kw = R.tie_cases()["select_ties"]
    r = R.prepare_cloud(pts, **kw)
    d2 = ((pts.astype(np.float64) - r["centroid"]) ** 2).sum(axis=1)
    kept = R.select_nearest(pts, 100, r["centroid"])
    cut = np.sort(d2)[99]
    assert (d2[kept] <= cut).all() and (d2 == cut).sum() > (d2[kept] == cut).sum() > 0   # the tie is cut through
    on = np.flatnonzero(d2 == cut)
    assert np.array_equal(np.intersect1d(kept, on), on[:(d2[kept] == cut).sum()])   # its lowest indices win
    assert np.array_equal(r["points"], pts[kept]) and (np.diff(kept) > 0).all()
    pts, kw = R.tie_cases()["select_ties_first"]
    assert np.array_equal(R.prepare_cloud(pts, **kw)["points"], pts[:100])
    empty = R.prepare_cloud(np.zeros((0, 3), np.float32), 8)
    assert empty["num_valid"] == 0 and tuple(empty["counts"]) == (0, 0, 0) and (empty["points"] == R.PAD).all()
    one = R.prepare_cloud(np.ones((1, 3), np.float32), 8)
    assert tuple(one["counts"]) == (1, 1, 0) and one["num_valid"] == 0
    wide = R.prepare_cloud(np.array([[0, 0, 0], [1e6, 0, 0]], np.float32), 8)       # 5e6 cells of 0.2 on x
    assert tuple(wide["counts"]) == (2, -1, -1) and wide["num_valid"] == 0
