"""CPU: the numpy restatement of point-to-plane ICP and of the normals (tests/icp_plane_reference.py) is what it claims to
be -- its step is the least-squares solution of its stacked rows, it recovers a small offset on noiseless planes in one
step, it converges faster than point-to-point on the demo pairs, and it leaves the pose where the fit is degenerate."""
import math

import numpy as np
import pytest

import icp_plane_reference as pr
import icp_reference as ir

DEMO = (("local_642", 2048), ("global_c", 2048), ("dso_9000", 1024))


@pytest.fixture(scope="module")
def demo():
    out = {}
    for name, n in DEMO:
        a, y, gt, Rt0 = ir.demo_pair(name, n, 1)
        out[name] = (a, y, gt, Rt0, pr.demo_normals(a, 16))
    return out


def _box(rng, n):
    """n points on the six faces of a 10 x 8 x 6 m box around the origin, with the faces' inward normals."""
    half = np.array([5.0, 4.0, 3.0])
    face = rng.integers(0, 6, n)
    p = (rng.random((n, 3)) * 2.0 - 1.0) * half
    nrm = np.zeros((n, 3))
    ax, sg = face // 2, np.where(face % 2 == 0, -1.0, 1.0)
    p[np.arange(n), ax] = sg * half[ax]
    nrm[np.arange(n), ax] = -sg
    return p.astype(np.float32), nrm.astype(np.float32)


def test_step_is_the_least_squares_solution_of_its_rows(demo):
    for name, _ in DEMO:
        a, y, _, Rt0, nrm = demo[name]
        nn = ir.associate(a, y, Rt0, 1.0)[0]
        _, rows, r, _ = pr.rows(a, nrm, y, nn, Rt0)
        new, info = pr.fit_plane(a, nrm, y, nn, Rt0)
        assert new is not None and info["n_pl"] == len(rows) > 100
        ls = np.linalg.lstsq(rows, r, rcond=None)[0]
        assert np.abs(info["s"] - ls).max() < 1e-10, (name, np.abs(info["s"] - ls).max())
        assert info["cond"] < 1e6 and info["pivot"] > 1e-6


def test_one_step_on_noiseless_planes():
    rng = np.random.default_rng(5)
    a, nrm = _box(rng, 3000)
    y_anchor_frame, _ = _box(rng, 1500)
    R, t = ir.rotation((0.3, -0.5, 1.0), 0.7), np.array([1.5, -2.0, 0.5])
    gt = np.concatenate([R, t[:, None]], axis=1)
    y = (y_anchor_frame.astype(np.float64) - t) @ R                    # exact in float64; the fit sees its float32 rounding
    off = np.concatenate([ir.rotation((1.0, 2.0, -1.0), math.radians(0.01)) @ R, (t + np.array([6e-4, -6e-4, 5e-4]))[:, None]], axis=1)
    # the nearest anchor of a point 1 mm off a face lies on that face (the faces' own points are decimetres apart), except
    # within that distance of an edge: pair by the true face instead, so that every residual is the plane's
    m = ir.move(off, y.astype(np.float32))
    nn = ir.associate(a, y.astype(np.float32), off, 1.0)[0]
    same_face = (np.abs((a[np.maximum(nn, 0)].astype(np.float64) - ir.move(gt, y.astype(np.float32))) * nrm[np.maximum(nn, 0)]).sum(axis=1) < 1e-5)
    nn = np.where(same_face, nn, -1).astype(np.int32)
    assert (nn >= 0).sum() > 1000 and m.shape == (1500, 3)
    new, info = pr.fit_plane(a, nrm, y.astype(np.float32), nn, off)
    dt, ddeg = ir.pose_errors(new, gt)
    # the linearisation's error is second order in the offset (1e-3 m, 1.7e-4 rad over 6 m: ~1e-7), float32 positives add
    # 2^-24 * 8 m / sqrt(pairs)
    assert dt < 1e-6 and math.radians(ddeg) < 1e-6, (dt, ddeg)
    assert np.abs(new[:, :3] @ new[:, :3].T - np.eye(3)).max() < 1e-14


def test_plane_converges_faster_than_point(demo):
    for name, _ in DEMO:
        a, y, gt, Rt0, nrm = demo[name]
        point = ir.icp(a, y, Rt0, max_dist=1.0, iterations=10)
        plane = pr.icp_plane(a, nrm, y, Rt0, max_dist=1.0, iterations=10)
        e_point = ir.pose_errors(point["states"][10]["Rt"], gt)[0]
        e_plane = ir.pose_errors(plane["states"][10]["Rt"], gt)[0]
        print(name, "point", e_point, "plane", e_plane, "cond", plane["cond"], "pivot", plane["pivot"])
        assert e_plane < 0.5 * e_point, (name, e_plane, e_point)
        assert plane["cond"] <= 1e6 and plane["pivot"] >= 1e-6
        st = plane["states"][10]
        assert st["num_plane"] == st["num_corr"] > 500 and st["rmse_plane"] < st["rmse"]


def test_clear_pair_plane_is_a_short_search():
    pair, nrm, run, seed = pr.clear_pair_plane("dso_9000", 1024, 1.0, 5)
    assert seed <= 3 and nrm.dtype == np.float32 and len(run["states"]) == 6


def test_degenerate_fits_leave_the_pose(demo):
    a, y, gt, Rt0, nrm = demo["dso_9000"]
    near = ir.move(gt, y).astype(np.float32)
    few = pr.icp_plane(near, nrm, y, gt, iterations=3, na=5, nb=5)      # five pairs
    assert few["states"][0]["num_plane"] == 5
    zero = pr.icp_plane(a, np.zeros_like(nrm), y, Rt0, iterations=3)
    assert zero["states"][3]["num_plane"] == 0 and math.isnan(zero["states"][3]["rmse_plane"]) and zero["states"][3]["num_corr"] > 100
    par = np.zeros_like(nrm)
    par[:, 2] = 1.0
    flat = a.copy()
    flat[:, 2] = 0.5                                                    # a coplanar anchor under parallel normals: rank 3
    yflat = y.copy()
    parallel = pr.icp_plane(flat, par, yflat, Rt0, iterations=3, max_dist=5.0)
    assert parallel["states"][0]["num_plane"] > 100
    for run in (few, zero, parallel):
        for st in run["states"]:
            assert np.array_equal(st["Rt"], run["states"][0]["Rt"])
    new, info = pr.fit_plane(flat, par, yflat, parallel["states"][0]["nn"], Rt0)
    assert new is None and info["pivot"] <= 1e-12


def test_normals_restatement_on_a_plane_and_its_margins(demo):
    rng = np.random.default_rng(6)
    x = np.concatenate([rng.random((300, 2)) * 4.0, np.full((300, 1), 2.5)], axis=1).astype(np.float32)
    nb = pr.knn_ids(x, 8)
    up = pr.normals(x, nb, viewpoint=(0.0, 0.0, 10.0))
    down = pr.normals(x, nb, viewpoint=(0.0, 0.0, 0.0))
    assert np.abs(up["normals"] - (0, 0, 1)).max() < 1e-15 and np.abs(down["normals"] - (0, 0, -1)).max() < 1e-15
    assert np.abs(up["curvature"]).max() < 1e-15
    # the margins the GPU comparison rests on: at k = 16 every demo point has an eigen gap of 1e-3 and an orientation margin
    # of 1e-6 (the issue measured none below the gap and 1.3e-4 as the smallest margin)
    for name, n in DEMO:
        a = demo[name][0]
        r = pr.normals(a, pr.knn_ids(a, 16))
        assert (r["gap"] < 1e-3).sum() == 0 and r["margin"].min() > 1e-5, (name, r["gap"].min(), r["margin"].min())
        assert np.abs(np.linalg.norm(r["normals"], axis=1) - 1.0).max() < 1e-12
