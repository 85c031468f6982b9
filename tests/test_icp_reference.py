"""CPU: the numpy restatement of dh3d_icp_refine (tests/icp_reference.py) does what ICP is for -- from a start 0.75 m /
3.2 degrees off it ends within 0.2 m / 0.5 degrees on disjoint 2 cm-noise subsets of the demo clouds -- keeps its own
special cases, and finds the neighbours that scipy's cKDTree finds."""
import numpy as np
import pytest

import icp_reference as ir

CASES = [("local_642", 2048), ("global_c", 2048), ("dso_9000", 1024)]


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name, n in CASES:
        pair = ir.demo_pair(name, n, 1)
        for md in (1.0, 2.0):
            out[name, md] = (pair, ir.icp(pair[0], pair[1], pair[3], max_dist=md, iterations=30))
    return out


@pytest.mark.parametrize("name,n", CASES)
@pytest.mark.parametrize("max_dist", [1.0, 2.0])
def test_converges_on_demo_subsets(runs, name, n, max_dist):
    (a, y, Rt_gt, Rt0), run = runs[name, max_dist]
    dt0, dd0 = ir.pose_errors(Rt0, Rt_gt)
    assert abs(dt0 - 0.75) < 1e-9 and abs(dd0 - 3.2) < 1e-6
    st = run["states"]
    assert len(st) == 31 and run["valid"]
    dt, dd = ir.pose_errors(st[30]["Rt"], Rt_gt)
    print(name, max_dist, "end", dt, dd, "rmse", st[1]["rmse"], st[30]["rmse"], "margins", run["gap"], run["thr"], run["eig"])
    assert dt < 0.2 and dd < 0.5, (dt, dd)
    assert st[30]["rmse"] <= st[1]["rmse"], (st[1]["rmse"], st[30]["rmse"])
    assert np.array_equal(st[0]["Rt"], Rt0)                       # iterations = 0 evaluates Rt0
    assert st[30]["num_corr"] == int((st[30]["nn"] >= 0).sum()) and st[30]["fitness"] == st[30]["num_corr"] / n


def test_zero_iterations_returns_the_start_pose():
    a, y, Rt_gt, Rt0 = ir.demo_pair("local_642", 512, 3)
    run = ir.icp(a, y, Rt0, iterations=0)
    assert len(run["states"]) == 1 and np.array_equal(run["states"][0]["Rt"], Rt0)
    nn = ir.associate(a, y, Rt0, 1.0)[0]
    assert np.array_equal(run["states"][0]["nn"], nn)


def test_a_cloud_against_itself_stays_at_the_identity():
    a = ir.demo_pair("local_642", 700, 4)[0]
    assert len(np.unique(a, axis=0)) == len(a)
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    run = ir.icp(a, a, eye, iterations=5)
    for st in run["states"]:
        assert np.array_equal(st["nn"], np.arange(len(a))) and st["num_corr"] == len(a)
        assert np.abs(st["Rt"] - eye).max() < 1e-12
    assert run["states"][0]["rmse"] == 0.0 and run["states"][5]["rmse"] < 1e-12


def test_counts_invalid_pairs_and_empty_associations():
    a, y, Rt_gt, Rt0 = ir.demo_pair("global_c", 256, 5)
    bad = Rt0.copy()
    bad[1, 2] = np.nan
    for run in (ir.icp(a, y, bad, iterations=2), ir.icp(a, y, Rt0, iterations=2, valid0=False)):
        assert not run["valid"] and len(run["states"]) == 3
        st = run["states"][2]
        assert np.isnan(st["Rt"]).all() and (st["nn"] == -1).all() and st["num_corr"] == 0 and st["fitness"] == 0.0
        assert np.isnan(st["rmse"])
    far = ir.icp(a, y + np.float32(500.0), Rt0, iterations=3)     # nothing within max_dist: the pose never moves
    st = far["states"][3]
    assert far["valid"] and st["num_corr"] == 0 and np.isnan(st["rmse"]) and np.array_equal(st["Rt"], Rt0)
    cut = ir.icp(a, y, Rt_gt, iterations=1, na=100, nb=77)
    st = cut["states"][1]
    assert (st["nn"][77:] == -1).all() and st["nn"].max() < 100 and st["fitness"] == st["num_corr"] / 77
    for na, nb in ((0, 50), (50, 0)):
        st = ir.icp(a, y, Rt_gt, iterations=1, na=na, nb=nb)["states"][1]
        assert st["num_corr"] == 0 and st["fitness"] == 0.0 and np.array_equal(st["Rt"], Rt_gt)


def test_duplicate_anchor_rows_tie_to_the_lowest_index():
    a, y, Rt_gt, _ = ir.demo_pair("local_642", 300, 6)
    a[200] = a[10]
    a[250] = a[10]
    y[0] = ((a[10].astype(np.float64) - Rt_gt[:, 3]) @ Rt_gt[:, :3]).astype(np.float32)
    nn, d2, gap, thr = ir.associate(a, y, Rt_gt, 1.0)
    assert nn[0] == 10 and gap > 0.0                              # bit-equal d2 is no gap: the index decides


def test_brute_force_agrees_with_ckdtree():
    spatial = pytest.importorskip("scipy.spatial")
    for name, n, md in (("local_642", 2048, 1.0), ("dso_9000", 1024, 2.0)):
        a, y, Rt_gt, Rt0 = ir.demo_pair(name, n, 1)
        nn, d2, gap, thr = ir.associate(a, y, Rt0, md)
        m = ir.move(Rt0, y)
        dist, idx = spatial.cKDTree(a.astype(np.float64)).query(m, k=1, distance_upper_bound=md)
        found = np.isfinite(dist)
        assert np.array_equal(found, nn >= 0)
        # the tree may name another of several bit-equal rows (dso_9000 has duplicates): compare the distances it found
        assert np.abs(np.sqrt(d2[found]) - dist[found]).max() < 1e-9
        same = a[idx[found]] == a[nn[found]]
        assert same.all()
