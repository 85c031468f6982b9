"""CPU: the numpy restatement of dh3d_icp_refine_gicp (tests/gicp_reference.py) against independent statements of the same
fit -- the whitened least-squares problem solved by np.linalg.lstsq with M from np.linalg.inv, the isotropic limit, the
sign of the normals, a noise-free recovery -- its two summation orders against each other, the demo pairs, and the corners
of the rule."""
import numpy as np
import pytest

import gicp_reference as gr
import icp_plane_reference as pr
import icp_reference as ir

N = 1024


@pytest.fixture(scope="module")
def pair():
    a, y, gt, Rt0 = ir.demo_pair("local_642", N, 1)
    return dict(a=a, y=y, gt=gt, Rt0=Rt0, an=pr.demo_normals(a), bn=pr.demo_normals(y))


def _assoc(p, Rt):
    return ir.associate(p["a"], p["y"], Rt, 1.0)[0]


def test_one_step_is_the_whitened_least_squares_solution(pair):
    """s of F_gicp minimises sum (J s - d)^T M (J s - d): the lstsq solution of the stacked rows chol(M)^T [J | d], with M the
    np.linalg.inv of the covariance sum built from outer products."""
    p, Rt, eps = pair, pair["Rt0"], 1e-3
    nn = _assoc(p, Rt)
    new, info = gr.fit_gicp(p["a"], p["an"], p["y"], p["bn"], nn, Rt, eps)
    assert new is not None and info["n_g"] > 300
    j = np.nonzero(nn >= 0)[0]
    m = ir.move(Rt, p["y"][j])
    d = p["a"][nn[j]].astype(np.float64) - m
    J = gr.jacobian(m, m.sum(axis=0) / len(j))

    def covm(v):
        s = v @ v
        return np.eye(3) - ((1.0 - eps) / s) * np.outer(v, v) if s > 0 else np.eye(3)

    rows, rhs = [], []
    for k in range(len(j)):
        W = covm(p["an"][nn[j[k]]].astype(np.float64)) + covm(Rt[:, :3] @ p["bn"][j[k]].astype(np.float64))
        Lc = np.linalg.cholesky(np.linalg.inv(W))
        rows.append(Lc.T @ J[k])
        rhs.append(Lc.T @ d[k])
    s = np.linalg.lstsq(np.concatenate(rows), np.concatenate(rhs), rcond=None)[0]
    assert np.abs(info["s"] - s).max() <= 1e-9 * np.abs(s).max(), (info["s"], s)
    assert info["det"] >= 8 * eps ** 3 * (1 - 1e-9)


def test_zero_normals_give_half_the_identity(pair):
    p, Rt = pair, pair["Rt0"]
    nn = _assoc(p, Rt)
    zero = np.zeros_like(p["an"])
    _, _, _, M, det, planar = gr.pairs(p["a"], zero, p["y"], zero, nn, Rt, 1e-3)
    assert np.array_equal(M, np.broadcast_to(np.eye(3) / 2.0, M.shape)) and np.array_equal(det, np.full(len(M), 8.0))
    assert not planar.any()
    # ... and so does epsilon = 1 with any normals, up to the rounding of n n^T / (n . n) * 0
    _, _, _, M1, _, planar1 = gr.pairs(p["a"], p["an"], p["y"], p["bn"], nn, Rt, 1.0)
    assert np.array_equal(M1, np.broadcast_to(np.eye(3) / 2.0, M1.shape)) and planar1.all()
    assert gr.gicp_stats(p["a"], zero, p["y"], zero, nn, Rt)[0] == 0
    # the isotropic rmse_gicp is the point-to-point rmse over sqrt(2)
    st = gr.icp_gicp(p["a"], zero, p["y"], zero, Rt, iterations=0)["states"][0]
    assert abs(st["rmse_gicp"] - st["rmse"] / np.sqrt(2.0)) < 1e-12


def test_the_sign_of_a_normal_changes_nothing(pair):
    p = pair
    rng = np.random.default_rng(3)
    fa, fb = rng.choice([-1.0, 1.0], N).astype(np.float32), rng.choice([-1.0, 1.0], N).astype(np.float32)
    one = gr.icp_gicp(p["a"], p["an"], p["y"], p["bn"], p["Rt0"], iterations=3)
    two = gr.icp_gicp(p["a"], p["an"] * fa[:, None], p["y"], p["bn"] * fb[:, None], p["Rt0"], iterations=3)
    for s1, s2 in zip(one["states"], two["states"]):
        assert np.array_equal(s1["Rt"], s2["Rt"]) and s1["rmse_gicp"] == s2["rmse_gicp"] and s1["num_planar"] == s2["num_planar"]


def test_a_noise_free_copy_returns_to_the_truth():
    a, _, gt, Rt0 = ir.demo_pair("local_642", N, 2, off_t=0.3, off_deg=1.5)
    y = ((a.astype(np.float64) - gt[:, 3]) @ gt[:, :3]).astype(np.float32)   # R^T (a - t): the same points, moved
    an = pr.demo_normals(a)
    bn = (an.astype(np.float64) @ gt[:, :3]).astype(np.float32)
    run = gr.icp_gicp(a, an, y, bn, Rt0, iterations=15)
    dt, ddeg = ir.pose_errors(run["states"][-1]["Rt"], gt)
    assert dt < 1e-4 and ddeg < 1e-3, (dt, ddeg)
    assert run["states"][-1]["num_corr"] == N and run["states"][-1]["rmse"] < 1e-4


@pytest.mark.parametrize("name,n", [("local_642", 2048), ("global_c", 2048), ("dso_9000", 1024)])
def test_demo_pairs_are_clear_and_improve(name, n):
    a, y, gt, Rt0 = ir.demo_pair(name, n, 1)
    run = gr.icp_gicp(a, pr.demo_normals(a), y, pr.demo_normals(y), Rt0, iterations=6, epsilon=1e-3)
    assert gr.is_clear(run), {k: run[k] for k in ("gap", "thr", "cond", "pivot", "refused", "det")}
    assert run["det"] >= 8e-9 * (1 - 1e-9)
    e0, e1 = ir.pose_errors(Rt0, gt)[0], ir.pose_errors(run["states"][-1]["Rt"], gt)[0]
    assert e1 < 0.5 * e0, (e0, e1)


def test_the_two_summation_orders_agree(pair):
    p = pair
    one = gr.icp_gicp(p["a"], p["an"], p["y"], p["bn"], p["Rt0"], iterations=4, nb=777)
    two = gr.icp_gicp(p["a"], p["an"], p["y"], p["bn"], p["Rt0"], iterations=4, nb=777, order="tree")
    for s1, s2 in zip(one["states"], two["states"]):
        assert np.array_equal(s1["nn"], s2["nn"]) and np.abs(s1["Rt"] - s2["Rt"]).max() < 1e-11
    v = np.random.default_rng(0).standard_normal((1001, 3))
    assert np.abs(gr.total(v, "tree") - v.sum(axis=0)).max() < 1e-12 and gr.total(v[:0], "tree").shape == (3,)


def test_corners(pair):
    p = pair
    near = ir.move(p["gt"], p["y"]).astype(np.float32)
    nnear = pr.demo_normals(near)
    for n in (1, 2):                                               # n_g < 3: the pose stays
        run = gr.icp_gicp(near, nnear, p["y"], p["bn"], p["gt"], iterations=2, na=n, nb=n)
        assert all(np.array_equal(s["Rt"], p["gt"]) for s in run["states"]) and run["states"][0]["num_corr"] == n
    run = gr.icp_gicp(near, nnear, p["y"], p["bn"], p["gt"], iterations=2, na=3, nb=3)
    assert not np.array_equal(run["states"][1]["Rt"], p["gt"]) and run["states"][0]["num_corr"] == 3
    # both clouds on one line: the rotation about it cannot be seen, a pivot is refused and the pose stays.  (A collinear
    # anchor alone does not do it: J is built from the moved positives.)
    line = np.zeros((64, 3), np.float32)
    line[:, 0] = np.linspace(-8.0, 8.0, 64)
    yl = ((line.astype(np.float64) - p["gt"][:, 3]) @ p["gt"][:, :3]).astype(np.float32)
    up = np.tile(np.float32([0, 0, 1]), (64, 1))
    run = gr.icp_gicp(line, up, yl, up, p["gt"], iterations=2)
    assert run["refused"] > -np.inf and run["refused"] <= 1e-12 and all(np.array_equal(s["Rt"], p["gt"]) for s in run["states"])
    # invalid pairs
    bad = p["Rt0"].copy()
    bad[1, 2] = np.inf
    for kw in (dict(Rt0=bad), dict(Rt0=p["Rt0"], valid0=False)):
        run = gr.icp_gicp(p["a"], p["an"], p["y"], p["bn"], kw["Rt0"], iterations=1, valid0=kw.get("valid0", True))
        st = run["states"][1]
        assert not run["valid"] and np.isnan(st["Rt"]).all() and (st["nn"] == -1).all() and st["num_planar"] == 0
        assert np.isnan(st["rmse_gicp"]) and st["num_corr"] == 0
    # nobody within max_dist
    run = gr.icp_gicp(p["a"], p["an"], p["y"] + np.float32(500.0), p["bn"], p["Rt0"], iterations=1)
    assert run["states"][1]["num_corr"] == 0 and np.isnan(run["states"][1]["rmse_gicp"]) and run["det"] == np.inf
