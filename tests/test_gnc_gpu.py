"""GPU: the graduated non-convexity pose fit (dh3d_amd.registration.gnc_rigid -> csrc/registration.hip gnc_kernel) against
the float64 restatement of include/dh3d_hip.h dh3d_gnc_rigid (tests/gnc_reference.py): equal counts, fit counts, masks and
validity, poses within 1e-9 and weights within that tolerance carried through a residual; rows read in place; determinism
and batch independence; no result from unwritten memory; graph capture; and the estimator= plumbing of register /
register_fpfh.  One batch of 21 pairs at Ma = Mb = 512 and one pair at 4096."""
import math

import numpy as np
import pytest
import torch

import gnc_reference as g
from poisoned_alloc import KINDS, poisoned

pytestmark = pytest.mark.gpu

POSE_TOLERANCE = 1e-9  # the project's tolerance for float64 poses against a numpy restatement
_REF = {}


def _t(dev, v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8),
                                                                     b.contiguous().reshape(-1).view(torch.uint8))


def _all_same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert (a[k] is None and b[k] is None) or _same_bits(a[k], b[k]), (what, k)  # (register_fpfh: anchor_ids None)


@pytest.fixture(scope="module")
def batch(dev):
    ax, bx, match, count, names, truth = g.edge_batch()
    return dict(ax=ax, bx=bx, match=match, count=count, names=names, truth=truth,
                dev=tuple(_t(dev, v) for v in (ax, bx, match, count)))


def _ref(key, raw, cfg):
    """The restatement on a raw batch (computed once per batch and configuration, never changed)."""
    key = (key,) + tuple(sorted(cfg.items()))
    if key not in _REF:
        _REF[key] = g.run_batch(*raw, **cfg)
    return _REF[key]


def _compare(got, refs, names, threshold):
    got = {k: v.cpu().numpy() for k, v in got.items()}
    M = got["inliers"].shape[1]
    worst_pose = worst_w = 0.0
    for p, (name, r) in enumerate(zip(names, refs)):
        rows, n = r["rows"], len(r["rows"])
        assert g.clear(r, threshold), name  # a condition on the fixture
        assert got["num_corr"][p] == n, (name, got["num_corr"][p], n)
        assert got["iterations"][p] == r["iterations"] == got["trials"][p], (name, got["iterations"][p], r["iterations"])
        assert bool(got["valid"][p]) == r["valid"], name
        assert got["num_inliers"][p] == r["num_inliers"], (name, got["num_inliers"][p], r["num_inliers"])
        mask = np.zeros(M, bool)
        mask[rows] = r["mask"]
        assert np.array_equal(got["inliers"][p], mask), name
        assert got["inlier_ratio"][p] == r["num_inliers"] / max(n, 1), name
        if r["valid"]:
            err = float(np.abs(got["Rt"][p] - r["Rt"]).max())
            worst_pose = max(worst_pose, err)
            assert err < POSE_TOLERANCE, (name, err)
        else:
            assert np.isnan(got["Rt"][p]).all(), name
        # the weights: the pose tolerance carried through a residual (1 + 3 * big, the centred coordinates' size) and the
        # weight's largest slope in the residual, 25 sqrt(5) / 54 / sqrt(mu) with mu >= threshold^2
        w = np.zeros(M)
        w[rows] = r["weights"]
        tol = POSE_TOLERANCE * (1.0 + 3.0 * r["big"]) * g.WEIGHT_SLOPE / threshold
        assert np.array_equal(np.isnan(got["weights"][p]), np.isnan(w)), name
        assert not got["weights"][p][np.setdiff1d(np.arange(M), rows)].any(), name
        if n:
            werr = float(np.nanmax(np.abs(got["weights"][p] - w), initial=0.0))
            worst_w = max(worst_w, werr / tol)
            assert werr <= tol, (name, werr, tol)
    print("worst pose error %.3g, worst weight error %.3g of its tolerance" % (worst_pose, worst_w))


@pytest.mark.parametrize("cfg", g.CONFIGS, ids=lambda c: ",".join("%s=%g" % kv for kv in sorted(c.items())))
def test_against_restatement(dev, batch, cfg):
    from dh3d_amd import registration as reg
    refs = _ref("edge", (batch["ax"], batch["bx"], batch["match"], batch["count"]), cfg)
    got = reg.gnc_rigid(*batch["dev"], **cfg)
    assert got["trials"] is got["iterations"]
    _compare(got, refs, batch["names"], cfg["threshold"])
    by_name = dict(zip(batch["names"], refs))
    for name in ("n_0", "n_1", "n_2", "all_unmatched"):
        assert by_name[name]["iterations"] == 0 and not by_name[name]["valid"]
    assert not by_name["one_nan"]["valid"] and by_name["one_nan"]["iterations"] > 0
    assert by_name["coincident"]["D2"] == 0.0 and by_name["coincident"]["valid"]
    assert len(by_name["count_300_of_512"]["rows"]) == 300 and 300 < len(by_name["ids_out_of_range"]["rows"]) < 512
    if cfg == dict(threshold=0.5):  # the outlier fixtures come back to the truth on the device too
        Rt = got["Rt"].cpu().numpy()
        for p, T in batch["truth"].items():
            dt, ddeg = g.pose_error(Rt[p], T)
            assert dt < 0.1 and ddeg < 0.5, (batch["names"][p], dt, ddeg)


def test_full_staging_pair(dev):
    """Ma = Mb = 4096 with every row a correspondence: the 112 KB staging, 16 rows a lane."""
    from dh3d_amd import registration as reg
    ax, bx, match, count, T = g.big_pair()
    cfg = dict(threshold=0.5)
    refs = _ref("big", (ax, bx, match, count), cfg)
    got = reg.gnc_rigid(_t(dev, ax), _t(dev, bx), _t(dev, match), _t(dev, count), **cfg)
    _compare(got, refs, ["big"], 0.5)
    dt, ddeg = g.pose_error(got["Rt"][0].cpu().numpy(), T)
    assert bool(got["valid"][0]) and dt < 0.1 and ddeg < 0.5, (dt, ddeg)


def test_rows_are_read_in_place(dev, batch):
    from dh3d_amd import registration as reg
    ax, bx, match, count = batch["dev"]
    P, M = match.shape
    wide_a = torch.full((P, M, 132), 7.0, device=dev)
    wide_b = torch.full((P, M, 132), -7.0, device=dev)
    wide_a[:, :, :3], wide_b[:, :, :3] = ax, bx
    plain = reg.gnc_rigid(ax, bx, match, count, threshold=0.5)
    _all_same(plain, reg.gnc_rigid(wide_a, wide_b, match, count, threshold=0.5), "keypoint rows")
    _all_same(plain, reg.gnc_rigid(wide_a[:, :, :3], wide_b[:, :, :3], match, count, threshold=0.5), "column views")


def test_determinism_and_batch_independence(dev, batch):
    from dh3d_amd import registration as reg
    ax, bx, match, count = batch["dev"]
    P = match.shape[0]
    full = reg.gnc_rigid(ax, bx, match, count, threshold=0.5)
    _all_same(full, reg.gnc_rigid(ax, bx, match, count, threshold=0.5), "second call")
    order = torch.from_numpy(np.random.default_rng(3).permutation(P)).to(dev)
    mixed = reg.gnc_rigid(ax[order], bx[order], match[order], count[order], threshold=0.5)
    _all_same({k: v[order] for k, v in full.items()}, mixed, "reordered")
    for p in range(P):
        one = reg.gnc_rigid(ax[p:p + 1], bx[p:p + 1], match[p:p + 1], count[p:p + 1], threshold=0.5)
        _all_same({k: v[p:p + 1] for k, v in full.items()}, one, batch["names"][p])


def test_no_result_depends_on_unwritten_memory(dev, batch):
    """Every output, weights and inliers past anchor_count and the pairs without a model included, is the plain run's bit
    for bit when every allocation starts from garbage; the call keeps no workspace."""
    from dh3d_amd import registration as reg
    import poisoned_alloc
    assert poisoned_alloc.WORKSPACE_CACHES == (("dh3d_amd.registration", "_ICP_WS"), ("dh3d_amd.registration", "_ISS_WS"))
    plain = reg.gnc_rigid(*batch["dev"], threshold=0.5)
    torch.cuda.synchronize()
    for kind in KINDS:
        with poisoned(kind):
            out = reg.gnc_rigid(*batch["dev"], threshold=0.5)
            torch.cuda.synchronize()
        _all_same(plain, out, kind)
        for t in out.values():  # the poisoned buffers go back to the allocator zeroed, not holding NaN / +-1e30
            t.zero_()
        torch.cuda.synchronize()


def test_graph_capture_replays_on_new_inputs(dev, batch):
    from dh3d_amd import registration as reg
    static = tuple(v.clone() for v in batch["dev"])
    # the eager call is the warm-up (it loads the kernel and sets its LDS cap): no stream of the test's own, so the
    # suite's later graph tests see the streams and the freed memory they would see without this test
    reg.gnc_rigid(*static, threshold=0.5)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gout = reg.gnc_rigid(*static, threshold=0.5)
    P = static[2].shape[0]
    for seed in (8, 9):
        order = torch.from_numpy(np.random.default_rng(seed).permutation(P)).to(dev)
        new = [v[order].contiguous() for v in batch["dev"]]
        new[3] = (new[3] - seed).clamp(min=0)  # other counts as well
        for s, v in zip(static, new):
            s.copy_(v)
        graph.replay()
        eager = reg.gnc_rigid(*new, threshold=0.5)
        torch.cuda.synchronize()
        _all_same(eager, gout, "replay %d" % seed)
    for t in gout.values():  # the graph's pool goes back zeroed
        t.zero_()
    torch.cuda.synchronize()


def _keypoint_rows(dev, P=4, M=256, D=128, outliers=0.4, seed=21):
    """Keypoint rows [x, y, z, descriptor, score] of P pairs: positives moved, permuted and noisy, with matching descriptors
    except for an outlier share whose anchors carry unrelated ones."""
    rng = np.random.default_rng(seed)
    ra, rb = np.zeros((P, M, 3 + D + 1), np.float32), np.zeros((P, M, 3 + D + 1), np.float32)
    T = []
    for p in range(P):
        x, y, Tp = g.outlier_fixture(seed + p, M, 0.0)
        da = rng.standard_normal((M, D)).astype(np.float32)
        da /= np.linalg.norm(da, axis=1, keepdims=True)
        db = da + 0.01 * rng.standard_normal((M, D)).astype(np.float32)
        out = rng.random(M) < outliers
        da[out] = rng.standard_normal((int(out.sum()), D)).astype(np.float32)
        da[out] /= np.linalg.norm(da[out], axis=1, keepdims=True)
        perm = rng.permutation(M)
        ra[p, :, :3], ra[p, :, 3:3 + D] = x, da
        rb[p, perm, :3], rb[p, perm, 3:3 + D] = y, db
        T.append(Tp)
    return _t(dev, ra), _t(dev, rb), np.stack(T)


def test_register_takes_the_estimator(dev):
    from dh3d_amd import registration as reg
    ra, rb, T = _keypoint_rows(dev)
    P, M = ra.shape[:2]
    cnt = torch.full((P,), M, dtype=torch.int32, device=dev)
    res = reg.register(ra, cnt, rb, cnt, estimator="gnc", threshold=0.5)
    ids, dist = reg.match_descriptors(ra[:, :, 3:131], cnt, rb[:, :, 3:131], cnt)
    exp = reg.gnc_rigid(ra, rb, ids, cnt, threshold=0.5)
    _all_same(exp, {k: res[k] for k in exp}, "register")
    assert _same_bits(res["match"], ids) and _same_bits(res["dist"], dist) and res["trials"] is res["iterations"]
    dt, ddeg = reg.transform_errors(T, res["Rt"], res["valid"])
    assert bool(res["valid"].all()) and (dt < 0.1).all() and (ddeg < 0.5).all(), (dt, ddeg)
    summary = reg.summarize_registration(dt, ddeg, res["inlier_ratio"], res["trials"])
    assert summary["success_rate"] == 100.0 and summary["mean_trials"] == float(res["iterations"].float().mean())
    # ... behind the ratio test and the mutual check
    opts = {"ratio": 0.9, "mutual": True}
    res2 = reg.register(ra, cnt, rb, cnt, match=opts, estimator="gnc", threshold=0.5)
    m2 = reg.match_descriptors2(ra[:, :, 3:131], cnt, rb[:, :, 3:131], cnt, **opts)
    exp2 = reg.gnc_rigid(ra, rb, m2["match"], cnt, threshold=0.5)
    _all_same(exp2, {k: res2[k] for k in exp2}, "register behind the filters")
    assert _same_bits(res2["match"], m2["match"]) and _same_bits(res2["num_kept"], m2["num_kept"])
    assert int(res2["num_corr"].sum()) < int(res["num_corr"].sum())
    # the default estimator is RANSAC, named or not
    _all_same(reg.register(ra, cnt, rb, cnt, seed=5), reg.register(ra, cnt, rb, cnt, estimator="ransac", seed=5), "ransac")
    with pytest.raises(ValueError, match='estimator="gnc"'):
        reg.register(ra, cnt, rb, cnt, estimator="gnc", seed=5)
    with pytest.raises(ValueError, match='estimator="ransac"'):
        reg.register(ra, cnt, rb, cnt, division=2.0)


def test_register_fpfh_takes_the_estimator(dev):
    """A 1024-point demo cloud against a moved, permuted copy with 2 cm of noise."""
    import icp_reference as ir
    from dh3d_amd import registration as reg
    N, sigma = 1024, 0.02
    rng = np.random.default_rng(78)
    a, _, Rt, _ = ir.demo_pair("local_642", N, 1)
    y = ((a.astype(np.float64) - Rt[:, 3]) @ Rt[:, :3] + rng.normal(0.0, sigma, a.shape))[rng.permutation(N)].astype(np.float32)
    A, B = _t(dev, a[None]), _t(dev, y[None])
    ransac = reg.register_fpfh(A, B)
    gnc = reg.register_fpfh(A, B, estimator="gnc")
    assert set(gnc) == set(ransac) | {"weights", "iterations"}
    _all_same(ransac, reg.register_fpfh(A, B, estimator="ransac"), "ransac")
    assert _same_bits(gnc["match"], ransac["match"]) and gnc["weights"].shape == (1, N) and bool(gnc["valid"][0])
    dt_r, dd_r = reg.transform_errors(Rt[None], ransac["Rt"], ransac["valid"])
    dt_g, dd_g = reg.transform_errors(Rt[None], gnc["Rt"], gnc["valid"])
    n_in = int(gnc["num_inliers"][0])
    print("register_fpfh: ransac %.4f m %.4f deg (%d inliers), gnc %.4f m %.4f deg (%d inliers, %d fits)"
          % (dt_r[0], dd_r[0], int(ransac["num_inliers"][0]), dt_g[0], dd_g[0], n_in, int(gnc["iterations"][0])))
    # "Within the error of the RANSAC result": both poses are least-squares fits over (nearly) the same inliers, so the two
    # errors are draws of one size, sigma * sqrt(3 / inliers) in translation and that over the cloud's radius in rotation;
    # three of those on top of RANSAC's own error is the allowance.
    radius = float(np.linalg.norm(a - a.mean(axis=0), axis=1).mean())
    step = 3.0 * sigma * math.sqrt(3.0 / max(n_in, 3))
    assert dt_g[0] <= dt_r[0] + step, (dt_g, dt_r, step)
    assert dd_g[0] <= dd_r[0] + math.degrees(step / radius) * 3.0, (dd_g, dd_r)  # (delta_deg sums three Euler angles)
    gnc2 = reg.register_fpfh(A, B, estimator="gnc", refine=True)
    assert _same_bits(gnc2["Rt_ransac"], gnc["Rt"]) and "fitness" in gnc2


def test_localize_passes_the_estimator_on(dev):
    """PlaceIndex.localize hands estimator= and gnc_rigid's keywords to register: the winner's pose is the single
    (place, query) pair's under gnc_rigid, bit for bit; a RANSAC keyword beside it is refused."""
    import test_retrieval_gpu as tr
    from dh3d_amd import registration as reg
    rng = np.random.default_rng(12)
    rows, count, gdesc = tr._places(rng)
    sel = np.array([3, 0, 11, 7])
    qrows, qcount, qdesc, T = tr._queries(rng, rows, count, gdesc, sel)
    index = tr._index(dev, rows, count, gdesc)
    tq, tc, td = _t(dev, qrows), _t(dev, qcount), _t(dev, qdesc)
    res = index.localize(td, tq, tc, k=3, estimator="gnc", threshold=0.5)
    assert res["place"].cpu().numpy().tolist() == sel.tolist()
    A, AC = _t(dev, rows), _t(dev, count)
    for q, p in enumerate(sel):
        one = reg.register(A[p:p + 1], AC[p:p + 1], tq[q:q + 1], tc[q:q + 1], estimator="gnc", threshold=0.5)
        assert bool(one["valid"][0]) and _same_bits(one["Rt"][0], res["Rt"][q]), q
        assert int(one["num_inliers"][0]) == int(res["num_inliers"][q]) and torch.equal(one["inliers"][0], res["inliers"][q]), q
    dt, ddeg = reg.transform_errors(T, res["Rt"], res["place"] >= 0)
    assert (dt < 0.1).all() and (ddeg < 1.0).all(), (dt, ddeg)  # (test_retrieval_gpu's bounds for the RANSAC pose)
    with pytest.raises(ValueError, match='estimator="gnc".*seed'):
        index.localize(td, tq, tc, k=3, estimator="gnc", seed=4)
