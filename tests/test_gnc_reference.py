"""CPU: the float64 restatement of dh3d_gnc_rigid (tests/gnc_reference.py) on cases with known answers, its independence
of the order of the correspondences, the closed form of its schedule, the seeds of the GPU test's fixtures, and the power of
that test: every one-line mistake of gnc_reference.VARIANTS moves a pose the GPU test compares by more than its tolerance."""
import math

import numpy as np
import pytest

import gnc_reference as g

GPU_POSE_TOLERANCE = 1e-9  # tests/test_gnc_gpu.py


def _fixtures():
    return [g.outlier_fixture(seed, n, share) for n, share, seed in g.OUTLIER_FIXTURES + (g.BIG_FIXTURE,)]


def test_clean_data_comes_back_exactly():
    """256 noise-free pairs under a 2 rad rotation: the pose to 1e-12 (measured: 1.1e-14), every weight 1 at the end."""
    rng = np.random.default_rng(0)
    T = g.random_pose(rng, 2.0)
    a = rng.standard_normal(3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T[:, :3] = np.eye(3) + math.sin(2.0) * K + (1 - math.cos(2.0)) * (K @ K)
    x = rng.random((256, 3)) * g.BOX - g.BOX / 2
    y = (x - T[:, 3]) @ T[:, :3]
    r = g.gnc(x, y)
    err = np.abs(r["Rt"] - T).max()
    print("clean data: pose error %.3g" % err)
    assert r["valid"] and r["num_inliers"] == 256 and err < 1e-12
    assert np.abs(r["weights"] - 1.0).max() < 1e-12


def test_small_n_and_the_plain_fit():
    rng = np.random.default_rng(1)
    for n in (0, 1, 2):
        r = g.gnc(rng.random((n, 3)), rng.random((n, 3)))
        assert not r["valid"] and r["iterations"] == 0 and r["num_inliers"] == 0 and np.isnan(r["Rt"]).all()
    x, y, _ = g.outlier_fixture(3, 40, 0.0)
    one = g.gnc(x, y, max_iterations=1)
    assert one["iterations"] == 1 and (one["weights"] == 1.0).all()
    import registration_reference as ref
    R, t, _ = ref.fit(x[None].astype(np.float64), y[None].astype(np.float64))
    assert np.abs(one["Rt"] - np.concatenate([R[0], t[0][:, None]], axis=1)).max() < 1e-12


def test_outlier_fixtures_recover_the_pose_and_are_clear():
    """The seeds listed in gnc_reference: the restatement alone recovers the truth within 0.1 m / 0.5 deg at threshold 0.5,
    and no residual lies within 1e-6 of the threshold in any configuration the GPU test runs."""
    for (n, share, seed), (x, y, T) in zip(g.OUTLIER_FIXTURES + (g.BIG_FIXTURE,), _fixtures()):
        r = g.gnc(x, y, threshold=0.5)
        dt, ddeg = g.pose_error(r["Rt"], T)
        print("n %d outliers %g seed %d: %.4f m %.4f deg, %d fits, %d inliers" % (n, share, seed, dt, ddeg, r["iterations"],
                                                                                  r["num_inliers"]))
        assert r["valid"] and dt < 0.1 and ddeg < 0.5, (n, share, seed, dt, ddeg)
        for cfg in g.CONFIGS:
            assert g.clear(g.gnc(x, y, **cfg), cfg["threshold"]), (n, share, seed, cfg)


def test_edge_batch_is_clear():
    ax, bx, match, count, names, _ = g.edge_batch()
    for cfg in g.CONFIGS:
        for name, r in zip(names, g.run_batch(ax, bx, match, count, **cfg)):
            assert g.clear(r, cfg["threshold"]), (name, cfg)


def test_order_of_the_correspondences_does_not_matter():
    """Permuted correspondences: the pose within 1e-11 (measured on the quaternion route: 8e-15), the weights and the mask
    permuted with them.  The bound leaves the factor of 100 to the GPU tolerance."""
    worst = 0.0
    for x, y, _ in _fixtures()[:4]:
        r = g.gnc(x, y, threshold=0.5)
        for s in range(5):
            p = np.random.default_rng(s).permutation(len(x))
            q = g.gnc(x[p], y[p], threshold=0.5)
            worst = max(worst, float(np.abs(q["Rt"] - r["Rt"]).max()))
            assert (q["mask"] == r["mask"][p]).all() and q["iterations"] == r["iterations"]
            assert np.abs(q["weights"] - r["weights"][p]).max() < 1e-11
    print("permutation spread of the pose: %.3g" % worst)
    assert worst < 1e-11 and 100.0 * 1e-11 <= GPU_POSE_TOLERANCE


def test_iterations_follow_the_closed_form():
    for x, y, _ in _fixtures():
        for cfg in g.CONFIGS + (dict(threshold=0.5, division=2.0, settle=3), dict(threshold=100.0)):
            r = g.gnc(x, y, **cfg)
            want, frac = g.schedule_length(r["D2"], **cfg)
            assert frac > 1e-6, (cfg, frac)  # (the fixture keeps clear of a whole number of divisions)
            assert r["iterations"] == want, (cfg, r["iterations"], want)
    x, y, _ = _fixtures()[0]
    assert g.gnc(x, y, threshold=100.0)["iterations"] == 9          # D2 <= d2: mu starts at the floor, settle + 1 fits
    assert g.gnc(x, y, threshold=0.5)["iterations"] == 38
    assert g.gnc(x, y, threshold=0.5, max_iterations=5)["iterations"] == 5


@pytest.mark.parametrize("variant", g.VARIANTS)
def test_gpu_comparison_would_see_the_mistake(variant):
    """The restatement with one mistake moves the pose of at least one (fixture, configuration) the GPU test compares by
    more than that test's tolerance."""
    worst = 0.0
    for x, y, _ in _fixtures()[:4]:
        for cfg in g.CONFIGS:
            r, v = g.gnc(x, y, **cfg), g.gnc(x, y, variant=variant, **cfg)
            if r["valid"]:  # (the GPU test compares Rt where the restatement is valid)
                worst = max(worst, float(np.abs(v["pose"] - r["pose"]).max()))
    print("%s moves a pose by %.3g" % (variant, worst))
    assert worst > 1000.0 * GPU_POSE_TOLERANCE, (variant, worst)
