"""CPU: the float64 restatement of the MATLAB registration loop (tests/registration_reference.py) on cases with known
answers, the host metrics of dh3d_amd.registration (compareTransform / GetEulerAngles, eval_align.m's summary), and the
status codes of the registration entry points (include/dh3d_hip.h, csrc/registration.hip) before any launch."""
import math

import numpy as np
import pytest

import registration_reference as ref


def _rot(yaw, pitch=0.0, roll=0.0):
    cz, sz, cy, sy, cx, sx = (math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll),
                              math.sin(roll))
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return Rz @ Ry @ Rx


def _pair(rng, n, R, t, side=40.0):
    x = rng.random((n, 3)) * side - side / 2
    y = (x - t) @ R  # R^T (x - t): anchor = R positive + t
    return x, y


def test_restatement_recovers_exact_pose():
    """Noise-free correspondences: R, t to 1e-12 in the sign convention anchor = R positive + t."""
    rng = np.random.default_rng(0)
    for yaw, t in ((0.3, [1.0, -2.0, 0.5]), (-2.9, [9.0, 3.0, -1.0]), (math.pi / 2, [0.0, 0.0, 0.0])):
        R = _rot(yaw, 0.05, -0.03)
        x, y = _pair(rng, 200, R, np.array(t))
        res = ref.ransac(x, y)
        assert res["valid"] and res["num_inliers"] == 200
        assert np.abs(res["Rt"][:, :3] - R).max() < 1e-12
        assert np.abs(res["Rt"][:, 3] - t).max() < 1e-12


def test_all_inliers_stop_at_ten_trials():
    rng = np.random.default_rng(1)
    x, y = _pair(rng, 300, _rot(1.0), np.array([2.0, 1.0, 0.0]))
    res = ref.ransac(x, y)
    assert res["trials"] == 10 and res["num_inliers"] == 300 and res["mask"].all()
    assert res["win"] == 9  # ties accepted with >=: the last of the ten


def test_all_outliers_run_to_max_trials_and_keep_the_last():
    rng = np.random.default_rng(2)
    x = rng.random((60, 3)) * 1000.0
    y = rng.random((60, 3)) * 1000.0
    res = ref.ransac(x, y)
    assert res["trials"] == 10001 and res["win"] == 10000
    assert res["num_inliers"] == 0 and not res["valid"] and np.isnan(res["Rt"]).all()
    res = ref.ransac(x, y, max_trials=37)
    assert res["trials"] == 38 and res["win"] == 37


def test_small_n():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2):
        res = ref.ransac(rng.random((n, 3)), rng.random((n, 3)))
        assert res["trials"] == 0 and not res["valid"] and res["num_inliers"] == 0
    x, y = _pair(rng, 3, _rot(0.7), np.array([1.0, 2.0, 3.0]))
    res = ref.ransac(x, y)
    assert res["trials"] == 0 and res["valid"] and res["num_inliers"] == 3


def test_sampler_ids_distinct_and_in_range():
    ks = np.arange(0, 3000)
    for n in list(range(3, 70)) + [127, 128, 129, 511, 512, 1000, 2047, 4095, 4096]:
        for seed in (0, 1, 2 ** 64 - 1):
            ids = ref.sample(seed, ks, n)
            assert ids.min() >= 0 and ids.max() < n, n
            assert (ids[:, 0] != ids[:, 1]).all() and (ids[:, 0] != ids[:, 2]).all() and (ids[:, 1] != ids[:, 2]).all(), n
    # a fixed value of the stream: splitmix64(0) is the published first output of the generator seeded with 0
    assert int(ref.splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF
    ids = ref.sample(0, np.arange(20000), 5)
    assert len(np.unique(ids[:, 0])) == 5  # every id is drawn


def _T(R, t):
    return np.concatenate([R, np.asarray(t, float)[:, None]], axis=1)[None]


def test_transform_errors():
    from dh3d_amd.registration import transform_errors
    I = np.eye(3)
    dt, dd = transform_errors(_T(I, [0, 0, 0]), _T(I, [0, 0, 0]))
    assert dt[0] == 0.0 and dd[0] == 0.0
    dt, dd = transform_errors(_T(I, [1, 2, 2]), _T(_rot(math.radians(3.0)), [0, 0, 0]))
    assert dt[0] == pytest.approx(3.0, abs=1e-12) and dd[0] == pytest.approx(3.0, abs=1e-9)
    for axis in range(3):
        ang = [0.0, 0.0, 0.0]
        ang[axis] = math.radians(2.0)
        _, dd = transform_errors(_T(I, [0, 0, 0]), _T(_rot(ang[2], ang[1], ang[0]), [0, 0, 0]))
        assert dd[0] == pytest.approx(2.0, abs=1e-5), axis  # (acos near 1: ~1e-8 rad of rounding, in MATLAB too)
    # a 180 degree flip about z: dR[0,0] = -1 -> rz = pi, rx = acos(1) = 0
    _, dd = transform_errors(_T(I, [0, 0, 0]), _T(np.diag([-1.0, -1.0, 1.0]), [0, 0, 0]))
    assert dd[0] == pytest.approx(180.0, abs=1e-9)
    # rounding pushes an acos argument past 1: MATLAB goes complex, abs() keeps the tiny imaginary part
    R = np.eye(3)
    R[0, 0] = 1.0 + 2.0 ** -52
    dt, dd = transform_errors(_T(I, [0, 0, 0]), _T(R, [0, 0, 0]))
    assert np.isfinite(dd[0]) and 0.0 < dd[0] < 1e-5
    # pairs without an estimate: eval_align.m's catch
    nan = np.full((3, 4), np.nan)[None]
    dt, dd = transform_errors(np.concatenate([_T(I, [0, 0, 0])] * 2), np.concatenate([_T(I, [0, 0, 1]), nan]),
                              np.array([True, False]))
    assert dt.tolist() == [1.0, 3.0] and dd.tolist() == [0.0, 6.0]


def test_summarize_registration():
    from dh3d_amd.registration import summarize_registration
    dt = [0.5, 1.0, 2.5, 0.3, 1.5]
    dd = [1.0, 4.0, 1.0, 5.5, 2.0]  # pairs 2 (dt) and 3 (deg) fail
    s = summarize_registration(dt, dd, [0.5, 0.25, 0.9, 0.9, 0.75], [10, 20, 30, 40, 60])
    assert s["num_pairs"] == 5 and s["num_failed"] == 2 and s["success_rate"] == pytest.approx(60.0)
    assert s["mean_inlier_ratio"] == pytest.approx(0.5)
    assert s["mean_trials"] == pytest.approx(30.0)
    assert s["rte_mean"] == pytest.approx(1.0) and s["rte_std"] == pytest.approx(0.5)
    assert s["rre_mean"] == pytest.approx(7.0 / 3.0) and s["rre_std"] == pytest.approx(math.sqrt(7.0 / 3.0))
    assert summarize_registration([2.0], [5.0], [1.0], [10])["success_rate"] == 100.0  # the bounds themselves pass


def _match(lib, a=256, ac=256, b=256, bc=256, P=2, Ma=512, Mb=512, D=128, m=256, d=256, sa=132, sb=132):
    return lib.dh3d_match_descriptors(a, sa, ac, b, sb, bc, P, Ma, Mb, D, m, d, None)


def _ransac(lib, ax=256, bx=256, m=256, ac=256, P=2, Ma=512, Mb=512, thr=1.0, conf=0.99, trials=10000, out=256, sa=132,
            sb=132):
    return lib.dh3d_ransac_rigid(ax, sa, bx, sb, m, ac, P, Ma, Mb, thr, conf, trials, 0, out, out, out, out, out, None, None)


def test_registration_status_codes():
    from dh3d_amd import _lib
    lib = _lib.lib()
    z = None  # (256: a non-null fake pointer; every check below fails before a launch)
    for kw in (dict(a=z), dict(ac=z), dict(b=z), dict(bc=z), dict(m=z), dict(d=z), dict(P=0), dict(Ma=0), dict(Mb=0),
               dict(D=0), dict(sa=64), dict(sb=100)):
        assert _match(lib, **kw) == 1, kw
    for kw in (dict(D=130), dict(D=258, sa=300, sb=300), dict(D=260, sa=300, sb=300), dict(Ma=4097), dict(Mb=4097)):
        assert _match(lib, **kw) == 2, kw
    for kw in (dict(ax=z), dict(bx=z), dict(m=z), dict(ac=z), dict(out=z), dict(P=0), dict(Ma=0), dict(Mb=0), dict(thr=0.0),
               dict(conf=1.0), dict(conf=0.0), dict(trials=-1), dict(sa=2)):
        assert _ransac(lib, **kw) == 1, kw
    for kw in (dict(Ma=4097), dict(Mb=4097)):
        assert _ransac(lib, **kw) == 2, kw


def test_python_entry_points_refuse_bad_input():
    import torch
    from dh3d_amd import registration as reg
    cpu = torch.zeros(1, 8, 132)
    cnt = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError):
        reg.match_descriptors(cpu[:, :, 3:131], cnt, cpu[:, :, 3:131], cnt)  # CPU tensors: no fallback
    with pytest.raises(ValueError):
        reg.ransac_rigid(cpu, cpu, torch.zeros(1, 8, dtype=torch.int32), cnt)
    with pytest.raises(ValueError):
        reg.register(cpu, cnt, cpu, cnt)
