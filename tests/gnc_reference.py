"""A numpy float64 restatement of include/dh3d_hip.h dh3d_gnc_rigid (dh3d_amd.registration.gnc_rigid -> csrc/registration.hip
gnc_kernel): graduated non-convexity on the Geman-McClure objective by re-weighted closed-form fits, on the quaternion
route of tests/registration_reference.py (_b_matrix weighted, quat2rot), so that restatement and kernel solve the same
eigenproblem.  With it: the compaction rule of the correspondences, the closed form of the schedule's length, the fixture
builders of tests/test_gnc_reference.py and tests/test_gnc_gpu.py, the seeds chosen for them, and `clear`, which says that
no inlier decision of a run hangs on a last-bit rounding.  VARIANTS names five one-line mistakes; gnc(..., variant=) makes
one of them, for the test that shows the GPU comparison would see it."""
import math

import numpy as np

import registration_reference as ref

VARIANTS = ("weights_not_squared", "mu_not_floored", "centroids_unweighted", "mu_after_division", "settle_off_by_one")
WEIGHT_SLOPE = 25.0 * math.sqrt(5.0) / 54.0  # max over s of |d/ds (1 / (1 + s^2))^2| = 4 s / (1 + s^2)^3 at s^2 = 1 / 5


def correspondences(ax, bx, match, count):
    """The rows of one pair that are correspondences: i < clamp(count, 0, Ma) with 0 <= match[i] < Mb, in ascending i.
    ax [Ma, 3], bx [Mb, 3] float32, match [Ma] int32 -> x [n, 3], y [n, 3] float64 and the anchor rows [n]."""
    Ma, Mb = len(ax), len(bx)
    na = min(max(int(count), 0), Ma)
    m = np.asarray(match[:na], np.int64)
    rows = np.nonzero((m >= 0) & (m < Mb))[0]
    return ax[rows, :3].astype(np.float64), bx[m[rows], :3].astype(np.float64), rows


def weighted_fit(X, Y, w, variant=None):
    """The fit of rigid_fit.h with every pair's share weighted: R [3, 3], t [3]."""
    W = w.sum()
    if variant == "centroids_unweighted":
        cx, cy = X.mean(axis=0), Y.mean(axis=0)
    else:
        cx, cy = (w[:, None] * X).sum(axis=0) / W, (w[:, None] * Y).sum(axis=0) / W
    r = np.sqrt(w)[:, None]  # (A is linear in the pair: w A^T A = (sqrt(w) A)^T (sqrt(w) A))
    B = ref._b_matrix((r * (X - cx))[None], (r * (Y - cy))[None])[0]
    if not np.isfinite(B).all():
        return np.full((3, 3), np.nan), np.full(3, np.nan)
    _, V = np.linalg.eigh(B)
    R = ref.quat2rot(V[:, 0])
    return R, cx - R @ cy


def residuals(R, t, x, y):
    """sqrt(|x - (R y + t)|^2) of every pair, registration_reference.residuals' (and is_inlier's) expression."""
    return ref.residuals(R[None], t[None], x, y)[0]


def gnc(x, y, threshold=1.0, division=1.4, settle=8, max_iterations=64, variant=None):
    """dh3d_gnc_rigid on n correspondences x [n, 3] (anchor) <-> y [n, 3] (positive), float64.  Returns a dict: Rt [3, 4]
    (NaN when not valid), valid, weights [n] (of the last fit), mask [n], num_inliers, iterations, and for the tests
    residual [n] (under the final pose), pose [3, 4] (the final pose whether valid or not), D2 and big (the largest centred
    coordinate)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = len(x)
    out = dict(Rt=np.full((3, 4), np.nan), valid=False, weights=np.zeros(n), mask=np.zeros(n, bool), num_inliers=0,
               iterations=0, residual=np.zeros(n), pose=np.full((3, 4), np.nan), D2=0.0, big=0.0)
    if n < 3:
        return out
    xc, yc = x.sum(axis=0) / n, y.sum(axis=0) / n
    X, Y = x - xc, y - yc
    with np.errstate(invalid="ignore"):
        D2 = float(np.fmax.reduce(np.concatenate([(X * X).sum(axis=1), (Y * Y).sum(axis=1), [0.0]])))  # (NaN terms skipped)
        d2 = threshold * threshold
        mu = D2 if D2 > d2 else d2
        w = np.ones(n)
        at = k = 0
        while True:
            R, t = weighted_fit(X, Y, w, variant)
            k += 1
            if mu == d2:
                at += 1
            if (at >= settle if variant == "settle_off_by_one" else at > settle) or k >= max_iterations:
                break
            e = X - (Y @ R.T + t)
            r2 = (e * e).sum(axis=1)
            nxt = mu / division
            if variant != "mu_not_floored":
                nxt = nxt if nxt > d2 else d2
            m = nxt if variant == "mu_after_division" else mu
            q = m / (r2 + m)
            w = q if variant == "weights_not_squared" else q * q
            mu = nxt
        tf = (xc - R @ yc) + t
        d = residuals(R, tf, x, y)
        mask = d < threshold
    finite = bool(np.isfinite(R).all() and np.isfinite(tf).all())
    valid = finite and int(mask.sum()) >= 3
    out.update(valid=valid, weights=w, mask=mask, num_inliers=int(mask.sum()), iterations=k, residual=d, D2=D2,
               big=float(np.nanmax(np.abs(np.concatenate([X, Y])))) if np.isfinite(D2) else 0.0)
    out["pose"] = np.concatenate([R, tf[:, None]], axis=1)
    if valid:
        out["Rt"] = out["pose"]
    return out


def schedule_length(D2, threshold=1.0, division=1.4, settle=8, max_iterations=64):
    """The closed form of `iterations`: m + settle + 1 fits, m = the divisions that bring D2 down to threshold^2, capped by
    max_iterations; and how far log(D2 / d2) / log(division) is from an integer (a fixture keeps clear of it)."""
    d2 = threshold * threshold
    if not D2 > d2:
        return min(max_iterations, settle + 1), math.inf
    f = math.log(D2 / d2) / math.log(division)
    return min(max_iterations, math.ceil(f) + settle + 1), abs(f - round(f))


def clear(run, threshold):
    """In the spirit of icp_reference.clear_pair: every correspondence's final residual differs from `threshold` by more
    than 1e-6, so the inlier mask does not depend on roundings six orders below it (NaN residuals are never inliers)."""
    d = run["residual"]
    d = d[np.isfinite(d)]
    return bool((np.abs(d - threshold) > 1e-6).all())


def pose_error(Rt, truth):
    """(translation error in m, rotation angle in degrees) between two [3, 4] poses."""
    dR = Rt[:, :3].T @ truth[:, :3]
    ang = math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(dR) - 1.0) / 2.0))))
    return float(np.linalg.norm(Rt[:, 3] - truth[:, 3])), ang


# ------------------------------------------------------------------------------------------------------------ fixtures

BOX = np.array([80.0, 80.0, 16.0])  # a street-like extent


def random_pose(rng, max_angle=math.pi):
    """A rotation about a uniform axis by up to max_angle, a translation of up to 10 m: Rt [3, 4]."""
    a = rng.standard_normal(3)
    a /= np.linalg.norm(a)
    ang = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)
    t = rng.standard_normal(3)
    t = t / np.linalg.norm(t) * rng.uniform(0.0, 10.0)
    return np.concatenate([R, t[:, None]], axis=1)


def outlier_fixture(seed, n, outlier_share, noise=0.05):
    """n correspondences in the box: x uniform, y = R^T (x - t) + noise, and an `outlier_share` of the partners replaced by
    uniform points.  Returns x, y float32 [n, 3] and the true pose [3, 4]."""
    rng = np.random.default_rng(seed)
    T = random_pose(rng)
    x = rng.random((n, 3)) * BOX - BOX / 2
    y = (x - T[:, 3]) @ T[:, :3] + rng.normal(0.0, noise, (n, 3))
    out = rng.permutation(n)[:int(round(outlier_share * n))]
    y[out] = rng.random((len(out), 3)) * BOX - BOX / 2
    return x.astype(np.float32), y.astype(np.float32), T


# The outlier fixtures of the GPU test, (n, outlier share, seed): seeds picked on the CPU (tests/test_gnc_reference.py checks
# it) so that the restatement alone recovers the true pose within 0.1 m / 0.5 deg at threshold 0.5 and `clear` holds at
# thresholds 0.5 and 1.0.
OUTLIER_FIXTURES = ((512, 0.5, 11), (512, 0.8, 13), (128, 0.5, 13), (64, 0.5, 14))
BIG_FIXTURE = (4096, 0.8, 15)  # the pair that fills the 112 KB staging, 16 rows a lane
# the argument sets the GPU test runs its batch with (the rest are gnc_rigid's defaults): both thresholds, no settling,
# the plain least-squares fit, and a stop in the middle of the schedule
CONFIGS = (dict(threshold=0.5), dict(threshold=1.0), dict(threshold=0.5, settle=0), dict(threshold=0.5, max_iterations=1),
           dict(threshold=0.5, max_iterations=5))


def pack(M, x, y, rng, rows=None):
    """One pair's raw rows: the n correspondences at anchor rows 0 .. n - 1 (or `rows`), their partners scattered over the M
    positive rows behind the match ids; every other anchor row is far away and unmatched, every other positive row too."""
    n = len(x)
    ax = np.full((M, 3), -1e6, np.float32)
    bx = np.full((M, 3), 1e6, np.float32)
    match = np.full(M, -1, np.int32)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    perm = rng.permutation(M)[:n]
    ax[rows] = x
    bx[perm] = y
    match[rows] = perm
    return ax, bx, match


def edge_batch(M=512):
    """The GPU test's batch: the outlier fixtures and the edge pairs, as raw rows.  Returns ax, bx [P, M, 3] float32,
    match [P, M] int32, count [P] int32, the names of the pairs and the true poses of the outlier fixtures."""
    rng = np.random.default_rng(2024)
    pairs, names, truth = [], [], {}

    def add(name, ax, bx, match, count):
        pairs.append((ax, bx, match, count))
        names.append(name)

    for n, share, seed in OUTLIER_FIXTURES:
        x, y, T = outlier_fixture(seed, n, share)
        truth[len(pairs)] = T
        add("outliers_%d_%g" % (n, share), *pack(M, x, y, rng), n)
    for n in (0, 1, 2, 3, 4, 255, 256, 257):  # no model; the smallest models; the lane-stride edge
        x, y, _ = outlier_fixture(100 + n, max(n, 8), 0.25 if n > 4 else 0.0)
        add("n_%d" % n, *pack(M, x, y, rng), n)  # (rows past the count hold correspondences too: the count cuts them off)
    x, y, _ = outlier_fixture(200, M, 0.3)
    add("count_300_of_512", *pack(M, x, y, rng), 300)
    ax, bx, match = pack(M, x, y, rng)
    add("all_unmatched", ax, bx, np.full(M, -1, np.int32), M)
    x, y, _ = outlier_fixture(201, M, 0.3)
    ax, bx, match = pack(M, x, y, rng)
    bad = np.array([-1, M, M + 5, 2 ** 31 - 1, -7, -2 ** 31], np.int64).astype(np.int32)
    match[::3] = bad[np.arange(len(match[::3])) % len(bad)]
    add("ids_out_of_range", ax, bx, match, M)
    one = np.ones((100, 1), np.float32)
    add("coincident", *pack(M, one * np.float32([1, 2, 3]), one * np.float32([-4, 0.5, 2]), rng), 100)
    x, _, _ = outlier_fixture(202, M, 0.0)
    ax, bx, match = pack(M, x, x, rng)
    add("itself", ax, ax.copy(), np.arange(M, dtype=np.int32), M)
    x, y, _ = outlier_fixture(203, 128, 0.3)
    x[5, 1] = np.nan
    add("one_nan", *pack(M, x, y, rng), 128)
    x, y, _ = outlier_fixture(204, 200, 0.3)
    add("scattered_rows", *pack(M, x, y, rng, rows=np.sort(rng.permutation(M)[:200])), M)
    stack = lambda k, dt: np.stack([p[k] for p in pairs]).astype(dt)
    return stack(0, np.float32), stack(1, np.float32), stack(2, np.int32), np.array([p[3] for p in pairs], np.int32), names, truth


def big_pair(M=4096):
    """The pair at Ma = Mb = 4096: raw rows as edge_batch's, and its true pose."""
    n, share, seed = BIG_FIXTURE
    x, y, T = outlier_fixture(seed, n, share)
    ax, bx, match = pack(M, x, y, np.random.default_rng(7))
    return ax[None], bx[None], match[None], np.array([n], np.int32), T


def run_batch(ax, bx, match, count, **kw):
    """gnc on every pair of a raw batch; each result also carries rows (the anchor rows of its correspondences)."""
    out = []
    for p in range(len(ax)):
        x, y, rows = correspondences(ax[p], bx[p], match[p], count[p])
        r = gnc(x, y, **kw)
        r["rows"] = rows
        out.append(r)
    return out
