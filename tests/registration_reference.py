"""A vectorised numpy float64 restatement of the serial registration loop of the reference's MATLAB evaluation
(evaluate/local_eval/matlab_code: eval_align.m -> pdist2 'smallest', ransacfitRt.m -> ransac.m -> estimateRigidTransform.m),
with the splitmix64 sampler of include/dh3d_hip.h dh3d_ransac_rigid in place of randsample.  The yardstick of
dh3d_amd.registration: trials are evaluated in chunks (every trial's model and inlier count at once) and ransac.m's stop rule
is replayed over the counts, which is exactly the serial loop.  Besides the results it reports how close the evaluated
hypotheses came to a decision boundary (inlier threshold, eigen gap, integer N_k), so that fixtures can avoid ties that
float64 rounding could break either way."""
import numpy as np

from pairs_reference import splitmix64  # the one numpy statement of include/dh3d_hip.h's generator

EPS = 2.0 ** -52


def sample(seed, ks, n):
    """[T, 3] ids of trials ks (n >= 4): i0 = u0 mod n, i1 = u1 mod (n-1) stepped past i0, i2 = u2 mod (n-2) stepped past
    the two chosen ids in ascending order."""
    ks = np.asarray(ks, dtype=np.uint64)
    h = splitmix64(splitmix64(np.uint64(seed)) ^ ks)
    with np.errstate(over="ignore"):
        u = [splitmix64(h + np.uint64(j)) for j in range(3)]
    i0 = (u[0] % np.uint64(n)).astype(np.int64)
    i1 = (u[1] % np.uint64(n - 1)).astype(np.int64)
    i1 = i1 + (i1 >= i0)
    i2 = (u[2] % np.uint64(n - 2)).astype(np.int64)
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 = i2 + (i2 >= lo)
    i2 = i2 + (i2 >= hi)
    return np.stack([i0, i1, i2], axis=1)


def _b_matrix(X, Y):
    """sum over axis 1 of A^T A, A = [0, (Y-X)^T; X-Y, crossTimesMatrix(Y+X)] (estimateRigidTransform.m); X, Y [T, m, 3]."""
    d, s = X - Y, Y + X
    z = np.zeros(d.shape[:2])
    A = np.stack([
        np.stack([z, -d[..., 0], -d[..., 1], -d[..., 2]], -1),
        np.stack([d[..., 0], z, -s[..., 2], s[..., 1]], -1),
        np.stack([d[..., 1], s[..., 2], z, -s[..., 0]], -1),
        np.stack([d[..., 2], -s[..., 1], s[..., 0], z], -1),
    ], -2)
    return np.einsum("tqki,tqkj->tij", A, A)


def quat2rot(q):
    q0, q1, q2, q3 = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([
        np.stack([q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)], -1),
        np.stack([2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)], -1),
        np.stack([2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3], -1),
    ], -2)


def fit(x, y):
    """estimateRigidTransform(x, y) for T point sets at once: x, y [T, m, 3] float64 -> R [T, 3, 3], t [T, 3] with
    x ~ R y + t, and the relative eigen gap (lambda_2 - lambda_1) / max(|lambda|, 1) of B."""
    m = x.shape[1]
    xs, ys = x[:, 0], y[:, 0]
    for q in range(1, m):  # (sums in set order, as the kernel's 3-point fit)
        xs, ys = xs + x[:, q], ys + y[:, q]
    xc, yc = xs / m, ys / m
    B = _b_matrix(x - xc[:, None], y - yc[:, None])
    w, V = np.linalg.eigh(B)
    R = quat2rot(V[:, :, 0])
    t = xc - np.einsum("tij,tj->ti", R, yc)
    gap = (w[:, 1] - w[:, 0]) / np.maximum(np.abs(w).max(axis=1), 1.0)
    return R, t, gap


def residuals(R, t, x, y):
    """[T, n] sqrt(|x - (R y + t)|^2) (ransacfitRt.m euc3Ddist)."""
    e = [x[None, :, r] - ((R[:, r, 0:1] * y[None, :, 0] + R[:, r, 1:2] * y[None, :, 1] + R[:, r, 2:3] * y[None, :, 2])
                          + t[:, r:r + 1]) for r in range(3)]
    return np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2])


def ransac(x, y, threshold=1.0, confidence=0.99, max_trials=10000, seed=0, chunk=512):
    """ransacfitRt([x'; y'], threshold) on n correspondences x [n, 3] (anchor) <-> y [n, 3] (positive), float64.  Returns a
    dict: Rt [3, 4] (NaN when not valid), valid, mask [n] (the winner's inliers), num_inliers, trials, and the margins of
    the evaluated hypotheses: margin (min |d - threshold|), gap (min relative eigen gap, refit included) and n_frac (min
    distance of an N_k >= 10 to an integer)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = x.shape[0]
    out = dict(Rt=np.full((3, 4), np.nan), valid=False, mask=np.zeros(n, bool), num_inliers=0, trials=0, win=-1,
               margin=np.inf, gap=np.inf, n_frac=np.inf)
    if n < 3:
        return out
    if n == 3:
        mask = np.ones(3, bool)
        trials = 0
        _, _, g = fit(x[None], y[None])
        out["gap"] = float(g[0])
    else:
        counts, margins, gaps = [], [], []
        log_fail = np.log(1.0 - confidence)
        best, win, N, kstar = 0, 0, 1.0, None
        k = 0
        while kstar is None:
            ks = np.arange(k, min(k + chunk, max_trials + 1))
            ids = sample(seed, ks, n)
            R, t, g = fit(x[ids], y[ids])
            d = residuals(R, t, x, y)
            c = (d < threshold).sum(axis=1)
            margins.append(np.abs(d - threshold).min(axis=1))
            gaps.append(g)
            counts.append(c)
            for q, kk in enumerate(ks):  # ransac.m's loop over the chunk's counts
                if c[q] >= best:
                    best, win = int(c[q]), int(kk)
                    frac = best / n
                    pno = min(max(1.0 - frac * frac * frac, EPS), 1.0 - EPS)
                    raw = log_fail / np.log(pno)
                    N = max(raw, 10.0)
                    if raw >= 10.0:
                        out["n_frac"] = min(out["n_frac"], abs(raw - np.round(raw)))
                if N <= kk + 1 or kk + 1 > max_trials:
                    kstar = int(kk)
                    break
            k += chunk
        margins, gaps = np.concatenate(margins), np.concatenate(gaps)
        out["margin"] = float(margins[:kstar + 1].min())
        out["gap"] = float(gaps[:kstar + 1].min())
        ids = sample(seed, [win], n)
        R, t, _ = fit(x[ids], y[ids])
        mask = residuals(R, t, x, y)[0] < threshold
        trials = kstar + 1
        out["win"] = win
    out.update(mask=mask, num_inliers=int(mask.sum()), trials=trials)
    if mask.sum() >= 3:
        R, t, g = fit(x[mask][None], y[mask][None])
        out["Rt"] = np.concatenate([R[0], t[0][:, None]], axis=1)
        out["valid"] = True
        out["gap"] = min(out["gap"], float(g[0]))
    return out


def match(a_desc, b_desc, chunk=512):
    """pdist2(b, a, 'euclidean', 'smallest', 1) in float64: for every row of a the lowest index of the nearest row of b,
    the distance, and the relative gap between the best and the runner-up distance (inf with one candidate).  Distances by
    the |a|^2 + |b|^2 - 2 a.b expansion (exact ties stay exact ties; float64 keeps the error far below the gaps tested)."""
    a, b = np.asarray(a_desc, np.float64), np.asarray(b_desc, np.float64)
    na = len(a)
    if len(b) == 0:
        return np.full(na, -1), np.full(na, np.inf), np.full(na, np.inf)
    ids, best, rel = np.empty(na, np.int64), np.empty(na), np.full(na, np.inf)
    bb = (b * b).sum(1)
    for s in range(0, na, chunk):
        aa = a[s:s + chunk]
        d = np.sqrt(np.maximum((aa * aa).sum(1)[:, None] + bb[None, :] - 2.0 * aa @ b.T, 0.0))
        i = d.argmin(axis=1)
        ids[s:s + chunk] = i
        best[s:s + chunk] = d[np.arange(len(aa)), i]
        if len(b) > 1:
            second = np.partition(d, 1, axis=1)[:, 1]
            rel[s:s + chunk] = (second - best[s:s + chunk]) / np.maximum(second, 1e-30)
    return ids, best, rel
