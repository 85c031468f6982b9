"""A numpy float64 restatement of include/dh3d_hip.h dh3d_estimate_normals and dh3d_icp_refine_plane.  normals() takes the
sums in list order and solves with np.linalg.eigh; icp_plane() runs icp_reference's association with the point-to-plane fit,
the operations in the header's order (numpy rounds every elementwise operation on its own; the sums are numpy's, so the pose
differs from the kernels' by the summation order and nothing else).  Both report how close a run came to a decision that a
last-bit rounding could turn: per point the relative eigen gap and the orientation margin of its normal, per run the
association's gap / thr of icp_reference, the largest cond(H) and the smallest Cholesky pivot relative to H's largest
diagonal entry."""
import math

import numpy as np

import icp_reference as ir


def knn_ids(x, k, n=None):
    """Brute-force ids [N, k] of the k nearest rows among x[:n] (the point itself included), by (d2, index); rows >= n get -1."""
    x = np.asarray(x, np.float64)
    N = len(x)
    n = N if n is None else n
    ids = np.full((N, k), -1, np.int32)
    d2 = ((x[:n, None, :] - x[None, :n, :]) ** 2).sum(axis=2)
    order = np.argsort(d2, axis=1, kind="stable")[:, :k]
    ids[:n, :order.shape[1]] = order
    return ids


def normals(x, nbr, n=None, viewpoint=(0.0, 0.0, 0.0)):
    """x [N, 3] float32, nbr [N, K] int ids.  Returns a dict: normals [N, 3] float64 (before the rounding to float32),
    curvature [N], lam [N, 3] ascending eigenvalues, gap [N] = (lam1 - lam0) / lam2, margin [N] = |s| / |v - x| (inf where the
    normal is zero), C [N, 3, 3] and m [N]."""
    x32 = np.asarray(x, np.float32)
    x = x32.astype(np.float64)
    nbr = np.asarray(nbr)
    N, K = nbr.shape
    n = N if n is None else min(max(int(n), 0), N)
    v = np.asarray(viewpoint, np.float64)
    out = dict(normals=np.zeros((N, 3)), curvature=np.zeros(N), lam=np.zeros((N, 3)), gap=np.full(N, np.inf),
               margin=np.full(N, np.inf), C=np.zeros((N, 3, 3)), m=np.zeros(N, np.int64))
    if n == 0:
        return out
    ids = nbr[:n].astype(np.int64)
    use = (ids >= 0) & (ids < n)                                    # [n, K]; adding 0.0 for a skipped entry changes no sum
    safe = np.where(use, ids, 0)
    m = use.sum(axis=1)
    out["m"][:n] = m
    c = np.zeros((n, 3))
    for k in range(K):
        c = c + np.where(use[:, k:k + 1], x[safe[:, k]], 0.0)
    md = np.maximum(m, 1).astype(np.float64)[:, None]
    c = c / md
    C = np.zeros((n, 3, 3))
    for k in range(K):
        d = np.where(use[:, k:k + 1], x[safe[:, k]] - c, 0.0)
        C = C + d[:, :, None] * d[:, None, :]
    C = C / md[:, :, None]
    lam, vec = np.linalg.eigh(C)
    tot = lam.sum(axis=1)
    ok = (m >= 3) & (tot > 0.0)
    e = vec[:, :, 0]
    d = v[None, :] - x[:n]
    s = (d[:, 0] * e[:, 0] + d[:, 1] * e[:, 1]) + d[:, 2] * e[:, 2]
    dist = np.linalg.norm(d, axis=1)
    with np.errstate(all="ignore"):
        out["C"][:n] = np.where((m >= 3)[:, None, None], C, 0.0)
        out["lam"][:n] = np.where((m >= 3)[:, None], lam, 0.0)
        out["normals"][:n] = np.where(ok[:, None], np.where((s < 0)[:, None], -e, e), 0.0)
        out["curvature"][:n] = np.where(ok, lam[:, 0] / tot, 0.0)
        out["gap"][:n] = np.where(ok, (lam[:, 1] - lam[:, 0]) / lam[:, 2], np.inf)
        out["margin"][:n] = np.where(ok, np.where(dist > 0, np.abs(s) / dist, 0.0), np.inf)
    return out


def rows(anchor, normal, positive, nn, Rt):
    """The pairs of F_plane: (j, a [n_pl, 6], r [n_pl], c [3]) -- the stacked rows of the linear system a . s = r."""
    x = np.asarray(anchor, np.float64)
    nr = np.asarray(normal, np.float64)
    i_all = np.maximum(nn, 0)
    nsq = (nr[i_all, 0] * nr[i_all, 0] + nr[i_all, 1] * nr[i_all, 1]) + nr[i_all, 2] * nr[i_all, 2]
    j = np.nonzero((nn >= 0) & (nsq > 0.0))[0]
    if len(j) == 0:
        return j, np.zeros((0, 6)), np.zeros(0), np.zeros(3)
    i = nn[j]
    m = ir.move(Rt, np.asarray(positive, np.float32)[j])
    c = m.sum(axis=0) / len(j)
    q, n = m - c, nr[i]
    a = np.stack([q[:, 1] * n[:, 2] - q[:, 2] * n[:, 1], q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2],
                  q[:, 0] * n[:, 1] - q[:, 1] * n[:, 0], n[:, 0], n[:, 1], n[:, 2]], axis=1)
    d = x[i] - m
    r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    return j, a, r, c


def cholesky_solve(H, g):
    """H s = g by the header's Cholesky.  Returns (s or None when a pivot is refused, the smallest pivot / max diag)."""
    big = float(np.max(np.diag(H)))
    L = np.zeros((6, 6))
    ratio = np.inf
    for k in range(6):
        for j in range(k + 1):
            v = H[j, k]
            for q in range(j):
                v = v - L[k, q] * L[j, q]
            if j < k:
                L[k, j] = v / L[j, j]
            else:
                if not np.isfinite(v) or not v > 1e-12 * big:
                    return None, (v / big if big > 0 and np.isfinite(v) else -np.inf)
                ratio = min(ratio, v / big)
                L[k, k] = math.sqrt(v)
    z, s = np.zeros(6), np.zeros(6)
    for k in range(6):
        v = g[k]
        for j in range(k):
            v = v - L[k, j] * z[j]
        z[k] = v / L[k, k]
    for k in range(5, -1, -1):
        v = z[k]
        for j in range(k + 1, 6):
            v = v - L[j, k] * s[j]
        s[k] = v / L[k, k]
    return s, ratio


def step_rotation(w):
    """dR of the rotation vector w, the header's closed form."""
    tt = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = math.sqrt(tt)
    if th == 0.0:
        return np.eye(3)
    hs = math.sin(th / 2.0)
    A, B = math.sin(th) / th, (2.0 * (hs * hs)) / (th * th)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    K2 = w[:, None] * w[None, :] - tt * np.eye(3)
    return (np.eye(3) + A * K) + B * K2


def compose(Rt, s, c):
    """The step s = (rotation vector, translation) about the centroid c composed with the pose Rt, in the header's order."""
    dR = step_rotation(s[:3])
    R, t = Rt[:, :3], Rt[:, 3]
    Rn = np.stack([(dR[:, 0] * R[0, k] + dR[:, 1] * R[1, k]) + dR[:, 2] * R[2, k] for k in range(3)], axis=1)
    u = t - c
    tn = (((dR[:, 0] * u[0] + dR[:, 1] * u[1]) + dR[:, 2] * u[2]) + c) + s[3:]
    return np.concatenate([Rn, tn[:, None]], axis=1)


def solve_compose(H, g, c, Rt, info):
    """The end of F_plane and F_gicp: (the new Rt or None on a refused pivot or a non-finite s, info with cond / pivot / s)."""
    with np.errstate(all="ignore"):
        info["cond"] = float(np.linalg.cond(H))
    s, info["pivot"] = cholesky_solve(H, g)
    if s is None or not np.isfinite(s).all():
        return None, info
    info["s"] = s
    return compose(Rt, s, c), info


def fit_plane(anchor, normal, positive, nn, Rt):
    """F_plane(nn, pose): (the new Rt [3, 4] or None when the pose stays, info dict n_pl / cond / pivot / s)."""
    j, a, r, c = rows(anchor, normal, positive, nn, Rt)
    info = dict(n_pl=len(j), cond=np.inf, pivot=-np.inf, s=None)
    if len(j) < 6:
        return None, info
    H = (a[:, :, None] * a[:, None, :]).sum(axis=0)
    g = (a * r[:, None]).sum(axis=0)
    return solve_compose(H, g, c, Rt, info)


def plane_stats(anchor, normal, positive, nn, Rt):
    j, _, r, _ = rows(anchor, normal, positive, nn, Rt)
    return len(j), (math.sqrt((r * r).sum() / len(j)) if len(j) else np.nan)


def icp_plane(anchor, normal, positive, Rt0, max_dist=1.0, iterations=20, na=None, nb=None, valid0=True):
    """dh3d_icp_refine_plane on one pair (normal [Na, 3] float32).  Returns icp_reference.icp's dict, every state with num_plane
    and rmse_plane besides, and the margins gap / thr, cond (the largest cond(H) of a step taken), pivot (the smallest
    Cholesky pivot ratio of a step taken) and refused (the largest pivot ratio that made a step with 6 or more pairs leave the
    pose; -inf without one)."""
    normal = np.asarray(normal, np.float32)

    def step(anchor, positive, nn, Rt, out):
        new, info = fit_plane(anchor, normal, positive, nn, Rt)
        return take_step(out, new, info, info["n_pl"] >= 6)
    return ir.loop(anchor, positive, Rt0, step, lambda a, y, nn, Rt: plane_stats(a, normal, y, nn, Rt),
                   ("num_plane", "rmse_plane"), SOLVE_MARGINS, max_dist, iterations, na, nb, valid0)


SOLVE_MARGINS = dict(cond=0.0, pivot=np.inf, refused=-np.inf)  # where icp_plane's and icp_gicp's margins of the solve start


def take_step(out, new, info, enough):
    """The margins of a step of icp_plane / icp_gicp into the run `out`: cond and pivot of a step taken, refused of one that
    had `enough` pairs and left the pose.  Returns new."""
    if new is not None:
        out["cond"], out["pivot"] = max(out["cond"], info["cond"]), min(out["pivot"], info["pivot"])
    elif enough:
        out["refused"] = max(out["refused"], info["pivot"])
    return new


def demo_normals(anchor, k=16, n=None):
    """The float32 normals of a demo anchor: the k nearest neighbours, oriented towards the origin."""
    return normals(anchor, knn_ids(anchor, k, n), n)["normals"].astype(np.float32)


def is_clear(run):
    """No decision of the run hangs on a last-bit rounding: the ids (gap, thr), the solve (cond, pivot) and the refusals."""
    return (run["gap"] > 1e-8 and run["thr"] > 1e-8 and run["cond"] <= 1e6 and run["pivot"] >= 1e-6
            and run["refused"] <= 1e-14)


def clear_pair_plane(name, n, max_dist, iterations, base=1, k=16):
    """The first demo_pair (seeds base, base + 1, ... at most 50) whose plane run keeps a d2 gap above 1e-8 m^2, 1e-8 m^2
    from the threshold, cond(H) <= 1e6 and a pivot ratio >= 1e-6.  Returns (pair, normals, run, seed)."""
    for s in range(base, base + 50):
        pair = ir.demo_pair(name, n, s)
        nrm = demo_normals(pair[0], k)
        run = icp_plane(pair[0], nrm, pair[1], pair[3], max_dist=max_dist, iterations=iterations)
        if is_clear(run):
            return pair, nrm, run, s
    raise AssertionError("no clear fixture for %s n=%d max_dist=%g" % (name, n, max_dist))
