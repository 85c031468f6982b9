"""A numpy float64 restatement of include/dh3d_hip.h dh3d_icp_refine_gicp: icp_reference's association with the generalized
(plane-to-plane) fit F_gicp, the operations in the header's order (numpy rounds every elementwise operation on its own, so
every per-pair quantity is the kernel's bit for bit; the sums are numpy's, so the pose differs from the kernel's by the
summation order and nothing else).  order="tree" takes the sums in the kernel's own order instead -- lane j % 256 over its
j, the xor butterfly of each 64-lane wave, then the four waves -- which is how the GPU test's tolerance is measured.  A run
reports icp_plane_reference's margins (gap, thr, cond, pivot, refused) and the smallest det(W) seen."""
import math

import numpy as np

import icp_plane_reference as pr
import icp_reference as ir

SYM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # the six kept entries of a symmetric 3 x 3


def total(v, order="numpy"):
    """The sum of v [n, ...] over its first axis: numpy's, or the kernel's lane-then-tree order."""
    v = np.asarray(v, np.float64)
    if order == "numpy":
        return v.sum(axis=0)
    lanes = np.zeros((256,) + v.shape[1:])
    for s in range(0, len(v), 256):                               # lane j % 256 over its j in ascending order, from 0
        blk = v[s:s + 256]
        lanes[:len(blk)] = lanes[:len(blk)] + blk
    w = lanes.reshape((4, 64) + v.shape[1:])
    for off in (32, 16, 8, 4, 2, 1):                              # l_i + l_(i xor off): every lane ends with the same sum
        w = w[:, :off] + w[:, off:2 * off]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def cov(v, e1):
    """cov(v) of the header for rows v [n, 3]: (the six entries [n, 6], s > 0 [n])."""
    s = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    with np.errstate(all="ignore"):
        f = np.where(s > 0.0, e1 / np.where(s > 0.0, s, 1.0), 0.0)
    a = f[:, None] * v
    return np.stack([(1.0 if u == w else 0.0) - a[:, u] * v[:, w] for u, w in SYM], axis=1), s > 0.0


def weights(na, kb, Rt, epsilon):
    """Per pair: (M [n, 3, 3] symmetric, det(W) [n], planar [n]) from the anchor normals na [n, 3] and the positive normals
    kb [n, 3] (both as float64 of the float32 values), steps 3 to 5 of F_gicp."""
    e1 = 1.0 - float(epsilon)
    u = np.stack([(Rt[r, 0] * kb[:, 0] + Rt[r, 1] * kb[:, 1]) + Rt[r, 2] * kb[:, 2] for r in range(3)], axis=1)
    CA, pa = cov(na, e1)
    CB, pb = cov(u, e1)
    W = CA + CB
    W00, W01, W02, W11, W12, W22 = (W[:, e] for e in range(6))
    cof = [W11 * W22 - W12 * W12, W02 * W12 - W01 * W22, W01 * W12 - W02 * W11,
           W00 * W22 - W02 * W02, W01 * W02 - W00 * W12, W00 * W11 - W01 * W01]
    det = (W00 * cof[0] + W01 * cof[1]) + W02 * cof[2]
    M = np.zeros((len(na), 3, 3))
    for e, (r, c) in enumerate(SYM):
        M[:, r, c] = M[:, c, r] = cof[e] / det
    return M, det, pa & pb


def pairs(anchor, a_normal, positive, b_normal, nn, Rt, epsilon):
    """The pairs of F_gicp under the pose: (j, m [n, 3], d [n, 3], M [n, 3, 3], det [n], planar [n])."""
    j = np.nonzero(nn >= 0)[0]
    i = nn[j]
    m = ir.move(Rt, np.asarray(positive, np.float32)[j])
    d = np.asarray(anchor, np.float64)[i] - m
    M, det, planar = weights(np.asarray(a_normal, np.float64)[i], np.asarray(b_normal, np.float64)[j], Rt, epsilon)
    return j, m, d, M, det, planar


def system(m, d, M, order="numpy"):
    """(H [6, 6], g [6], c [3]) of steps 2, 6 and 7."""
    n = len(m)
    c = total(m, order) / n
    q = m - c
    q0, q1, q2 = q[:, 0], q[:, 1], q[:, 2]
    b = np.zeros((6, n, 3))                                        # b_v = M j_v
    for r in range(3):
        b[0][:, r] = M[:, r, 2] * q1 - M[:, r, 1] * q2
        b[1][:, r] = M[:, r, 0] * q2 - M[:, r, 2] * q0
        b[2][:, r] = M[:, r, 1] * q0 - M[:, r, 0] * q1
        b[3][:, r], b[4][:, r], b[5][:, r] = M[:, r, 0], M[:, r, 1], M[:, r, 2]
    H, g = np.zeros((6, 6)), np.zeros(6)
    for u in range(6):
        for v in range(u, 6):
            h = (q1 * b[v][:, 2] - q2 * b[v][:, 1] if u == 0 else q2 * b[v][:, 0] - q0 * b[v][:, 2] if u == 1
                 else q0 * b[v][:, 1] - q1 * b[v][:, 0] if u == 2 else b[v][:, u - 3])
            H[u, v] = H[v, u] = total(h, order)
        g[u] = total((b[u][:, 0] * d[:, 0] + b[u][:, 1] * d[:, 1]) + b[u][:, 2] * d[:, 2], order)
    return H, g, c


def jacobian(m, c):
    """J [n, 3, 6] of step 6: the columns j_0 .. j_5 per pair."""
    q = m - c
    J = np.zeros((len(m), 3, 6))
    J[:, 1, 0], J[:, 2, 0] = -q[:, 2], q[:, 1]
    J[:, 0, 1], J[:, 2, 1] = q[:, 2], -q[:, 0]
    J[:, 0, 2], J[:, 1, 2] = -q[:, 1], q[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
    return J


def fit_gicp(anchor, a_normal, positive, b_normal, nn, Rt, epsilon=1e-3, order="numpy"):
    """F_gicp(nn, pose): (the new Rt [3, 4] or None when the pose stays, info dict n_g / cond / pivot / det / s)."""
    j, m, d, M, det, _ = pairs(anchor, a_normal, positive, b_normal, nn, Rt, epsilon)
    info = dict(n_g=len(j), cond=np.inf, pivot=-np.inf, det=float(det.min()) if len(j) else np.inf, s=None)
    if len(j) < 3:
        return None, info
    H, g, c = system(m, d, M, order)
    return pr.solve_compose(H, g, c, Rt, info)


def gicp_stats(anchor, a_normal, positive, b_normal, nn, Rt, epsilon=1e-3, order="numpy"):
    """(num_planar, rmse_gicp) of an association under a pose."""
    j, _, d, M, _, planar = pairs(anchor, a_normal, positive, b_normal, nn, Rt, epsilon)
    if len(j) == 0:
        return 0, np.nan
    y = [(M[:, r, 0] * d[:, 0] + M[:, r, 1] * d[:, 1]) + M[:, r, 2] * d[:, 2] for r in range(3)]
    z = (d[:, 0] * y[0] + d[:, 1] * y[1]) + d[:, 2] * y[2]
    return int(planar.sum()), math.sqrt(total(z, order) / len(j))


def icp_gicp(anchor, a_normal, positive, b_normal, Rt0, max_dist=1.0, iterations=20, na=None, nb=None, valid0=True, epsilon=1e-3,
             order="numpy"):
    """dh3d_icp_refine_gicp on one pair (a_normal [Na, 3], b_normal [Nb, 3] float32).  Returns icp_reference.icp's dict, every
    state with num_planar and rmse_gicp besides, and the margins gap / thr, cond (the largest cond(H) of a step taken), pivot
    (the smallest Cholesky pivot ratio of a step taken), refused (the largest pivot ratio that made a step with 3 or more pairs
    leave the pose; -inf without one) and det (the smallest det(W) of a fit)."""
    a_normal, b_normal = np.asarray(a_normal, np.float32), np.asarray(b_normal, np.float32)

    def step(anchor, positive, nn, Rt, out):
        new, info = fit_gicp(anchor, a_normal, positive, b_normal, nn, Rt, epsilon, order)
        out["det"] = min(out["det"], info["det"])
        return pr.take_step(out, new, info, info["n_g"] >= 3)
    return ir.loop(anchor, positive, Rt0, step, lambda a, y, nn, Rt: gicp_stats(a, a_normal, y, b_normal, nn, Rt, epsilon, order),
                   ("num_planar", "rmse_gicp"), dict(pr.SOLVE_MARGINS, det=np.inf), max_dist, iterations, na, nb, valid0)


def is_clear(run):
    """icp_plane_reference.is_clear's caps: no decision of the run hangs on a last-bit rounding."""
    return pr.is_clear(run)


def clear_pair_gicp(name, n, max_dist, iterations, base=1, k=16, epsilon=1e-3):
    """The first demo_pair (seeds base, base + 1, ... at most 50) whose generalized run is clear, normals of both clouds from
    icp_plane_reference.demo_normals.  Returns (pair, anchor normals, positive normals, run, seed)."""
    for s in range(base, base + 50):
        pair = ir.demo_pair(name, n, s)
        an, bn = pr.demo_normals(pair[0], k), pr.demo_normals(pair[1], k)
        run = icp_gicp(pair[0], an, pair[1], bn, pair[3], max_dist=max_dist, iterations=iterations, epsilon=epsilon)
        if is_clear(run):
            return pair, an, bn, run, s
    raise AssertionError("no clear fixture for %s n=%d max_dist=%g" % (name, n, max_dist))
