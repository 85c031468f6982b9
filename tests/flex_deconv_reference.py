"""float64 numpy restatement of flex_convolution_transpose (FlexDeconv) and its gradients, the yardstick of
tests/test_flex_deconv_*.py.  Written from the operator's definition, one edge (n, k) at a time with np.add.at:
centre s = nbr[b,0,n], target m = nbr[b,k,n],

    out[b,:,m]        += sum_din f[b,din,s] (bias[din,:] + sum_dp theta[dp,din,:] (p[b,dp,m] - p[b,dp,s]))
    grad_f[b,:,s]     += (bias + sum_dp theta_dp (p_m - p_s)_dp) @ g[b,:,m]
    grad_bias         += f[b,:,s] (x) g[b,:,m]
    grad_theta[dp]    += (p_m - p_s)_dp f[b,:,s] (x) g[b,:,m]
"""
import numpy as np


def _edges(nbr):
    """Per cloud: centre ids [K*N], target ids [K*N] of every edge (n, k)."""
    K, N = nbr.shape
    return np.broadcast_to(nbr[0], (K, N)).reshape(-1), nbr.reshape(-1)


def flex_deconv(features, position, neighborhood, theta, bias):
    f, p = np.asarray(features, np.float64), np.asarray(position, np.float64)
    th, bi = np.asarray(theta, np.float64), np.asarray(bias, np.float64)
    B, Din, N = f.shape
    Dout = th.shape[2]
    out = np.zeros((B, Dout, N))
    for b in range(B):
        s, m = _edges(np.asarray(neighborhood[b]))
        q = p[b][:, m] - p[b][:, s]                                   # [Dp, E]
        fs = f[b][:, s].T                                             # [E, Din]
        contrib = fs @ bi                                             # [E, Dout]: per edge, w = bias + sum_d q_d theta_d
        for d in range(th.shape[0]):
            contrib += q[d][:, None] * (fs @ th[d])
        acc = np.zeros((N, Dout))
        np.add.at(acc, m, contrib)
        out[b] = acc.T
    return out


def flex_deconv_grad(features, position, neighborhood, theta, bias, topdiff):
    f, p = np.asarray(features, np.float64), np.asarray(position, np.float64)
    th, bi = np.asarray(theta, np.float64), np.asarray(bias, np.float64)
    g = np.asarray(topdiff, np.float64)
    B, Din, N = f.shape
    gf, gt, gb = np.zeros_like(f), np.zeros_like(th), np.zeros_like(bi)
    for b in range(B):
        s, m = _edges(np.asarray(neighborhood[b]))
        q = p[b][:, m] - p[b][:, s]                                   # [Dp, E]
        gm = g[b][:, m]                                               # [Dout, E]
        fs = f[b][:, s]                                               # [Din, E]
        per_edge = (bi @ gm).T                                        # [E, Din]: w(e) @ g[m_e]
        for d in range(th.shape[0]):
            per_edge += q[d][:, None] * (th[d] @ gm).T
        acc = np.zeros((N, Din))
        np.add.at(acc, s, per_edge)
        gf[b] = acc.T
        gb += fs @ gm.T
        for d in range(th.shape[0]):
            gt[d] += (fs * q[d]) @ gm.T
    return gf, gt, gb


def flex_deconv_loops(features, position, neighborhood, theta, bias):
    """The same forward as literal loops over (b, n, k, din, dout) (tiny sizes only)."""
    B, Din, N = features.shape
    Dp, _, Dout = theta.shape
    K = neighborhood.shape[1]
    out = np.zeros((B, Dout, N))
    for b in range(B):
        for n in range(N):
            s = int(neighborhood[b, 0, n])
            for k in range(K):
                m = int(neighborhood[b, k, n])
                for i in range(Din):
                    for o in range(Dout):
                        w = float(bias[i, o])
                        for d in range(Dp):
                            w += float(theta[d, i, o]) * (float(position[b, d, m]) - float(position[b, d, s]))
                        out[b, o, m] += float(features[b, i, s]) * w
    return out


def knn_lists(position, K):
    """[B, K, N] int32 kNN lists (rank 0 = the point itself for distinct points), brute force in float64 (small N)."""
    p = np.asarray(position, np.float64)
    B, _, N = p.shape
    out = np.empty((B, K, N), np.int32)
    for b in range(B):
        d = ((p[b][:, :, None] - p[b][:, None, :]) ** 2).sum(0)
        out[b] = np.argsort(d, axis=1, kind="stable")[:, :K].T
    return out


def neighbourhood(kind, B, N, K, rng, position=None):
    """[B, K, N] int32 test neighbourhoods: 'knn', 'random' (rank 0 not the point), 'dup' (repeated ids within a list),
    'hub' (rank 1 of every list is point 0: in-degree >= N), 'hub0' (rank 0 of every list is point 0: every point's centre),
    'holes' (ids from the first half only: the rest is named by no list)."""
    if kind == "knn":
        return knn_lists(position, K)
    if kind == "random":
        nb = rng.integers(0, N, (B, K, N)).astype(np.int32)
        nb[:, 0] = (np.arange(N) + 1 + rng.integers(0, N - 1, (B, N))) % N  # never the point itself
        return nb
    if kind == "dup":
        nb = rng.integers(0, N, (B, K, N)).astype(np.int32)
        nb[:, 0] = np.arange(N)
        nb[:, K - 1] = nb[:, 1]
        nb[:, K - 2] = nb[:, 0]
        return nb
    if kind == "hub":
        nb = rng.integers(0, N, (B, K, N)).astype(np.int32)
        nb[:, 0] = np.arange(N)
        nb[:, 1] = 0
        return nb
    if kind == "hub0":
        nb = rng.integers(0, N, (B, K, N)).astype(np.int32)
        nb[:, 0] = 0
        return nb
    if kind == "holes":
        nb = rng.integers(0, N // 2, (B, K, N)).astype(np.int32)
        return nb
    raise ValueError(kind)
