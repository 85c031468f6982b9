"""A numpy float64 restatement of include/dh3d_hip.h dh3d_spfh_counts and dh3d_fpfh, the operations in the header's order
(numpy rounds every elementwise operation on its own, so the pair coordinates s1..s3 are the kernel's up to the last bits of
atan2, and the sums run in list order as the kernel's do).  The yardstick of dh3d_amd.registration.compute_fpfh.  Besides
the counts it reports per point how close a bin decision came to being turned by a last-bit rounding: `margin`, the smallest
distance of any of the point's pair coordinates to an interior bin edge (1 .. 10)."""
import numpy as np

BINS, COLS = 11, 36


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _clamp(n, N):
    return N if n is None else min(max(int(n), 0), N)


def pairs(x, nbr, n=None, max_dist=None):
    """The pairs of every point i < n: (safe [n, K] ids (0 where the pair is not near), near [n, K] bool, d [n, K, 3],
    d2 [n, K])."""
    x = np.asarray(x, np.float32).astype(np.float64)
    nbr = np.asarray(nbr)
    n = _clamp(n, len(x))
    ids = nbr[:n].astype(np.int64)
    inb = (ids >= 0) & (ids < n) & (ids != np.arange(n)[:, None])
    safe = np.where(inb, ids, 0)
    d = x[:n][safe] - x[:n, None, :] if n else np.zeros((0, nbr.shape[1], 3))
    d2 = dot(d, d)
    near = inb & (d2 > 0.0)
    if max_dist is not None and max_dist > 0.0:
        near &= d2 <= float(max_dist) * float(max_dist)
    return np.where(near, safe, 0), near, d, d2


def edge_distance(s):
    """Distance of a bin coordinate to the nearest interior bin edge 1 .. 10."""
    return np.abs(s - np.clip(np.rint(s), 1.0, 10.0))


def spfh_counts(x, normals, nbr, n=None, max_dist=None):
    """Stage 1 on one cloud: x [N, 3], normals [N, 3] float32, nbr [N, K].  Returns a dict: counts [N, 36] uint8, margin [N]
    (inf for a point without usable pairs), usable / near [N, K] bool, s [N, K, 3] (the bin coordinates, NaN where unusable)
    and bins [N, K, 3]."""
    N, K = np.asarray(nbr).shape
    n = _clamp(n, N)
    nr = np.asarray(normals, np.float32).astype(np.float64)
    out = dict(counts=np.zeros((N, COLS), np.uint8), margin=np.full(N, np.inf), usable=np.zeros((N, K), bool),
               near=np.zeros((N, K), bool), s=np.full((N, K, 3), np.nan), bins=np.zeros((N, K, 3), np.int64))
    if n == 0:
        return out
    safe, near, d, d2 = pairs(x, nbr, n, max_dist)
    ni = np.broadcast_to(nr[:n, None, :], d.shape)
    nj = nr[:n][safe]
    with np.errstate(all="ignore"):
        ok = near & (dot(ni, ni) > 0.0) & (dot(nj, nj) > 0.0)
        ln = np.sqrt(d2)
        a1, a2 = dot(ni, d) / ln, dot(nj, d) / ln
        swap = np.abs(a1) < np.abs(a2)
        n1, n2 = np.where(swap[..., None], nj, ni), np.where(swap[..., None], ni, nj)
        dd = np.where(swap[..., None], -d, d)
        f3 = np.where(swap, -a2, a1)
        v = cross(dd, n1)
        vn = np.sqrt(dot(v, v))
        ok &= vn > 0.0
        v = v / vn[..., None]
        w = cross(n1, v)
        f2 = dot(v, n2)
        f1 = np.arctan2(dot(w, n2), dot(n1, n2))
        s = np.stack([(f1 + np.pi) * (11.0 / (2.0 * np.pi)), (f2 + 1.0) * 5.5, (f3 + 1.0) * 5.5], axis=-1)
    s = np.where(ok[..., None], s, np.nan)
    bins = np.where(ok[..., None], np.minimum(np.maximum(np.floor(np.nan_to_num(s)), 0.0), 10.0), 0.0).astype(np.int64)
    cnt = np.zeros((n, COLS), np.int64)
    rows = np.broadcast_to(np.arange(n)[:, None], ok.shape)
    for f in range(3):
        np.add.at(cnt, (rows[ok], f * BINS + bins[..., f][ok]), 1)
    cnt[:, 3 * BINS] = ok.sum(axis=1)
    out["counts"][:n] = cnt.astype(np.uint8)
    edge = np.where(ok[..., None], edge_distance(np.nan_to_num(s)), np.inf)
    out["margin"][:n] = edge.reshape(n, -1).min(axis=1)
    out["usable"][:n], out["near"][:n], out["s"][:n], out["bins"][:n] = ok, near, s, bins
    return out


def spfh(counts):
    """SPFH rows [N, 33] float64 of count rows [N, 36]: counts * (100.0 / m), zero where m = 0."""
    c = np.asarray(counts).astype(np.float64)
    m = c[:, 3 * BINS]
    with np.errstate(all="ignore"):
        f = np.where(m > 0, 100.0 / m, 0.0)
    return c[:, :3 * BINS] * f[:, None]


def fpfh(x, nbr, counts, n=None, max_dist=None, ids=None):
    """Stage 2 on one cloud from stage 1's counts [N, 36].  Returns (rows [M, 36] float64 before the rounding to float32,
    columns 33-35 zero; M = N without ids)."""
    N, K = np.asarray(nbr).shape
    n = _clamp(n, N)
    sp = spfh(counts)
    full = np.zeros((N, COLS))
    if n:
        safe, near, _, d2 = pairs(x, nbr, n, max_dist)
        with np.errstate(all="ignore"):
            w = np.where(near, 1.0 / d2, 0.0)
        acc = np.zeros((n, 3 * BINS))
        for k in range(K):  # list order; a pair that is not near adds 0.0, which changes no sum
            acc = acc + w[:, k:k + 1] * np.where(near[:, k:k + 1], sp[safe[:, k]], 0.0)
        for t in range(3):
            blk = acc[:, t * BINS:(t + 1) * BINS]
            S = np.zeros(n)
            for e in range(BINS):
                S = S + blk[:, e]
            with np.errstate(all="ignore"):
                scale = np.where(S > 0.0, 100.0 / S, 0.0)
            full[:n, t * BINS:(t + 1) * BINS] = blk * scale[:, None] + sp[:n, t * BINS:(t + 1) * BINS]
    if ids is None:
        return full
    ids = np.asarray(ids).astype(np.int64)
    ok = (ids >= 0) & (ids < n)
    return np.where(ok[:, None], full[np.where(ok, ids, 0)], 0.0)


def compute(x, normals, nbr, n=None, max_dist=None, ids=None):
    """Both stages.  Returns stage 1's dict plus fpfh [M, 36] float64 and clear [N] bool: the point's own margin and the
    margins of all its near neighbours are >= 1e-9 (its FPFH row then depends on no bin decision a rounding could turn)."""
    out = spfh_counts(x, normals, nbr, n, max_dist)
    out["fpfh"] = fpfh(x, nbr, out["counts"], n, max_dist, ids)
    N = len(out["margin"])
    nn = _clamp(n, N)
    own = out["margin"] >= 1e-9
    clear = own.copy()
    if nn:
        safe, near, _, _ = pairs(x, nbr, nn, max_dist)
        clear[:nn] &= np.where(near, own[:nn][safe], True).all(axis=1)
    out["clear"] = clear
    return out


# ------------------------------------------------------------------------------------------------------------ fixtures

N_DEMO, COUNTS, KS = 2048, (2048, 2048, 1024), (1, 3, 16, 17, 33, 64)
_DEMO = {}


def demo_fixture():
    """The anchors of the three demo pairs (icp_reference.demo_pair(name, 2048, 1); dso_9000 behind a count of 1024, real
    points after it), their 64 nearest neighbours by brute force among the counted rows (the point itself first) and the
    normals of the restatement (icp_plane_reference.normals at k = 16, viewpoint 0) rounded to float32.  Computed once."""
    if not _DEMO:
        import icp_plane_reference as pr
        import icp_reference as ir
        X = np.stack([ir.demo_pair(name, N_DEMO, 1)[0] for name in ("local_642", "global_c", "dso_9000")])
        ids = np.stack([pr.knn_ids(X[p], 64, COUNTS[p]) for p in range(3)])
        nrm = np.stack([pr.normals(X[p], ids[p][:, :16], COUNTS[p])["normals"].astype(np.float32) for p in range(3)])
        _DEMO.update(X=X, ids=ids, normals=nrm, count=np.array(COUNTS, np.int32))
    return _DEMO
