"""A numpy float64 / uint64 restatement of the training-batch builders (include/dh3d_hip.h "Training batches"), written
from that text: one cloud or one pair at a time, the way the reference's loader runs (core/datasets.py loadPair / loadPC).
Nothing here looks at the kernels.  Every function takes the cloud's index b in its batch: the draws are a pure function
of (seed, stream, b, element)."""
import numpy as np

U64 = np.uint64
RESAMPLE, PAD, ROTATE1D, JITTER, SCALE, ROTATESMALL, SHIFT, PAIRROT, SUBSET, FIRST = range(1, 11)
AUG_ORDER = ("Rotate1D", "Jitter", "Scale", "RotateSmall", "Shift")
DEFAULTS = dict(sigma=0.05, clip=0.1, scale_low=0.8, scale_high=1.25, angle_sigma=0.06, angle_clip=0.18, shift_range=0.1)


def splitmix64(z):
    z = np.asarray(z, dtype=U64)
    with np.errstate(over="ignore"):
        z = z + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def h(seed, stream, b):
    return splitmix64(splitmix64(U64(int(seed) & 0xFFFFFFFFFFFFFFFF)) ^ U64((int(stream) << 32) | int(b)))


def u(seed, stream, b, j):
    """u(stream, b, j) for an array (or one value) of j."""
    with np.errstate(over="ignore"):
        return splitmix64(h(seed, stream, b) + np.asarray(j, dtype=U64))


def unit_co(x):  # [0, 1)
    return (np.asarray(x, dtype=U64) >> U64(11)).astype(np.float64) * 2.0 ** -53


def unit_oc(x):  # (0, 1]
    return unit_co(x) + 2.0 ** -53


def normal(seed, stream, b, e):
    e = np.asarray(e, dtype=U64)
    u1 = unit_oc(u(seed, stream, b, U64(2) * e))
    u2 = unit_co(u(seed, stream, b, U64(2) * e + U64(1)))
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def choice(seed, stream, b, n, m):
    """m of n without replacement: the m smallest (u, i), in index order."""
    keys = u(seed, stream, b, np.arange(n))
    return np.sort(np.argsort(keys, kind="stable")[:m])


def resample_cloud(points, n, targetnum, seed, b):
    """points [Nsrc, 3] float32, of which rows 0 .. n-1 are the cloud -> (out [targetnum, 3] float32, num_orig)."""
    n = int(min(max(n, 0), points.shape[0]))
    if n == 0:
        return np.full((targetnum, 3), 100000.0, dtype=np.float32), 0
    cloud = points[:n]
    if n >= targetnum:
        return cloud[choice(seed, RESAMPLE, b, n, targetnum)].copy(), targetnum
    draws = (u(seed, PAD, b, np.arange(targetnum - n)) % U64(n)).astype(np.int64)
    return np.concatenate([cloud, cloud[draws]], axis=0), n


def rot_z(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])


def mat3_mul(A, B):
    C = np.empty((3, 3))
    for r in range(3):
        for c in range(3):
            C[r, c] = (A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]
    return C


def rows_mat3(P, M):
    """row * M for every row of P [N, 3] float64, each element (x M0c + y M1c) + z M2c."""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([(x * M[0, c] + y * M[1, c]) + z * M[2, c] for c in range(3)], axis=1)


def augment_params(aug, seed, b, **kw):
    p = dict(DEFAULTS, **kw)
    out = {"rot1d": np.eye(3), "scale": 1.0, "rot_small": np.eye(3), "shift": np.zeros(3)}
    if "Rotate1D" in aug:
        out["rot1d"] = rot_z(float(unit_co(u(seed, ROTATE1D, b, 0))) * 2 * np.pi)
    if "Scale" in aug:
        out["scale"] = p["scale_low"] + (p["scale_high"] - p["scale_low"]) * float(unit_co(u(seed, SCALE, b, 0)))
    if "RotateSmall" in aug:
        a = np.clip(p["angle_sigma"] * normal(seed, ROTATESMALL, b, np.arange(3)), -p["angle_clip"], p["angle_clip"])
        Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        Rz = np.array([[np.cos(a[2]), -np.sin(a[2]), 0], [np.sin(a[2]), np.cos(a[2]), 0], [0, 0, 1]])
        out["rot_small"] = mat3_mul(Rz, mat3_mul(Ry, Rx))
    if "Shift" in aug:
        r = p["shift_range"]
        out["shift"] = -r + (r - -r) * unit_co(u(seed, SHIFT, b, np.arange(3)))
    return out


def jitter_values(n, seed, b, sigma=0.05, clip=0.1):
    """The clipped jitter [n, 3] and the normals before scaling and clipping."""
    z = normal(seed, JITTER, b, np.arange(3 * n)).reshape(n, 3)
    return np.clip(sigma * z, -clip, clip), z


def augment_cloud64(points, aug, seed, b, **kw):
    """The float64 chain on points [N, 3] float32 -> (float64 result, params)."""
    for name in aug:
        if name not in AUG_ORDER:
            raise ValueError(name)
    p = dict(DEFAULTS, **kw)
    par = augment_params(aug, seed, b, **kw)
    v = points.astype(np.float64)
    if "Rotate1D" in aug:
        v = rows_mat3(v, par["rot1d"])
    if "Jitter" in aug:
        v = jitter_values(v.shape[0], seed, b, p["sigma"], p["clip"])[0] + v
    if "Scale" in aug:
        v = v * par["scale"]
    if "RotateSmall" in aug:
        v = rows_mat3(v, par["rot_small"])
    if "Shift" in aug:
        v = v + par["shift"]
    return v, par


def augment_cloud(points, aug, seed, b, **kw):
    v, par = augment_cloud64(points, aug, seed, b, **kw)
    return v.astype(np.float32), par


def pair_rotation(seed, b, rot_maxv=np.pi):
    return rot_z((2.0 * float(unit_co(u(seed, PAIRROT, b, 0))) - 1.0) * rot_maxv)


def rotate_cloud(pc2, Rot):
    return rows_mat3(pc2.astype(np.float64), Rot).astype(np.float32)


def d2(p, Q):
    """(dx*dx + dy*dy) + dz*dz in float64 from point p [3] to every row of Q [n, 3] (float32 inputs)."""
    d = p.astype(np.float64)[None, :] - Q.astype(np.float64)
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def _gap(values, rows, best_at, largest):
    """Relative gap between the best value and the best among rows not identical to the best row (inf: there is none)."""
    other = ~np.all(rows == rows[best_at], axis=1)
    if not other.any():
        return np.inf
    best = values[best_at]
    second = values[other].max() if largest else values[other].min()
    scale = max(best, second)
    return abs(best - second) / scale if scale > 0 else 0.0


def sample_pair_nodes(pc1, pc2, sample_nodes, seed, b, nn="brute", report=None):
    """pc1, pc2 [N, 3] float32 -> (anc [M], pos [M]) int32.  nn: "brute" (the rule itself) or "kdtree"
    (scipy.spatial.cKDTree, the arrangement of the reference's loader; used for timing only).  report: a dict that
    receives min_gap, the smallest relative gap between the best and the second-best d2 among non-identical rows."""
    N = pc1.shape[0]
    half = N // 2
    subset = choice(seed, SUBSET, b, N, half)
    pts = pc1[subset]
    picks = [int(u(seed, FIRST, b, 0) % U64(half))]
    dmin = d2(pts[picks[0]], pts)
    gaps = []
    for _ in range(1, sample_nodes):
        nxt = int(np.argmax(dmin))  # the first maximum
        if report is not None:
            gaps.append(_gap(dmin, pts, nxt, True))
        picks.append(nxt)
        dmin = np.minimum(dmin, d2(pts[nxt], pts))
    anc = subset[np.asarray(picks)]
    if nn == "kdtree":
        from scipy.spatial import cKDTree
        pos = cKDTree(pc2).query(pc1[anc], k=1)[1].reshape(-1)
    else:
        pos = np.empty(sample_nodes, dtype=np.int64)
        for t, a in enumerate(anc):
            d = d2(pc1[a], pc2)
            pos[t] = int(np.argmin(d))  # the lowest j on ties
            if report is not None:
                gaps.append(_gap(d, pc2, pos[t], False))
    if report is not None:
        report["min_gap"] = min(gaps) if gaps else np.inf
    return anc.astype(np.int32), pos.astype(np.int32)


def make_local_pairs(src, num_valid, numpts, sample_nodes, seed, rot_maxv=np.pi, aug=("Jitter",), nn="brute"):
    """src [B, Nsrc, 3] float32 -> the dict of dh3d_amd.pairs.make_local_pairs, built pair by pair."""
    B = len(src)
    pc1, pc2, pc2t, R, anc, pos = [], [], [], [], [], []
    for b in range(B):
        a = augment_cloud(resample_cloud(src[b], num_valid[b], numpts, seed, b)[0], aug, seed, b)[0]
        c = augment_cloud(resample_cloud(src[b], num_valid[b], numpts, seed, B + b)[0], aug, seed, B + b)[0]
        Rot = pair_rotation(seed, b, rot_maxv)
        i, j = sample_pair_nodes(a, c, sample_nodes, seed, b, nn=nn)
        pc1.append(a), pc2.append(c), pc2t.append(rotate_cloud(c, Rot)), R.append(Rot.astype(np.float32)), anc.append(i), pos.append(j)
    return {"points": np.stack(pc1 + pc2t), "R": np.stack(R), "sample_idx": np.stack(anc + pos), "pc2": np.stack(pc2)}


def make_global_batch(clouds, num_valid, numpts, seed, aug=("Jitter", "RotateSmall", "Shift", "Rotate1D")):
    return np.stack([augment_cloud(resample_cloud(clouds[b], num_valid[b], numpts, seed, b)[0], aug, seed, b)[0]
                     for b in range(len(clouds))])
