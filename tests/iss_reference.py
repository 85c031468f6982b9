"""numpy restatement of ISS keypoints as include/dh3d_hip.h dh3d_iss_keypoints states them (steps 1 to 5), for the tests of
csrc/iss.hip: brute-force memberships in float32 exactly as stated, float64 moments, np.linalg.eigvalsh, the suppression
with ties to the lowest index and the selection.  Per point it also reports the decision margin of step 3,
min(|l2 - g21 l1|, |l3 - g32 l2|, |l3|) / r_s^2: where it is large the saliency's sign cannot depend on the last bits of
the eigenvalues.  Everything here works on ONE cloud [N, 3] float32 with n valid rows."""

import numpy as np

import icp_reference as ir
import scan_context_reference as scr
import spatial_reference as sr

F = np.float32
GAMMA = 0.975
MIN_NEIGHBORS = 5
CHUNK = 256


def membership(X, n, r, rows):
    """Step 1 for the points `rows` (a slice): bool [len(rows), n], j in the ball of i.  float32, unfused, strict."""
    X = np.ascontiguousarray(X, F)
    r = F(r)
    if not r > 0:                                   # <= 0 or NaN: no members
        return np.zeros((len(X[rows]), n), bool)
    d = X[None, :n, :] - X[rows, None, :]           # float32 differences x_j - x_i
    dx, dy, dz = d[:, :, 0], d[:, :, 1], d[:, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz              # every product and sum a float32 operation of its own
    return d2 < r * r                               # the product in float32


def compute(X, n, r_s, r_n, gamma_21=GAMMA, gamma_32=GAMMA, min_neighbors=MIN_NEIGHBORS):
    """Steps 1 to 3 -> dict(num_nbr [N, 2] int32, lam [N, 3] float64 (l1 >= l2 >= l3; 0 where m = 0 or i >= n),
    saliency [N] float32, margin [N] float64 (inf where i >= n or m < min_neighbors))."""
    X = np.ascontiguousarray(X, F)
    N = len(X)
    X64 = X.astype(np.float64)
    num = np.zeros((N, 2), np.int32)
    lam = np.zeros((N, 3), np.float64)
    for s in range(0, n, CHUNK):
        rows = slice(s, min(s + CHUNK, n))
        S = membership(X, n, r_s, rows)
        T = membership(X, n, r_n, rows)
        num[rows, 0], num[rows, 1] = S.sum(1), T.sum(1)
        e = (X64[None, :n, :] - X64[rows, None, :]) * S[:, :, None]      # float64 differences of their own, 0 outside S_i
        m = np.maximum(S.sum(1), 1).astype(np.float64)
        u = e.sum(1) / m[:, None]
        C = np.einsum("ija,ijb->iab", e, e) / m[:, None, None] - u[:, :, None] * u[:, None, :]
        lam[rows] = np.linalg.eigvalsh(C)[:, ::-1]
    m = num[:, 0]
    lam[m == 0] = 0.0
    l1, l2, l3 = lam[:, 0], lam[:, 1], lam[:, 2]
    ok = (m >= min_neighbors) & (l2 < gamma_21 * l1) & (l3 < gamma_32 * l2) & (l3 > 0) & (np.arange(N) < n)
    sal = np.where(ok, l3.astype(F), F(0)).astype(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.minimum(np.minimum(np.abs(l2 - gamma_21 * l1), np.abs(l3 - gamma_32 * l2)), np.abs(l3)) / (float(r_s) ** 2)
    margin = np.where((np.arange(N) < n) & (m >= min_neighbors), margin, np.inf)   # below min_neighbors the eigenvalues decide nothing
    return dict(num_nbr=num, lam=lam, saliency=sal, margin=margin)


def keypoint_mask(X, n, r_n, sal, num_t, min_neighbors=MIN_NEIGHBORS):
    """Step 4 on given saliencies [N] float32 and |T_i| [N] -> (is keypoint [N] bool, decided by the tie rule [N] bool: a
    candidate that no neighbour beats outright and that has a neighbour of its own saliency -- it wins or loses by its index)."""
    N = len(X)
    sal = np.asarray(sal, F)
    key = np.zeros(N, bool)
    tie = np.zeros(N, bool)
    idx = np.arange(n)
    for s in range(0, n, CHUNK):
        rows = slice(s, min(s + CHUNK, n))
        T = membership(X, n, r_n, rows)
        si = sal[rows, None]
        sj = sal[None, :n]
        other = T & (idx[None, :] != np.arange(rows.start, rows.stop)[:, None])
        with np.errstate(invalid="ignore"):
            greater = other & (sj > si)
            equal = other & (sj == si)
            cand = (sal[rows] > 0) & (num_t[rows] >= min_neighbors)
        lower = equal & (idx[None, :] < np.arange(rows.start, rows.stop)[:, None])
        key[rows] = cand & ~greater.any(1) & ~lower.any(1)
        tie[rows] = cand & ~greater.any(1) & equal.any(1)
    return key, tie


def select(key, sal, M):
    """Step 5 -> (ids [M] int32, -1 padded, count)."""
    k = np.flatnonzero(key)
    order = k[np.lexsort((k, -np.asarray(sal, np.float64)[k]))][:M]     # s descending, index ascending
    ids = np.full(M, -1, np.int32)
    ids[:len(order)] = order
    return ids, len(order)


def keypoints(X, n, r_n, sal, num_t, M, min_neighbors=MIN_NEIGHBORS):
    key, _ = keypoint_mask(X, n, r_n, sal, num_t, min_neighbors)
    return select(key, sal, M)


def shell_pairs(X, n, r):
    """Pairs (i, j), i != j, at exactly d2 == r * r in the float32 arithmetic of step 1."""
    X = np.ascontiguousarray(X, F)
    r2 = F(r) * F(r)
    hits = 0
    for s in range(0, n, CHUNK):
        d = X[None, :n, :] - X[s:min(s + CHUNK, n), None, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        hits += int((d2 == r2).sum())
    return hits


# ------------------------------------------------------------------------------------------------------------ the sort
def packed(X, n):
    """What the sort sees: rows r >= n are copies of row r % n (csrc/cloud_pack.h)."""
    X = np.ascontiguousarray(X, F)
    if n == 0 or n == len(X):
        return X
    r = np.arange(len(X))
    return X[np.where(r < n, r, r % n)]


def grid_facts(X, n, r):
    """(crowded flag, the number of table cells the box x_i +- r meets for every valid point) through
    spatial_reference.restate -- the margin as csrc/iss.hip's iss_walk forms it, in float32."""
    P = packed(X, n)
    g = sr.restate(P)
    lo, scale = g["lo"], g["scale"]
    qmax = np.array([(4 << b) - 1 for b in g["nb"]], F)
    q, r = P[:n], F(r)
    marg = r * F(1e-5) + np.abs(q) * F(1e-6)

    def cell(p):
        t = np.minimum(np.maximum((p - lo[None, :]) * scale[None, :], F(0)), F(1.0e6))
        return np.minimum(qmax[None, :].astype(np.int64), np.trunc(t).astype(np.int64)) >> 2
    cn = cell((q + r) + marg) - cell((q - r) - marg) + 1
    return int(g["cells"][4106]), cn.prod(1)


# ------------------------------------------------------------------------------------------------------------ fixtures
N_DEMO = 2048
SMALL, WIDE = (2.0, 1.5), (12.0, 9.0)
DEMO_NAMES = ("local_642", "global_c", "dso_9000")
_CLOUDS = {}


def cloud(name):
    """The named cloud [N, 3] float32 and its count n."""
    if name not in _CLOUDS:
        if name == "cube":
            c = (np.random.default_rng(2009).uniform(-20.0, 20.0, (N_DEMO, 3)).astype(F), N_DEMO)
        elif name == "scene0":
            c = (scr.scene(0)[:N_DEMO].astype(F), N_DEMO)
        elif name in DEMO_NAMES:
            c = (ir.demo_pair(name, N_DEMO, 1)[0], N_DEMO)
        elif name == "dso_9000_cut":
            x = cloud("dso_9000")[0].copy()
            x[1024:] = F(100000.0)
            c = (x, 1024)
        elif name == "lattice":
            g = np.arange(12, dtype=F) * F(0.5)
            c = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F), 12 ** 3)
        else:
            raise KeyError(name)
        _CLOUDS[name] = c
    return _CLOUDS[name]


# (case id, cloud, (r_s, r_n)); the lattice is compared on its counts only
CASES = (("cube-5-4", "cube", (5.0, 4.0)), ("cube-wide", "cube", WIDE), ("scene0-small", "scene0", SMALL),
         ("scene0-wide", "scene0", WIDE)) + \
    tuple(("%s-%s" % (nm, tag), nm, rr) for nm in DEMO_NAMES for tag, rr in (("small", SMALL), ("wide", WIDE))) + \
    (("dso_9000_cut-small", "dso_9000_cut", SMALL), ("lattice", "lattice", (1.5, 1.0)))
CASE_IDS = tuple(c[0] for c in CASES)
_RESULTS = {}


def case(case_id):
    """(X, n, r_s, r_n, the restatement's compute()) of a named case; computed once, never changed."""
    if case_id not in _RESULTS:
        _, name, (r_s, r_n) = CASES[CASE_IDS.index(case_id)]
        X, n = cloud(name)
        _RESULTS[case_id] = (X, n, r_s, r_n, compute(X, n, r_s, r_n))
    return _RESULTS[case_id]


def moved_pairs():
    """The three moved pairs of the FPFH end-to-end test, built here again: the anchor subset of a demo pair and the same
    points moved by the inverse of Rt_gt, permuted, with 0.02 m of noise (anchor ~ R positive + t)."""
    rng = np.random.default_rng(77)
    A, B, T = [], [], []
    for name in DEMO_NAMES:
        a, _, Rt, _ = ir.demo_pair(name, N_DEMO, 1)
        R, t = Rt[:, :3], Rt[:, 3]
        y = ((a.astype(np.float64) - t) @ R + rng.normal(0.0, 0.02, a.shape))[rng.permutation(N_DEMO)].astype(F)
        A.append(a), B.append(y), T.append(Rt)
    return np.stack(A), np.stack(B), np.stack(T)
