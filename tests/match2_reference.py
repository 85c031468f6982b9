"""numpy restatement of dh3d_match_descriptors2 (include/dh3d_hip.h, csrc/match.hip) and the fixtures of its tests.

    rule_sums     S(i, j): the float32 sum over d ascending of (a_d - b_d)^2, every operation rounded on its own
    match2        the two best, the reverse best and the kept mask from S alone
    screen        what the kernel's f32 MFMA screen computes for a pair -- the norms in the kernel's order, the dot product
                  as an fma chain in the kernel's k order, each fma rounded through float64 -- next to its bound E
    unit, planted, fpfh_like, shared_offset, all_equal, ulp_neighbours, with_duplicates     case builders
"""
import numpy as np

F = np.float32


def rule_sums(a, b, chunk=512):
    """S [na, nb] float32."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    na, nb, D = len(a), len(b), a.shape[1]
    S = np.zeros((na, nb), F)
    bt = np.ascontiguousarray(b.T)
    for s in range(0, na, chunk):
        acc = S[s:s + chunk]
        d = np.empty_like(acc)
        for c in range(D):
            np.subtract(a[s:s + chunk, c, None], bt[c][None, :], out=d)
            np.multiply(d, d, out=d)
            np.add(acc, d, out=acc)
    return S


def _two_smallest(S):
    """Per row of S the two smallest (value, column) in lexicographic order; -1 / inf where none (inf and NaN are no
    neighbour)."""
    n, m = S.shape
    id1, id2 = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    s1, s2 = np.full(n, np.inf, F), np.full(n, np.inf, F)
    if n == 0 or m == 0:
        return id1, s1, id2, s2
    W = np.where(S < np.inf, S, np.inf).astype(F)
    rows = np.arange(n)
    j = W.argmin(axis=1)                         # first occurrence: the lowest id of a tie
    ok = W[rows, j] < np.inf
    id1[ok], s1[ok] = j[ok], W[rows, j][ok]
    W[rows, j] = np.inf
    j = W.argmin(axis=1)
    ok = W[rows, j] < np.inf
    id2[ok], s2[ok] = j[ok], W[rows, j][ok]
    return id1, s1, id2, s2


def match2(a, b, na, nb, ratio=None, mutual=False, S=None):
    """The outputs of one pair, as arrays over all Ma = len(a) / Mb = len(b) rows.  S: rule_sums(a[:na], b[:nb]) when the
    caller has it already.  Also s1 / s2, the float32 sums behind dist1 / dist2."""
    Ma, Mb = len(a), len(b)
    na, nb = min(max(int(na), 0), Ma), min(max(int(nb), 0), Mb)
    if S is None:
        S = rule_sums(a[:na], b[:nb])
    out = dict(nn1=np.full(Ma, -1, np.int32), nn2=np.full(Ma, -1, np.int32), s1=np.full(Ma, np.inf, F), s2=np.full(Ma, np.inf, F),
               rev=np.full(Mb, -1, np.int32), rev_s=np.full(Mb, np.inf, F))
    out["nn1"][:na], out["s1"][:na], out["nn2"][:na], out["s2"][:na] = _two_smallest(S)
    out["rev"][:nb], out["rev_s"][:nb] = _two_smallest(np.ascontiguousarray(S.T))[:2]
    keep = out["nn1"] >= 0
    if ratio is not None:
        ratio2 = F(ratio * ratio)
        with np.errstate(invalid="ignore"):
            keep &= out["s1"] < (ratio2 * out["s2"]).astype(F)
    if mutual:
        keep &= out["rev"][np.maximum(out["nn1"], 0)] == np.arange(Ma)
    out["match"] = np.where(keep, out["nn1"], -1).astype(np.int32)
    out["num_kept"] = int(keep.sum())
    for k in ("1", "2"):
        out["dist" + k] = np.sqrt(out["s" + k])          # float32 sqrt: correctly rounded, as sqrtf
    out["rev_dist"] = np.sqrt(out["rev_s"])
    return out


def _norms(x):
    """|x|^2 as match.hip's stage_rows sums it: lane q of four takes the float4 groups q, q + 4, ..., then (p0 + p1) + (p2 + p3)."""
    n, D = x.shape
    Dp = (D + 7) & ~7
    xp = np.zeros((n, Dp), F)
    xp[:, :D] = x
    part = np.zeros((n, 4), F)
    for q in range(4):
        for c0 in range(4 * q, Dp, 16):
            for c in range(c0, c0 + 4):
                part[:, q] = part[:, q] + xp[:, c] * xp[:, c]
    return (part[:, 0] + part[:, 1]) + (part[:, 2] + part[:, 3])


def screen(a, b):
    """(s, E) [na, nb] float32: s = (|a|^2 + |b|^2) - 2 dot with dot the fma chain over d = 8 g + (0, 4, 1, 5, 2, 6, 3, 7), and
    E = 4 (D + 4) 2^-24 (|a|^2 + |b|^2) + 2^-100 in float32."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    D = a.shape[1]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    dot = np.zeros((len(a), len(b)), F)
    for g in range(0, D, 8):
        for c in (0, 4, 1, 5, 2, 6, 3, 7):
            if g + c < D:
                dot = (a64[:, None, g + c] * b64[None, :, g + c] + dot.astype(np.float64)).astype(F)
    t = _norms(a)[:, None] + _norms(b)[None, :]
    s = t - F(2) * dot
    E = F(4 * (D + 4) * 2.0 ** -24) * t + F(2.0 ** -100)
    return s.astype(F), E.astype(F)


# ---------------------------------------------------------------------------------------------------------- builders

def unit(rng, M, D):
    v = rng.standard_normal((M, D))
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)


def fpfh_like(rng, M):
    """Three blocks of 11 bins summing to 200, in 36 columns (the last three zero), as compute_fpfh's rows."""
    h = rng.random((M, 3, 11)) ** 3
    h = 200.0 * h / h.sum(-1, keepdims=True)
    return np.concatenate([h.reshape(M, 33), np.zeros((M, 3))], 1).astype(F)


def shared_offset(rng, M, D):
    """Unit rows on top of one offset of length 100: |a|^2 + |b|^2 - 2 a.b cancels five digits, nearly every pair survives."""
    off = unit(rng, 1, D).astype(np.float64) * 100.0
    return (unit(rng, M, D) + off).astype(F), (unit(rng, M, D) + off).astype(F)


def all_equal(M, D):
    row = (np.arange(D) % 7 - 3).astype(F) / F(4)
    return np.tile(row, (M, 1)), np.tile(row, (M, 1))


def ulp_neighbours(rng, M, D):
    """Anchors at the origin, positives (0.75, k 2^-12, 0, ...) with k in 0 .. 3: S = 0.5625 + k^2 2^-24 exactly, neighbours
    one ulp (2^-24 in [0.5, 1)) apart and many exact ties."""
    a = np.zeros((M, D), F)
    b = np.zeros((M, D), F)
    b[:, 0] = 0.75
    b[:, 1] = rng.integers(0, 4, M).astype(F) * F(2.0 ** -12)
    b[:3, 1] = F(3 * 2.0 ** -12)                 # the lowest ids are not the nearest
    return a, b


def with_duplicates(rng, M, D):
    """Unit rows; positives 9 = 5 and 30 = 21 = 20; anchors 0 and 1 next to them, anchor 2 equal to positive 30, anchor 3
    equal to positive 7."""
    a, b = unit(rng, M, D), unit(rng, M, D)
    b[9], b[21], b[30] = b[5], b[20], b[20]
    a[0] = unit(rng, 1, D)[0] * F(0.01) + b[5]
    a[1] = unit(rng, 1, D)[0] * F(0.01) + b[20]
    a[2], a[3] = b[30], b[7]
    return a, b


def planted(seed=11, M=512, D=128, orphan_share=0.4, noise=0.03, side=40.0, P=1):
    """P pairs of keypoint rows [x, y, z, descriptor, score] (132 columns at D = 128) with a known pose and known partners:
    anchor i's true positive is truth[p, i], its descriptor the anchor's plus `noise` per component, its position the
    anchor's under the pose plus 5 cm; an `orphan_share` of the anchors has no partner (truth -1): their positives carry
    unrelated descriptors and lie anywhere in the box.  Returns rows_a, rows_b [P, M, 3 + D + 1] float32, truth [P, M], T
    [P, 3, 4] (anchor ~ R positive + t)."""
    rng = np.random.default_rng(seed)
    rows_a, rows_b = np.zeros((P, M, 3 + D + 1), F), np.zeros((P, M, 3 + D + 1), F)
    truth, T = np.full((P, M), -1, np.int64), np.zeros((P, 3, 4))
    for p in range(P):
        yaw = rng.uniform(-np.pi, np.pi)
        R = np.array([[np.cos(yaw), -np.sin(yaw), 0.0], [np.sin(yaw), np.cos(yaw), 0.0], [0.0, 0.0, 1.0]])
        t = rng.uniform(-5.0, 5.0, 3)
        x = rng.random((M, 3)) * side - side / 2
        y = (x - t) @ R + rng.normal(0.0, 0.05, (M, 3))
        da = unit(rng, M, D)
        db = da + (noise * rng.standard_normal((M, D))).astype(F)
        orphan = rng.random(M) < orphan_share
        db[orphan] = unit(rng, int(orphan.sum()), D)
        y[orphan] = rng.random((int(orphan.sum()), 3)) * side - side / 2
        perm = rng.permutation(M)
        rows_a[p, :, :3], rows_a[p, :, 3:3 + D] = x, da
        rows_b[p, perm, :3], rows_b[p, perm, 3:3 + D] = y, db
        truth[p] = np.where(orphan, -1, perm)
        T[p] = np.concatenate([R, t[:, None]], axis=1)
    return rows_a, rows_b, truth, T
