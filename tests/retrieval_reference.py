"""The numpy restatement of dh3d_retrieve (include/dh3d_hip.h): d2(q, j) = the sum over c ASCENDING, starting from 0, of
((double)q_c - (double)r_jc)^2 with every operation rounded on its own, and the first k of the order (d2, j).  The sum is an
explicit loop over c (np.sum adds pairwise, in another order), vectorised over Q x R.  `dtype=np.float32` is the same rule
ranked in float32: the twin the power check compares with.  Below them, the data both test files share."""
import numpy as np


def sqdist(ref, qry, dtype=np.float64):
    """[Q, R] squared distances by the rule above, in `dtype`."""
    ref = np.asarray(ref, np.float32).astype(dtype)
    qry = np.asarray(qry, np.float32).astype(dtype)
    d2 = np.zeros((qry.shape[0], ref.shape[0]), dtype)
    for c in range(ref.shape[1]):
        diff = qry[:, c, None] - ref[None, :, c]
        d2 = d2 + diff * diff
    return d2


def topk(ref, qry, k, count=None, dtype=np.float64):
    """(idx int32 [Q, k], dist2 `dtype` [Q, k]) over the live rows ref[:count] (None: all); -1 / +inf past their end."""
    ref = np.asarray(ref, np.float32)
    r = ref.shape[0] if count is None else min(max(int(count), 0), ref.shape[0])
    Q = np.asarray(qry).shape[0]
    idx = np.full((Q, k), -1, np.int32)
    dist2 = np.full((Q, k), np.inf, dtype)
    if r == 0:
        return idx, dist2
    d2 = sqdist(ref[:r], qry, dtype)
    ids = np.arange(r)
    n = min(k, r)
    for q in range(Q):
        order = np.lexsort((ids, d2[q]))[:n]  # by d2, ties to the lowest id
        idx[q, :n] = order
        dist2[q, :n] = d2[q, order]
    return idx, dist2


def unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def clustered_map(rng, R, D, clusters=50):
    """R unit-norm rows: half drawn round `clusters` centres, the other half near-duplicates of those ('revisits')."""
    centres = rng.standard_normal((clusters, D))
    first = unit(centres[rng.integers(0, clusters, R // 2)] + 0.3 * rng.standard_normal((R // 2, D)))
    again = unit(first[rng.integers(0, R // 2, R - R // 2)] + 0.01 * rng.standard_normal((R - R // 2, D)))
    return np.concatenate([first, again])[rng.permutation(R)]


def near_tie_case(D=8, R=16):
    """The query is the zero vector.  Row 3 = [1, 2^-13, 0, ...], row 7 = [1, 0, ...], every other row far.
    In float64 d2(3) = 1 + 2^-26 > d2(7) = 1; in float32 1 + 2^-26 rounds to 1 and the two tie, so id 3 comes first."""
    ref = np.full((R, D), 4.0, np.float32)
    ref[3] = 0.0
    ref[7] = 0.0
    ref[3, 0], ref[3, 1] = 1.0, 2.0 ** -13
    ref[7, 0] = 1.0
    qry = np.zeros((1, D), np.float32)
    return ref, qry
