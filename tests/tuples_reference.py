"""A numpy float64 / uint64 restatement of include/dh3d_hip.h "Training tuples", written from that text: one query slot at
a time, the way the reference's loader walks its queries (core/datasets.py Global_train_dataset_triplet.__iter__).
Nothing here looks at the kernels.  The draws are pairs_reference's u(seed, stream, b, j)."""
import numpy as np

from pairs_reference import u, unit_co

POS_KEYS, NEG_KEYS, POOL, OTHER_KEYS, QUERY_KEYS = 11, 12, 13, 14, 15


def live(count, M):
    return M if count is None else int(min(max(int(count), 0), M))


def d2_from(pos, i, n):
    """d2(i, j) for j < n: (dx*dx) + (dy*dy), every operation rounded to float64 on its own."""
    dx = pos[:n, 0] - pos[i, 0]
    dy = pos[:n, 1] - pos[i, 1]
    return dx * dx + dy * dy


def radii2(pos_radius, neg_radius):
    return np.float64(pos_radius) * np.float64(pos_radius), np.float64(neg_radius) * np.float64(neg_radius)


def sets(pos, q, n, pos_radius=10.0, neg_radius=50.0):
    """(POS(q), NEG(q)) as ascending id arrays."""
    rp2, rn2 = radii2(pos_radius, neg_radius)
    d2 = d2_from(pos, q, n)
    ids = np.arange(n)
    return ids[(d2 <= rp2) & (ids != q)], ids[d2 > rn2]


def smallest(members, k, seed, stream, b):
    """The k smallest of `members` (ids) by (u(stream, b, j), j), in ascending key order."""
    members = np.asarray(members, dtype=np.int64)
    keys = u(seed, stream, b, members)
    order = np.lexsort((members, keys))
    return members[order[:k]]


def tuple_counts(pos, count=None, pos_radius=10.0, neg_radius=50.0):
    M = pos.shape[0]
    n = live(count, M)
    n_pos, n_neg = np.zeros(M, dtype=np.int32), np.zeros(M, dtype=np.int32)
    for i in range(n):
        p, g = sets(pos, i, n, pos_radius, neg_radius)
        n_pos[i], n_neg[i] = len(p), len(g)
    return n_pos, n_neg


def draw_queries(n_pos, n_neg, Q, num_pos, num_neg, count=None, seed=0):
    n = live(count, len(n_pos))
    ids = np.arange(n)
    eligible = ids[(n_pos[:n] >= num_pos) & (n_neg[:n] >= num_neg)]
    chosen = smallest(eligible, Q, seed, QUERY_KEYS, 0)
    queries = np.full(Q, -1, dtype=np.int32)
    queries[:len(chosen)] = chosen
    return queries, np.int32(1 if len(eligible) >= Q else 0)


def desc_d2(desc, q, rows):
    """D2(q, j) for j in rows: one accumulator per row over ascending columns, every operation rounded on its own."""
    a = desc[q].astype(np.float64)
    r = desc[np.asarray(rows, dtype=np.int64)].astype(np.float64)
    acc = np.zeros(len(rows), dtype=np.float64)
    for c in range(desc.shape[1]):
        d = a[c] - r[:, c]
        acc = acc + d * d
    return acc


def sample_slot(pos, q, b, num_pos, num_neg, count=None, other_neg=True, desc=None, num_hard=0, pool_fraction=1.0,
                pos_radius=10.0, neg_radius=50.0, seed=0):
    """(pos_row [num_pos], neg_row [num_neg], other (None when not asked for), valid) of slot b holding query q."""
    n = live(count, pos.shape[0])
    pos_row, neg_row = np.full(num_pos, -1, dtype=np.int32), np.full(num_neg, -1, dtype=np.int32)
    other = -1 if other_neg else None
    if q < 0 or q >= n:
        return pos_row, neg_row, other, 0
    rp2, _ = radii2(pos_radius, neg_radius)
    P, N = sets(pos, q, n, pos_radius, neg_radius)
    pos_filled, neg_filled = len(P) >= num_pos, len(N) >= num_neg
    if pos_filled:
        pos_row[:] = smallest(P, num_pos, seed, POS_KEYS, b)
    if neg_filled:
        hard = np.zeros(0, dtype=np.int64)
        if num_hard > 0 and desc is not None:
            pool = N[unit_co(u(seed, POOL, b, N)) < pool_fraction]
            bits = desc_d2(desc, q, pool).view(np.uint64)
            hard = pool[np.lexsort((pool, bits))[:min(num_hard, len(pool))]]
        rest = N[~np.isin(N, hard)]
        neg_row[:] = np.concatenate([hard, smallest(rest, num_neg - len(hard), seed, NEG_KEYS, b)])
    if other_neg and neg_filled:
        barred = np.zeros(n, dtype=bool)
        for g in [q] + [int(g) for g in neg_row]:
            barred |= d2_from(pos, g, n) <= rp2
        free = smallest(np.arange(n)[~barred], 1, seed, OTHER_KEYS, b)
        other = int(free[0]) if len(free) else -1
    valid = int(pos_filled and neg_filled and (not other_neg or other >= 0))
    return pos_row, neg_row, other, valid


def sample_tuples(pos, queries, num_pos, num_neg, **kw):
    """The restatement of dh3d_sample_tuples: a dict of pos [Q, num_pos], neg [Q, num_neg], other [Q] (or None), valid [Q]."""
    rows = [sample_slot(pos, int(q), b, num_pos, num_neg, **kw) for b, q in enumerate(queries)]
    other = None if rows[0][2] is None else np.array([r[2] for r in rows], dtype=np.int32)
    return {"pos": np.stack([r[0] for r in rows]), "neg": np.stack([r[1] for r in rows]), "other": other,
            "valid": np.array([r[3] for r in rows], dtype=np.int32)}


# ------------------------------------------------------------------------------------- the two maps the tests run on
OFFSET = np.array([5735000.0, 620000.0])


def grid_positions():
    """24 x 24 places at 2.5 m spacing (exact in float64): 1920 ordered pairs at exactly d2 == 100, 1152 at d2 == 2500."""
    i, j = np.meshgrid(np.arange(24), np.arange(24), indexing="ij")
    return OFFSET + 2.5 * np.stack([i.ravel(), j.ravel()], axis=1).astype(np.float64)


def route_positions():
    """Two 300-place traversals (4 m steps, 0.5 m Gaussian noise; the second 3 m to the side and staggered 2 m along the
    track) and two places 700 m away, 4 m apart: 600 valid queries at (2, 18), |POS| from 1 to 10, 8 positives at place 150."""
    rng = np.random.default_rng(7)
    s = 4.0 * np.arange(300)
    a = np.stack([s, np.zeros(300)], axis=1) + 0.5 * rng.standard_normal((300, 2))
    b = np.stack([s + 2.0, np.full(300, 3.0)], axis=1) + 0.5 * rng.standard_normal((300, 2))
    far = np.array([[600.0, 700.0], [604.0, 700.0]])
    return OFFSET + np.concatenate([a, b, far])
