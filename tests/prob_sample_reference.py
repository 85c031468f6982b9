"""A numpy float32 restatement of ProbSample (include/dh3d_hip.h "Weighted sampling"; upstream tf_sampling_g.cu:7-104),
written from that text: the cumulative sums with their own summation tree, the halving walk vectorised over the draws of a
row level by level, the seeded draws and the whole op, one row at a time.  Nothing here looks at the kernels.  Every float32
addition below is one numpy float32 operation, so it is rounded on its own."""
import numpy as np

from pairs_reference import u

F32 = np.float32
CHUNK = 8192
DRAW_STREAM = 16


def quad_sums(x):
    """One chunk x (float32, 1 .. 8192 entries) -> (local [4 G] the sums inside each quad, s [G] the quad totals)."""
    L = x.shape[0]
    G = (L + 3) // 4
    full = L // 4
    local = np.zeros(4 * G, dtype=F32)
    s = np.zeros(G, dtype=F32)
    if full:
        a, b, c, d = (x[i:4 * full:4] for i in range(4))
        l1 = b + a
        t = d + c
        local[0:4 * full:4] = a
        local[1:4 * full:4] = l1
        local[2:4 * full:4] = c + l1
        local[3:4 * full:4] = t + l1
        s[:full] = local[3:4 * full:4]
    if G > full:                      # the partial last quad: a plain running sum from 0
        v = F32(0.0)
        for i in range(4 * full, L):
            v = F32(v + x[i])
            local[i] = v
        local[L:] = v
        s[full] = v
    return local, s


def tree(s):
    """The two sweeps over the quad totals, in place: afterwards s[g] is the inclusive sum of the quads 0 .. g."""
    G = s.shape[0]
    u_ = 0
    while (2 << u_) <= G:
        k = np.arange(G >> (u_ + 1))
        s[((2 * k + 2) << u_) - 1] += s[((2 * k + 1) << u_) - 1]
        u_ += 1
    for u_ in range(u_ - 1, -1, -1):
        k = np.arange((G - (1 << u_)) >> (u_ + 1))
        s[((2 * k + 3) << u_) - 1] += s[((2 * k + 2) << u_) - 1]
    return s


def cumsum(w):
    """The cumulative sums of one row of float32 weights, bit for bit."""
    w = np.ascontiguousarray(w, dtype=F32)
    n = w.shape[0]
    out = np.empty(n, dtype=F32)
    run, comp = F32(0.0), F32(0.0)
    for j in range(0, n, CHUNK):
        L = min(n - j, CHUNK)
        local, s = quad_sums(w[j:j + L])
        tree(s)
        local[4:] += np.repeat(s[:-1], 4)
        out[j:j + L] = local[:L] + run
        t = F32(s[-1] + comp)
        r2 = F32(run + t)
        comp = F32(t - F32(r2 - run))
        run = r2
    return out


def walk(cum, r_in):
    """The ids of the draws r_in (float32 array) on the sums cum of one row: the literal halving walk, all draws at once."""
    cum = np.asarray(cum, dtype=F32)
    n = cum.shape[0]
    q = np.asarray(r_in, dtype=F32) * cum[n - 1]
    r = np.full(q.shape, n - 1, dtype=np.int64)
    k = 1
    while k < n:
        k <<= 1
    while k >= 1:
        can = r >= k
        step = np.zeros(q.shape, dtype=bool)
        step[can] = cum[r[can] - k] >= q[can]
        r[step] -= k
        k >>= 1
    return r.astype(np.int32)


def walk_scalar(cum, r_in):
    """One draw, as the loop is written (the vectorised walk is checked against it)."""
    n = len(cum)
    q = F32(F32(r_in) * cum[n - 1])
    base = 1
    while base < n:
        base <<= 1
    r, k = n - 1, base
    while k >= 1:
        if r >= k and cum[r - k] >= q:
            r -= k
        k >>= 1
    return r


def prob_sample(inp, inpr):
    """The op: inp [b, n], inpr [b, m] float32 -> (ids [b, m] int32, cum [b, n] float32)."""
    inp, inpr = np.asarray(inp, dtype=F32), np.asarray(inpr, dtype=F32)
    cum = np.stack([cumsum(row) for row in inp])
    return np.stack([walk(c, r) for c, r in zip(cum, inpr)]), cum


def seeded_draws(seed, b, m):
    """r_in(b, j), j < m: (float)((u(16, b, j) >> 40) + 1) * 2^-24, exact in float32, in (0, 1]."""
    top = (u(seed, DRAW_STREAM, b, np.arange(m)) >> np.uint64(40)).astype(np.int64) + 1
    return top.astype(F32) * F32(2.0 ** -24)


def sample_row(weights, n_b, m, seed, b):
    """One row of the seeded form: the ids [m] of slot b, on the first n_b = clamp(count, 0, n) weights."""
    n_b = min(max(int(n_b), 0), len(weights))
    if n_b == 0:
        return np.full(m, -1, dtype=np.int32)
    cum = cumsum(np.asarray(weights, dtype=F32)[:n_b])
    if not cum[n_b - 1] > 0:
        return np.full(m, -1, dtype=np.int32)
    return walk(cum, seeded_draws(seed, b, m))


def sample_by_weight(weights, m, count=None, seed=0):
    weights = np.asarray(weights, dtype=F32)
    B, n = weights.shape
    count = np.full(B, n) if count is None else count
    return np.stack([sample_row(weights[b], count[b], m, seed, b) for b in range(B)])


def wide_range_row(rng, n):
    """Non-negative float32 weights over nine decades: rand * 10 ** randint(-6, 3)."""
    return (rng.random(n) * 10.0 ** rng.integers(-6, 4, n)).astype(F32)


def non_monotone_row(seed=0, tries=400):
    """The first wide-range row (n in 9 .. 79, fixed seed) whose sums decrease somewhere AND on which some draw gets another
    id from searchsorted than from the walk: (weights, cum, a draw r_in that shows it)."""
    rng = np.random.default_rng(seed)
    for _ in range(tries):
        w = wide_range_row(rng, int(rng.integers(9, 80)))
        cum = cumsum(w)
        down = np.flatnonzero(np.diff(cum) < 0)
        if down.size == 0:
            continue
        # draws whose q is one of the sums round the dip
        cand = np.unique(np.concatenate([cum[down], cum[down + 1]]) / cum[-1]).astype(F32)
        cand = np.concatenate([cand, np.nextafter(cand, F32(0)), np.nextafter(cand, F32(2))])
        cand = cand[(cand >= 0) & (cand <= 1)]
        ids = walk(cum, cand)
        other = np.minimum(np.searchsorted(cum, cand * cum[-1], side="left"), len(cum) - 1)
        differs = np.flatnonzero(ids != other)
        if differs.size:
            return w, cum, cand[differs[0]]
    raise AssertionError("no non-monotone row within %d tries" % tries)
