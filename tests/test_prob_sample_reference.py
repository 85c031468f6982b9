"""CPU: pins the numpy restatement of ProbSample (tests/prob_sample_reference.py) without the kernel -- its sums against
float64, their sensitivity to summation order, the halving walk on monotone, tied and non-monotone rows, and the
frequencies of the seeded draws."""
import numpy as np
import pytest

import prob_sample_reference as R

F32 = np.float32


def seq64(w):
    return np.cumsum(np.asarray(w, dtype=np.float64))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 37, 129, 8192, 8195, 16389])
def test_small_integer_weights_sum_exactly(n):
    """Integers whose total stays below 2^24: every partial sum in any order is exact, so the tree's sums are the float64
    prefix sums bit for bit -- each index of the tree is right, whatever the rounding."""
    rng = np.random.default_rng(n)
    w = rng.integers(0, 9, n).astype(F32)
    w[rng.random(n) < 0.3] = 0
    got = R.cumsum(w)
    assert got.dtype == F32 and np.array_equal(got.astype(np.float64), seq64(w))


@pytest.mark.parametrize("n", [37, 1000, 8192, 8195, 20000])
def test_error_bound_on_uniform_weights(n):
    """Relative error against the float64 sequential sums <= 16 * 2^-24 (each rounding of a sum of non-negative parts adds
    at most 2^-24 relative).  The roundings an entry passes through in this code: 2 in its quad, up to 10 up-sweep levels
    and up to 10 down-sweep additions on the way to the quad prefix s[g-1] (g = 2047: s[1023], then one addition a level),
    the prefix addition and the running sum -- a worst case of 24, reached only by the first weights of a chunk inside the
    last quads and only if every rounding errs the same way; most of a sum's mass passes through far fewer.  Measured here:
    below 3e-7 at every n."""
    w = np.random.default_rng(n).random(n).astype(F32)
    got, exact = R.cumsum(w).astype(np.float64), seq64(w)
    rel = np.abs(got - exact) / exact
    print("n = %d: max relative error %.3g" % (n, rel.max()))
    assert rel.max() <= 16 * 2.0 ** -24


def test_sums_depend_on_the_order():
    """At n = 37 the sums differ from a sequential float32 prefix sum: a test on the sums' bits sees the summation order."""
    w = np.random.default_rng(37).random(37).astype(F32)
    assert np.count_nonzero(R.cumsum(w) != np.cumsum(w, dtype=F32)) >= 1


def test_chunks_join_through_the_compensated_sum():
    """Past 8192 entries the output is chunk-local sum + R, with R carried by t = s + C, R' = R + t, C = t - (R' - R)."""
    w = np.random.default_rng(5).random(8195).astype(F32)
    got = R.cumsum(w)
    first, tail = R.cumsum(w[:8192]), R.cumsum(w[8192:])
    assert np.array_equal(got[:8192], first)
    local, s = R.quad_sums(w[:8192])
    run = F32(F32(0) + F32(R.tree(s)[-1] + F32(0)))
    assert np.array_equal(got[8192:], tail + run)


def test_non_monotone_fixture():
    """Non-negative weights whose sums decrease somewhere; a draw at the dip gets another id from searchsorted than from the
    walk, and the vectorised walk is the scalar loop."""
    w, cum, r_in = R.non_monotone_row()
    assert (w >= 0).all() and (np.diff(cum) < 0).any()
    by_walk = R.walk(cum, np.array([r_in], dtype=F32))[0]
    by_search = min(int(np.searchsorted(cum, F32(r_in * cum[-1]), side="left")), len(cum) - 1)
    assert by_walk != by_search
    draws = np.concatenate([np.random.default_rng(1).random(500).astype(F32), cum / cum[-1], [r_in, 0, 1]]).astype(F32)
    assert np.array_equal(R.walk(cum, draws), [R.walk_scalar(cum, d) for d in draws])


def test_non_monotone_rows_are_common():
    """The fixture is no freak: of 300 wide-range rows (n in 9 .. 79) a good number have sums that decrease somewhere."""
    rng = np.random.default_rng(0)
    hits = sum(bool((np.diff(R.cumsum(R.wide_range_row(rng, int(rng.integers(9, 80))))) < 0).any()) for _ in range(300))
    assert hits >= 5


@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 1000, 8195])
def test_walk_is_searchsorted_on_monotone_rows(n):
    rng = np.random.default_rng(n)
    cum = R.cumsum(rng.integers(0, 5, n).astype(F32) + F32(rng.integers(0, 2)))   # exact sums: monotone, with flat runs
    if not cum[-1] > 0:
        cum = R.cumsum(np.ones(n, dtype=F32))
    assert (np.diff(cum) >= 0).all()
    draws = np.concatenate([rng.random(400).astype(F32), cum / cum[-1], [0, 1]]).astype(F32)
    exp = np.minimum(np.searchsorted(cum, draws * cum[-1], side="left"), n - 1)
    assert np.array_equal(R.walk(cum, draws), exp)
    assert np.array_equal(R.walk(cum, draws[:50]), [R.walk_scalar(cum, d) for d in draws[:50]])


def tie_row():
    """Integer weights with zero runs and a total of 16: the draws cum[r] / 16 are exact."""
    w = np.array([1, 0, 0, 2, 0, 1, 0, 0, 0, 4, 0, 0, 8, 0], dtype=F32)
    assert w.sum() == 16
    return w


def test_ties_and_the_zero_draw():
    w = tie_row()
    cum = R.cumsum(w)
    assert np.array_equal(cum, np.cumsum(w))
    at = (cum / cum[-1]).astype(F32)                 # draws exactly at cum[r] / total
    above = np.nextafter(at, F32(2))                 # and one float above
    first_reaching = np.array([np.flatnonzero(cum >= c)[0] for c in cum])             # the lowest index of the flat run
    next_rise = np.array([np.flatnonzero(cum > c)[0] if (cum > c).any() else len(w) - 1 for c in cum])
    assert np.array_equal(R.walk(cum, at), first_reaching)
    assert np.array_equal(R.walk(cum, above), next_rise)
    assert (w[R.walk(cum, at)] > 0).all() and (w[R.walk(cum, above)[:-2]] > 0).all()
    assert R.walk(cum, np.zeros(1, dtype=F32))[0] == 0
    zero_first = np.array([0, 0, 3, 1], dtype=F32)   # a draw of 0 gives index 0 whatever its weight
    assert R.walk(R.cumsum(zero_first), np.zeros(1, dtype=F32))[0] == 0


def test_seeded_draws_are_exact_and_in_the_half_open_interval():
    r = R.seeded_draws(3, 1, 100000)
    assert r.dtype == F32 and r.min() > 0 and r.max() <= 1
    assert np.array_equal(r.astype(np.float64) * 2 ** 24, np.round(r.astype(np.float64) * 2 ** 24))
    assert not np.array_equal(r[:100], R.seeded_draws(4, 1, 100)) and not np.array_equal(r[:100], R.seeded_draws(3, 2, 100))


def test_seeded_frequencies():
    """200k seeded draws over a fixed 16-weight row: every frequency within 5 binomial standard deviations, and no index of
    weight 0 (r_in > 0 and the integer sums are exact)."""
    w = np.array([3, 0, 1, 7, 0, 0, 2, 12, 1, 0, 5, 9, 0, 4, 16, 4], dtype=F32)
    N = 200000
    ids = R.sample_row(w, 16, N, seed=11, b=0)
    freq = np.bincount(ids, minlength=16)
    p = w.astype(np.float64) / w.sum()
    sd = np.sqrt(N * p * (1 - p))
    assert (freq[w == 0] == 0).all()
    assert (np.abs(freq - N * p) <= 5 * sd).all(), (freq, N * p)


def test_seeded_rows_counts_and_void_rows():
    rng = np.random.default_rng(2)
    w = rng.random((6, 40)).astype(F32)
    w[4] = 0
    count = np.array([0, 1, 17, 40, 47, -3])
    ids = R.sample_by_weight(w, 9, count=count, seed=5)
    assert (ids[0] == -1).all() and (ids[5] == -1).all()
    assert (ids[1] == 0).all()
    assert ids[2].min() >= 0 and ids[2].max() < 17 and ids[3].max() < 40
    assert (R.sample_by_weight(w, 9, seed=5)[4] == -1).all()                 # a zero total
    assert np.array_equal(ids[4], R.sample_row(w[4], 40, 9, 5, 4))           # count beyond n is n
    assert np.array_equal(ids[2], R.sample_row(w[2, :17], 17, 9, 5, 2))      # the row's own entries and slot only
