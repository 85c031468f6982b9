"""CPU: the float32 restatement of select_top_k / knn_point (tests/knn_point_reference.py) is the reference's partial
selection sort -- the known answer of the reference twin's own driver; the candidate-set lemma both kernels rest on, proven
here on random tie-heavy rows over the WHOLE row; and numpy's own sort on the rows it can judge (no ties among the k + 1
smallest values)."""
import numpy as np
import pytest

import knn_point_reference as R


def test_known_answer_of_the_twins_driver():
    # b=2, n=4, m=2, k=3, dist[i] = 10 - i over the flat array: every row is descending
    b, n, m, k = 2, 4, 2, 3
    dist = (10 - np.arange(b * m * n)).astype(np.float32).reshape(b, m, n)
    idx, out = R.select_top_k(k, dist)
    for r in range(b):
        for j in range(m):
            assert idx[r, j].tolist() == [3, 2, 1, 0]
            assert np.all(np.diff(out[r, j]) > 0) and np.array_equal(out[r, j], dist[r, j][::-1])
    for bad in (0, 5):
        with pytest.raises(ValueError, match="1 <= k <= n"):
            R.select_top_k(bad, dist)


def test_tie_order_is_the_walks_not_lowest_id_first():
    rng = np.random.default_rng(5)
    differ = 0
    for _ in range(400):
        row = rng.integers(0, 4, 30).astype(np.float32)
        idx, _ = R.swap_walk_row(8, row)
        by_id = np.lexsort((np.arange(30), row))[:8]
        differ += not np.array_equal(idx[:8], by_id)
    assert differ > 40                        # a swapped-out entry re-enters at a higher position


def test_candidate_set_lemma_on_tie_heavy_rows():
    rng = np.random.default_rng(20261017)
    rows = 0
    for trial in range(12000):
        n = int(rng.integers(1, 40))
        k = int(rng.integers(1, n + 1))
        distinct = int(rng.integers(1, 8))
        row = rng.integers(0, distinct, n).astype(np.float32) * np.float32(0.25) - np.float32(0.5)
        wi, wv = R.swap_walk_row(k, row)
        ci, cv = R.candidate_walk_row(k, row)
        assert np.array_equal(wi, ci) and np.array_equal(wv, cv), (trial, n, k, row.tolist())
        rows += 1
    assert rows >= 10000
    # longer rows, the shapes of the kernels' own tiles
    for n, k in ((64, 8), (65, 33), (200, 64), (1000, 3), (1000, 128), (257, 256)):
        for distinct in (1, 2, 5, 50):
            row = rng.integers(0, distinct, n).astype(np.float32)
            wi, wv = R.swap_walk_row(k, row)
            ci, cv = R.candidate_walk_row(k, row)
            assert np.array_equal(wi, ci) and np.array_equal(wv, cv), (n, k, distinct)


def test_select_top_k_leaves_the_rest_of_the_row():
    rng = np.random.default_rng(9)
    dist = rng.random((2, 3, 50), dtype=np.float32)
    idx, out = R.select_top_k(5, dist)
    assert np.array_equal(np.sort(idx, -1), np.broadcast_to(np.arange(50), idx.shape))       # a permutation
    assert np.array_equal(np.take_along_axis(dist, idx.astype(np.int64), -1), out)            # of the row itself
    assert np.array_equal(out[..., :5], np.sort(dist, -1)[..., :5])
    moved = (idx != np.arange(50)).sum(-1)
    assert moved.max() <= 10                                                                  # at most 2k positions


@pytest.mark.parametrize("n,m,k", [(8192, 1024, 32), (8192, 1024, 64), (512, 128, 64)])
def test_restatement_equals_numpy_sort_where_it_can_judge(n, m, k):
    rng = np.random.default_rng(n + k)
    x1 = rng.random((1, n, 3), dtype=np.float32)
    x2 = rng.random((1, m, 3), dtype=np.float32)
    val, idx = R.knn_point(k, x1, x2)
    d = R.sqdist(x1, x2)[0]
    order = np.argsort(d, axis=1, kind="stable")[:, :k + 1]
    srt = np.take_along_axis(d, order, 1)
    judge = np.all(np.diff(srt, axis=1) > 0, axis=1)       # the k + 1 smallest values are distinct
    assert judge.mean() >= 0.99, judge.mean()
    assert np.array_equal(idx[0][judge], order[judge][:, :k].astype(np.int32))
    assert np.array_equal(val[0][judge], srt[judge][:, :k])


def test_sqdist_rounding_and_gather_point():
    rng = np.random.default_rng(2)
    x1, x2 = rng.random((2, 9, 3), dtype=np.float32) * 50, rng.random((2, 4, 3), dtype=np.float32) * 50
    d = R.sqdist(x1, x2)
    for bi, j, i in ((0, 0, 0), (1, 3, 8), (0, 2, 5)):
        dx, dy, dz = (np.float32(x1[bi, i, c] - x2[bi, j, c]) for c in range(3))
        assert d[bi, j, i] == np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz))
    idx = np.array([[0, 3, 3, 8], [1, 1, 1, 1]], np.int32)
    out = R.gather_point(x1, idx)
    assert out.shape == (2, 4, 3) and np.array_equal(out[0, 2], x1[0, 3])
    g = R.gather_point_grad(x1.shape, idx, np.ones((2, 4, 3), np.float32))
    assert g[0, 3].tolist() == [2, 2, 2] and g[1, 1].tolist() == [4, 4, 4] and g.sum() == 24
