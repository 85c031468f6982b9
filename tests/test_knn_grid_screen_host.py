"""The threshold rule of knn_grid_kernel's screened pass-0 drain (csrc/knn.hip, `drain_screened`), restated in numpy
(tests/knn_grid_screen_cases.py) and checked without a GPU:

  - whatever way a pool is dealt to the query's four lanes, the candidates with s <= fl(U * 1.000001f) include every candidate
    whose (rounded distance, rank code) key is among the K smallest, K = 1..8;
  - a lane with fewer than two candidates makes U infinite (and then nothing is screened out);
  - the clouds of tests/test_knn_grid_screen_gpu.py put their queries where that file says they are (the choice between the
    two drains is a wave's, 16 consecutive queries of the sorted order): on the uniform clouds at least 90 % take the screened
    drain, and lattices, the many-copies cloud, the dense cell and the margin cloud leave some to the old drain -- so the GPU
    file cannot pass with every query on one of the two."""
import numpy as np
import pytest

import knn_grid_screen_cases as C

F = np.float32
N = 8192


def _pools(kind, n_queries, seed):
    """(s, ids) of the pass-0 pools of n_queries random queries of one 8192-point cloud"""
    rng = np.random.default_rng(seed)
    pts = C.cloud(kind, N, rng)
    cell, dims, flag, _ = C.coarse_cells(pts, 0)
    assert flag == 0
    out = []
    for qi in rng.choice(N, n_queries, replace=False):
        ids = C.pool_of(cell, qi)
        out.append((C.sqdist(pts[qi], pts[ids]), ids))
    return out


def _dealings(s, rng):
    """50 random orders of the pool, and the adversarial one: its eight smallest all in lane 0 (as many of them as lane 0 has
    slots)"""
    for _ in range(50):
        yield rng.permutation(len(s))
    by_s = np.argsort(s, kind="stable")
    lane0 = np.arange(0, len(s), C.LANES)
    take = min(8, len(lane0))
    order = np.empty(len(s), np.int64)
    order[lane0[:take]] = by_s[:take]
    rest = np.setdiff1d(np.arange(len(s)), lane0[:take])
    order[rest] = rng.permutation(by_s[take:])
    yield order


@pytest.mark.parametrize("kind", ["uniform", "lattice", "duplicates"])
def test_the_screened_set_holds_the_k_smallest_keys_under_any_dealing(kind):
    rng = np.random.default_rng(11)
    screened = dropped = 0
    for s, ids in _pools(kind, 40, seed=len(kind)):
        if len(s) < 2 * C.LANES:
            continue
        key = C.keys(s, ids, N)
        best = np.argsort(key)[:8]  # keys are unique: the rank code is
        for order in _dealings(s, rng):
            u, thr = C.threshold(s[order])
            assert np.isfinite(u)  # 2 L or more candidates: every lane has two
            keep = s <= thr
            assert keep[best].all(), (kind, "a candidate among the 8 smallest keys is screened out", s[best], thr)
            assert keep.sum() >= 8
            screened += 1
            dropped += int((~keep).sum())
    assert screened >= 30 * 51 and dropped > 0  # the rule was exercised, and it does screen


def test_a_lane_with_fewer_than_two_candidates_makes_the_threshold_infinite():
    rng = np.random.default_rng(12)
    for t in range(1, 2 * C.LANES):
        s = rng.random(t, dtype=F)
        u, thr = C.threshold(s)
        assert u == np.inf and thr == np.inf and (s <= thr).all()  # (a short pool in a screening wave is ranked whole)
    s = rng.random(2 * C.LANES, dtype=F)
    assert np.isfinite(C.threshold(s)[0])
    s[5] = np.nan  # a NaN is no candidate: lane 1 is left with one
    u, thr = C.threshold(s)
    assert u == np.inf and (s <= thr).sum() == 2 * C.LANES - 1


def test_copies_of_the_query_give_a_zero_threshold_that_keeps_exactly_the_copies():
    s = np.array([0] * 9 + [1e-4, 2e-4, 3e-3] * 5, F)
    u, thr = C.threshold(s)  # the first eight slots: two copies per lane
    assert u == 0 and thr == 0 and (s <= thr).sum() == 9


def _shares():
    out = {}
    for case, (n, _, kinds, flags, _) in C.CASES.items():
        pts = C.batch(case)
        for b, kind in enumerate(kinds[:6]):
            cell, dims, flag, order = C.coarse_cells(pts[b], C.grid_drop(n))
            assert flag == flags[b], (case, b, kind, "the sort's crowded flag")
            if flag == 0:
                t = C.pool_sizes(cell, dims)
                out.setdefault((case, kind), []).append((C.screened(t, order), t))
    return out


def test_which_drain_the_gpu_clouds_take():
    shares = _shares()
    for (case, kind), clouds in shares.items():
        el = np.concatenate([e for e, _ in clouds])
        t = np.concatenate([t for _, t in clouds])
        print("%-14s %-13s screened %.4f  pools: mean %.1f, %d below 8, %d above 80" % (case, kind, el.mean(), t.mean(),
                                                                                      (t < 8).sum(), (t > 80).sum()))
        if case in ("uniform_d0", "uniform_d1", "uniform_d3", "mixed_6x8192"):
            assert el.mean() >= 0.9, (case, el.mean())
        if case in ("uniform_code2", "uniform_code0", "lattice_4096", "plane"):  # one point per cell: short pools, both drains
            assert 0 < el.mean() < 1, (case, el.mean())
        if case.startswith("tiny_"):
            assert not el.any()

    def left_out(*cases):
        return sum(int((~e).sum()) for (c, _), clouds in shares.items() if c in cases for e, _ in clouds)
    assert left_out("lattice_8192", "lattice_4096") > 0
    assert left_out("many_copies") > 0 and left_out("margin") > 0 and left_out("dense_cell") > 0
    for case in ("lattice_8192", "duplicates", "many_copies", "collapse", "dense_cell", "margin", "oxford_extent"):
        el = np.concatenate([e for (c, _), clouds in shares.items() if c == case for e, _ in clouds])
        assert el.mean() >= 0.5, (case, "most queries should be screened", el.mean())
    t = shares[("dense_cell", "dense_cell")][0][1]
    assert (t > 256).sum() >= 400  # pools that overflow kGridCap: direct()


def test_uniform_pools_are_what_the_design_counts_on():
    """8192 uniform points: pools of 48 on average, a handful above the screened drain's 80, every sampled query with two
    candidates in every lane under a random dealing."""
    rng = np.random.default_rng(13)
    pts = C.cloud("uniform", N, rng)
    cell, dims, _, _ = C.coarse_cells(pts, 0)
    t = C.pool_sizes(cell, dims)
    assert 46 <= t.mean() <= 51 and t.max() <= 100 and (t > C.SCREEN_CAP).mean() < 0.002
    survivors = []
    for qi in rng.choice(N, 600, replace=False):
        ids = C.pool_of(cell, qi)
        assert len(ids) == t[qi]
        s = C.sqdist(pts[qi], pts[ids])[rng.permutation(len(ids))]
        u, thr = C.threshold(s)
        assert np.isfinite(u)
        survivors.append(int((s <= thr).sum()))
    print("survivors per query: mean %.1f, max %d" % (np.mean(survivors), max(survivors)))
    assert np.mean(survivors) < 16


def test_collapse_cloud_premises():
    """every site: s(A) < s(B) by one unit, one rounded distance, the pair is the 8th and 9th candidate, the query is screened"""
    pts = C.batch("collapse")[0]
    cell, dims, _, order = C.coarse_cells(pts, 0)
    t = C.pool_sizes(cell, dims)
    scr = C.screened(t, order)
    for j in range(C.COLLAPSE_SITES):
        q = 9 * j
        assert np.array_equal(pts[q].astype(np.float64) * 65536, C.collapse_site(j))
        ids = C.pool_of(cell, q)
        assert scr[q] and 2 * C.LANES <= t[q] <= C.SCREEN_CAP and set(range(q, q + 9)) <= set(ids.tolist())
        s_all = C.sqdist(pts[q], pts)
        a, b = (q + 8, q + 7) if j % 2 == 0 else (q + 7, q + 8)
        assert s_all[a] * 2.0 ** 32 == 4413625 and s_all[b] * 2.0 ** 32 == 4413626
        assert np.sqrt(s_all[a]) == np.sqrt(s_all[b])
        assert np.argsort(C.keys(s_all, np.arange(N), N))[:9].tolist() == list(range(q, q + 9))
        if j % 2 == 0:  # B at the lower index: ordered by s the list would end with A
            assert np.lexsort((np.arange(N), s_all))[7] == q + 8
