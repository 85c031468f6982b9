"""CPU: the numpy restatement of query_ball_point (tests/ball_query_reference.py) against the rows of the reference's own
query_ball_point_cpu (golden/twins_ball.npz, made by golden/make_ball_golden.py) -- bit for bit on every row the twin
wrote; on the rows it left unwritten (empty balls) the restatement names the brute-force nearest point; and the conditions
that keep the fixture from going hollow."""
import numpy as np
import pytest

import ball_query_reference as R

CASES = R.golden_cases()
REQUIRED = ("cube_r02_k16", "cube_r01_k32", "cube_offcloud_r025_k24", "demo_global_c_r15_k32", "slab_r015_k16",
            "lattice_r0375_k64", "duplicates_r02_k12", "cube_r01_k1", "nsample_gt_n_r08_k32")


def _row_kinds(c):
    idx, k = c["idx"][0], c["nsample"]
    written = idx[:, 0] >= 0
    # a written row is full when the walk stopped at nsample hits: nsample ascending ids (a repeat of the first id marks
    # the padding of a partly filled row; nsample = 1: every written row is full)
    full = written & (np.all(np.diff(idx, axis=1) > 0, axis=1) if k > 1 else True)
    return written, full


def test_fixture_holds_the_cases_and_is_not_hollow():
    assert set(REQUIRED) <= set(CASES)
    n_full = n_part = n_rows = 0
    for name, c in CASES.items():
        written, full = _row_kinds(c)
        assert (~written).mean() <= 0.10, "%s: %.1f %% of the rows are empty balls" % (name, 100 * (~written).mean())
        assert np.all(c["idx"][0][~written] == -1)
        n_full += int(full.sum()); n_part += int((written & ~full).sum()); n_rows += len(written)
    assert n_full >= 0.2 * n_rows, (n_full, n_rows)
    assert n_part >= 0.2 * n_rows, (n_part, n_rows)
    c = CASES["cube_r02_k16"]
    assert c["xyz1"].shape == (1, 8192, 3) and c["xyz2"].shape == (1, 1024, 3) and np.array_equal(c["xyz2"][0], c["xyz1"][0, :1024])
    q, p = CASES["cube_offcloud_r025_k24"]["xyz2"][0], CASES["cube_offcloud_r025_k24"]["xyz1"][0]
    outside = np.any((q < p.min(0)) | (q > p.max(0)), axis=1)
    assert 0.1 < outside.mean() < 0.9
    assert CASES["nsample_gt_n_r08_k32"]["nsample"] > CASES["nsample_gt_n_r08_k32"]["xyz1"].shape[1]
    slab = CASES["slab_r015_k16"]["xyz1"][0]
    ext = slab.max(0) - slab.min(0)
    assert ext[2] < 0.11 * ext[0] and ext[2] < 0.11 * ext[1]
    dup = CASES["duplicates_r02_k12"]["xyz1"][0]
    assert len(np.unique(dup, axis=0)) * 4 == len(dup)


def test_lattice_has_points_exactly_at_the_radius():
    c = CASES["lattice_r0375_k64"]
    d = R.distances(c["xyz1"][0], c["xyz2"][0, :64])
    r = np.float32(c["radius"])
    assert (d == r).sum() >= 64 * 8          # (1,2,2)-type offsets: up to 24 per query, all computed exactly
    idx, _ = R.query_ball_point(c["radius"], c["nsample"], c["xyz1"], c["xyz2"][:, :64])
    for j in range(64):
        assert not np.isin(np.flatnonzero(d[j] == r), idx[0, j]).any()   # strict <: none of them is in a row


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_twin_on_written_rows(name):
    c = CASES[name]
    idx, cnt = R.query_ball_point(c["radius"], c["nsample"], c["xyz1"], c["xyz2"])
    written, full = _row_kinds(c)
    assert idx.dtype == np.int32 and cnt.dtype == np.int32
    assert np.array_equal(idx[0][written], c["idx"][0][written])
    assert np.array_equal(cnt[0] > 0, written)
    assert np.all(cnt[0][full] == c["nsample"])
    distinct = np.array([len(set(r)) for r in c["idx"][0][written]])
    assert np.array_equal(cnt[0][written], distinct)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_names_the_nearest_point_on_empty_balls(name):
    c = CASES[name]
    # the golden radius, and one that empties every ball
    for radius in (c["radius"], 1e-21):   # d >= 1e-20: nothing is inside 1e-21
        idx, cnt = R.query_ball_point(radius, c["nsample"], c["xyz1"], c["xyz2"])
        empty = np.flatnonzero(cnt[0] == 0)
        if radius != c["radius"]:
            assert len(empty) == c["xyz2"].shape[1]
        empty = empty[:256]
        if len(empty) == 0:
            continue
        rows = idx[0][empty]
        assert np.all(rows == rows[:, :1])
        q, p = c["xyz2"][0][empty].astype(np.float64), c["xyz1"][0].astype(np.float64)
        d64 = np.sqrt(((q[:, None] - p[None]) ** 2).sum(-1))
        part = np.partition(d64, 1, axis=1) if p.shape[0] > 1 else np.concatenate([d64, d64 + 1], 1)
        clear = part[:, 1] - part[:, 0] > 1e-6 * part[:, 1]   # the two nearest distances differ by more than 1e-6 relative
        assert np.array_equal(rows[clear, 0], np.argmin(d64, axis=1)[clear])
        # ties: the lowest index among the points at the float32 minimum
        d32 = R.distances(c["xyz1"][0], c["xyz2"][0][empty])
        assert np.array_equal(rows[:, 0], np.argmax(d32 == d32.min(axis=1, keepdims=True), axis=1))


def test_per_query_radii_and_dead_radii():
    c = CASES["cube_r02_k16"]
    m = 256
    rng = np.random.default_rng(5)
    radii = (10.0 ** rng.uniform(-2.0, 0.0, (1, m))).astype(np.float32)
    radii[0, ::7] = 0.0
    radii[0, 3::7] = -1.0
    radii[0, 5::11] = np.nan
    idx, cnt = R.query_ball_point(radii, 8, c["xyz1"], c["xyz2"][:, :m])
    dead = ~(radii[0] > 0)
    assert np.all(cnt[0][dead] == 0) and np.all(cnt[0][~dead] >= 1)   # the queries are dataset points: d = 1e-20 < r
    for j in range(0, m, 17):
        one, c1 = R.query_ball_point(float(radii[0, j]) if not dead[j] else 1e-30, 8, c["xyz1"], c["xyz2"][:, j:j + 1])
        assert np.array_equal(one[0, 0], idx[0, j]) and c1[0, 0] == cnt[0, j]
