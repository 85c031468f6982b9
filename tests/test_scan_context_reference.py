"""CPU: the numpy restatement of Scan Context (tests/scan_context_reference.py) has the properties the rules of
include/dh3d_hip.h promise -- exact rolls under exact rotations, a zero distance at the roll's shift, every boundary case
of the bin rules where the header puts it -- reads the tables the package builds, and leaves the GPU test the margin it
relies on."""
import numpy as np
import pytest

import scan_context_reference as R

NR, NS, RADIUS = 20, 60, 20.0


@pytest.fixture(scope="module")
def images():
    clouds = np.stack([R.scene(s) for s in range(8)])
    return clouds, R.scan_context(clouds, None, None, NR, NS, RADIUS, 2.0)[0]


def test_tables_are_the_packages():
    from dh3d_amd import scancontext
    for grid in ((20, 60, 80.0), (20, 60, 20.0), (4, 8, 3.5), (32, 128, 100.0)):
        for mine, theirs in zip(R.tables(*grid), scancontext.tables(*grid)):
            assert mine.dtype == theirs.dtype == np.float64 and mine.shape == theirs.shape
            assert np.array_equal(mine.view(np.uint64), theirs.view(np.uint64)), grid
    sector_dir, ring_edge2 = R.tables(20, 60, 80.0)
    assert sector_dir.shape == (29, 2) and ring_edge2.shape == (21,) and ring_edge2[20] == 6400.0 and ring_edge2[0] == 0.0
    assert (np.diff(ring_edge2) > 0).all() and (sector_dir[:, 1] > 0).all()


def test_scenes_fill_the_image(images):
    clouds, desc = images
    assert clouds.shape == (8, 4000, 3) and np.abs(clouds).max() <= 20.0
    occupied = (desc > 0).mean()
    assert 0.4 < occupied < 0.9, occupied
    assert (desc >= 0).all() and desc.max() < 8.1


def test_half_turn_rolls_by_half_exactly(images):
    """(x, y) -> (-x, -y) is the half rule itself: every point moves Ns/2 sectors on, whatever the rounding."""
    clouds, desc = images
    turned, _ = R.scan_context(R.rotate_quarter(clouds, 2), None, None, NR, NS, RADIUS, 2.0)
    assert np.array_equal(turned, np.roll(desc, NS // 2, axis=2))
    rng = np.random.default_rng(0)
    wild = (rng.standard_normal((1, 5000, 3)) * [9, 9, 1]).astype(np.float32)   # odd grids, points on no lattice
    for nr, ns in ((4, 8), (12, 36), (32, 128)):
        a, _ = R.scan_context(wild, None, None, nr, ns, 15.0, 2.0)
        b, _ = R.scan_context(R.rotate_quarter(wild, 2), None, None, nr, ns, 15.0, 2.0)
        assert np.array_equal(b, np.roll(a, ns // 2, axis=2)), (nr, ns)


def test_quarter_turn_rolls_by_a_quarter(images):
    clouds, desc = images
    for quarters in (1, 3):
        turned, keys = R.scan_context(R.rotate_quarter(clouds, quarters), None, None, NR, NS, RADIUS, 2.0)
        assert np.array_equal(turned, np.roll(desc, quarters * NS // 4, axis=2)), quarters


def test_distance_of_a_roll_is_zero_at_its_shift(images):
    """Direction: if the map image is the query's rolled by n (the map cloud = Rz(n 2 pi / Ns) applied to the query cloud),
    the best shift is n."""
    _, desc = images
    for s, n in ((0, 0), (1, 1), (2, 17), (3, 30), (4, 59)):
        d = R.shifted_distances(desc[s], np.roll(desc[s], n, axis=1))
        assert d[n] <= 1e-15 and int(np.argmin(d)) == n
        assert np.partition(d, 1)[1] - d[n] > 0.05                  # the scenes are not symmetric: one clear minimum
    dist, shift, gap = R.distance(desc[:2], np.roll(desc, 7, axis=2), np.array([[0, 1, -1], [1, 9, 0]], np.int32), map_count=8)
    assert shift.tolist() == [[7, shift[0, 1], -1], [7, -1, shift[1, 2]]] and dist[0, 0] <= 1e-15 and dist[1, 0] <= 1e-15
    assert np.isinf(dist[0, 2]) and np.isinf(dist[1, 1]) and np.isinf(gap[0, 2])
    turned, _ = R.scan_context(R.rotate_quarter(R.scene(0), 1)[None], None, None, NR, NS, RADIUS, 2.0)
    d = R.shifted_distances(desc[0], turned[0])                     # map cloud = Rz(90 deg) query cloud: shift Ns/4
    assert int(np.argmin(d)) == NS // 4 and d[NS // 4] <= 1e-15


def test_distance_with_a_side_of_zeros_is_exactly_one(images):
    _, desc = images
    zero = np.zeros_like(desc[0])
    for q, c in ((zero, zero), (zero, desc[0]), (desc[0], zero)):
        d = R.shifted_distances(q, c)
        assert (d == 1.0).all() and int(np.argmin(d)) == 0
    one_column = zero.copy()
    one_column[:, 5] = desc[0][:, np.argmax(desc[0].sum(0))]
    d = R.shifted_distances(one_column, np.roll(one_column, 3, axis=1))   # empty columns are left out, not counted as 0
    assert d[3] <= 1e-15 and (np.delete(d, 3) == 1.0).all()


def test_bin_rules_on_every_edge():
    pts, counts, ring, sector = R.boundary_cloud()
    sector_dir, ring_edge2 = R.tables(NR, NS, RADIUS)
    got_counts, got_ring, got_sector, h = R.bins_of(pts, None, sector_dir, ring_edge2, 2.0)
    assert got_counts.tolist() == counts.tolist()
    assert got_ring[counts].tolist() == ring[counts].tolist()
    assert got_sector[counts].tolist() == sector[counts].tolist()
    desc, keys = R.scan_context(pts[None], None, None, NR, NS, RADIUS, 2.0)
    assert desc[0, 5, 8] == 3.0 and desc[0, 0, 59] == 3.0 and desc[0, 2, 7] > 0 and desc[0, 2, 7] < 1e-6
    assert int((desc > 0).sum()) == len({(r, s) for r, s, c in zip(ring, sector, counts) if c})
    assert keys[0, 5] == np.float32((3.0 + 3.0) / 60)               # ring 5: (3, 4) and (-3, -4)
    # a centre moves the edges with it; num_valid cuts the cloud; the count is clamped
    moved, _ = R.scan_context(pts[None] + np.float32([10, -5, 0]), None, np.float32([[10, -5]]), NR, NS, RADIUS, 2.0)
    assert np.array_equal(moved, desc)
    first, _ = R.scan_context(pts[None], [1], None, NR, NS, RADIUS, 2.0)
    assert int((first > 0).sum()) == 1 and first[0, 5, 8] == 3.0
    none, keys = R.scan_context(pts[None], [-3], None, NR, NS, RADIUS, 2.0)
    assert not none.any() and not keys.any()
    every, _ = R.scan_context(pts[None], [1000], None, NR, NS, RADIUS, 2.0)
    assert np.array_equal(every, desc)


def test_ring_key_is_the_mean_and_survives_a_roll(images):
    _, desc = images
    keys = R.ring_keys(desc)
    assert keys.dtype == np.float32 and np.allclose(keys, desc.astype(np.float64).mean(2), rtol=1e-6)
    assert np.abs(R.ring_keys(np.roll(desc, 11, axis=2)) - keys).max() <= 1e-6


@pytest.mark.parametrize("grid", [(20, 60, 48, 8, 24), (4, 8, 3, 64, 6), (32, 128, 3, 64, 6)])
def test_margin_the_gpu_test_relies_on(grid):
    """The GPU test compares shifts only where the best shift wins by more than 1e-9 and may skip 2 % of the pairs: the
    restatement's own share of closer calls stays inside that on every fixture used there."""
    nr, ns, Q, C, n_scenes = grid
    qry, mp, cand, count = R.distance_fixture(nr, ns, Q, C, n_scenes)
    dist, shift, gap = R.distance(qry, mp, cand, count)
    valid = (cand >= 0) & (cand < count)
    assert valid.sum() > 0.6 * Q * C and (~valid).sum() >= 4
    close = valid & (gap <= 1e-9)
    assert close.sum() <= 0.02 * Q * C, (int(close.sum()), Q * C)
    assert dist[Q - 1, 0] == 1.0 and shift[Q - 1, 0] == 0             # zeros against zeros
    assert (dist[valid] >= -1e-15).all() and (dist[valid] <= 2.0).all()
    assert np.isinf(dist[~valid]).all() and (shift[~valid] == -1).all()
    order = R.order_of(dist, cand)
    assert (np.sort(order, 1) == np.arange(C)).all()
