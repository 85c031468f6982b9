"""CPU: the numpy restatement of the FPFH rule (tests/fpfh_reference.py; include/dh3d_hip.h dh3d_spfh_counts / dh3d_fpfh) on
hand-worked pairs whose bins are known, the properties the rule promises (blocks that sum to 200, a point without near
pairs keeps its own SPFH, counts that do not change under a rigid motion) and the condition on the fixtures that
tests/test_fpfh_gpu.py compares the kernels on: no point of them has a pair coordinate within 1e-9 of a bin edge."""
import numpy as np
import pytest

import fpfh_reference as fr
import icp_reference as ir


def _one(counts, row, f1=None, f2=None, f3=None, m=1):
    """The count row holds m pairs, all in the given bins."""
    exp = np.zeros(36, np.uint8)
    for f, b in enumerate((f1, f2, f3)):
        if b is not None:
            exp[11 * f + b] = m
    exp[33] = m if f1 is not None else 0
    assert np.array_equal(counts[row], exp), (row, counts[row], exp)


def test_parallel_normals_across_the_line():
    """Two points one metre apart along x, both normals along z: a1 = a2 = 0 (no swap), v = d x n = (0, -1, 0), w = n x v =
    (1, 0, 0), f2 = 0, f1 = atan2(0, 1) = 0, f3 = 0: every coordinate is 5.5, bin 5 of each histogram, seen from both ends."""
    x = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    nr = np.array([[0, 0, 1], [0, 0, 1]], np.float32)
    nbr = np.array([[0, 1], [1, 0]])                     # lists that hold the point itself: it never pairs with itself
    r = fr.compute(x, nr, nbr)
    assert np.allclose(r["s"][0, 1], 5.5, atol=1e-12) and np.allclose(r["s"][1, 1], 5.5, atol=1e-12)
    assert not r["usable"][:, 0].any() and r["usable"][:, 1].all()
    for i in range(2):
        _one(r["counts"], i, 5, 5, 5)
    assert np.allclose(r["margin"], 0.5, atol=1e-12)
    # SPFH = 100 in bin 5 of each block; the one neighbour's SPFH, weighted and scaled to 100, adds 100: 200 per block
    exp = np.zeros(36)
    exp[[5, 16, 27]] = 200.0
    assert np.array_equal(r["fpfh"][0], exp) and np.array_equal(r["fpfh"][1], exp)


def test_swap_branch():
    """n_0 = z, n_1 = (0.6, 0, 0.8), d = x: from point 0, a1 = 0 and a2 = 0.6, so the roles swap: n1 = n_1, n2 = n_0, d = -x,
    f3 = -0.6 -> s3 = 2.2; v = (0, 1, 0) (0.8 / 0.8), f2 = 0 -> s2 = 5.5; w = (-0.8, 0, 0.6), f1 = atan2(0.6, 0.8) = 0.6435 ->
    s1 = 6.6266.  From point 1 nothing swaps (|a1| = 0.6 >= |a2| = 0) and the frame is the same one: the same bins."""
    x = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    nr = np.array([[0, 0, 1], [0.6, 0, 0.8]], np.float32)
    r = fr.compute(x, nr, np.array([[1], [0]]))
    s1 = (np.arctan2(0.6, 0.8) + np.pi) * 11.0 / (2.0 * np.pi)
    for i in range(2):
        assert np.allclose(r["s"][i, 0], [s1, 5.5, 2.2], atol=1e-6), r["s"][i, 0]
        _one(r["counts"], i, 6, 5, 2)
    # a repeated id counts as often as it occurs
    r3 = fr.spfh_counts(x, nr, np.array([[1, 1, 1], [0, -1, 0]]))
    _one(r3["counts"], 0, 6, 5, 2, m=3)
    _one(r3["counts"], 1, 6, 5, 2, m=2)


def test_unusable_and_not_near_pairs():
    # |v| = 0: the normal of the frame lies along the line, from either end (the second end swaps into it)
    x = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    nr = np.array([[1, 0, 0], [0, 0, 1]], np.float32)
    r = fr.compute(x, nr, np.array([[1], [0]]))
    assert r["near"].all() and not r["usable"].any() and not r["counts"].any() and not r["fpfh"].any()
    assert np.isinf(r["margin"]).all()
    # a zero normal at either end
    nz = np.array([[0, 0, 1], [0, 0, 0]], np.float32)
    r = fr.compute(x, nz, np.array([[1], [0]]))
    assert r["near"].all() and not r["usable"].any() and not r["counts"].any()
    # coincident points are not near; neither are ids out of range, the point itself, rows behind the count
    x4 = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
    n4 = np.tile(np.array([0, 0, 1], np.float32), (4, 1))
    nbr = np.array([[1, 0, -1, 4, 3, 7], [0, 1, 2, 2, -7, 2 ** 31 - 1], [0, 1, 2, 3, 3, 3], [0, 1, 2, 3, 3, 3]])
    r = fr.compute(x4, n4, nbr, n=3)
    assert not r["near"][0].any() and list(r["near"][1]) == [False, False, True, True, False, False]
    assert list(r["near"][2]) == [True, True, False, False, False, False]
    _one(r["counts"], 0)
    _one(r["counts"], 1, 5, 5, 5, m=2)
    _one(r["counts"], 2, 5, 5, 5, m=2)
    assert not r["counts"][3].any() and not r["fpfh"][3].any()                 # a row behind the count
    assert not r["fpfh"][0].any()                                              # no near pair and no pair of its own
    # max_dist: the pair at distance 2 drops out at 1.5, stays at exactly 2
    nb = np.array([[2, 3], [2, 3], [0, 3], [0, 2]])
    assert fr.spfh_counts(x4, n4, nb, max_dist=1.5)["counts"][0, 33] == 1
    assert fr.spfh_counts(x4, n4, nb, max_dist=2.0)["counts"][0, 33] == 2
    assert fr.spfh_counts(x4, n4, nb, max_dist=None)["counts"][0, 33] == 2
    # ids: rows gathered, zero rows for ids outside 0 .. n - 1
    full = fr.compute(x4, n4, nbr, n=3)["fpfh"]
    got = fr.compute(x4, n4, nbr, n=3, ids=[2, -1, 1, 3, 4, 2])["fpfh"]
    assert np.array_equal(got[[0, 2, 5]], full[[2, 1, 2]]) and not got[[1, 3, 4]].any()


@pytest.fixture(scope="module")
def demo():
    return fr.demo_fixture()


@pytest.mark.parametrize("K", (8, 32))
def test_blocks_sum_to_200_and_lonely_points_keep_their_spfh(demo, K):
    for p, n in enumerate(fr.COUNTS):
        x, nr, nbr = demo["X"][p], demo["normals"][p], demo["ids"][p][:, :K]
        r = fr.compute(x, nr, nbr, n)
        f = r["fpfh"]
        assert f.shape == (fr.N_DEMO, 36) and not f[n:].any() and not f[:, 33:].any() and (f >= 0).all()
        sums = f[:n, :33].reshape(n, 3, 11).sum(axis=2)
        own = fr.spfh(r["counts"])[:n].reshape(n, 3, 11).sum(axis=2)
        assert (np.abs(own[r["counts"][:n, 33] > 0] - 100.0) <= 1e-9).all()
        full = (r["counts"][:n, 33] > 0) & (r["counts"][:n][np.where(r["near"][:n], nbr[:n], 0), 33] * r["near"][:n]).any(axis=1)
        assert full.sum() > 0.95 * n
        assert (np.abs(sums[full] - 200.0) <= 1e-9).all(), np.abs(sums[full] - 200.0).max()
        assert ((np.abs(sums - 200.0) <= 1e-9) | (np.abs(sums - 100.0) <= 1e-9) | (sums == 0.0)).all()
        # cut some points' lists off: with stage 1's counts kept, such a point's row is its own SPFH
        cut = nbr.copy()
        cut[5:n:7] = -1
        lone = fr.fpfh(x, cut, r["counts"], n)
        assert np.array_equal(lone[5:n:7, :33], fr.spfh(r["counts"])[5:n:7]) and lone[5:n:7].any()


def test_counts_do_not_change_under_an_exact_rigid_motion():
    """The cloud on a 1/1024 m lattice, turned by a quarter turn about z composed with a cyclic change of axes and moved by
    a lattice vector: every moved coordinate and every turned normal is exact in float32, so the moved pairs are the same
    pairs; only the order of the terms inside dot / cross changes, an error of 1e-15 in a coordinate.  The counts are equal
    at every point with margin >= 1e-9 (and the test requires nearly all points to be such)."""
    import icp_plane_reference as pr
    a = ir.demo_pair("local_642", 512, 3)[0]
    x = (np.rint(a.astype(np.float64) * 1024.0) / 1024.0).astype(np.float32)
    ids = pr.knn_ids(x, 24)
    nr = pr.normals(x, ids[:, :16])["normals"].astype(np.float32)
    R = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float64) @ np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    assert abs(np.linalg.det(R) - 1.0) < 1e-12
    t = np.array([3.5, -2.25, 10.0])
    xm = x.astype(np.float64) @ R.T + t
    assert np.array_equal(xm, xm.astype(np.float32).astype(np.float64))         # the motion is exact
    nm = (nr.astype(np.float64) @ R.T).astype(np.float32)
    for K, md in ((24, None), (12, 0.6)):
        r0 = fr.spfh_counts(x, nr, ids[:, :K], max_dist=md)
        r1 = fr.spfh_counts(xm.astype(np.float32), nm, ids[:, :K], max_dist=md)
        sure = r0["margin"] >= 1e-9
        assert sure.sum() >= 0.99 * len(x)
        assert np.array_equal(r0["counts"][sure], r1["counts"][sure])
        assert r0["counts"][:, 33].sum() > 0.9 * (r0["near"].sum())


def test_fixture_margins(demo):
    """The condition on the fixtures of tests/test_fpfh_gpu.py: no point has a pair coordinate within 1e-9 of a bin edge, at
    any K compared there, so the kernels' counts can be required bit-equal at EVERY point."""
    low = np.inf
    for K in fr.KS + (8, 32):
        for p, n in enumerate(fr.COUNTS):
            r = fr.spfh_counts(demo["X"][p], demo["normals"][p], demo["ids"][p][:, :K], n)
            low = min(low, float(r["margin"].min()))
            assert (r["margin"] >= 1e-9).all(), (K, p, r["margin"].min())
            if K == 1:
                assert not r["counts"].any()                                     # the self-only list: m = 0 everywhere
    print("smallest margin", low)
