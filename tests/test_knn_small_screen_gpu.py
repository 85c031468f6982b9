"""knn_small_kernel (clouds of N <= 2048, a wave per query) against oracle.knn_bruteforce: ids AND distance bits equal, through
both layouts (pm.knn_xyz on [B, N, 3], ops.knn_bruteforce on [B, 3, N]).

For K <= 8 the kernel takes a square root and builds a key only for the candidates whose SQUARED distance s passes an exact
screen (csrc/knn.hip): U = the largest of the eight minima of s over the lane groups (j % 64) // 8, keep s <= U * 1.000001f,
compact the survivors to one per lane.  A query with more than 64 survivors, and every query at K > 8, takes the unscreened
selection instead.  `survivors()` restates the screen in numpy so that each case can say which of the two paths its queries
took; the restatement evaluates the fma chain in float64 and rounds once more, which can move a count by one on a handful of
queries and is exact on the lattices.

The replay of the local forward against the eager forward at the sampled set's own shape (8 x 1024, ids against the oracle) is
tests/test_engine_gpu.py::test_local_pipeline_depth4_B8_N8192_slots_equal_serial_and_oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def sqdist(cloud):
    """[N, 3] float32 -> [N(query), N(candidate)] float32, the kernel's chain fma(dz, dz, fma(dy, dy, dx * dx))."""
    d = cloud[:, None, :].astype(np.float32) - cloud[None, :, :].astype(np.float32)  # query - candidate, rounded to f32
    d = d.astype(np.float64)
    s = (d[..., 0] * d[..., 0]).astype(np.float32).astype(np.float64)
    s = (d[..., 1] * d[..., 1] + s).astype(np.float32).astype(np.float64)
    return (d[..., 2] * d[..., 2] + s).astype(np.float32)


def survivors(cloud):
    """Per query: how many candidates pass the screen."""
    n = cloud.shape[0]
    s = sqdist(cloud)
    grp = (np.arange(n) % 64) // 8
    gmin = np.full((n, 8), np.inf, np.float32)
    for g in range(8):
        if np.any(grp == g):
            gmin[:, g] = s[:, grp == g].min(axis=1)
    ub = gmin.max(axis=1) * np.float32(1.000001)
    assert ub.dtype == np.float32
    return (s <= ub[:, None]).sum(axis=1)


def check(dev, oracle, xyz, K):
    """xyz [B, N, 3]: both layouts, ids and distance bits against the oracle.  Returns the oracle's (ids, distances)."""
    from dh3d_amd import ops, pm
    pos = np.ascontiguousarray(xyz.transpose(0, 2, 1))
    enn, ed = oracle.knn_bruteforce(pos, K)
    nn, d = pm.knn_xyz(T(xyz, dev), K)
    assert np.array_equal(nn.cpu().numpy(), enn), "knn_xyz ids"
    assert np.array_equal(d.cpu().numpy(), ed), "knn_xyz distances"
    nn, d = ops.knn_bruteforce(T(pos, dev), K)
    assert np.array_equal(nn.cpu().numpy(), enn), "knn_bruteforce ids"
    assert np.array_equal(d.cpu().numpy(), ed), "knn_bruteforce distances"
    return enn, ed


@pytest.mark.parametrize("B,N,K", [(2, 1024, 8), (1, 2048, 8), (2, 512, 8), (1, 1000, 8), (1, 70, 8), (1, 65, 3)])
def test_uniform_cube_takes_the_screened_path(dev, oracle, B, N, K):
    """The <16>, <32> and <8> instantiations at full width, and ragged last slots (N = 1000, 70, 65).  On the full-width
    clouds at most 1 % of the queries may have more than 64 survivors: the screened path is what ran."""
    xyz = np.random.default_rng(7000 + N).random((B, N, 3), dtype=np.float32)
    if N in (1024, 2048, 512):
        over = np.concatenate([survivors(c) for c in xyz]) > 64
        print("N=%d: %.2f %% of the queries above 64 survivors" % (N, 100.0 * over.mean()))
        assert over.mean() <= 0.01
    check(dev, oracle, xyz, K)


@pytest.mark.parametrize("K", [1, 3, 4, 8, 12, 16, 33])
def test_k_values_on_both_paths(dev, oracle, K):
    """K <= 8: screened; K = 12, 16, 33: every query takes the unscreened selection."""
    xyz = np.random.default_rng(7100).random((1, 1024, 3), dtype=np.float32) * 40 - 20
    check(dev, oracle, xyz, K)


def test_fewer_than_k_points_and_all_equal_points(dev, oracle):
    """N = 3, K = 4: groups without a candidate make the bound infinite, the list is padded with -1 / FLT_MAX.  300 copies of
    one point: U = 0 and the whole cloud survives, which is more than the 64 a wave compacts."""
    p3 = np.random.default_rng(0).random((1, 3, 3), dtype=np.float32)
    enn, ed = check(dev, oracle, p3, 4)
    assert np.all(enn[:, :, 3] == -1) and np.all(ed[:, :, 3] == np.finfo(np.float32).max)
    same = np.broadcast_to(np.float32([0.25, 0.5, 0.75]), (1, 300, 3)).copy()
    assert np.all(survivors(same[0]) == 300)
    check(dev, oracle, same, 8)


def test_coarse_lattice_mixes_both_paths_in_one_launch(dev, oracle):
    """Coordinates rounded to multiples of 1/4: many exact ties, ordered by the reference's rank code.  Some queries have more
    than 64 survivors and some do not, so the wave-uniform choice is made both ways within one launch."""
    xyz = np.random.default_rng(7200).random((2, 1024, 3), dtype=np.float32)
    xyz[0] = np.round(xyz[0] * 4) / 4
    n = survivors(xyz[0])
    print("lattice: %d of 1024 queries above 64 survivors (most: %d)" % (int((n > 64).sum()), int(n.max())))
    assert np.any(n > 64) and np.any(n <= 64)
    check(dev, oracle, xyz, 8)


# Two candidates whose squared distances differ by one unit of 2^-24 and whose square roots round to the same float32: on the
# 2^-12 lattice every term of the chain is exact.  The reference orders them by (distance, rank code), so the LOWER INDEX
# wins the last place of the list whichever has the smaller s.
_Q = np.array([2048, 2048, 2048], np.int64)
_A = _Q + np.array([1200, 1264, 1173], np.int64)   # s * 2^24 = 4413625
_B = _Q + np.array([2045, 465, 124], np.int64)     # s * 2^24 = 4413626


def _collapse_cloud(N, b_first):
    rng = np.random.default_rng(7300 + N)
    far = []
    while len(far) < N - 5:
        p = rng.integers(0, 4096, 3)
        if int(((p - _Q) ** 2).sum()) > 6000000:  # well behind A and B (4413625 / 4413626)
            far.append(p)
    near = [_Q, _Q + np.array([40, -12, 7]), _Q + np.array([-100, 3, 55])]  # the query and two points much nearer
    pair = [_B, _A] if b_first else [_A, _B]
    pts = np.array(near + pair + far, np.int64)
    return (pts.astype(np.float64) / 4096).astype(np.float32)[None]  # [1, N, 3], the query is point 0, the pair 3 and 4


@pytest.mark.parametrize("N", [128, 1024])
@pytest.mark.parametrize("b_first", [True, False])
def test_square_root_collapse_at_the_rank_boundary(dev, oracle, N, b_first):
    """K = 4: the query, two near points, and ONE of A and B.  With B at the lower index the reference keeps B although
    s(A) < s(B) -- a selection ordered by s would keep A.  The mirrored cloud (A lower) must keep A."""
    xyz = _collapse_cloud(N, b_first)
    assert np.array_equal(xyz[0, 0] * 4096, _Q)
    s = sqdist(xyz[0])[0]
    assert s[3 if b_first else 4] * 2.0 ** 24 == 4413626 and s[4 if b_first else 3] * 2.0 ** 24 == 4413625
    assert np.sqrt(np.float32(4413625 / 2.0 ** 24)) == np.sqrt(np.float32(4413626 / 2.0 ** 24))  # float32 sqrt, correctly rounded
    enn, _ = check(dev, oracle, xyz, 4)
    by_s = np.lexsort((np.arange(N), s))[:4]  # ordered by (s, id)
    assert list(enn[0, 0]) == [0, 1, 2, 3]  # the lower index of the pair, whichever point it is
    if b_first:
        assert list(by_s) == [0, 1, 2, 4], "the input must discriminate: by s the list ends with A"
    else:
        assert list(by_s) == [0, 1, 2, 3]
    assert survivors(xyz[0])[0] <= 64  # the query takes the screened path, A and B both among its survivors
