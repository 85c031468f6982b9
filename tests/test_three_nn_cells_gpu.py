"""GPU parity of three_nn through the candidate set's cell table (pm.three_nn_sorted(..., cells2=), csrc/pointnet2.hip
three_nn_pruned_kernel_cells): ids and distance bits == the plain kernel (ops.three_nn) on both kinds of table -- the
candidate set's own grid (spatial_sort_cells: queries may lie outside it) and the cloud's grid (fps_sorted_ordered) -- on
clouds that stress the cell arithmetic, through the level dispatcher, and on the sizes that fall back to the old kernels.
Every comparison is np.array_equal on ids and on distance bits."""
import numpy as np
import pytest
import torch

from test_levels_gpu import _cloud
from test_ops_gpu import _knn_clouds

pytestmark = pytest.mark.gpu

B = 3
SHAPES = [(64 * 5 + 17, 128), (1000, 200), (2048, 512), (4096, 1024)]  # ragged last group | m % 32 != 0 | ... | the cap
CLOUDS = ["uniform", "blob", "dup", "lattice", "slab", "plane", "cluster", "one_point", "mixed"]
SCHED_CUBE = 0x186186


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _subset(xyz1, m, rng):
    sel = np.stack([rng.choice(xyz1.shape[1], m, replace=False) for _ in range(len(xyz1))])
    return np.take_along_axis(xyz1, sel[:, :, None], 1)


def _pair(kind, n, m, rng):
    """(queries [B,n,3], candidates [B,m,3]); the candidates are points of the query cloud (distance-0 hits) unless the
    kind says otherwise."""
    seed = int(rng.integers(1 << 30))
    if kind in ("uniform", "blob", "dup", "lattice"):
        xyz1 = _cloud(kind, B, n, seed)
    elif kind == "slab":      # 60 x 60 x 8: the grid bits are not dealt 4 + 4 + 4
        xyz1 = _knn_clouds("oxford_extent", B, n, rng)
    elif kind == "plane":     # z = const: a zero-extent axis
        xyz1 = _knn_clouds("plane", B, n, rng)
    elif kind == "cluster":   # the candidates in a box a tenth as wide as the queries': queries outside the table's grid
        xyz1 = rng.random((B, n, 3), dtype=np.float32)
        return xyz1, (0.45 + 0.1 * rng.random((B, m, 3), dtype=np.float32)).astype(np.float32)
    elif kind == "one_point":  # every candidate in ONE cell (a zero-extent grid), the queries spread around it
        xyz1 = rng.random((B, n, 3), dtype=np.float32)
        return xyz1, np.tile(rng.random((B, 1, 3), dtype=np.float32), (1, m, 1))
    elif kind == "mixed":     # one batch: a uniform, a crowded (street scene) and a clustered cloud
        xyz1 = np.concatenate([_knn_clouds(k, 1, n, rng) for k in ("uniform", "scene", "clusters")])
    else:
        raise KeyError(kind)
    return xyz1, _subset(xyz1, m, rng)


def _bits(t):
    return t.view(torch.int32).cpu().numpy()


def _assert_same(got, want, what):
    (d, i), (d0, i0) = got, want
    assert np.array_equal(i.cpu().numpy(), i0.cpu().numpy()), (what, "ids")
    assert np.array_equal(_bits(d), _bits(d0)), (what, "distance bits")


@pytest.mark.parametrize("kind", CLOUDS)
def test_cells_on_the_candidates_own_grid(dev, oracle, kind):
    from dh3d_amd import ops, pm
    rng = np.random.default_rng(CLOUDS.index(kind) + 77)
    for n, m in SHAPES:
        xyz1, xyz2 = _pair(kind, n, m, rng)
        t1, t2 = T(xyz1, dev), T(xyz2, dev)
        s1, g1 = pm.spatial_sort(t1)
        s2, g2, c2 = pm.spatial_sort_cells(t2)
        if kind == "slab":
            assert all(int(s) != SCHED_CUBE for s in c2[:, 4107].cpu().tolist())
        got = pm.three_nn_sorted(s1, g1, s2, g2, cells2=c2)
        _assert_same(got, ops.three_nn(t1, t2), (kind, n, m))
        if kind == "dup" and n == 1000:
            de, ie = oracle.three_nn(xyz1, xyz2)
            assert np.array_equal(got[1].cpu().numpy(), ie), (kind, "ids vs the oracle")
            assert np.array_equal(_bits(got[0]), de.view(np.int32)), (kind, "distance bits vs the oracle")


@pytest.mark.parametrize("N,m", [(4096, 512), (8192, 1024)])
def test_cells_on_the_clouds_grid(dev, N, m):
    """The table the FPS kernel writes for its picks on the cloud's own grid."""
    from dh3d_amd import ops, pm
    xyz = _cloud("blob", 2, N, seed=N + m)
    xyz[1] = np.random.default_rng(N).random((N, 3), dtype=np.float32)
    t = T(xyz, dev)
    srt, gbox, cells = pm.spatial_sort_cells(t)
    _, xyz_s, srt_s, gbox_s, cells_s = pm.fps_sorted_ordered(srt, gbox, m, cells=cells)
    assert cells_s is not None
    got = pm.three_nn_sorted(srt, gbox, srt_s, gbox_s, cells2=cells_s)
    _assert_same(got, pm.three_nn_sorted(srt, gbox, srt_s, gbox_s), "vs the box-pruned kernel")
    _assert_same(got, ops.three_nn(t, xyz_s), "vs the plain kernel")


@pytest.mark.parametrize("cells", [True, False])
def test_level_passes_the_table(dev, oracle, cells):
    from dh3d_amd import backbones as bb
    xyz = _cloud("uniform", 2, 4096, seed=4096 + int(cells))
    geo = bb.Geometry(T(xyz, dev), 8)
    geo.ordered(cells=cells)
    lv = geo.level(8, 8)
    assert lv["_path"]["nn3"] == "sorted"
    assert lv["_path"]["nn3_cells"] is cells
    d3, i3 = oracle.three_nn(xyz, lv["xyz_s"].cpu().numpy())
    assert np.array_equal(lv["nn3_idx"].cpu().numpy(), i3)
    assert np.array_equal(_bits(lv["nn3_dist"]), d3.view(np.int32))


@pytest.mark.parametrize("m", [127, 767, 768, 1025])
def test_size_thresholds(dev, m):
    """127 / 1025: outside the cell kernel's range, the old kernels serve them with a table given; 767 / 768: the two
    coarsenings of the grid (csrc/pointnet2.hip nn3_cell_drop)."""
    from dh3d_amd import ops, pm
    rng = np.random.default_rng(m)
    xyz1 = rng.random((B, 2048, 3), dtype=np.float32)
    xyz2 = _subset(xyz1, m, rng)
    t1, t2 = T(xyz1, dev), T(xyz2, dev)
    s1, g1 = pm.spatial_sort(t1)
    s2, g2, c2 = pm.spatial_sort_cells(t2)
    _assert_same(pm.three_nn_sorted(s1, g1, s2, g2, cells2=c2), ops.three_nn(t1, t2), m)
