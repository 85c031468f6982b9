"""pm.knn_grid on the clouds that decide pass 1 of knn_grid_kernel (dh3d_amd/csrc/knn.hip): the cells of a query's box outside its
27 inner cells, listed per wave and dealt over all 64 lanes.  Ids and distance BITS equal to the brute-force kernel (pm.knn_xyz,
which has no cells) on every cloud.  A lane pools for whichever query its cell belongs to, through LDS atomics whose order changes
from run to run: every case runs twice and the two outputs are compared.

Each case first holds, on the host, the regime it is there for (tests/knn_grid_box_cases.py restates the cell-set rule; the grid
it works on is checked against the table the sort returned):
  uniform_2x4096   one point per cell: most queries reach past the 27 cells, in several directions at once (K = 8), few (K = 3)
  uniform_3x8192   most queries have an empty set; some waves of 16 have no cell at all and skip the pass, some do not; K = 1:
                   nobody has one
  holes_2x8192     27-cell neighbourhoods emptied but for 0 / 3 / 8 points, at the grid's corners, edges, faces and inside: no
                   K-th distance after pass 0 (the +-2 block, then the restart), K-th neighbours two cells away, clipped boxes
  slab_2x8192      a 32 x 32 x 4 grid: the box has its own extent per axis and spans the whole thin axis.  (At this density no
                   bound from 27 cells reaches past +-2 cells in z: 0 such queries in the restatement; it is not asserted.)
  lattice / duplicates   points on cell faces, ties at the box's edge
  coarse_*         the grid with 3, 4 and 6 bits dropped; 2 x 5: N < K, no query ever has a K-th distance
  overflow_1x8192  300 copies of one point two cells from a query whose 27 cells hold just K: the cell of the copies belongs to
                   the query's set and its pool passes kGridCap, in the hands of a lane of whatever query -- the query restarts
                   over the group boxes
A ball wider than kGridBoxCells = 640 cells cannot come from a bound within 27 cells of a grid whose cells are at most twice as
long as wide (at most 8 cells per axis: 512); the device code sends it to the restart, no case reaches it."""
import numpy as np
import pytest
import torch

import knn_grid_box_cases as C
from test_knn_grid_regimes_gpu import _knn_grid_checked

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(C.CASES))
def test_knn_grid_box_pass_bit_equal_twice(dev, case):
    from dh3d_amd import pm
    N, Ks, kinds, drop, want = C.CASES[case]
    B = len(kinds)
    pts = C.batch(case)
    t = torch.from_numpy(pts).to(dev)
    srt, gbox, cells = pm.spatial_sort_cells(t)
    table = cells.cpu().numpy()
    assert not table[:, 4106].any(), (case, "crowded flags", table[:, 4106])
    for K in Ks:
        assert pm.knn_grid_plan(B, N, K) == (4, drop), (case, K)
        # the regime, on the grid of the returned table
        st = C.restate(pts[0], K, drop)
        head = C.S.R.restate(pts[0])["cells"]
        assert np.array_equal(table[0, 4100:4108], head[4100:4108]), (case, "the restated grid is not the table's")
        got = C.regimes(st)
        if K == Ks[0]:
            for w in want:
                assert got[w] > 0, (case, K, w, got)
        waves = C.wave_cells(st)
        if case == "uniform_2x4096" and K == 8:
            assert got["nonempty"] > N // 2 and ((st["lo"] < -1).sum(1) + (st["hi"] > 1).sum(1) >= 2).sum() > N // 4, got
        if case == "uniform_3x8192":
            if K == 8:
                assert got["empty"] > 0.8 * N and (waves == 0).any() and (waves > 0).any(), got
            else:
                assert got["empty"] == N
        if case == "holes_2x8192":
            far = np.isfinite(st["bound"]) & ((st["lo"] <= -2) & (st["hi"] >= 2)).all(1)   # two cells away in every direction
            clipped = (st["ncell"] > 0) & ((st["cell"] == 0) | (st["cell"] == st["dims"] - 1)).any(1)
            assert far.any() and clipped.any() and got["no_kth"] >= 5, (got, far.sum(), clipped.sum())
        if case == "slab_2x8192":
            assert list(st["dims"]) == [32, 32, 4]
            b = st["hi"] - st["lo"] + 1
            assert (b[:, 2] == 4).any() and (b[:, 0] != b[:, 2]).any()
        if case == "coarse_2x5":
            assert got["no_kth"] == N
        if case == "overflow_1x8192":
            assert np.isfinite(st["bound"][C.OVERFLOW_QUERY]) and C.pass1_pool(pts[0], st, C.OVERFLOW_QUERY) > C.POOL_CAP
        nn, dist = _knn_grid_checked(srt, gbox, cells, K)
        nn2, dist2 = _knn_grid_checked(srt, gbox, cells, K)
        assert torch.equal(nn, nn2) and torch.equal(dist.view(torch.int32), dist2.view(torch.int32)), (case, K, "two runs differ")
        nn_b, d_b = pm.knn_xyz(t, K)
        bad = (nn != nn_b).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, (case, K, "clouds whose ids differ from knn_xyz", bad)
        assert torch.equal(dist.view(torch.int32), d_b.view(torch.int32)), (case, K)
