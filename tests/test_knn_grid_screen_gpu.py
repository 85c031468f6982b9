"""pm.knn_grid on the clouds that decide the screened pass-0 drain of knn_grid_kernel (csrc/knn.hip, `drain_screened`): ids and
distance BITS equal to the brute-force kernel (pm.knn_xyz, which the screen does not touch) on every cloud and to the CPU oracle
on one cloud per case.  The candidates reach a query's lanes through LDS atomics in an order that changes from run to run, so
the screen's threshold varies between runs and the result must not: every case runs twice and the two outputs are compared.

What a case is there for (tests/knn_grid_screen_cases.py builds the clouds; tests/test_knn_grid_screen_host.py counts, without
a GPU, how many of their queries take the screened drain and how many the old one; the choice is a wave's, 16 queries):
  uniform_d0 / _d1 / _d3   the grid at full resolution and with 1 and 3 bits dropped, K = 8, 5, 3, 1: nearly all screened
  uniform_code2 / _code0   the other two instantiations, knn_grid_kernel<4, 2> and <4, 0>; one point per cell: about half the
                           waves have no pool past 32 and keep the old drain
  lattice_*                exact ties everywhere: many candidates at the threshold itself, the rank code decides
  duplicates               every point twice: U = 0 for a query whose copy sits in every lane's first two
  many_copies              9..12 identical points, more than K: the rank decides which K, the screen keeps exactly the copies;
                           three such groups side by side push the pool past the screened drain's size: both drains see copies
  collapse                 s1 < s2 with one rounded distance as the 8th / 9th neighbour: both survive, the rank code decides
  dense_cell               400 points in one cell of a cloud that is not crowded: pools overflow, records go down direct(), the
                           waves around the cell take the old drain whole
  margin / plane / oxford_extent   a grid stretched by a few far points, a grid without a z axis (short pools, the restart
                           over the group boxes), the per-axis box of pass 1
  tiny_5 / _7 / _9         N < K: padding with -1 / FLT_MAX; pools below 2 L (in a screening wave such a pool is ranked whole:
                           lattice_4096 and plane have them)
  mixed_6x8192             crowded clouds on the pruned scan in the same launch, intact"""
import numpy as np
import pytest
import torch

import knn_grid_screen_cases as C
from test_knn_grid_regimes_gpu import _knn_grid_checked

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(C.CASES))
def test_knn_grid_screened_drain_bit_equal_twice(dev, oracle, case):
    from dh3d_amd import pm
    N, Ks, kinds, flags, code = C.CASES[case]
    B = len(kinds)
    pts = C.batch(case)
    t = torch.from_numpy(pts).to(dev)
    srt, gbox, cells = pm.spatial_sort_cells(t)
    assert (cells[:, 4106] != 0).int().cpu().tolist() == list(flags), case
    ob = flags.index(0)  # the oracle's cloud: the first one the cell lists serve
    pos = np.ascontiguousarray(pts[ob:ob + 1].transpose(0, 2, 1))
    for K in Ks:
        assert pm.knn_grid_plan(B, N, K) == (code, C.grid_drop(N)), (case, K)
        nn, dist = _knn_grid_checked(srt, gbox, cells, K)
        nn2, dist2 = _knn_grid_checked(srt, gbox, cells, K)
        assert torch.equal(nn, nn2) and torch.equal(dist.view(torch.int32), dist2.view(torch.int32)), (case, K, "two runs differ")
        nn_b, d_b = pm.knn_xyz(t, K)
        bad = (nn != nn_b).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, (case, K, "clouds whose ids differ from knn_xyz", bad, [kinds[b] for b in bad])
        assert torch.equal(dist.view(torch.int32), d_b.view(torch.int32)), (case, K)
        nn_o, d_o = oracle.knn_bruteforce(pos, K)
        assert np.array_equal(nn[ob].cpu().numpy(), nn_o[0]), (case, K, "ids differ from the oracle")
        assert np.array_equal(dist[ob].cpu().numpy().view(np.uint32), d_o[0].view(np.uint32)), (case, K)
        if case == "collapse":
            for j in range(C.COLLAPSE_SITES):  # the query, its six near points, then the pair's lower rank code: record 9 j + 7
                assert nn_o[0, 9 * j].tolist() == list(range(9 * j, 9 * j + 8)), (j, nn_o[0, 9 * j])
        if N < K:
            assert np.all(nn_o[0, :, N:] == -1) and np.all(d_o[0, :, N:] == np.finfo(np.float32).max)
