"""The premise of pass 1's cell set in knn_grid_kernel (dh3d_amd/csrc/knn.hip), held without a GPU on the bench's own cube
(tests/knn_grid_box_cases.py restates the rule): nearly every query's box is the 27 cells pass 0 has served, so enumerating the
cells outside them finds one or two per query where walking the box's columns looked up more than fifteen ranges; and the clouds
of tests/test_knn_grid_box_gpu.py reach the regimes they are there for."""
import numpy as np
import pytest

import knn_grid_box_cases as C


def test_most_queries_of_the_bench_cube_have_nothing_to_look_at():
    st = C.restate(C.bench_cube(8192), 8, 0)
    assert st["flag"] == 0 and list(st["dims"]) == [16, 16, 16]
    empty = (st["ncell"] == 0).mean()
    print("8192: empty %.3f, cells of the set %.2f / query, %.1f / wave, the column rule: %.2f columns, %.2f ranges / query"
          % (empty, st["ncell"].mean(), C.wave_cells(st).mean(), st["columns"].mean(), st["ranges_old"].mean()))
    assert empty > 0.80
    assert st["ncell"].mean() < 2 and st["ranges_old"].mean() > 15


def test_most_waves_of_the_cfg5_cube_skip_the_pass():
    st = C.restate(C.bench_cube(16384), 8, 0)
    assert st["flag"] == 0
    none = (C.wave_cells(st) == 0).mean()
    print("16384: waves without a cell %.3f, empty queries %.4f" % (none, (st["ncell"] == 0).mean()))
    assert none > 0.90


def test_the_set_is_the_box_without_its_inner_block():
    """the count against an enumeration, on the cloud with the widest variety of boxes (holes: clipped, +-2 blocks, wide balls)"""
    pts = C.batch("holes_2x8192")[0]
    st = C.restate(pts, 8, 0)
    for qi in np.random.default_rng(5).choice(len(pts), 200, replace=False):
        lo, hi = st["lo"][qi], st["hi"][qi]
        cells = [(x, y, z) for x in range(lo[0], hi[0] + 1) for y in range(lo[1], hi[1] + 1) for z in range(lo[2], hi[2] + 1)
                 if max(abs(x), abs(y), abs(z)) > 1]
        assert st["wide"][qi] or st["ncell"][qi] == len(cells), qi
        c = st["cell"][qi]
        assert (c + lo >= 0).all() and (c + hi <= st["dims"] - 1).all(), qi


@pytest.mark.parametrize("case", list(C.CASES))
def test_case_reaches_its_regimes(case):
    n, Ks, kinds, drop, want = C.CASES[case]
    assert drop == C.S.grid_drop(n)
    pts = C.batch(case)
    st = C.restate(pts[0], Ks[0], drop)
    got = C.regimes(st)
    print(case, got)
    assert st["flag"] == 0, "the cloud must stay with the cell lists"
    for w in want:
        assert got[w] > 0, (case, w, got)
    assert got["empty"] + got["nonempty"] + got["no_kth"] + got["wide"] >= n   # (a query without a bound has a set too)
