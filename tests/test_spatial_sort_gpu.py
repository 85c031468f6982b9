"""GPU: the spatial sort (csrc/spatial.hip) against its numpy restatement (tests/spatial_reference.py), bit for bit -- the
Morton order, the records, the boxes, the cell table and its header -- on every instantiation from both sides of its limit
and on the cloud kinds the kernel branches on (cube / deposit-table path, clamp, clip, ties, degenerate extents); then the
consumers of the sort on clouds far from the origin, where the grid's float32 boundary arithmetic has the least room.  No
tolerance anywhere: tests/test_spatial_reference.py holds the restatement and the cases to their premises on the CPU."""
import numpy as np
import pytest
import torch

import spatial_reference as R

pytestmark = pytest.mark.gpu


def _bits(t):
    """A float32 / int32 tensor -> its int32 bit patterns on the host."""
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.int32)


def _differs(name, got, exp, out):
    """Bitwise comparison of two equally shaped arrays; a difference is described in `out`."""
    exp = np.ascontiguousarray(exp)
    got = np.ascontiguousarray(got).view(exp.dtype)      # (reported as what it is: a float, an index, a position)
    assert got.shape == exp.shape and exp.dtype.itemsize == 4, (name, got.shape, exp.shape)
    bad = np.argwhere(got.view(np.int32) != exp.view(np.int32))
    if len(bad):
        at = tuple(bad[0])
        out.append("%s: %d of %d differ, first at %s: got %r, restated %r" % (name, len(bad), got.size, list(map(int, at)),
                                                                              got[at].item(), exp[at].item()))


def _sort(t):
    from dh3d_amd import pm
    srt, gbox, cells = pm.spatial_sort_cells(t)
    return _bits(srt), _bits(gbox), _bits(cells)


@pytest.mark.parametrize("case", R.SORT_CASES, ids=R.case_id)
def test_sort_equals_the_restatement(dev, case):
    from dh3d_amd import pm
    n, kinds = case
    xyz = R.make_batch(case)
    t = torch.from_numpy(xyz).to(dev)
    srt, gbox, cells = _sort(t)
    plain = pm.spatial_sort(t)                   # without the table
    srt_p, gbox_p = _bits(plain[0]), _bits(plain[1])
    srt_2, gbox_2, cells_2 = _sort(t)            # again
    assert srt.shape == (len(kinds), n, 4) and gbox.shape == (len(kinds), (n + 63) // 64, 8) and cells.shape[1] == R.CELL_INTS
    report = []
    for b, kind in enumerate(kinds):
        r, out = R.restate(xyz[b]), []
        _differs("permutation", srt[b, :, 3], r["order"], out)
        _differs("record coordinates", srt[b, :, :3], r["records"], out)
        _differs("gbox", gbox[b], r["gbox"], out)
        _differs("cell table", cells[b, :4097], r["cells"][:4097], out)
        _differs("header origin / scale (slots 4100..4105)", cells[b, 4100:4106], r["cells"][4100:4106], out)
        _differs("crowded flag (slot 4106; restated %d occupied, threshold %d)" % (r["occupied"], r["threshold"]),
                 cells[b, 4106:4107], r["cells"][4106:4107], out)
        _differs("schedule (slot 4107; restated steps %s)" % "".join("xyz"[a] for a in R.step_axes(r["sched"])[:12]),
                 cells[b, 4107:4108], r["cells"][4107:4108], out)
        _differs("records of spatial_sort without the table", srt_p[b], srt[b], out)
        _differs("gbox of spatial_sort without the table", gbox_p[b], gbox[b], out)
        _differs("records of a second call", srt_2[b], srt[b], out)
        _differs("gbox of a second call", gbox_2[b], gbox[b], out)
        _differs("cells of a second call", cells_2[b, R.COMPARED_SLOTS], cells[b, R.COMPARED_SLOTS], out)
        report += ["cloud %d (%s, N = %d): %s" % (b, kind, n, o) for o in out]
    if report:
        raise AssertionError("the sort departs from its restatement:\n  " + "\n  ".join(report))


# ------------------------------------------------------------------------------------------------ consumers, far away
@pytest.mark.parametrize("case", R.FAR_CASES, ids=R.case_id)
def test_consumers_far_from_the_origin(dev, oracle, case):
    """A 40 m cube and a 60 x 60 x 6 slab at (+5000, -3000, +200): |coordinate| >> extent.  Everything built on the sort
    stays bit-equal to brute force there: knn_grid / knn_sorted (ids and distance bits, brute force itself against the
    oracle), fps_sorted, three_nn_sorted and the cell-list ball query."""
    from dh3d_amd import ops, pm
    import ball_query_reference as BR
    from test_ball_query_gpu import _check
    n, kinds = case
    xyz = R.make_batch(case)
    ref = [R.restate(p) for p in xyz]
    assert all(np.abs(p).max() > 50 * r["ext"].max() for p, r in zip(xyz, ref))
    t = torch.from_numpy(xyz).to(dev)
    srt, gbox, cells = pm.spatial_sort_cells(t)
    assert not cells[:, 4106].any().item(), "the uniform clouds must take the cell-list path"
    assert all(r["cells"][4106] == 0 for r in ref)
    # kNN
    nn_b, d_b = pm.knn_xyz(t, 8)
    nn_o, d_o = oracle.knn_bruteforce(np.ascontiguousarray(xyz.transpose(0, 2, 1)), 8)
    assert np.array_equal(nn_b.cpu().numpy(), nn_o), "knn_xyz ids vs the oracle"
    assert np.array_equal(_bits(d_b), d_o.view(np.int32)), "knn_xyz distance bits vs the oracle"
    for name, (nn, d) in (("knn_grid", pm.knn_grid(srt, gbox, cells, 8)), ("knn_sorted", pm.knn_sorted(srt, gbox, 8))):
        assert torch.equal(nn, nn_b), (name, "ids", int((nn != nn_b).sum()))
        assert torch.equal(d.view(torch.int32), d_b.view(torch.int32)), (name, "distance bits")
    # FPS
    idx = pm.fps_sorted(srt, gbox, R.FPS_M)
    assert torch.equal(idx, ops.farthest_point_sample(R.FPS_M, t)), "fps_sorted vs farthest_point_sample"
    idx_h = idx.cpu().numpy()
    assert np.array_equal(idx_h, oracle.farthest_point_sample(R.FPS_M, xyz)), "fps_sorted vs the oracle"
    # three_nn of the cloud against its FPS subset
    sub = np.take_along_axis(xyz, idx_h[:, :, None].astype(np.int64), 1)
    ts = torch.from_numpy(sub).to(dev)
    srt_s, gbox_s = pm.spatial_sort(ts)
    d3, i3 = pm.three_nn_sorted(srt, gbox, srt_s, gbox_s)
    d3_b, i3_b = ops.three_nn(t, ts)
    assert torch.equal(i3, i3_b) and torch.equal(d3.view(torch.int32), d3_b.view(torch.int32)), "three_nn_sorted vs three_nn"
    d3_o, i3_o = oracle.three_nn(xyz, sub)
    assert np.array_equal(i3.cpu().numpy(), i3_o) and np.array_equal(_bits(d3), d3_o.view(np.int32)), "three_nn vs the oracle"
    # ball query: radius = two cell widths (of the widest axis), the subset as queries, every second one moved off its point
    width = np.array([r["width"].max() for r in ref], np.float32)
    radii = np.ascontiguousarray(np.broadcast_to((np.float32(2) * width)[:, None], (len(kinds), R.FPS_M)), np.float32)
    rng = np.random.default_rng(n)
    qry = sub.copy()
    qry[:, 1::2] += (rng.uniform(-1, 1, (len(kinds), R.FPS_M // 2, 3)) * width[:, None, None]).astype(np.float32)
    ref_idx, ref_cnt = BR.query_ball_point(radii, 16, xyz, qry)
    assert ref_cnt.min() >= 1 and ref_cnt.max() == 16 and 0 < (ref_cnt == 16).mean()
    tq, tr = torch.from_numpy(qry).to(dev), torch.from_numpy(radii).to(dev)
    scan = pm.ball_query_scan(tr, 16, t, tq)
    grid = pm.ball_query_grid(tr, 16, t, tq, sort=(srt, gbox, cells))
    _check("%s scan vs restatement" % (case,), scan, ref_idx, ref_cnt)
    _check("%s grid vs restatement" % (case,), grid, ref_idx, ref_cnt)
    assert torch.equal(grid[0], scan[0]) and torch.equal(grid[1], scan[1]), "cell-list ball query vs the scan"
    _check("%s grid, sorted inside" % (case,), pm.ball_query_grid(tr, 16, t, tq), ref_idx, ref_cnt)
