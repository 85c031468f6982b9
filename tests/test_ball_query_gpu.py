"""GPU: query_ball_point / query_ball_point2 -- the scan kernel (pm.ball_query_scan), the cell-list kernel
(pm.ball_query_grid) and the op -- bit-equal (torch.equal on idx and pts_cnt, no tolerance anywhere) to the rows of the
reference's own CPU twin (golden/twins_ball.npz, every row it wrote) and to the float32 restatement
(tests/ball_query_reference.py, every row, empty balls included); on fresh clouds over the shapes, radii and cloud kinds the
kernels branch on; with per-query radii; as the producer of group_point's idx; across shardings and runs; and under graph
capture."""
import zlib

import numpy as np
import pytest
import torch

import ball_query_reference as R
from test_ops_gpu import _knn_clouds

pytestmark = pytest.mark.gpu

GOLDEN = R.golden_cases()
IDX_SENTINEL, CNT_SENTINEL = -7, -9


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _kernels(n):
    from dh3d_amd import ops, pm
    k = [("scan", pm.ball_query_scan), ("op", ops.query_ball_point)]
    if n <= 16384:
        k.append(("grid", pm.ball_query_grid))
    return k


def _check(name, got, exp_idx, exp_cnt, rows=None):
    idx, cnt = got
    assert idx.dtype == torch.int32 and cnt.dtype == torch.int32
    idx, cnt, ei, ec = idx.cpu(), cnt.cpu(), torch.from_numpy(exp_idx), torch.from_numpy(exp_cnt)
    if rows is not None:
        idx, cnt, ei, ec = idx[rows], cnt[rows], ei[rows], ec[rows]
    if not torch.equal(cnt, ec):
        bad = (cnt != ec).nonzero()
        raise AssertionError("%s: pts_cnt differs at %d places, first %s: %d vs %d" % (
            name, len(bad), bad[0].tolist(), int(cnt[tuple(bad[0])]), int(ec[tuple(bad[0])])))
    if not torch.equal(idx, ei):
        bad = (idx != ei).any(-1).nonzero()
        r = tuple(bad[0])
        raise AssertionError("%s: idx differs in %d rows, first %s:\n%s\nvs\n%s" % (name, len(bad), bad[0].tolist(),
                                                                                   idx[r].tolist(), ei[r].tolist()))


# ------------------------------------------------------------------------------------------------ the twin's rows
@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_twin_rows_and_restatement(dev, name):
    c = GOLDEN[name]
    x1, x2 = _t(c["xyz1"], dev), _t(c["xyz2"], dev)
    ref_idx, ref_cnt = R.query_ball_point(c["radius"], c["nsample"], c["xyz1"], c["xyz2"])
    written = torch.from_numpy(c["idx"][:, :, 0] >= 0)
    assert written.float().mean() >= 0.9
    for kname, fn in _kernels(c["xyz1"].shape[1]):
        got = fn(c["radius"], c["nsample"], x1, x2)
        # the twin wrote no count: its rows, and the count the restatement derives from the same walk
        _check("%s/%s vs twin" % (name, kname), got, c["idx"], ref_cnt, rows=written)
        _check("%s/%s vs restatement" % (name, kname), got, ref_idx, ref_cnt)


# ------------------------------------------------------------------------------------------------ fresh clouds
NS = (1, 63, 64, 65, 1000, 4096, 8192, 16384)
KS = (1, 8, 32, 64, 128)
RADII = ("none", 0.02, 0.08, 0.2, 0.6, "all")   # as a fraction of the cloud's largest extent
KINDS = ("uniform", "scene", "clusters", "duplicates", "lattice", "oxford_extent", "plane", "outliers", "one_point")


def _shape_cases():
    cases, i = [], 0
    for n in NS:
        for m in sorted({1, 64, 1000, n}):
            cases.append((KINDS[i % len(KINDS)] if n >= 1000 else "uniform", 1 if n * m > 1 << 26 else 2, n, m,
                          KS[i % len(KS)], RADII[(i // 2) % len(RADII)]))
            i += 1
    # every nsample and every radius regime on the two sizes the benchmark runs, both cloud families
    for j, (k, r) in enumerate([(k, r) for k in KS for r in RADII]):
        cases.append((("uniform", "scene", "clusters")[j % 3], 2, (4096, 8192)[j % 2], (64, 1000)[(j // 2) % 2], k, r))
    return cases


SHAPE_CASES = _shape_cases()


def test_shape_cases_cover_what_they_claim():
    assert {c[2] for c in SHAPE_CASES} == set(NS) and {c[4] for c in SHAPE_CASES} == set(KS)
    assert {c[5] for c in SHAPE_CASES} == set(RADII)
    for n in NS:
        assert {c[3] for c in SHAPE_CASES if c[2] == n} >= {1, 64, 1000, n}
    assert {c[0] for c in SHAPE_CASES} >= {"uniform", "scene", "clusters", "duplicates", "lattice", "one_point"}


def _make(kind, b, n, m, key):
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    x1 = np.ascontiguousarray(_knn_clouds(kind, b, n, rng), np.float32)
    ext = float((x1.max(1) - x1.min(1)).max())
    ext = ext if ext > 0 else 1.0
    if m == n:
        x2 = x1.copy()                                   # the cloud queries itself
    else:                                                # half the queries are cloud points, half lie around them
        pick = rng.integers(0, n, (b, m))
        x2 = np.take_along_axis(x1, pick[..., None], 1)
        x2[:, m // 2:] += rng.normal(0, 0.05 * ext, (b, m - m // 2, 3)).astype(np.float32)
    return x1, np.ascontiguousarray(x2, np.float32), ext


def _radius(spec, ext):
    return 1e-21 if spec == "none" else 4.0 * ext if spec == "all" else float(np.float32(spec * ext))


@pytest.mark.parametrize("case", SHAPE_CASES, ids=lambda c: "%s-b%d-n%d-m%d-k%d-r%s" % c)
def test_kernels_equal_restatement_on_fresh_clouds(dev, case):
    kind, b, n, m, k, rspec = case
    x1, x2, ext = _make(kind, b, n, m, case)
    radius = _radius(rspec, ext)
    ref_idx, ref_cnt = R.query_ball_point(radius, k, x1, x2)
    if rspec == "none":
        assert not ref_cnt.any()
    if rspec == "all":
        assert np.all(ref_cnt == min(k, n)) and np.array_equal(ref_idx[0, 0, :min(k, n)], np.arange(min(k, n)))
    t1, t2 = _t(x1, dev), _t(x2, dev)
    outs = {}
    for kname, fn in _kernels(n):
        outs[kname] = fn(radius, k, t1, t2)
        _check("%s %s" % (case, kname), outs[kname], ref_idx, ref_cnt)
    if "grid" in outs:
        assert torch.equal(outs["grid"][0], outs["scan"][0]) and torch.equal(outs["grid"][1], outs["scan"][1])
    if kind == "oxford_extent" and "grid" in outs:
        # the table of a slab is no cube's and not crowded.  (These cases do not reach the cell walk with anything to find:
        # one query with an empty ball, and a ball over the whole cloud -- test_cell_walk_on_a_grid_that_is_no_cube does.)
        from dh3d_amd import pm
        sort = pm.spatial_sort_cells(t1)
        assert bool((sort[2][:, 4107] != 0x186186).all()) and bool((sort[2][:, 4106] == 0).all())
        _check("%s grid, this table" % (case,), pm.ball_query_grid(radius, k, t1, t2, sort=sort), ref_idx, ref_cnt)


def test_cell_walk_on_a_grid_that_is_no_cube(dev):
    """The cell walk (flag 0, a box of at most 512 cells) on a 60 x 60 x 8 m slab: its schedule deals 5 + 5 + 2 bits, where a
    cube's 4 + 4 + 4 hides a wrong axis, bit position or slot in the decode.  A ball of 1.5 m meets at most 3 x 3 x 3 of the
    1.875 x 1.875 x 2 m cells.  Half the queries are points of the cloud (each finds itself at least), half lie uniformly
    inside the slab: at 2048 / 28800 points per m^3 a 14.1 m^3 ball holds one point on average, so a walk that reads the
    wrong cells loses hits that the restatement and the scan kernel have."""
    from dh3d_amd import pm
    b, n, m, k, r = 2, 2048, 64, 16, 1.5
    rng = np.random.default_rng(6082)
    x1 = np.ascontiguousarray(_knn_clouds("oxford_extent", b, n, rng), np.float32)
    x2 = np.stack([x1[i, rng.permutation(n)[:m]] for i in range(b)])
    x2[:, m // 2:] = _knn_clouds("oxford_extent", b, m - m // 2, rng)
    x2 = np.ascontiguousarray(x2, np.float32)
    ref_idx, ref_cnt = R.query_ball_point(r, k, x1, x2)
    assert (ref_cnt[:, :m // 2] > 0).all() and (ref_cnt > 0).mean() > 0.7 and (ref_cnt > 1).mean() > 0.3
    assert ref_cnt.max() < k                                  # no ball is cut short: every hit of every cell is in the row
    t1, t2 = _t(x1, dev), _t(x2, dev)
    sort = pm.spatial_sort_cells(t1)
    assert bool((sort[2][:, 4107] != 0x186186).all()) and bool((sort[2][:, 4106] == 0).all())
    scan = pm.ball_query_scan(r, k, t1, t2)
    _check("slab scan", scan, ref_idx, ref_cnt)
    for name, grid in (("slab grid, this table", pm.ball_query_grid(r, k, t1, t2, sort=sort)),
                       ("slab grid", pm.ball_query_grid(r, k, t1, t2))):
        _check(name, grid, ref_idx, ref_cnt)
        assert torch.equal(grid[0], scan[0]) and torch.equal(grid[1], scan[1])


def test_batch_of_eight_extents_crowded_and_coincident(dev):
    from dh3d_amd import pm
    rng = np.random.default_rng(77)
    kinds = ("scene", "uniform", "clusters", "one_point", "scene", "duplicates", "uniform", "outliers")
    n, m, k = 4096, 512, 32
    scale = np.array([1, 40, 0.01, 3, 100, 1, 0.5, 1], np.float32)[:, None, None]
    x1 = np.concatenate([_knn_clouds(kd, 1, n, rng) for kd in kinds]) * scale
    x1 = np.ascontiguousarray(x1 + rng.uniform(-5, 5, (8, 1, 3)).astype(np.float32) * scale, np.float32)
    x2 = np.ascontiguousarray(x1[:, rng.permutation(n)[:m]] + (rng.normal(0, 0.01, (8, m, 3)) * scale).astype(np.float32))
    x2[:, ::2] = x1[:, :m:2]
    ext = (x1.max(1) - x1.min(1)).max(1)
    ext[ext == 0] = 1.0
    radii = np.ascontiguousarray(np.broadcast_to((0.1 * ext)[:, None], (8, m)), np.float32)
    t1, t2, tr = _t(x1, dev), _t(x2, dev), _t(radii, dev)
    sort = pm.spatial_sort_cells(t1)
    crowded = (sort[2][:, 4106] != 0).cpu().tolist()
    assert any(crowded) and not all(crowded), crowded     # both ways through the cell-list kernel in one launch
    ref_idx, ref_cnt = R.query_ball_point(radii, k, x1, x2)
    assert 0 < (ref_cnt == k).mean() < 1
    _check("b8 scan", pm.ball_query_scan(tr, k, t1, t2), ref_idx, ref_cnt)
    _check("b8 grid", pm.ball_query_grid(tr, k, t1, t2), ref_idx, ref_cnt)
    _check("b8 grid, caller's sort", pm.ball_query_grid(tr, k, t1, t2, sort=sort), ref_idx, ref_cnt)
    # across shardings and from run to run: a cloud's rows do not depend on its batch
    from dh3d_amd import ops
    whole = ops.query_ball_point2(tr, k, t1, t2)
    _check("b8 op", whole, ref_idx, ref_cnt)
    again = ops.query_ball_point2(tr, k, t1, t2)
    assert torch.equal(whole[0], again[0]) and torch.equal(whole[1], again[1])
    for i in range(8):
        for fn in (ops.query_ball_point2, pm.ball_query_scan, pm.ball_query_grid):
            one = fn(tr[i:i + 1].contiguous(), k, t1[i:i + 1].contiguous(), t2[i:i + 1].contiguous())
            assert torch.equal(one[0][0], whole[0][i]) and torch.equal(one[1][0], whole[1][i]), (i, fn.__name__)
        if ext[i] > 0 and kinds[i] != "one_point":
            one = ops.query_ball_point(float(radii[i, 0]), k, t1[i:i + 1].contiguous(), t2[i:i + 1].contiguous())
            assert torch.equal(one[0][0], whole[0][i]) and torch.equal(one[1][0], whole[1][i]), i


def test_scan_kernel_beyond_the_sort(dev):
    from dh3d_amd import ops, pm
    case = ("uniform", 2, 20000, 300, 32, 0.08)
    x1, x2, ext = _make(*case[:4], case)
    ref = R.query_ball_point(_radius(0.08, ext), 32, x1, x2)
    assert 0 < (ref[1] == 32).mean() < 1
    _check("n=20000 scan", pm.ball_query_scan(_radius(0.08, ext), 32, _t(x1, dev), _t(x2, dev)), *ref)
    _check("n=20000 op", ops.query_ball_point(_radius(0.08, ext), 32, _t(x1, dev), _t(x2, dev)), *ref)
    with pytest.raises(ValueError):
        pm.ball_query_grid(0.1, 32, _t(x1, dev), _t(x2, dev))


@pytest.mark.parametrize("kind,n", [("uniform", 8192), ("scene", 4096), ("uniform", 500)])
def test_query_ball_point2_radii_over_two_decades(dev, kind, n):
    from dh3d_amd import ops, pm
    b, m, k = 3, 700, 24
    x1, x2, ext = _make(kind, b, n, m, ("qbp2", kind, n))
    rng = np.random.default_rng(n)
    radii = (ext * 10.0 ** rng.uniform(-2.3, -0.3, (b, m))).astype(np.float32)
    radii[:, ::9] = 0.0
    radii[:, 4::9] = -0.5
    radii[:, 7::27] = np.nan
    radii[:, 8::27] = np.inf
    ref_idx, ref_cnt = R.query_ball_point(radii, k, x1, x2)
    dead = ~(radii > 0)
    assert not ref_cnt[dead].any() and (ref_cnt == k).any() and ((ref_cnt > 0) & (ref_cnt < k)).any()
    t1, t2, tr = _t(x1, dev), _t(x2, dev), _t(radii, dev)
    _check("qbp2 op", ops.query_ball_point2(tr, k, t1, t2), ref_idx, ref_cnt)
    _check("qbp2 scan", pm.ball_query_scan(tr, k, t1, t2), ref_idx, ref_cnt)
    _check("qbp2 grid", pm.ball_query_grid(tr, k, t1, t2), ref_idx, ref_cnt)


def test_group_point_consumes_the_rows(dev):
    from dh3d_amd import ops
    c = GOLDEN["cube_offcloud_r025_k24"]      # has empty balls: their rows must be valid indices too
    x1, x2 = _t(c["xyz1"], dev), _t(c["xyz2"], dev)
    feats = torch.from_numpy(np.random.default_rng(3).standard_normal((1, c["xyz1"].shape[1], 5)).astype(np.float32)).to(dev)
    points = torch.cat([x1, feats], -1).contiguous()
    idx, cnt = ops.query_ball_point(c["radius"], c["nsample"], x1, x2)
    assert bool((cnt == 0).any()) and int(idx.min()) >= 0 and int(idx.max()) < c["xyz1"].shape[1]
    out = ops.group_point(points, idx)
    ref_idx, _ = R.query_ball_point(c["radius"], c["nsample"], c["xyz1"], c["xyz2"])
    expect = points.cpu().numpy()[0][ref_idx[0]][None]             # group_point_cpu: out[j, l] = points[idx[j, l]]
    assert torch.equal(out.cpu(), torch.from_numpy(expect))
    written = c["idx"][0, :, 0] >= 0
    twin_group = points.cpu().numpy()[0][c["idx"][0][written]]       # ... on the twin's own rows
    assert np.array_equal(out.cpu().numpy()[0][written], twin_group)


@pytest.mark.parametrize("n,per_query", [(8192, False), (8192, True), (1000, False)])
def test_graph_capture_and_replay_equal_eager(dev, n, per_query):
    from dh3d_amd import ops
    b, m, k = 2, 512, 16
    xa1, xa2, ext = _make("uniform", b, n, m, ("graph-a", n))
    xb1, xb2, _ = _make("uniform", b, n, m, ("graph-b", n))
    ra = np.full((b, m), 0.1 * ext, np.float32)
    s1, s2, sr = _t(xa1, dev), _t(xa2, dev), _t(ra, dev)

    def run():
        return ops.query_ball_point2(sr, k, s1, s2) if per_query else ops.query_ball_point(float(ra[0, 0]), k, s1, s2)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        g_idx, g_cnt = run()
    for x1, x2 in ((xb1, xb2), (xa1, xa2)):
        s1.copy_(_t(x1, dev)); s2.copy_(_t(x2, dev))
        g_idx.fill_(IDX_SENTINEL); g_cnt.fill_(CNT_SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        e_idx, e_cnt = run()
        assert torch.equal(g_idx, e_idx) and torch.equal(g_cnt, e_cnt)
        _check("graph n=%d" % n, (g_idx, g_cnt), *R.query_ball_point(float(ra[0, 0]), k, x1, x2))
