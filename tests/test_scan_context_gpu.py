"""GPU: Scan Context (dh3d_amd.scancontext -> csrc/scan_context.hip) against the numpy restatement
(tests/scan_context_reference.py): the image and the ring key bit for bit -- counts, poisoned rows, several workgroups per
cloud, every boundary of the bin rules, the grid limits, column views, real clouds --, the shifted distance to 1e-12 with
its invalid ids, order and the image of zeros, the whole search / relocalisation chain on rotated scenes, and search under
graph capture while the map grows."""
import os

import numpy as np
import pytest
import torch

import scan_context_reference as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
RADIUS = 20.0


def _gpu_build(dev, pts, num_valid=None, center=None, **grid):
    from dh3d_amd import scancontext
    t = pts if isinstance(pts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
    nv = None if num_valid is None else torch.tensor(list(num_valid), dtype=torch.int32, device=dev)
    ctr = None if center is None else torch.from_numpy(np.asarray(center, np.float32)).to(dev)
    out = scancontext.scan_context(t, nv, ctr, **grid)
    return out["desc"].cpu().numpy(), out["ring_key"].cpu().numpy()


def _assert_build(dev, pts, num_valid=None, center=None, what="", gpu_pts=None, **grid):
    desc, key = _gpu_build(dev, pts if gpu_pts is None else gpu_pts, num_valid, center, **grid)
    exp_desc, exp_key = R.scan_context(pts, num_valid, center, **grid)
    assert desc.shape == exp_desc.shape and desc.dtype == np.float32 and key.shape == exp_key.shape and key.dtype == np.float32
    bad = np.argwhere(desc.view(np.uint32) != exp_desc.view(np.uint32))
    assert bad.shape[0] == 0, (what, bad.shape[0], bad[:5].tolist())
    assert np.array_equal(key.view(np.uint32), exp_key.view(np.uint32)), what
    return exp_desc


def test_build_counts_and_poisoned_rows(dev):
    """P = 4, N = 1000 with num_valid (0, 1, 777, 1000): the rows past a count hold points that would top every bin."""
    counts = (0, 1, 777, 1000)
    pts = np.stack([R.scene(20 + p)[:1000] for p in range(4)])
    for p, n in enumerate(counts):
        pts[p, n:, 2] = 1000.0
    desc = _assert_build(dev, pts, counts, num_rings=20, num_sectors=60, max_radius=RADIUS, z_offset=2.0)
    assert not desc[0].any() and int((desc[1] > 0).sum()) == 1 and desc.max() < 100.0
    over = _assert_build(dev, pts, (-5, 2000, 777, 1001), num_rings=20, num_sectors=60, max_radius=RADIUS, z_offset=2.0)
    assert over[1].max() == 1002.0                                          # the count is clamped to [0, N]


def test_build_several_workgroups_per_cloud(dev):
    """P = 2, N = 70001 with counts (70001, 33): many workgroups fold into one image; the second cloud's stay idle."""
    rng = np.random.default_rng(3)
    pts = (rng.standard_normal((2, 70001, 3)) * [8, 8, 1.5]).astype(np.float32)
    desc = _assert_build(dev, pts, (70001, 33), num_rings=20, num_sectors=60, max_radius=RADIUS, z_offset=2.0)
    assert (desc[0] > 0).mean() > 0.9 and 0 < (desc[1] > 0).sum() <= 33
    _assert_build(dev, pts, None, num_rings=20, num_sectors=60, max_radius=RADIUS, z_offset=2.0)


def test_build_on_every_edge_of_the_bin_rules(dev):
    """The boundary cloud of the CPU test, three times over (duplicates), and 500 points in one bin."""
    edge, counts, ring, sector = R.boundary_cloud(RADIUS)
    rng = np.random.default_rng(4)
    crowd = np.stack([5.5 + 0.3 * rng.random(500), 0.2 + 0.1 * rng.random(500), rng.standard_normal(500)], 1).astype(np.float32)
    pts = np.concatenate([edge, crowd, edge, edge[::-1]], 0)[None]
    desc = _assert_build(dev, pts, None, num_rings=20, num_sectors=60, max_radius=RADIUS, z_offset=2.0)
    assert desc[0, 5, 8] == 3.0 and desc[0, 0, 59] == 3.0 and desc[0, 5, 0] == np.float32(crowd[:, 2].max() + np.float32(2.0))
    for r, s, c in zip(ring, sector, counts):
        assert not c or desc[0, r, s] > 0, (r, s)


@pytest.mark.parametrize("grid", [(4, 8), (32, 128), (12, 36)])
def test_build_at_the_grid_limits(dev, grid):
    pts = np.stack([R.scene(40 + p) for p in range(3)])
    _assert_build(dev, pts, (4000, 2500, 4000), num_rings=grid[0], num_sectors=grid[1], max_radius=17.5, z_offset=2.5)


def test_build_reads_a_column_view_in_place_with_a_center(dev):
    rng = np.random.default_rng(5)
    rows = (rng.standard_normal((3, 2111, 6)) * [50, 7, 7, 1.5, 50, 50]).astype(np.float32)
    center = (rng.standard_normal((3, 2)) * 3).astype(np.float32)
    full = torch.from_numpy(rows).to(dev)
    view = full[:, :, 1:4]
    assert view.stride() == (2111 * 6, 6, 1) and view.data_ptr() != full.data_ptr()
    _assert_build(dev, rows[:, :, 1:4], (2111, 2000, 7), center, gpu_pts=view, num_rings=20, num_sectors=60, max_radius=15.0,
                  z_offset=2.0)
    _assert_build(dev, rows[:, :, :3], None, center, gpu_pts=full, num_rings=20, num_sectors=60, max_radius=80.0, z_offset=2.0)


def test_build_on_the_demo_clouds(dev):
    demo = np.load(os.path.join(HERE, "golden", "demo_clouds.npz"))
    for name in ("local_268", "local_642", "dso_9000", "global_a", "global_b", "global_c"):
        pts = demo[name][None]
        desc = _assert_build(dev, pts, None, what=name, num_rings=20, num_sectors=60, max_radius=30.0, z_offset=2.0)
        assert (desc > 0).sum() >= 40, name              # (the 4096-point clouds reach 12 m: few rings of a 30 m image)
        _assert_build(dev, pts, None, what=name, num_rings=20, num_sectors=60, max_radius=80.0, z_offset=2.0)


@pytest.mark.parametrize("grid", [(20, 60, 48, 8, 24), (4, 8, 3, 64, 6), (32, 128, 3, 64, 6)])
def test_distance(dev, grid):
    """dist within 1e-12 of the restatement (values in [0, 2] from sums of at most 128 unit-size terms: rounding differences
    of order 1e-14, 100 x that for another summation order); shift equal wherever the restatement's best shift wins by more
    than 1e-9, at most 2 % of the pairs skipped (tests/test_scan_context_reference.py holds the restatement to that);
    invalid ids +inf / -1; order exactly the (dist, id, slot) order of the call's own dist."""
    from dh3d_amd import scancontext
    nr, ns, Q, C, n_scenes = grid
    qry, mp, cand, count = R.distance_fixture(nr, ns, Q, C, n_scenes)
    exp_dist, exp_shift, gap = R.distance(qry, mp, cand, count)
    poisoned = mp.copy()
    poisoned[count:] = np.nan                                                # rows past the count are never read
    tq, tm, tc = (torch.from_numpy(a).to(dev) for a in (qry, poisoned, cand))
    tcount = torch.tensor([count], dtype=torch.int32, device=dev)
    dist, shift, order = (t.cpu().numpy() for t in scancontext.scan_context_distance(tq, tm, tc, tcount))
    assert dist.dtype == np.float64 and shift.dtype == np.int32 and order.dtype == np.int32
    valid = (cand >= 0) & (cand < count)
    assert np.isinf(dist[~valid]).all() and (dist[~valid] > 0).all() and (shift[~valid] == -1).all()
    err = np.abs(dist[valid] - exp_dist[valid]).max()
    print("scan_context_distance %s: max |dist - reference| = %.3e over %d pairs" % (grid, err, int(valid.sum())))
    assert err <= 1e-12, err
    sure = valid & (gap > 1e-9)
    assert (valid & ~sure).sum() <= 0.02 * Q * C
    assert np.array_equal(shift[sure], exp_shift[sure])
    assert ((shift[valid] >= 0) & (shift[valid] < ns)).all()
    assert np.array_equal(order, R.order_of(dist, cand))
    assert dist[Q - 1, 0] == 1.0 and shift[Q - 1, 0] == 0                    # zeros against zeros: exactly (1.0, 0)
    assert (dist[Q - 1][valid[Q - 1]] == 1.0).all() and (shift[Q - 1][valid[Q - 1]] == 0).all()
    # without a count the whole buffer is the map; a row does not depend on the other queries
    d2, s2, o2 = (t.cpu().numpy() for t in scancontext.scan_context_distance(tq[1:2], torch.from_numpy(mp).to(dev), tc[1:2]))
    e2, es2, g2 = R.distance(qry[1:2], mp, cand[1:2], None)
    ok = np.isfinite(e2)
    assert np.array_equal(np.isfinite(d2), ok) and np.abs(d2[ok] - e2[ok]).max() <= 1e-12
    assert np.array_equal(s2[g2 > 1e-9], es2[g2 > 1e-9]) and np.array_equal(o2, R.order_of(d2, cand[1:2]))
    same = valid[1] & (cand[1] < count)
    assert np.array_equal(d2[0][same], dist[1][same])


@pytest.fixture(scope="module")
def chain(dev):
    """16 scenes in a ScanContextIndex(capacity=32, points=4000); the queries are the scenes turned by 0 / 90 / 180 / 270
    degrees exactly, their points shuffled."""
    from dh3d_amd import scancontext
    scenes = np.stack([R.scene(60 + s) for s in range(16)])
    rng = np.random.default_rng(6)
    quarters = np.arange(16) % 4
    queries = np.stack([rng.permutation(R.rotate_quarter(scenes[s], int(quarters[s]))) for s in range(16)])
    index = scancontext.ScanContextIndex(capacity=32, points=4000, max_radius=RADIUS, device=dev)
    ids = index.add(torch.from_numpy(scenes[:10]).to(dev))
    ids2 = index.add(torch.from_numpy(scenes[10:]).to(dev), pos=torch.arange(12, dtype=torch.float64).view(6, 2))
    assert list(ids) == list(range(10)) and list(ids2) == list(range(10, 16)) and len(index) == 16
    map_desc, map_keys = R.scan_context(scenes, None, None, 20, 60, RADIUS, 2.0)
    qry_desc, qry_keys = R.scan_context(queries, None, None, 20, 60, RADIUS, 2.0)
    return dict(index=index, scenes=scenes, queries=queries, tq=torch.from_numpy(queries).to(dev), quarters=quarters,
                map_desc=map_desc, map_keys=map_keys, qry_desc=qry_desc, qry_keys=qry_keys)


def test_chain_finds_every_place_and_its_yaw(dev, chain):
    index = chain["index"]
    assert np.array_equal(index.desc[:16].cpu().numpy().view(np.uint32), chain["map_desc"].view(np.uint32))
    assert np.array_equal(index.places.desc[:16].cpu().numpy().view(np.uint32), chain["map_keys"].view(np.uint32))
    assert int(index.places.count.item()) == 16 and not index.desc[16:].any()
    assert np.array_equal(index.places.cloud[:16].cpu().numpy(), chain["scenes"])
    res = {k: v.cpu().numpy() for k, v in index.search(chain["tq"], k=3, candidates=10).items()}
    assert sorted(res) == ["dist", "place", "shift", "yaw"] and all(v.shape == (16, 3) for v in res.values())
    assert res["place"].dtype == np.int32 and res["shift"].dtype == np.int32 and res["yaw"].dtype == np.float64
    # the map cloud is Rz(-quarters * 90 deg) applied to the query cloud
    want_shift = ((4 - chain["quarters"]) % 4) * 15
    assert np.array_equal(res["place"][:, 0], np.arange(16)) and (res["dist"][:, 0] <= 1e-12).all()
    assert np.array_equal(res["shift"][:, 0], want_shift)
    place, dist, shift, yaw, gap = R.search(chain["map_desc"], chain["map_keys"], 16, chain["qry_desc"], chain["qry_keys"], 3, 10)
    assert np.array_equal(res["place"], place) and np.abs(res["dist"] - dist).max() <= 1e-12
    assert np.array_equal(res["shift"][gap > 1e-9], shift[gap > 1e-9]) and (gap[:, 0] > 0.05).all()
    assert np.array_equal(res["yaw"], res["shift"].astype(np.float64) * (2.0 * np.pi) / 60)
    # more candidates than places: -1 / +inf / -1 / NaN past the map's end
    res = {k: v.cpu().numpy() for k, v in index.search(chain["tq"][:3], k=20, candidates=20).items()}
    assert (res["place"][:, :16] >= 0).all() and (np.sort(res["place"][:, :16], 1) == np.arange(16)).all()
    assert (res["place"][:, 16:] == -1).all() and np.isinf(res["dist"][:, 16:]).all() and (res["shift"][:, 16:] == -1).all()
    assert np.isnan(res["yaw"][:, 16:]).all() and np.isfinite(res["yaw"][:, :16]).all()
    assert (np.diff(res["dist"][:, :16], axis=1) >= 0).all()
    with pytest.raises(ValueError):
        index.search(chain["tq"], k=11, candidates=10)
    with pytest.raises(ValueError):
        index.add(torch.from_numpy(chain["scenes"]).to(dev).repeat(2, 1, 1)[:17])       # 16 + 17 > 32


def test_relocalize_pose_and_refinement(dev, chain):
    from dh3d_amd import registration, scancontext
    index, tq = chain["index"], chain["tq"]
    res = scancontext.relocalize_scan_context(index, tq, k=2, candidates=10)
    assert res["Rt"].shape == (16, 3, 4) and res["Rt"].dtype == torch.float64 and res["valid"].all()
    yaw, Rt = res["yaw"][:, 0].cpu().numpy(), res["Rt"].cpu().numpy()
    want = np.zeros((16, 3, 4))
    want[:, 0, 0], want[:, 0, 1], want[:, 1, 0], want[:, 1, 1], want[:, 2, 2] = np.cos(yaw), -np.sin(yaw), np.sin(yaw), np.cos(yaw), 1
    assert np.abs(Rt - want).max() <= 1e-15                                  # no centres: t = 0
    ref = scancontext.relocalize_scan_context(index, tq, k=2, candidates=10, refine=True)
    assert torch.equal(ref["Rt_scan"], res["Rt"]) and torch.equal(ref["place"], res["place"])
    place = ref["place"][:, 0].long()
    direct = registration.refine_pose(index.places.cloud.index_select(0, place), tq, ref["Rt_scan"], ref["valid"],
                                      anchor_count=index.places.cloud_count.index_select(0, place), positive_count=None)
    for key in ("Rt", "fitness", "rmse"):
        assert torch.equal(ref[key], direct[key]), key
    assert (ref["fitness"] > 0.999).all() and (ref["rmse"] < 1e-3).all()
    assert (ref["Rt"] - ref["Rt_scan"]).abs().max() < 1e-3
    with pytest.raises(ValueError, match="points > 0"):
        scancontext.relocalize_scan_context(scancontext.ScanContextIndex(4, max_radius=RADIUS, device=dev), tq, refine=True)


def test_relocalize_with_centres(dev):
    """Clouds given in two different frames with their centres: Rt = [Rz(yaw) | c_place - Rz(yaw) c_query] takes the query's
    points onto the place's."""
    from dh3d_amd import scancontext
    scenes = np.stack([R.scene(80 + s) for s in range(4)]).astype(np.float64)
    cm = np.array([[100.0, -40.0], [3.5, 7.25], [-60.0, 12.0], [0.0, 0.0]])
    cq = np.array([[-8.0, 16.0], [200.0, 100.0], [1.0, -1.0], [5.0, 5.0]])
    turned = np.stack([R.rotate_quarter(scenes[s].astype(np.float32), s).astype(np.float64) for s in range(4)])
    place_pts, query_pts = scenes.copy(), turned.copy()
    place_pts[:, :, :2] += cm[:, None]
    query_pts[:, :, :2] += cq[:, None]
    index = scancontext.ScanContextIndex(capacity=4, max_radius=RADIUS, device=dev)
    index.add(torch.from_numpy(place_pts.astype(np.float32)).to(dev), center=torch.from_numpy(cm.astype(np.float32)).to(dev))
    res = scancontext.relocalize_scan_context(index, torch.from_numpy(query_pts.astype(np.float32)).to(dev),
                                              center=torch.from_numpy(cq.astype(np.float32)).to(dev), k=1, candidates=4)
    assert res["place"][:, 0].tolist() == [0, 1, 2, 3] and res["shift"][:, 0].tolist() == [0, 45, 30, 15]
    Rt, yaw = res["Rt"].cpu().numpy(), res["yaw"][:, 0].cpu().numpy()
    for s in range(4):
        rz = np.array([[np.cos(yaw[s]), -np.sin(yaw[s]), 0], [np.sin(yaw[s]), np.cos(yaw[s]), 0], [0, 0, 1]])
        assert np.abs(Rt[s, :, :3] - rz).max() <= 1e-15
        t = np.append(cm[s] - rz[:2, :2] @ cq[s], 0.0)
        assert np.abs(Rt[s, :, 3] - t).max() <= 1e-12
        moved = query_pts[s] @ Rt[s, :, :3].T + Rt[s, :, 3]
        assert np.abs(moved - place_pts[s]).max() < 1e-9


def test_search_under_graph_capture_while_the_map_grows(dev, chain):
    from dh3d_amd import scancontext
    scenes = torch.from_numpy(chain["scenes"]).to(dev)
    index = scancontext.ScanContextIndex(capacity=16, max_radius=RADIUS, device=dev)
    index.add(scenes[:8])
    static_q = chain["tq"][8:16].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        index.search(static_q, k=2, candidates=6)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gout = index.search(static_q, k=2, candidates=6)
    g.replay()
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in gout.items()}
    assert (before["place"] < 8).all() and (before["place"] >= 0).all() and (before["dist"][:, 0] > 1e-3).all()
    index.add(scenes[8:])
    g.replay()
    torch.cuda.synchronize()
    assert gout["place"][:, 0].tolist() == list(range(8, 16)) and (gout["dist"][:, 0] <= 1e-12).all()
    eager = index.search(static_q, k=2, candidates=6)
    for key in ("place", "dist", "shift"):
        assert torch.equal(gout[key], eager[key]), key
    assert torch.equal(gout["yaw"].nan_to_num(-9.0), eager["yaw"].nan_to_num(-9.0))
    static_q.copy_(chain["tq"][:8])                                          # new queries through the same graph
    g.replay()
    torch.cuda.synchronize()
    assert gout["place"][:, 0].tolist() == list(range(8))
