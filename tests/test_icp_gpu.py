"""GPU: dense ICP refinement (dh3d_amd.registration.refine_icp -> csrc/icp.hip) against the numpy restatement of the rule
(tests/icp_reference.py): equal ids, counts and validity, poses within 1e-9; the scan and the cell-list association bit for
bit on every kind of cloud that sends the cell lists another way; batch independence over a garbage workspace; graph
capture; and the plumbing through register_clouds and PlaceIndex.localize."""
import math
import os

import numpy as np
import pytest
import torch

import icp_reference as ir
from icp_fixtures import _assert_same, _bits_equal, place_scene

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N = 2048
ITERS = (0, 1, 2, 5, 30)
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)


def _edge_pairs(seed):
    """The pairs at the rule's corners, as (name, anchor, positive, Rt0, na, nb, valid0) over slices of a demo pair."""
    a, y, Rt_gt, Rt0 = ir.demo_pair("local_642", N, seed)
    near = ir.move(Rt_gt, y).astype(np.float32)              # the positive's points in the anchor's frame: true partners
    nan = Rt0.copy()
    nan[2, 1] = np.nan
    return [
        ("no anchor", a, y, Rt0, 0, 300, True),
        ("no positive", a, y, Rt0, 300, 0, True),
        ("one point", near, y, Rt_gt, 1, 1, True),
        ("two points", near, y, Rt_gt, 2, 2, True),
        ("three points", near, y, Rt_gt, 3, 3, True),
        ("all beyond max_dist", a, y + np.float32(500.0), Rt0, 400, 300, True),
        ("a cloud against itself", a, a, EYE, 500, 500, True),
        ("NaN start pose", a, y, nan, 300, 300, True),
        ("valid0 = 0", a, y, Rt0, 300, 300, False),
        ("counts off the tile", a, y, Rt0, 777, 1001, True),
    ]


def _clear_edges(max_dist):
    """_edge_pairs of the first seed whose every run keeps the margins of icp_reference.clear_pair."""
    for seed in range(1, 51):
        pairs = _edge_pairs(seed)
        runs = [ir.icp(a, y, Rt0, max_dist=max_dist, iterations=max(ITERS), na=na, nb=nb, valid0=v)
                for _, a, y, Rt0, na, nb, v in pairs]
        if all(r["gap"] > 1e-8 and r["thr"] > 1e-8 and r["eig"] > 1e-6 for r in runs):
            return pairs, runs
    raise AssertionError("no clear edge fixture")


def _build(max_dist):
    """One [P, 2048, 2048] batch: the three demo subsets, then the edge pairs; and the restatement's run of every pair."""
    A, Y, R0, na, nb, v0, runs, names = [], [], [], [], [], [], [], []
    for name, n in (("local_642", N), ("global_c", N), ("dso_9000", 1024)):
        (a, y, _, Rt0), run, _ = ir.clear_pair(name, n, max_dist, max(ITERS))
        # (dso_9000: 1024 points and a count; the rows behind it are points of the cloud that must never be chosen)
        pad = ir.demo_pair(name, N, 99)
        A.append(np.concatenate([a, pad[0][n:]])); Y.append(np.concatenate([y, pad[1][n:]]))
        R0.append(Rt0); na.append(n); nb.append(n); v0.append(1); runs.append(run); names.append(name)
    pairs, eruns = _clear_edges(max_dist)
    for (name, a, y, Rt0, ca, cb, v), run in zip(pairs, eruns):
        A.append(a); Y.append(y); R0.append(Rt0); na.append(ca); nb.append(cb); v0.append(int(v)); runs.append(run)
        names.append(name)
    return dict(A=np.stack(A), Y=np.stack(Y), Rt0=np.stack(R0), na=np.array(na, np.int32), nb=np.array(nb, np.int32),
                v0=np.array(v0, np.int32), runs=runs, names=names, max_dist=max_dist)


@pytest.fixture(scope="module")
def batches():
    return {md: _build(md) for md in (1.0, 2.0)}


def _run(dev, b, iterations, path=0, sel=None):
    from dh3d_amd import registration as reg
    s = slice(None) if sel is None else sel
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v[s])).to(dev)
    return reg.refine_icp(t(b["A"]), t(b["Y"]), t(b["Rt0"]), t(b["v0"]), t(b["na"]), t(b["nb"]), max_dist=b["max_dist"],
                          iterations=iterations, path=path)


# ------------------------------------------------------------------------------------------------ against the restatement

@pytest.mark.parametrize("max_dist", [1.0, 2.0])
@pytest.mark.parametrize("iterations", ITERS)
def test_against_restatement(dev, batches, max_dist, iterations):
    b = batches[max_dist]
    got = {k: v.cpu().numpy() for k, v in _run(dev, b, iterations).items()}
    for p, run in enumerate(b["runs"]):
        st, what = run["states"][iterations], (p, b["names"][p], max_dist, iterations)
        assert bool(got["valid"][p]) == run["valid"], what
        nn = np.full(N, -1, np.int32)
        nn[:len(st["nn"])] = st["nn"]                                # (dso_9000's run is over its 1024 rows)
        assert np.array_equal(got["nn"][p], nn), (what, int((got["nn"][p] != nn).sum()))
        assert got["num_corr"][p] == st["num_corr"], what
        assert got["fitness"][p] == st["fitness"], what
        if run["valid"]:
            err = np.abs(got["Rt"][p] - st["Rt"]).max()
            assert err < 1e-9, (what, err)
        else:
            assert np.isnan(got["Rt"][p]).all(), what
        if st["num_corr"]:
            big = max(float(np.abs(b["A"][p][:b["na"][p]]).max()), float(np.abs(b["Y"][p][:b["nb"][p]]).max()))
            assert abs(got["rmse"][p] - st["rmse"]) <= 1e-9 * (1.0 + 3.0 * big), (what, got["rmse"][p], st["rmse"])
        else:
            assert np.isnan(got["rmse"][p]), what
    names = b["names"]
    far, own = names.index("all beyond max_dist"), names.index("a cloud against itself")
    assert got["num_corr"][far] == 0 and np.array_equal(got["Rt"][far], b["Rt0"][far])      # the pose never moved
    assert np.array_equal(got["nn"][own, :500], np.arange(500)) and got["rmse"][own] < 1e-12
    assert iterations < 30 or got["num_corr"][:3].min() > 800                               # the demo pairs do overlap


# ------------------------------------------------------------------------------------------------------- the two paths

@pytest.mark.parametrize("max_dist", [1.0, 2.0])
def test_scan_and_grid_agree_on_the_batch(dev, batches, max_dist):
    b = batches[max_dist]
    _assert_same(_run(dev, b, 5, path=2), _run(dev, b, 5, path=1), max_dist)
    _assert_same(_run(dev, b, 5, path=0), _run(dev, b, 5, path=1), max_dist)


def _cube(rng, n, side=40.0):
    return (rng.random((n, 3)) * side - side / 2).astype(np.float32)


def _box_cells(anchor, centre, max_dist):
    """How many cells of the sort's grid of `anchor` the box centre +- max_dist meets (tests/spatial_reference.py)."""
    import spatial_reference as sr
    r = sr.restate(np.ascontiguousarray(anchor, np.float32))
    lo, scale, nb = r["lo"].astype(np.float64), r["scale"].astype(np.float64), r["nb"]
    n = 1
    for a in range(3):
        cell = lambda v: min((4 << int(nb[a])) - 1, int(min(max((v - lo[a]) * scale[a], 0.0), 1.0e6))) >> 2
        n *= cell(centre[a] + max_dist) - cell(centre[a] - max_dist) + 1
    return n


def test_scan_and_grid_agree_where_the_cell_walk_gives_way(dev):
    from dh3d_amd import registration as reg
    rng = np.random.default_rng(21)
    a, y, Rt_gt, Rt0 = ir.demo_pair("local_642", N, 7)
    # (0) rows of 100000.0 behind the counts, as prepare_clouds pads: no such row is chosen, and none is in the anchor's grid
    pa, py = a.copy(), y.copy()
    pa[1500:], py[1300:] = 100000.0, 100000.0
    # (1) a uniform cube (2.5 m cells) and a ball of 12 m, whose box meets more than 512 of its cells; (2) the same cube with
    # one far outlier, which stretches the grid to cells of about 157 x 189 x 102 m: at 12 m that cloud stays on its cells,
    # and it takes a ball of 2500 m for the box to meet more than 512 of them (_box_cells counts them)
    ca = _cube(rng, N)
    cy = (ca[rng.permutation(N)] + rng.normal(0.0, 0.05, (N, 3))).astype(np.float32)
    oa = ca.copy()
    oa[17] = (5000.0, -3000.0, 800.0)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    cnt = lambda *c: torch.tensor(c, dtype=torch.int32, device=dev)
    shift = EYE.copy()
    shift[:, 3] = (0.4, -0.3, 0.2)
    mid = np.zeros(3)
    assert _box_cells(ca, mid, 12.0) > 512 and _box_cells(oa, mid, 12.0) <= 512 and _box_cells(oa, mid, 2500.0) > 512
    assert _box_cells(ca, mid, 1.0) <= 512
    for what, A, Y, R0, ca_, cb_, md in (("padded", pa[None], py[None], Rt0[None], cnt(1500), cnt(1300), 1.0),
                                        ("wide box", np.stack([ca, oa]), np.stack([cy, cy]), np.stack([shift, shift]),
                                         cnt(N, N), cnt(N, N), 12.0),
                                        ("wide box on the outlier's grid", oa[None], cy[None], shift[None], cnt(N), cnt(N), 2500.0),
                                        ("sparse cells", np.stack([ca, oa]), np.stack([cy, cy]), np.stack([shift, shift]),
                                         cnt(N, N - 5), cnt(N - 3, N), 1.0)):
        scan = reg.refine_icp(t(A), t(Y), t(R0), None, ca_, cb_, max_dist=md, iterations=2, path=1)
        grid = reg.refine_icp(t(A), t(Y), t(R0), None, ca_, cb_, max_dist=md, iterations=2, path=2)
        _assert_same(grid, scan, what)
        assert int(scan["num_corr"].min()) > 1000, what
        assert int(scan["nn"].max()) < int(ca_.max()), what    # no row behind the count, no padding row
        if what != "padded":                                   # row 17 is a point of the cube, or the outlier nobody is near
            on_outlier_cloud = [A[p, 17, 0] == 5000.0 for p in range(len(A))]
            assert [bool((scan["nn"][p] == 17).any()) for p in range(len(A))] == [not o for o in on_outlier_cloud], what
    # column views are read in place (the cell lists sort a packed copy): [x, y, z, other columns]
    wide_a = torch.cat([t(a[None]), torch.full((1, N, 2), 7.0, device=dev)], dim=2)
    wide_y = torch.cat([t(y[None]), torch.full((1, N, 5), -3.0, device=dev)], dim=2)
    exp = reg.refine_icp(t(a[None]), t(y[None]), t(Rt0[None]), iterations=3, path=1)
    for path in (1, 2):
        _assert_same(reg.refine_icp(wide_a[:, :, :3], wide_y[:, :, :3], t(Rt0[None]), iterations=3, path=path), exp, path)


@pytest.mark.parametrize("max_dist", [1.0, 4.0, 12.0])
def test_scan_and_grid_agree_on_a_grid_that_is_no_cube(dev, max_dist):
    """The cell walk on a table whose schedule is not a cube's 4 + 4 + 4 (which would hide a wrong axis or bit position in
    the header's decode or the cell's code): a uniform 60 x 60 x 8 slab deals 5 + 5 + 2 bits, 32 x 32 x 4 cells of
    1.875 x 1.875 x 2 m.  The box of +-1 m meets at most 27 of them and that of +-4 m at most 6 x 6 x 4 = 144, so both walk
    the cells; at +-12 m most boxes meet more than 512 and take the 64-point groups (_box_cells counts them)."""
    from dh3d_amd import pm, registration as reg
    rng = np.random.default_rng(355)
    P, Na, Nb = 2, 2048, 1000
    A = (rng.random((P, Na, 3)) * (60, 60, 8) - (30, 30, 4)).astype(np.float32)
    c, s = math.cos(math.radians(3.0)), math.sin(math.radians(3.0))
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    Y = (A[:, :Nb].astype(np.float64) @ rot.T + 0.3).astype(np.float32)     # the anchor's own points, turned and shifted
    most = max(_box_cells(A[0], Y[0, j].astype(np.float64), max_dist) for j in range(0, Nb, 50))
    assert (most > 512) == (max_dist == 12.0) and most > 8, most
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    cells = pm.spatial_sort_cells(t(A))[2]                                  # (the table the cell lists build: no counts)
    assert bool((cells[:, 4107] != 0x186186).all()) and bool((cells[:, 4106] == 0).all())
    Rt0 = t(np.stack([EYE] * P))
    scan = reg.refine_icp(t(A), t(Y), Rt0, max_dist=max_dist, iterations=2, path=1)
    grid = reg.refine_icp(t(A), t(Y), Rt0, max_dist=max_dist, iterations=2, path=2)
    _assert_same(grid, scan, max_dist)
    assert int(scan["num_corr"].min()) > 300, scan["num_corr"]


def test_the_limit_of_the_cell_lists(dev):
    from dh3d_amd import registration as reg
    demo = np.load(os.path.join(HERE, "golden", "demo_clouds.npz"))
    cloud = demo["local_268"].astype(np.float32)                      # 16384 points
    rng = np.random.default_rng(22)
    sub = cloud[rng.permutation(len(cloud))[:N]].astype(np.float64)
    R, tr = ir.rotation((0.2, -0.1, 1.0), 0.02), np.array([0.3, -0.2, 0.1])
    y = ((sub - tr) @ R + rng.normal(0.0, 0.02, sub.shape)).astype(np.float32)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    Rt0 = t(EYE[None])
    assert reg.icp_plan(16384, N) == "grid" and reg.icp_plan(16385, N) == "scan"
    scan = reg.refine_icp(t(cloud[None]), t(y[None]), Rt0, iterations=2, path=1)
    _assert_same(reg.refine_icp(t(cloud[None]), t(y[None]), Rt0, iterations=2, path=2), scan, 16384)
    _assert_same(reg.refine_icp(t(cloud[None]), t(y[None]), Rt0, iterations=2, path=0), scan, 16384)
    assert int(scan["num_corr"][0]) > 1900
    more = np.concatenate([cloud, cloud[:1] + np.float32(300.0)])[None]   # 16385 anchors, the last one far from everything
    with pytest.raises(ValueError):
        reg.refine_icp(t(more), t(y[None]), Rt0, iterations=2, path=2)
    _assert_same(reg.refine_icp(t(more), t(y[None]), Rt0, iterations=2, path=0), scan, 16385)
    # more positives than a sort takes: the cell lists need the anchor's only
    many = t(np.concatenate([y] * 9)[None])
    assert many.shape[1] > 16384
    _assert_same(reg.refine_icp(t(cloud[None]), many, Rt0, iterations=2, path=2),
                 reg.refine_icp(t(cloud[None]), many, Rt0, iterations=2, path=1), "18432 positives")


# -------------------------------------------------------------------------------------------------- batch independence

def test_batch_independence_over_a_garbage_workspace(dev):
    """Every pair alone equals the same pair inside P = 32 with mixed counts, bit for bit, NaN included."""
    from dh3d_amd import registration as reg
    rng = np.random.default_rng(23)
    P, n = 32, 512
    A, Y, R0 = np.zeros((P, n, 3), np.float32), np.zeros((P, n, 3), np.float32), np.zeros((P, 3, 4))
    for p in range(P):
        A[p], Y[p], _, R0[p] = ir.demo_pair(("local_642", "global_c", "dso_9000")[p % 3], n, 100 + p)
    na, nb = rng.integers(0, n + 1, P).astype(np.int32), rng.integers(0, n + 1, P).astype(np.int32)
    na[:5], nb[5:10] = [0, 1, 2, 3, n], [0, 1, 2, 3, n]
    v0 = np.ones(P, np.int32)
    v0[11] = 0
    R0[12, 0, 3] = np.inf
    A[13, 300:], na[13] = 100000.0, 300                              # a padded cloud inside the batch
    t = lambda v: torch.from_numpy(v).to(dev)
    tA, tY, tR, tna, tnb, tv = t(A), t(Y), t(R0), t(na), t(nb), t(v0)

    def garbage():
        for ws in reg._ICP_WS.values():
            ws.view(torch.int32)[:].random_(-2 ** 31, 2 ** 31 - 1)

    for path in (0, 1):
        reg.refine_icp(tA, tY, tR, tv, tna, tnb, iterations=1, path=path)     # (the workspaces exist from here on)
        reg.refine_icp(tA[:1], tY[:1], tR[:1], tv[:1], tna[:1], tnb[:1], iterations=1, path=path)
        garbage()
        full = reg.refine_icp(tA, tY, tR, tv, tna, tnb, iterations=5, path=path)
        for p in range(P):
            garbage()
            s = slice(p, p + 1)
            one = reg.refine_icp(tA[s], tY[s], tR[s], tv[s], tna[s], tnb[s], iterations=5, path=path)
            _assert_same(one, {k: v[s] for k, v in full.items()}, (path, p))
        assert full["valid"].cpu().tolist() == [p not in (11, 12) for p in range(P)]
        assert int((full["num_corr"] >= 3).sum()) > 15


# ------------------------------------------------------------------------------------------------------- graph capture

def test_graph_capture_replays_on_new_inputs(dev):
    from dh3d_amd import registration as reg
    P, n = 6, 1024

    def inputs(seed):
        r = np.random.default_rng(seed)
        A, Y, R0 = np.zeros((P, n, 3), np.float32), np.zeros((P, n, 3), np.float32), np.zeros((P, 3, 4))
        for p in range(P):
            A[p], Y[p], _, R0[p] = ir.demo_pair(("local_642", "global_c")[p % 2], n, seed * 10 + p)
        cnt = r.integers(n // 2, n + 1, (2, P)).astype(np.int32)
        t = lambda v: torch.from_numpy(v).to(dev)
        return t(A), t(Y), t(R0), t(cnt[0]), t(cnt[1])

    sA, sY, sR, sna, snb = inputs(1)
    for path in (0, 1):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            reg.refine_icp(sA, sY, sR, None, sna, snb, iterations=4, path=path)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gout = reg.refine_icp(sA, sY, sR, None, sna, snb, iterations=4, path=path)
        for seed in (2, 3):
            new = inputs(seed)
            for dst, src in zip((sA, sY, sR, sna, snb), new):
                dst.copy_(src)
            g.replay()
            torch.cuda.synchronize()
            held = {k: v.clone() for k, v in gout.items()}
            eout = reg.refine_icp(new[0], new[1], new[2], None, new[3], new[4], iterations=4, path=path)
            torch.cuda.synchronize()
            _assert_same(held, eout, (path, seed))
            assert int(eout["num_corr"].min()) > 100


# ------------------------------------------------------------------------------------------------------------ plumbing

@pytest.fixture(scope="module")
def det_model(dev):
    from dh3d_amd import ConfigFactory
    from dh3d_amd.model import DH3D
    return DH3D(ConfigFactory("detection_config").getconfig()).init_synthetic(0).to(dev).eval().prepare()


def test_register_clouds_with_and_without_refinement(dev, det_model):
    from dh3d_amd import registration as reg
    demo = np.load(os.path.join(HERE, "golden", "demo_clouds.npz"))
    A = torch.from_numpy(demo["local_268"][None].astype(np.float32)).to(dev)
    B = torch.from_numpy(demo["local_642"][None].astype(np.float32)).to(dev)
    nv = torch.tensor([16000], dtype=torch.int32, device=dev)
    for num_valid, counts in ((None, (None, None)), (nv, (nv, nv))):
        plain = reg.register_clouds(det_model, A, B, num_valid=num_valid)
        oa = det_model.forward(A, fetch=("kp_count", "xyz_feat_att_nms"), num_valid=num_valid)
        ob = det_model.forward(B, fetch=("kp_count", "xyz_feat_att_nms"), num_valid=num_valid)
        today = reg.register(oa["xyz_feat_att_nms"], oa["kp_count"], ob["xyz_feat_att_nms"], ob["kp_count"])
        _assert_same(reg.register_clouds(det_model, A, B, num_valid=num_valid, refine=None), today, "refine=None")
        _assert_same(plain, today, "default")
        for refine, kw in ((True, {}), (dict(max_dist=2.0, iterations=3, path=1), dict(max_dist=2.0, iterations=3, path=1))):
            got = reg.register_clouds(det_model, A, B, num_valid=num_valid, refine=refine)
            icp = reg.refine_icp(A, B, plain["Rt"], plain["valid"], anchor_count=counts[0], positive_count=counts[1], **kw)
            exp = dict(plain, Rt_ransac=plain["Rt"], Rt=icp["Rt"], fitness=icp["fitness"], rmse=icp["rmse"],
                       num_corr_icp=icp["num_corr"], nn=icp["nn"])
            _assert_same(got, exp, refine)


def test_localize_refines_the_winner(dev):
    from dh3d_amd import registration as reg
    from dh3d_amd import retrieval
    s = place_scene(("local_268", "local_642", "global_c"), N)
    clouds, rows, count, g, T = s["clouds"], s["rows"], s["count"], s["g"], s["T"]
    index = retrieval.PlaceIndex(dim=256, capacity=8, device=dev, keypoints=64, row_dim=rows.shape[2], points=N)
    index.add(g[:1], None, rows[:1], count[:1], cloud=clouds[:1])
    index.add(g[1:], None, rows[1:], count[1:], cloud=torch.from_numpy(clouds[1:]).to(dev),
              cloud_count=np.array([N, N - 100], np.int32))
    assert index.cloud_count.cpu().tolist()[:3] == [N, N, N - 100] and torch.equal(index.cloud[1].cpu(), torch.from_numpy(clouds[1]))
    # the queries: the scene's moved copy of place 1, and one without keypoints, which no candidate can fit
    qrows = np.concatenate([s["qrows"], np.zeros_like(s["qrows"])])
    qcloud = np.concatenate([s["qcloud"], s["qcloud"]])
    t = lambda v: torch.from_numpy(v).to(dev)
    qd, qr, qc, qp = t(np.stack([g[1], g[2]])), t(qrows), torch.tensor([count[1], 0], dtype=torch.int32, device=dev), t(qcloud)
    plain = index.localize(qd, qr, qc, k=3)
    res = index.localize(qd, qr, qc, k=3, refine=True, query_cloud=qp)
    assert res["place"].cpu().tolist() == [1, -1]
    for k in plain:
        assert _bits_equal(res["Rt_ransac" if k == "Rt" else k], plain[k]), k
    assert set(res) == set(plain) | {"Rt_ransac", "fitness", "rmse"}
    icp = reg.refine_icp(index.cloud[[1, 0]], qp, plain["Rt"], plain["place"] >= 0, anchor_count=index.cloud_count[[1, 0]])
    for k in ("Rt", "fitness", "rmse"):
        assert _bits_equal(res[k], icp[k]), k
    assert bool(torch.isnan(res["Rt"][1]).all()) and float(res["fitness"][1]) == 0.0 and math.isnan(float(res["rmse"][1]))
    e_ransac = ir.pose_errors(plain["Rt"][0].cpu().numpy(), T)
    e_icp = ir.pose_errors(res["Rt"][0].cpu().numpy(), T)
    print("ransac", e_ransac, "icp", e_icp, "fitness", float(res["fitness"][0]), "rmse", float(res["rmse"][0]))
    assert e_icp[0] < e_ransac[0] or (e_icp[0] < 0.05 and e_ransac[0] < 0.05), (e_ransac, e_icp)
    assert float(res["fitness"][0]) > 0.95 and float(res["rmse"][0]) < 0.1
    bare = retrieval.PlaceIndex(dim=256, capacity=8, device=dev, keypoints=64, row_dim=rows.shape[2])
    bare.add(g, None, rows, count)
    with pytest.raises(ValueError, match="points > 0"):
        bare.localize(qd, qr, qc, k=3, refine=True, query_cloud=qp)
    with pytest.raises(ValueError):
        bare.add(g[:1], None, rows[:1], count[:1], cloud=clouds[:1])
