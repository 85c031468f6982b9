"""GPU: dense point-to-plane ICP (dh3d_amd.registration.refine_icp_plane -> csrc/icp.hip) against the numpy restatement of
the rule (tests/icp_plane_reference.py): equal ids, counts and validity, poses within 1e-9 (the sibling test's bound: the
error sources are the same, summation order and solver, and cond(H) <= 1e6 keeps a step's error below 1e6 * 2^-53); the
two association paths bit for bit; batch independence over a garbage workspace; graph capture; the point method untouched;
the device normals end to end; and the plumbing through register_clouds and PlaceIndex.localize.  The normals of the
comparisons come from the restatement as float32 inputs, so nothing there depends on the normals kernel."""
import math
import os

import numpy as np
import pytest
import torch

import icp_plane_reference as pr
import icp_reference as ir
from icp_fixtures import _assert_same, _bits_equal, place_index, place_scene

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N = 2048
ITERS = (0, 1, 2, 5, 30)
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
KEYS = ("Rt", "valid", "nn", "num_corr", "fitness", "rmse", "num_plane", "rmse_plane")


def _edge_pairs(seed):
    """The pairs at the rule's corners, as (name, anchor, normals, positive, Rt0, na, nb, valid0): test_icp_gpu's list, then
    the corners of the plane fit."""
    a, y, Rt_gt, Rt0 = ir.demo_pair("local_642", N, seed)
    near = ir.move(Rt_gt, y).astype(np.float32)              # the positive's points in the anchor's frame: true partners
    nan = Rt0.copy()
    nan[2, 1] = np.nan
    na_, nnear = pr.demo_normals(a), pr.demo_normals(near)
    zero = np.zeros_like(na_)
    up = zero.copy()
    up[:, 2] = 1.0
    flat = a.copy()
    flat[:, 2] = np.float32(0.5)
    some = na_.copy()
    some[::3] = 0.0
    return [
        ("no anchor", a, na_, y, Rt0, 0, 300, True),
        ("no positive", a, na_, y, Rt0, 300, 0, True),
        ("one point", near, nnear, y, Rt_gt, 1, 1, True),
        ("two points", near, nnear, y, Rt_gt, 2, 2, True),
        ("three points", near, nnear, y, Rt_gt, 3, 3, True),
        ("all beyond max_dist", a, na_, y + np.float32(500.0), Rt0, 400, 300, True),
        ("a cloud against itself", a, na_, a, EYE, 500, 500, True),
        ("NaN start pose", a, na_, y, nan, 300, 300, True),
        ("valid0 = 0", a, na_, y, Rt0, 300, 300, False),
        ("counts off the tile", a, na_, y, Rt0, 777, 1001, True),
        ("five pairs", near, nnear, y, Rt_gt, 5, 5, True),
        ("all normals zero", a, zero, y, Rt0, 400, 300, True),
        ("parallel normals on a coplanar anchor", flat, up, y, Rt0, 700, 600, True),
        ("zero and non-zero normals", a, some, y, Rt0, 900, 800, True),
    ]


def _clear_edges(max_dist):
    """_edge_pairs of the first seed whose every run keeps the margins of icp_plane_reference.is_clear."""
    for seed in range(1, 51):
        pairs = _edge_pairs(seed)
        runs = [pr.icp_plane(a, nr, y, Rt0, max_dist=max_dist, iterations=max(ITERS), na=na, nb=nb, valid0=v)
                for _, a, nr, y, Rt0, na, nb, v in pairs]
        if all(pr.is_clear(r) for r in runs):
            return pairs, runs
    raise AssertionError("no clear edge fixture")


def _build(max_dist):
    """One [P, 2048, 2048] batch in test_icp_gpu._build's shape: the three demo subsets, then the edge pairs; and the
    restatement's run of every pair."""
    A, Nr, Y, R0, na, nb, v0, runs, names = [], [], [], [], [], [], [], [], []
    for name, n in (("local_642", N), ("global_c", N), ("dso_9000", 1024)):
        (a, y, _, Rt0), nrm, run, _ = pr.clear_pair_plane(name, n, max_dist, max(ITERS))
        # (dso_9000: 1024 points and a count; the rows behind it are points of the cloud that must never be chosen)
        pad = ir.demo_pair(name, N, 99)
        A.append(np.concatenate([a, pad[0][n:]])); Y.append(np.concatenate([y, pad[1][n:]]))
        Nr.append(np.concatenate([nrm, np.full((N - n, 3), 0.5, np.float32)]))
        R0.append(Rt0); na.append(n); nb.append(n); v0.append(1); runs.append(run); names.append(name)
    pairs, eruns = _clear_edges(max_dist)
    for (name, a, nr, y, Rt0, ca, cb, v), run in zip(pairs, eruns):
        A.append(a); Nr.append(nr); Y.append(y); R0.append(Rt0); na.append(ca); nb.append(cb); v0.append(int(v))
        runs.append(run); names.append(name)
    return dict(A=np.stack(A), Nr=np.stack(Nr), Y=np.stack(Y), Rt0=np.stack(R0), na=np.array(na, np.int32),
                nb=np.array(nb, np.int32), v0=np.array(v0, np.int32), runs=runs, names=names, max_dist=max_dist)


@pytest.fixture(scope="module")
def batches():
    return {md: _build(md) for md in (1.0, 2.0)}


def _run(dev, b, iterations, path=0, sel=None):
    from dh3d_amd import registration as reg
    s = slice(None) if sel is None else sel
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v[s])).to(dev)
    return reg.refine_icp_plane(t(b["A"]), t(b["Y"]), t(b["Rt0"]), t(b["v0"]), t(b["na"]), t(b["nb"]), max_dist=b["max_dist"],
                                iterations=iterations, path=path, anchor_normals=t(b["Nr"]))


# ------------------------------------------------------------------------------------------------ against the restatement

@pytest.mark.parametrize("max_dist", [1.0, 2.0])
@pytest.mark.parametrize("iterations", ITERS)
def test_against_restatement(dev, batches, max_dist, iterations):
    b = batches[max_dist]
    res = _run(dev, b, iterations)
    assert set(res) == set(KEYS)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    for p, run in enumerate(b["runs"]):
        st, what = run["states"][iterations], (p, b["names"][p], max_dist, iterations)
        assert bool(got["valid"][p]) == run["valid"], what
        nn = np.full(N, -1, np.int32)
        nn[:len(st["nn"])] = st["nn"]                                # (dso_9000's run is over its 1024 rows)
        assert np.array_equal(got["nn"][p], nn), (what, int((got["nn"][p] != nn).sum()))
        assert got["num_corr"][p] == st["num_corr"], what
        assert got["num_plane"][p] == st["num_plane"], what
        assert got["fitness"][p] == st["fitness"], what
        if run["valid"]:
            err = np.abs(got["Rt"][p] - st["Rt"]).max()
            assert err < 1e-9, (what, err)
        else:
            assert np.isnan(got["Rt"][p]).all(), what
        big = max(float(np.abs(b["A"][p][:max(b["na"][p], 1)]).max()), float(np.abs(b["Y"][p][:max(b["nb"][p], 1)]).max()))
        for key, cnt in (("rmse", "num_corr"), ("rmse_plane", "num_plane")):
            if st[cnt]:
                assert abs(got[key][p] - st[key]) <= 1e-9 * (1.0 + 3.0 * big), (what, key, got[key][p], st[key])
            else:
                assert np.isnan(got[key][p]), (what, key)
    names = b["names"]
    same = lambda name: np.array_equal(got["Rt"][names.index(name)], b["Rt0"][names.index(name)])   # the pose never moved
    far, own = names.index("all beyond max_dist"), names.index("a cloud against itself")
    assert got["num_corr"][far] == 0 and same("all beyond max_dist")
    assert np.array_equal(got["nn"][own, :500], np.arange(500)) and got["rmse"][own] < 1e-12 and got["rmse_plane"][own] < 1e-12
    five, zero = names.index("five pairs"), names.index("all normals zero")
    assert got["num_plane"][five] == 5 and same("five pairs") and same("three points")
    assert got["num_plane"][zero] == 0 and got["num_corr"][zero] > 100 and same("all normals zero") and np.isnan(got["rmse_plane"][zero])
    par, mix = names.index("parallel normals on a coplanar anchor"), names.index("zero and non-zero normals")
    assert got["num_plane"][par] >= 6 and same("parallel normals on a coplanar anchor")          # a refused pivot, bit-equal
    assert 6 <= got["num_plane"][mix] < got["num_corr"][mix]
    assert iterations == 0 or not same("zero and non-zero normals")
    assert iterations < 30 or got["num_corr"][:3].min() > 800                                   # the demo pairs do overlap


# ------------------------------------------------------------------------------------------------------- the two paths

@pytest.mark.parametrize("max_dist", [1.0, 2.0])
def test_scan_and_grid_agree_on_the_batch(dev, batches, max_dist):
    b = batches[max_dist]
    _assert_same(_run(dev, b, 5, path=2), _run(dev, b, 5, path=1), max_dist)
    _assert_same(_run(dev, b, 5, path=0), _run(dev, b, 5, path=1), max_dist)


def test_strided_normals_are_read_in_place(dev, batches):
    from dh3d_amd import registration as reg
    b = batches[1.0]
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v[:3])).to(dev)
    wide = torch.full((3, N, 6), -4.0, device=dev)
    wide[:, :, 1:4] = t(b["Nr"])
    args = (t(b["A"]), t(b["Y"]), t(b["Rt0"]), t(b["v0"]), t(b["na"]), t(b["nb"]))
    _assert_same(reg.refine_icp_plane(*args, iterations=3, anchor_normals=wide[:, :, 1:4]),
                 reg.refine_icp_plane(*args, iterations=3, anchor_normals=t(b["Nr"])), "column view")


# -------------------------------------------------------------------------------------------------- batch independence

def test_one_pair_alone_equals_the_batch_over_a_garbage_workspace(dev, batches):
    from dh3d_amd import registration as reg
    b = batches[1.0]
    P = len(b["names"])

    def garbage():
        for ws in reg._ICP_WS.values():
            ws.view(torch.int32)[:].random_(-2 ** 31, 2 ** 31 - 1)

    for path in (0, 1):
        _run(dev, b, 1, path=path)                                   # (the workspaces exist from here on)
        _run(dev, b, 1, path=path, sel=slice(0, 1))
        garbage()
        full = _run(dev, b, 5, path=path)
        for p in range(P):
            garbage()
            one = _run(dev, b, 5, path=path, sel=slice(p, p + 1))
            _assert_same(one, {k: v[p:p + 1] for k, v in full.items()}, (path, b["names"][p]))


# ------------------------------------------------------------------------------------------------------- graph capture

def test_graph_capture_and_two_replays(dev):
    from dh3d_amd import registration as reg
    P, n = 6, 1024

    def inputs(seed):
        r = np.random.default_rng(seed)
        A, Y, R0 = np.zeros((P, n, 3), np.float32), np.zeros((P, n, 3), np.float32), np.zeros((P, 3, 4))
        for p in range(P):
            A[p], Y[p], _, R0[p] = ir.demo_pair(("local_642", "global_c")[p % 2], n, seed * 10 + p)
        cnt = r.integers(n // 2, n + 1, (2, P)).astype(np.int32)
        Nr = np.stack([pr.demo_normals(A[p], 8) for p in range(P)])
        t = lambda v: torch.from_numpy(v).to(dev)
        return t(A), t(Nr), t(Y), t(R0), t(cnt[0]), t(cnt[1])

    call = lambda A, Nr, Y, R0, na, nb, path: reg.refine_icp_plane(A, Y, R0, None, na, nb, iterations=4, path=path, anchor_normals=Nr)
    static = inputs(1)
    for path in (0, 1):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call(*static, path)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gout = call(*static, path)
        for seed in (2, 3):
            new = inputs(seed)
            for dst, src in zip(static, new):
                dst.copy_(src)
            g.replay()
            torch.cuda.synchronize()
            held = {k: v.clone() for k, v in gout.items()}
            eout = call(*new, path)
            torch.cuda.synchronize()
            _assert_same(held, eout, (path, seed))
            assert int(eout["num_plane"].min()) > 100


# ------------------------------------------------------------------------------------------- the point method, untouched

def test_method_point_is_a_direct_call(dev, batches):
    from dh3d_amd import _lib as L
    from dh3d_amd import registration as reg
    b = batches[1.0]
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    A, Y, R0, v0, na, nb = t(b["A"]), t(b["Y"]), t(b["Rt0"]), t(b["v0"]), t(b["na"]), t(b["nb"])
    P = A.shape[0]
    lib = L.lib()
    ws = torch.empty((lib.dh3d_icp_refine_ws_bytes(P, N, N),), dtype=torch.uint8, device=dev)
    out = dict(Rt=torch.empty((P, 3, 4), dtype=torch.float64, device=dev), nn=torch.empty((P, N), dtype=torch.int32, device=dev),
               num_corr=torch.empty((P,), dtype=torch.int32, device=dev), fitness=torch.empty((P,), dtype=torch.float64, device=dev),
               rmse=torch.empty((P,), dtype=torch.float64, device=dev), valid=torch.empty((P,), dtype=torch.int32, device=dev))
    L.check(lib.dh3d_icp_refine(A.data_ptr(), 3, na.data_ptr(), Y.data_ptr(), 3, nb.data_ptr(), R0.data_ptr(), v0.data_ptr(), P,
                                N, N, 1.0, 5, 0, out["Rt"].data_ptr(), out["nn"].data_ptr(), out["num_corr"].data_ptr(),
                                out["fitness"].data_ptr(), out["rmse"].data_ptr(), out["valid"].data_ptr(), ws.data_ptr(),
                                ws.numel(), L.stream_ptr()), "direct")
    torch.cuda.synchronize()
    out["valid"] = out["valid"].bool()
    _assert_same(reg.refine_pose(A, Y, R0, v0, na, nb, method="point", iterations=5), out, "method=point")
    _assert_same(reg.refine_pose(A, Y, R0, v0, na, nb, iterations=5), out, "default method")
    _assert_same(reg.refine_icp(A, Y, R0, v0, na, nb, iterations=5), out, "refine_icp")
    plane = reg.refine_pose(A, Y, R0, v0, na, nb, method="plane", iterations=5, anchor_normals=t(b["Nr"]))
    _assert_same(plane, _run(dev, b, 5), "method=plane")


# ---------------------------------------------------------------------------------------------------------- end to end

def test_device_normals_end_to_end(dev):
    """refine_icp_plane with anchor_normals=None -- the device kNN and the normals kernel at k = 16 -- on the 2048-point
    local_642 pair: after 10 iterations less than half the translation error of the point method (the restatement gives
    0.028 m against 0.204 m)."""
    from dh3d_amd import registration as reg
    a, y, gt, Rt0 = ir.demo_pair("local_642", N, 1)
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    plane = reg.refine_icp_plane(t(a[None]), t(y[None]), t(Rt0[None]), iterations=10)
    point = reg.refine_icp(t(a[None]), t(y[None]), t(Rt0[None]), iterations=10)
    e_plane = ir.pose_errors(plane["Rt"][0].cpu().numpy(), gt)[0]
    e_point = ir.pose_errors(point["Rt"][0].cpu().numpy(), gt)[0]
    print("translation error after 10 iterations: plane", e_plane, "point", e_point)
    assert e_plane < 0.5 * e_point, (e_plane, e_point)
    assert int(plane["num_plane"][0]) == int(plane["num_corr"][0]) > 800
    given = reg.refine_icp_plane(t(a[None]), t(y[None]), t(Rt0[None]), iterations=10,
                                 anchor_normals=reg.estimate_normals(t(a[None]), k=16)["normals"])
    _assert_same(given, plane, "the normals of estimate_normals")


# ------------------------------------------------------------------------------------------------------------ plumbing

def test_register_clouds_passes_the_method_through(dev):
    from dh3d_amd import ConfigFactory
    from dh3d_amd import registration as reg
    from dh3d_amd.model import DH3D
    model = DH3D(ConfigFactory("detection_config").getconfig()).init_synthetic(0).to(dev).eval().prepare()
    demo = np.load(os.path.join(HERE, "golden", "demo_clouds.npz"))
    A = torch.from_numpy(demo["local_268"][None].astype(np.float32)).to(dev)
    B = torch.from_numpy(demo["local_642"][None].astype(np.float32)).to(dev)
    plain = reg.register_clouds(model, A, B)
    kw = dict(iterations=3, normals_k=8, viewpoint=(0.0, 0.0, 5.0))
    got = reg.register_clouds(model, A, B, refine=dict(kw, method="plane"))
    icp = reg.refine_icp_plane(A, B, plain["Rt"], plain["valid"], **kw)
    exp = dict(plain, Rt_ransac=plain["Rt"], Rt=icp["Rt"], fitness=icp["fitness"], rmse=icp["rmse"], num_corr_icp=icp["num_corr"],
               nn=icp["nn"], num_plane=icp["num_plane"], rmse_plane=icp["rmse_plane"])
    _assert_same(got, exp, "method=plane")
    point = reg.register_clouds(model, A, B, refine=dict(method="point", iterations=3))
    _assert_same(point, reg.register_clouds(model, A, B, refine=dict(iterations=3)), "method=point")
    assert "rmse_plane" not in point


def test_localize_passes_the_method_through(dev):
    from dh3d_amd import registration as reg
    s = place_scene(("local_268", "local_642"), N)
    index, T = place_index(dev, s), s["T"]
    t = lambda v: torch.from_numpy(v).to(dev)
    qd, qr, qc, qp = t(s["g"][1:2]), t(s["qrows"]), torch.tensor([s["count"][1]], dtype=torch.int32, device=dev), t(s["qcloud"])
    plain = index.localize(qd, qr, qc, k=2)
    res = index.localize(qd, qr, qc, k=2, refine={"method": "plane", "iterations": 5}, query_cloud=qp)
    assert res["place"].cpu().tolist() == [1]
    assert set(res) == set(plain) | {"Rt_ransac", "fitness", "rmse", "rmse_plane"}
    icp = reg.refine_icp_plane(index.cloud[[1]], qp, plain["Rt"], plain["place"] >= 0, anchor_count=index.cloud_count[[1]],
                               iterations=5)
    for k in ("Rt", "fitness", "rmse", "rmse_plane"):
        assert _bits_equal(res[k], icp[k]), k
    e_ransac = ir.pose_errors(plain["Rt"][0].cpu().numpy(), T)
    e_icp = ir.pose_errors(res["Rt"][0].cpu().numpy(), T)
    print("ransac", e_ransac, "plane icp", e_icp, "fitness", float(res["fitness"][0]), "rmse_plane", float(res["rmse_plane"][0]))
    assert e_icp[0] < e_ransac[0] or (e_icp[0] < 0.05 and e_ransac[0] < 0.05), (e_ransac, e_icp)
    assert float(res["fitness"][0]) > 0.95 and float(res["rmse_plane"][0]) < float(res["rmse"][0])   # |n . d| <= |d|
