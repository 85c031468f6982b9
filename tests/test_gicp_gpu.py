"""GPU: dense generalized ICP (dh3d_amd.registration.refine_icp_gicp -> csrc/icp.hip) against the numpy restatement of the
rule (tests/gicp_reference.py): equal ids, counts, num_planar, fitness and validity; poses within POSE_TOL; the two
association paths bit for bit; batch independence over a garbage workspace; graph capture; the point and plane methods
untouched by a generalized call on the same shape; and the plumbing through register_fpfh and PlaceIndex.localize.  The
normals come from the restatement as float32 inputs, so nothing here depends on the normals kernel.

The tolerance.  Every per-pair quantity of the fit is the kernel's bit for bit (elementwise float64, no contraction), so
kernel and restatement differ by the order of the 31 sums of a step and nothing else, as in the plane test; its bound was
1e-9 with cond(H) <= 1e6.  Measured on the CPU, before any GPU run: the restatement with numpy's sums against the
restatement with the kernel's own order (lane j % 256, xor butterfly, four waves; gicp_reference.total(order="tree")), over
every pair of both batches below and every iteration count of ITERS, the largest pose difference was 8.4e-15;
100 x that is under 1e-9, so POSE_TOL = 1e-9.  rmse keeps the plane test's bound 1e-9 * (1 + 3 * big); rmse_gicp is
that bound times sqrt(1 / (2 * epsilon)), the largest gain sqrt(lambda_max(M)) the whitening can apply to a residual
(the eigenvalues of W = C_A + C_B lie in [2 epsilon, 2]); the two orders differed by 1.3e-14 in rmse_gicp."""
import numpy as np
import pytest
import torch

import gicp_reference as gr
import icp_plane_reference as pr
import icp_reference as ir
from icp_fixtures import _assert_same, _bits_equal, place_index, place_scene

pytestmark = pytest.mark.gpu

N = 2048
ITERS = (0, 1, 2, 5, 12)
EPS = 1e-3
POSE_TOL = 1e-9
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
KEYS = ("Rt", "valid", "nn", "num_corr", "fitness", "rmse", "num_planar", "rmse_gicp")


def _edge_pairs(seed):
    """The pairs at the rule's corners, as (name, anchor, anchor normals, positive, positive normals, Rt0, na, nb, valid0):
    test_icp_gpu's list at no more than 1024 valid rows, then the corners of the generalized fit."""
    a, y, Rt_gt, Rt0 = ir.demo_pair("local_642", N, seed)
    near = ir.move(Rt_gt, y).astype(np.float32)              # the positive's points in the anchor's frame: true partners
    nan = Rt0.copy()
    nan[2, 1] = np.nan
    na_, ny, nnear = pr.demo_normals(a, n=1024), pr.demo_normals(y, n=1024), pr.demo_normals(near, n=1024)
    zero = np.zeros_like(na_)
    some_a, some_y = na_.copy(), ny.copy()
    some_a[::3] = 0.0
    some_y[1::3] = 0.0
    # both clouds on one line: J, built from the moved positives, has no say about the rotation about it -- a refused pivot
    line, yline = a.copy(), y.copy()
    line[:64] = 0.0
    line[:64, 0] = np.linspace(-8.0, 8.0, 64)
    yline[:64] = ((line[:64].astype(np.float64) - Rt_gt[:, 3]) @ Rt_gt[:, :3]).astype(np.float32)
    up = zero.copy()
    up[:, 2] = 1.0
    return [
        ("no anchor", a, na_, y, ny, Rt0, 0, 300, True),
        ("no positive", a, na_, y, ny, Rt0, 300, 0, True),
        ("one point", near, nnear, y, ny, Rt_gt, 1, 1, True),
        ("two points", near, nnear, y, ny, Rt_gt, 2, 2, True),
        ("three points", near, nnear, y, ny, Rt_gt, 3, 3, True),
        ("all beyond max_dist", a, na_, y + np.float32(500.0), ny, Rt0, 400, 300, True),
        ("a cloud against itself", a, na_, a, na_, EYE, 500, 500, True),
        ("NaN start pose", a, na_, y, ny, nan, 300, 300, True),
        ("valid0 = 0", a, na_, y, ny, Rt0, 300, 300, False),
        ("counts off the tile", a, na_, y, ny, Rt0, 777, 1001, True),
        ("anchor normals zero", a, zero, y, ny, Rt0, 400, 300, True),
        ("positive normals zero", a, na_, y, zero, Rt0, 400, 300, True),
        ("all normals zero", a, zero, y, zero, Rt0, 400, 300, True),
        ("every third normal zero", a, some_a, y, some_y, Rt0, 900, 800, True),
        ("a collinear anchor", line, up, yline, up, Rt_gt, 64, 64, True),
    ]


def _clear_edges(max_dist, iterations, epsilon):
    """_edge_pairs of the first seed whose every run keeps the margins of gicp_reference.is_clear."""
    for seed in range(1, 51):
        pairs = _edge_pairs(seed)
        runs = [gr.icp_gicp(a, an, y, bn, Rt0, max_dist=max_dist, iterations=iterations, na=na, nb=nb, valid0=v, epsilon=epsilon)
                for _, a, an, y, bn, Rt0, na, nb, v in pairs]
        if all(gr.is_clear(r) for r in runs):
            return pairs, runs
    raise AssertionError("no clear edge fixture")


def _build(max_dist, iterations, epsilon):
    """One [P, 2048, 2048] batch: the three demo subsets, then the edge pairs; and the restatement's run of every pair."""
    A, An, Y, Bn, R0, na, nb, v0, runs, names = [], [], [], [], [], [], [], [], [], []
    for name, n in (("local_642", N), ("global_c", N), ("dso_9000", 1024)):
        (a, y, _, Rt0), an, bn, run, _ = gr.clear_pair_gicp(name, n, max_dist, iterations, epsilon=epsilon)
        # (dso_9000: 1024 points and a count; the rows behind it are points of the cloud that must never be chosen)
        pad = ir.demo_pair(name, N, 99)
        A.append(np.concatenate([a, pad[0][n:]])); Y.append(np.concatenate([y, pad[1][n:]]))
        An.append(np.concatenate([an, np.full((N - n, 3), 0.5, np.float32)]))
        Bn.append(np.concatenate([bn, np.full((N - n, 3), 0.5, np.float32)]))
        R0.append(Rt0); na.append(n); nb.append(n); v0.append(1); runs.append(run); names.append(name)
    pairs, eruns = _clear_edges(max_dist, iterations, epsilon)
    for (name, a, an, y, bn, Rt0, ca, cb, v), run in zip(pairs, eruns):
        A.append(a); An.append(an); Y.append(y); Bn.append(bn); R0.append(Rt0); na.append(ca); nb.append(cb); v0.append(int(v))
        runs.append(run); names.append(name)
    return dict(A=np.stack(A), An=np.stack(An), Y=np.stack(Y), Bn=np.stack(Bn), Rt0=np.stack(R0), na=np.array(na, np.int32),
                nb=np.array(nb, np.int32), v0=np.array(v0, np.int32), runs=runs, names=names, max_dist=max_dist, epsilon=epsilon)


@pytest.fixture(scope="module")
def batches():
    return {EPS: _build(1.0, max(ITERS), EPS), 1.0: _build(1.0, 2, 1.0)}


def _run(dev, b, iterations, path=0, sel=None):
    from dh3d_amd import registration as reg
    s = slice(None) if sel is None else sel
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v[s])).to(dev)
    return reg.refine_icp_gicp(t(b["A"]), t(b["Y"]), t(b["Rt0"]), t(b["v0"]), t(b["na"]), t(b["nb"]), max_dist=b["max_dist"],
                               iterations=iterations, path=path, anchor_normals=t(b["An"]), positive_normals=t(b["Bn"]),
                               epsilon=b["epsilon"])


# ------------------------------------------------------------------------------------------------ against the restatement

@pytest.mark.parametrize("epsilon,iterations", [(EPS, k) for k in ITERS] + [(1.0, 2)])
def test_against_restatement(dev, batches, epsilon, iterations):
    b = batches[epsilon]
    res = _run(dev, b, iterations)
    assert set(res) == set(KEYS)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    gain = np.sqrt(1.0 / (2.0 * epsilon))
    for p, run in enumerate(b["runs"]):
        st, what = run["states"][iterations], (p, b["names"][p], epsilon, iterations)
        assert bool(got["valid"][p]) == run["valid"], what
        nn = np.full(N, -1, np.int32)
        nn[:len(st["nn"])] = st["nn"]                                # (dso_9000's run is over its 1024 rows)
        assert np.array_equal(got["nn"][p], nn), (what, int((got["nn"][p] != nn).sum()))
        assert got["num_corr"][p] == st["num_corr"], what
        assert got["num_planar"][p] == st["num_planar"], what
        assert got["fitness"][p] == st["fitness"], what
        if run["valid"]:
            err = np.abs(got["Rt"][p] - st["Rt"]).max()
            print(what, "pose error", err)
            assert err < POSE_TOL, (what, err)
        else:
            assert np.isnan(got["Rt"][p]).all(), what
        big = max(float(np.abs(b["A"][p][:max(b["na"][p], 1)]).max()), float(np.abs(b["Y"][p][:max(b["nb"][p], 1)]).max()))
        for key, tol in (("rmse", 1e-9 * (1.0 + 3.0 * big)), ("rmse_gicp", 1e-9 * (1.0 + 3.0 * big) * gain)):
            if st["num_corr"]:
                assert abs(got[key][p] - st[key]) <= tol, (what, key, got[key][p], st[key])
            else:
                assert np.isnan(got[key][p]), (what, key)
    names = b["names"]
    at = names.index
    same = lambda name: np.array_equal(got["Rt"][at(name)], b["Rt0"][at(name)])                   # the pose never moved
    assert got["num_corr"][at("all beyond max_dist")] == 0 and same("all beyond max_dist")
    own = at("a cloud against itself")
    assert np.array_equal(got["nn"][own, :500], np.arange(500)) and got["rmse"][own] < 1e-12 and got["rmse_gicp"][own] < 1e-12
    assert same("one point") and same("two points") and got["num_corr"][at("two points")] == 2
    assert got["num_corr"][at("three points")] == 3 and (iterations == 0 or not same("three points"))
    for name in ("anchor normals zero", "positive normals zero", "all normals zero"):            # isotropic, still in the fit
        assert got["num_planar"][at(name)] == 0 and got["num_corr"][at(name)] > 100 and (iterations == 0 or not same(name))
    zz = at("all normals zero")
    assert abs(got["rmse_gicp"][zz] - got["rmse"][zz] / np.sqrt(2.0)) < 1e-12                      # M = I / 2
    mix = at("every third normal zero")
    assert 0 < got["num_planar"][mix] < got["num_corr"][mix]
    line = at("a collinear anchor")
    assert got["num_corr"][line] == 64 and same("a collinear anchor")                             # a refused pivot, bit-equal
    assert iterations < 12 or got["num_corr"][:3].min() > 800                                     # the demo pairs do overlap


# ------------------------------------------------------------------------------------------------------- the two paths

def test_scan_and_grid_agree_on_the_batch(dev, batches):
    b = batches[EPS]
    _assert_same(_run(dev, b, 5, path=2), _run(dev, b, 5, path=1), "grid / scan")
    _assert_same(_run(dev, b, 5, path=0), _run(dev, b, 5, path=1), "plan / scan")


def test_strided_normals_are_read_in_place(dev, batches):
    from dh3d_amd import registration as reg
    b = batches[EPS]
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v[:3])).to(dev)
    wa, wb = torch.full((3, N, 6), -4.0, device=dev), torch.full((3, N, 5), 7.0, device=dev)
    wa[:, :, 1:4], wb[:, :, 2:5] = t(b["An"]), t(b["Bn"])
    args = (t(b["A"]), t(b["Y"]), t(b["Rt0"]), t(b["v0"]), t(b["na"]), t(b["nb"]))
    _assert_same(reg.refine_icp_gicp(*args, iterations=3, anchor_normals=wa[:, :, 1:4], positive_normals=wb[:, :, 2:5]),
                 reg.refine_icp_gicp(*args, iterations=3, anchor_normals=t(b["An"]), positive_normals=t(b["Bn"])), "column views")


# -------------------------------------------------------------------------------------------------- batch independence

def test_one_pair_alone_equals_the_batch_over_a_garbage_workspace(dev, batches):
    from dh3d_amd import registration as reg
    b = batches[EPS]
    P = len(b["names"])

    def garbage():
        for ws in reg._ICP_WS.values():
            ws.view(torch.int32)[:].random_(-2 ** 31, 2 ** 31 - 1)

    _run(dev, b, 1)                                                  # (the workspaces exist from here on)
    _run(dev, b, 1, sel=slice(0, 1))
    garbage()
    full = _run(dev, b, 5)
    for p in range(P):
        garbage()
        one = _run(dev, b, 5, sel=slice(p, p + 1))
        _assert_same(one, {k: v[p:p + 1] for k, v in full.items()}, b["names"][p])


# ------------------------------------------------------------------------------------------------------- graph capture

def test_graph_capture_replays_to_the_eager_result(dev, batches):
    b = batches[EPS]
    from dh3d_amd import registration as reg
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    static = [t(b[k]) for k in ("A", "Y", "Rt0", "v0", "na", "nb", "An", "Bn")]
    call = lambda A, Y, R0, v0, na, nb, An, Bn: reg.refine_icp_gicp(A, Y, R0, v0, na, nb, iterations=4, anchor_normals=An,
                                                                    positive_normals=Bn)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gout = call(*static)
    new = [v.flip(0).contiguous() for v in static]                   # the same pairs in another order: other inputs
    for dst, src in zip(static, new):
        dst.copy_(src)
    g.replay()
    torch.cuda.synchronize()
    held = {k: v.clone() for k, v in gout.items()}
    eout = call(*new)
    torch.cuda.synchronize()
    _assert_same(held, eout, "replay")
    _assert_same({k: v.flip(0) for k, v in eout.items()}, _run(dev, b, 4), "the flipped batch")


# --------------------------------------------------------------------------------- the other two methods, untouched

def test_point_and_plane_are_unchanged_by_a_gicp_call(dev, batches):
    from dh3d_amd import registration as reg
    b = batches[EPS]
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    args = (t(b["A"]), t(b["Y"]), t(b["Rt0"]), t(b["v0"]), t(b["na"]), t(b["nb"]))
    point = reg.refine_icp(*args, iterations=5)
    plane = reg.refine_icp_plane(*args, iterations=5, anchor_normals=t(b["An"]))
    torch.cuda.synchronize()
    gicp = _run(dev, b, 5)                                           # the same shape: the same workspace
    _assert_same(reg.refine_icp(*args, iterations=5), point, "refine_icp")
    _assert_same(reg.refine_icp_plane(*args, iterations=5, anchor_normals=t(b["An"])), plane, "refine_icp_plane")
    _assert_same(reg.refine_pose(*args, method="gicp", iterations=5, anchor_normals=t(b["An"]), positive_normals=t(b["Bn"])),
                 gicp, "method=gicp")
    for k in ("valid", "num_corr"):                                  # ... and the three are three fits, not one
        assert gicp[k].shape == point[k].shape
    assert not torch.equal(gicp["Rt"][0], plane["Rt"][0]) and not torch.equal(gicp["Rt"][0], point["Rt"][0])


# ------------------------------------------------------------------------------------------------------------ plumbing

def test_register_fpfh_passes_the_method_through(dev):
    from dh3d_amd import registration as reg
    a, y, _, _ = ir.demo_pair("local_642", N, 5)
    A, B = torch.from_numpy(a[None]).to(dev), torch.from_numpy(y[None]).to(dev)
    plain = reg.register_fpfh(A, B)
    kw = dict(method="gicp", iterations=3, normals_k=8, epsilon=1e-2)
    got = reg.register_fpfh(A, B, refine=kw)
    icp = reg.refine_pose(A, B, plain["Rt"], plain["valid"], **kw)
    exp = dict(plain, Rt_ransac=plain["Rt"], Rt=icp["Rt"], fitness=icp["fitness"], rmse=icp["rmse"], num_corr_icp=icp["num_corr"],
               nn=icp["nn"], num_planar=icp["num_planar"], rmse_gicp=icp["rmse_gicp"])
    assert set(got) == set(exp)
    for k in exp:
        assert (got[k] is None and exp[k] is None) or _bits_equal(got[k], exp[k]), k
    assert "rmse_plane" not in got and "rmse_gicp" not in reg.register_fpfh(A, B, refine=True)


def test_localize_passes_the_method_through(dev):
    from dh3d_amd import registration as reg
    s = place_scene(("local_268", "local_642"), N)
    index, T = place_index(dev, s), s["T"]
    t = lambda v: torch.from_numpy(v).to(dev)
    qd, qr, qc, qp = t(s["g"][1:2]), t(s["qrows"]), torch.tensor([s["count"][1]], dtype=torch.int32, device=dev), t(s["qcloud"])
    plain = index.localize(qd, qr, qc, k=2)
    res = index.localize(qd, qr, qc, k=2, refine={"method": "gicp", "iterations": 5}, query_cloud=qp)
    assert res["place"].cpu().tolist() == [1]
    assert set(res) == set(plain) | {"Rt_ransac", "fitness", "rmse", "rmse_gicp"}
    icp = reg.refine_pose(index.cloud[[1]], qp, plain["Rt"], plain["place"] >= 0, anchor_count=index.cloud_count[[1]],
                          method="gicp", iterations=5)
    for k in ("Rt", "fitness", "rmse", "rmse_gicp"):
        assert _bits_equal(res[k], icp[k]), k
    print("ransac", ir.pose_errors(plain["Rt"][0].cpu().numpy(), T), "gicp", ir.pose_errors(res["Rt"][0].cpu().numpy(), T),
          "fitness", float(res["fitness"][0]), "rmse_gicp", float(res["rmse_gicp"][0]))
    assert float(res["fitness"][0]) > 0.95 and np.isfinite(float(res["rmse_gicp"][0]))
