"""GPU: on-device normal estimation (dh3d_amd.registration.estimate_normals -> csrc/normals.hip) against the numpy
restatement of the rule (tests/icp_plane_reference.py normals): the normals of the three demo subsets at K = 3, 8, 16 and 64
within float32 rounding wherever the eigen gap and the orientation margin leave no doubt, the eigen residuals of EVERY
returned normal against the restatement's covariance, the corners of the rule, batch independence and graph capture.

The share of points whose margins are too small to compare: the restatement finds none at K = 8 and 16 and one of 2048 at
K = 64, and the test requires at most 1 % there.  At K = 3 the covariance of three points has rank two and the gap is
lam_1 / lam_2, which is below 1e-3 whenever the three are nearly collinear -- 52, 60 and 23 points of the three clouds
(2.5 %, 2.9 %, 2.2 %; a property of the clouds, found with numpy alone); the test requires at most 4 % there.  The residual
checks cover those points too."""
import numpy as np
import pytest
import torch

import icp_plane_reference as pr
import icp_reference as ir

pytestmark = pytest.mark.gpu

N = 2048
KS = (3, 8, 16, 64)
COUNTS = (2048, 2048, 1024)
VIEW = (0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def clouds():
    """The anchors of the three demo pairs (dso_9000 behind a count of 1024, real points after it), their 64 nearest
    neighbours by brute force and the restatement's normals at every K."""
    X = np.stack([ir.demo_pair(name, N, 1)[0] for name in ("local_642", "global_c", "dso_9000")])
    ids = np.stack([pr.knn_ids(X[p], 64, COUNTS[p]) for p in range(3)])
    ref = {K: [pr.normals(X[p], ids[p][:, :K], COUNTS[p], VIEW) for p in range(3)] for K in KS}
    return dict(X=X, ids=ids, ref=ref, count=np.array(COUNTS, np.int32))


def _t(dev, v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("K", KS)
def test_against_restatement(dev, clouds, K):
    from dh3d_amd import registration as reg
    got = reg.estimate_normals(_t(dev, clouds["X"]), _t(dev, clouds["count"]), viewpoint=VIEW,
                               nbr=_t(dev, clouds["ids"][:, :, :K]))
    nrm, cur = got["normals"].cpu().numpy(), got["curvature"].cpu().numpy()
    assert nrm.dtype == np.float32 and nrm.shape == (3, N, 3) and cur.shape == (3, N)
    v = np.asarray(VIEW)
    for p, n in enumerate(COUNTS):
        r = clouds["ref"][K][p]
        sure = (r["gap"][:n] >= 1e-3) & (r["margin"][:n] >= 1e-6)
        left_out = int(n - sure.sum())
        print("K", K, "cloud", p, "left out", left_out, "of", n)
        assert left_out <= (0.04 if K == 3 else 0.01) * n, (K, p, left_out)        # a condition on the fixture: see the docstring
        err = np.abs(nrm[p, :n][sure] - r["normals"][:n][sure].astype(np.float32)).max()
        print("  normal error", err)
        assert err <= 2e-7, (K, p, err)
        cerr = np.abs(cur[p, :n].astype(np.float64) - r["curvature"][:n]).max()
        print("  curvature error", cerr)
        assert cerr <= 1e-6, (K, p, cerr)
        # every point with a normal, in float64 on the returned float32 normal
        g = nrm[p, :n].astype(np.float64)
        has = (g * g).sum(axis=1) > 0
        assert np.array_equal(has, (r["normals"][:n] ** 2).sum(axis=1) > 0), (K, p)
        C, lam = r["C"][:n][has], r["lam"][:n][has]
        g = g[has]
        Cn = np.einsum("iab,ib->ia", C, g)
        ray = (g * Cn).sum(axis=1)
        resid = np.linalg.norm(Cn - ray[:, None] * g, axis=1)
        assert (resid <= 1e-6 * lam[:, 2]).all(), (K, p, (resid / lam[:, 2]).max())
        assert (ray <= lam[:, 0] + 1e-6 * lam[:, 2]).all(), (K, p)
        assert np.abs(np.linalg.norm(g, axis=1) - 1.0).max() <= 1e-6, (K, p)
        d = v[None, :] - clouds["X"][p, :n][has].astype(np.float64)
        s = (d[:, 0] * g[:, 0] + d[:, 1] * g[:, 1]) + d[:, 2] * g[:, 2]
        assert (s >= -1e-6 * np.linalg.norm(d, axis=1)).all(), (K, p)
        assert has.sum() >= 0.99 * n
        # rows behind the count are written as zeros
        assert not nrm[p, n:].any() and not cur[p, n:].any()


def test_device_knn_ids_and_the_given_ids_agree(dev, clouds):
    """nbr=None takes the ids of utils.batched_knn; handing the same ids back gives the same bits, and the restatement on
    those ids gives the same normals."""
    from dh3d_amd import registration as reg
    x = _t(dev, clouds["X"][:2])
    auto = reg.estimate_normals(x, k=16)
    assert auto["nbr"].shape == (2, N, 16) and auto["nbr"].dtype == torch.int32
    again = reg.estimate_normals(x, nbr=auto["nbr"])
    assert _same_bits(auto["normals"], again["normals"]) and _same_bits(auto["curvature"], again["curvature"])
    ids = auto["nbr"].cpu().numpy()
    for p in range(2):
        assert (np.sort(ids[p], axis=1) == np.sort(clouds["ids"][p][:, :16], axis=1)).mean() > 0.99   # the exact kNN, up to float32 near-ties
        r = pr.normals(clouds["X"][p], ids[p], N, VIEW)
        sure = (r["gap"] >= 1e-3) & (r["margin"] >= 1e-6)
        assert sure.sum() >= 0.99 * N
        assert np.abs(auto["normals"][p].cpu().numpy()[sure] - r["normals"][sure].astype(np.float32)).max() <= 2e-7


def test_corners_of_the_rule(dev):
    from dh3d_amd import registration as reg
    rng = np.random.default_rng(31)
    M = 300
    # cloud 0: points on the plane z = 2.5.  cloud 1: rows 0..7 coincide, rows 8..39 lie on a line, the rest is a plane.
    plane = np.concatenate([rng.random((M, 2)) * 4.0 - 2.0, np.full((M, 1), 2.5)], axis=1).astype(np.float32)
    mixed = plane.copy()
    mixed[:8] = (1.0, -2.0, 0.25)
    mixed[8:40] = np.array([0.5, 0.25, -1.0], np.float32) + np.arange(32, dtype=np.float32)[:, None] * np.array([0.25, 0.5, 0.125], np.float32)
    X = np.stack([plane, mixed])
    nbr = np.stack([pr.knn_ids(plane, 8), pr.knn_ids(plane, 8)])
    nbr[1, :8] = np.arange(8)                                          # coincident neighbours
    nbr[1, 8:40] = 8 + (np.arange(32)[:, None] + np.arange(8)[None, :]) % 32   # collinear neighbours
    for view, z in (((0.0, 0.0, 10.0), 1.0), ((0.0, 0.0, 0.0), -1.0), ((50.0, -20.0, 2.75), 1.0)):
        got = reg.estimate_normals(_t(dev, X), nbr=_t(dev, nbr), viewpoint=view)
        nrm, cur = got["normals"].cpu().numpy(), got["curvature"].cpu().numpy()
        assert np.array_equal(nrm[0], np.tile(np.array([0.0, 0.0, z], np.float32), (M, 1))), view     # exactly
        assert not cur[0].any()
        assert not nrm[1, :8].any() and not cur[1, :8].any()                                        # coincident: no normal
        line = nrm[1, 8:40].astype(np.float64)
        assert np.isfinite(line).all() and np.isfinite(cur[1, 8:40]).all()
        ln = np.linalg.norm(line, axis=1)
        assert ((np.abs(ln - 1.0) <= 1e-6) | (ln == 0.0)).all()
        assert np.abs(line[ln > 0] @ np.array([0.25, 0.5, 0.125])).max() < 1e-6                       # across the line
        clean = np.concatenate([np.zeros(40, bool), (nbr[1, 40:] >= 40).all(axis=1)])   # no moved point in the list
        assert clean.sum() > 50 and np.array_equal(nrm[1][clean], nrm[0][clean])
    # counts 0, 1, 2, 3 (and a count beyond N): nothing behind a count is read into a normal, every element is written
    X4 = np.stack([plane] * 5)
    ids4 = np.stack([pr.knn_ids(plane, 8)] * 5)
    cnt = np.array([0, 1, 2, 3, M + 7], np.int32)
    got = reg.estimate_normals(_t(dev, X4), _t(dev, cnt), nbr=_t(dev, ids4), viewpoint=(0.0, 0.0, 10.0))
    nrm = got["normals"].cpu().numpy()
    assert not nrm[:3].any() and not got["curvature"][:4].cpu().numpy().any()
    ref3 = pr.normals(plane, ids4[3], 3, (0.0, 0.0, 10.0))
    assert np.array_equal(nrm[3], ref3["normals"].astype(np.float32)) and (ref3["m"][:3] <= 3).all()
    assert np.array_equal(nrm[4], np.tile(np.array([0.0, 0.0, 1.0], np.float32), (M, 1)))
    # lists holding -1, ids >= n and duplicates, on a real cloud behind a count
    a = ir.demo_pair("local_642", 512, 3)[0]
    n = 400
    ids = pr.knn_ids(a, 16, n)
    ids[n:] = rng.integers(0, 512, (512 - n, 16))                      # rows behind the count hold ids all the same
    holes = rng.random(ids.shape)
    ids = np.where(holes < 0.1, -1, np.where(holes < 0.2, rng.integers(n, 100000, ids.shape), ids)).astype(np.int32)
    ids[:, 5] = ids[:, 2]                                              # a duplicate in every list
    ids[7] = [0, 1, -1, -5, n, n + 1, 2 ** 31 - 1, -2 ** 31, 0, 1, -1, -1, -1, -1, -1, -1]   # two usable ids, twice each
    r = pr.normals(a, ids, n, (3.0, 4.0, 5.0))
    wide = torch.full((1, 512, 7), 9.0, device=dev)
    wide[0, :, 2:5] = _t(dev, a)
    got = reg.estimate_normals(wide[:, :, 2:5], _t(dev, np.array([n], np.int32)), nbr=_t(dev, ids[None]), viewpoint=(3.0, 4.0, 5.0))
    packed = reg.estimate_normals(_t(dev, a[None]), _t(dev, np.array([n], np.int32)), nbr=_t(dev, ids[None]), viewpoint=(3.0, 4.0, 5.0))
    assert _same_bits(got["normals"], packed["normals"]) and _same_bits(got["curvature"], packed["curvature"])   # read in place
    nrm = got["normals"][0].cpu().numpy()
    assert r["m"][7] == 4
    assert np.array_equal((nrm ** 2).sum(axis=1) > 0, (r["normals"] ** 2).sum(axis=1) > 0)
    sure = (r["gap"] >= 1e-3) & (r["margin"] >= 1e-6) & (r["m"] >= 3)
    assert sure[:n].sum() > 0.8 * n
    assert np.abs(nrm[sure] - r["normals"][sure].astype(np.float32)).max() <= 2e-7
    assert not nrm[n:].any()


def test_batch_independence_and_graph_capture(dev, clouds):
    from dh3d_amd import registration as reg
    x, cnt, nbr = _t(dev, clouds["X"]), _t(dev, clouds["count"]), _t(dev, clouds["ids"][:, :, :16])
    full = reg.estimate_normals(x, cnt, nbr=nbr, viewpoint=(1.0, 2.0, 3.0))
    for p in range(3):
        s = slice(p, p + 1)
        one = reg.estimate_normals(x[s], cnt[s], nbr=nbr[s], viewpoint=(1.0, 2.0, 3.0))
        assert _same_bits(one["normals"], full["normals"][s]) and _same_bits(one["curvature"], full["curvature"][s]), p
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        reg.estimate_normals(x, cnt, nbr=nbr, viewpoint=(1.0, 2.0, 3.0))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gout = reg.estimate_normals(x, cnt, nbr=nbr, viewpoint=(1.0, 2.0, 3.0))
    for _ in range(2):
        gout["normals"].fill_(7.0)
        gout["curvature"].fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert _same_bits(gout["normals"], full["normals"]) and _same_bits(gout["curvature"], full["curvature"])
