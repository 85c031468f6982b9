"""GPU: FPFH descriptors on the device (dh3d_amd.registration.compute_fpfh -> csrc/fpfh.hip) against the numpy restatement
of the rule (tests/fpfh_reference.py), and the model-free registration register_fpfh end to end.

The fixtures: the anchors of the three demo pairs, P = 3, N = 2048, counts 2048 / 2048 / 1024, the restatement's normals as
float32 input and brute-force neighbour ids, at K = 1, 3, 16, 17, 33 and 64 (the edges of the sub-wave groups of 4 / 16 /
32 / 64 lanes; K = 1 is the self-only list, m = 0 everywhere) and at K = 8 (the groups of 8 lanes: every launch branch runs).

Tolerances.  The counts are integers: they must be bit-equal wherever no pair coordinate lies within 1e-9 of a bin edge (the
kernel's coordinates differ from numpy's by the last bits of atan2 only, 1e-15); the restatement finds no such point on
these fixtures (tests/test_fpfh_reference.py: the smallest margin is 1.3e-7) and the test allows at most 1 %.  The FPFH
values are compared at 2e-5 absolute: one float32 ulp at 200, the largest value a bin can take.

The matches of the end-to-end test are compared where the restatement's gap between the nearest and the second nearest
descriptor is larger than what those tolerances can close: an error of 2e-5 in each of 33 columns moves a row by at most
sqrt(33) * 2e-5 = 1.15e-4, a distance between two rows by 2.3e-4, the difference of two distances by 4.6e-4; the float32
distance of dh3d_match_descriptors (36 squares summed in float32, a square root) adds at most 38 * 2^-24 = 2.3e-6 of each
distance.  Gap > 4.6e-4 + 2.3e-6 * (nearest + second); at most 1 % of the anchors may fall below it."""
import numpy as np
import pytest
import torch

import fpfh_reference as fr
import icp_plane_reference as pr
import icp_reference as ir
import registration_reference as reg_ref

pytestmark = pytest.mark.gpu

N = fr.N_DEMO
COUNTS = fr.COUNTS
TOL = 2e-5
_REF = {}


@pytest.fixture(scope="module")
def demo():
    return fr.demo_fixture()


def _ref(demo, K, max_dist=None):
    """The restatement on the three clouds at K (computed once per (K, max_dist), never changed)."""
    key = (K, max_dist)
    if key not in _REF:
        _REF[key] = [fr.compute(demo["X"][p], demo["normals"][p], demo["ids"][p][:, :K], COUNTS[p], max_dist) for p in range(3)]
    return _REF[key]


def _t(dev, v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _inputs(dev, demo, K):
    return _t(dev, demo["X"]), _t(dev, demo["normals"]), _t(dev, demo["count"]), _t(dev, demo["ids"][:, :, :K].astype(np.int32))


def _compare(got, ref, label):
    cnt, f = got["counts"].cpu().numpy(), got["fpfh"].cpu().numpy()
    assert cnt.dtype == np.uint8 and cnt.shape == (3, N, 36) and f.dtype == np.float32 and f.shape == (3, N, 36)
    for p, n in enumerate(COUNTS):
        r = ref[p]
        sure = r["margin"][:n] >= 1e-9
        print(label, "cloud", p, "counts: left out", int(n - sure.sum()), "of", n, "; rows differing",
              int((cnt[p, :n] != r["counts"][:n]).any(axis=1).sum()))
        assert n - sure.sum() <= 0.01 * n, (label, p)
        assert np.array_equal(cnt[p, :n][sure], r["counts"][:n][sure]), (label, p)
        assert not cnt[p, n:].any() and not cnt[p, :, 34:].any() and not f[p, n:].any() and not f[p, :, 33:].any(), (label, p)
        clear = r["clear"][:n]
        assert n - clear.sum() <= 0.01 * n, (label, p)
        err = np.abs(f[p, :n][clear].astype(np.float64) - r["fpfh"][:n][clear]).max() if clear.any() else 0.0
        bit = np.array_equal(f[p, :n][clear], r["fpfh"][:n][clear].astype(np.float32))
        print(label, "cloud", p, "fpfh: left out", int(n - clear.sum()), "max error %.3g" % err, "bit-equal to the rounded restatement:", bit)
        assert err <= TOL, (label, p, err)


@pytest.mark.parametrize("K", fr.KS + (8,))                   # (8: the 8-lane groups, which none of the other K launches)
def test_against_restatement(dev, demo, K):
    from dh3d_amd import registration as reg
    x, nrm, cnt, nbr = _inputs(dev, demo, K)
    got = reg.compute_fpfh(x, nrm, cnt, nbr=nbr)
    assert got["nbr"].shape == (3, N, K) and got["normals"].shape == (3, N, 3)
    _compare(got, _ref(demo, K), "K %d" % K)
    c = got["counts"].cpu().numpy()
    if K == 1:
        assert not c.any() and not got["fpfh"].cpu().numpy().any()              # the self-only list: no pair at all
    else:
        assert (c[0, :, 33] > 0).mean() > 0.95 and c[:, :, 33].max() <= K - 1


def test_max_dist_at_the_median_neighbour_distance(dev, demo):
    from dh3d_amd import registration as reg
    K = 16
    x, nrm, cnt, nbr = _inputs(dev, demo, K)
    d = np.concatenate([np.linalg.norm(demo["X"][p][demo["ids"][p][:n, 1:K]] - demo["X"][p][:n, None, :], axis=2).ravel()
                        for p, n in enumerate(COUNTS)])
    md = float(np.median(d))
    ref = _ref(demo, K, md)
    inside = np.mean([ref[p]["near"][:n, 1:].mean() for p, n in enumerate(COUNTS)])
    assert 0.3 < inside < 0.7, inside                                            # some pairs in, some out
    got = reg.compute_fpfh(x, nrm, cnt, nbr=nbr, max_dist=md)
    _compare(got, ref, "max_dist %.3f" % md)
    assert not _same_bits(got["counts"], reg.compute_fpfh(x, nrm, cnt, nbr=nbr)["counts"])


def test_ids_strides_and_defaults(dev, demo):
    from dh3d_amd import registration as reg
    K = 17
    x, nrm, cnt, nbr = _inputs(dev, demo, K)
    full = reg.compute_fpfh(x, nrm, cnt, nbr=nbr)
    # ids: the all-points rows gathered; ids outside 0 .. count - 1 give zero rows
    rng = np.random.default_rng(5)
    M = 301
    ids = np.stack([rng.integers(0, n, M) for n in COUNTS]).astype(np.int32)
    ids[:, 7], ids[:, 100], ids[2, 200], ids[0, 300] = -1, N, COUNTS[2], -2 ** 31
    some = reg.compute_fpfh(x, nrm, cnt, nbr=nbr, ids=_t(dev, ids))
    assert some["fpfh"].shape == (3, M, 36) and _same_bits(some["counts"], full["counts"])
    ok = (ids >= 0) & (ids < np.array(COUNTS)[:, None])
    exp = np.where(ok[:, :, None], np.take_along_axis(full["fpfh"].cpu().numpy(), np.where(ok, ids, 0)[:, :, None], axis=1), 0.0)
    assert np.array_equal(some["fpfh"].cpu().numpy().view(np.int32), exp.astype(np.float32).view(np.int32))
    assert not some["fpfh"][:, 7].any() and not some["fpfh"][:, 100].any() and not some["fpfh"][2, 200].any()
    # strided inputs: columns of wider rows are read in place and give the same bits
    wide = torch.full((3, N, 7), 9.0, device=dev)
    wide[:, :, 2:5] = x
    wn = torch.full((3, N, 5), -3.0, device=dev)
    wn[:, :, :3] = nrm
    strided = reg.compute_fpfh(wide[:, :, 2:5], wn[:, :, :3], cnt, nbr=nbr)
    assert strided["normals"].data_ptr() == wn.data_ptr()                        # (no copy was made)
    assert _same_bits(strided["counts"], full["counts"]) and _same_bits(strided["fpfh"], full["fpfh"])
    # nbr=None / normals=None equal the explicit calls (the first two clouds: whole clouds, no padding behind a count)
    from dh3d_amd.utils import batched_knn
    auto = reg.compute_fpfh(x[:2], k=16)
    knn = batched_knn(x[:2].contiguous(), 16)[0]
    n16 = reg.estimate_normals(x[:2], None, 16, (0., 0., 0.))["normals"]
    given = reg.compute_fpfh(x[:2], n16, nbr=knn)
    assert auto["nbr"].shape == (2, N, 16) and torch.equal(auto["nbr"], knn) and _same_bits(auto["normals"], n16)
    assert _same_bits(auto["counts"], given["counts"]) and _same_bits(auto["fpfh"], given["fpfh"])
    sums = auto["fpfh"][:, :, :33].reshape(2, N, 3, 11).sum(dim=3).cpu().numpy()
    assert (np.abs(sums - 200.0) < 1e-3).mean() > 0.95


def test_batch_independence_and_graph_capture(dev, demo):
    from dh3d_amd import registration as reg
    K = 33
    x, nrm, cnt, nbr = _inputs(dev, demo, K)
    ids = _t(dev, np.stack([np.arange(0, N, 3, dtype=np.int32)] * 3))
    full = reg.compute_fpfh(x, nrm, cnt, nbr=nbr, ids=ids, max_dist=1.0)
    for p in range(3):
        s = slice(p, p + 1)
        one = reg.compute_fpfh(x[s], nrm[s], cnt[s], nbr=nbr[s], ids=ids[s], max_dist=1.0)
        assert _same_bits(one["counts"], full["counts"][s]) and _same_bits(one["fpfh"], full["fpfh"][s]), p
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        reg.compute_fpfh(x, nrm, cnt, nbr=nbr, ids=ids, max_dist=1.0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gout = reg.compute_fpfh(x, nrm, cnt, nbr=nbr, ids=ids, max_dist=1.0)
    for _ in range(2):
        gout["counts"].fill_(7)
        gout["fpfh"].fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert _same_bits(gout["counts"], full["counts"]) and _same_bits(gout["fpfh"], full["fpfh"])


@pytest.fixture(scope="module")
def moved():
    """Three pairs: the anchor subset of a demo pair and the same points moved by the inverse of Rt_gt, permuted, with 0.02 m
    of noise (anchor ~ R positive + t); the restatement's normals (k = 16), FPFH rows (K = 32, brute-force ids) and matches."""
    rng = np.random.default_rng(77)
    A, B, T, ref = [], [], [], []
    for name in ("local_642", "global_c", "dso_9000"):
        a, _, Rt, _ = ir.demo_pair(name, N, 1)
        R, t = Rt[:, :3], Rt[:, 3]
        y = ((a.astype(np.float64) - t) @ R + rng.normal(0.0, 0.02, a.shape))[rng.permutation(N)].astype(np.float32)
        side = []
        for c in (a, y):
            ids = pr.knn_ids(c, 32)
            nrm = pr.normals(c, ids[:, :16])["normals"].astype(np.float32)
            r = fr.compute(c, nrm, ids)
            assert (r["margin"] >= 1e-9).all()                                   # a condition on the fixture
            side.append(dict(ids=ids.astype(np.int32), normals=nrm, fpfh=r["fpfh"]))
        m, best, rel = reg_ref.match(side[0]["fpfh"], side[1]["fpfh"])
        A.append(a), B.append(y), T.append(Rt), ref.append(dict(a=side[0], b=side[1], match=m, best=best, rel=rel))
    return dict(A=np.stack(A), B=np.stack(B), T=np.stack(T), ref=ref)


def test_matches_of_a_moved_copy(dev, moved):
    from dh3d_amd import registration as reg
    full = torch.full((3,), N, dtype=torch.int32, device=dev)
    f = []
    for src, key in (("A", "a"), ("B", "b")):
        got = reg.compute_fpfh(_t(dev, moved[src]), _t(dev, np.stack([r[key]["normals"] for r in moved["ref"]])),
                               nbr=_t(dev, np.stack([r[key]["ids"] for r in moved["ref"]])))
        err = max(np.abs(got["fpfh"][p].cpu().numpy().astype(np.float64) - moved["ref"][p][key]["fpfh"]).max() for p in range(3))
        print(src, "fpfh max error %.3g" % err)
        assert err <= TOL
        f.append(got["fpfh"])
    match, dist = reg.match_descriptors(f[0], full, f[1], full)
    match = match.cpu().numpy()
    for p, r in enumerate(moved["ref"]):
        second = r["best"] / np.maximum(1.0 - r["rel"], 1e-30)
        sure = (second - r["best"]) > 4.6e-4 + 2.3e-6 * (r["best"] + second)
        print("pair", p, "matches left out", int(N - sure.sum()), "differing", int((match[p] != r["match"]).sum()))
        assert N - sure.sum() <= 0.01 * N, p
        assert np.array_equal(match[p][sure], r["match"][sure]), p


def test_register_fpfh_end_to_end(dev, moved):
    from dh3d_amd import registration as reg
    a, b = _t(dev, moved["A"]), _t(dev, moved["B"])
    res = reg.register_fpfh(a, b)
    for key in ("Rt", "valid", "inliers", "num_inliers", "inlier_ratio", "trials", "num_corr", "match", "dist"):
        assert key in res, key
    assert res["anchor_ids"] is None and res["match"].shape == (3, N) and bool(res["valid"].all())
    dt, dd = reg.transform_errors(moved["T"], res["Rt"], res["valid"])
    print("ransac: dt", dt, "ddeg", dd, "inlier ratio", res["inlier_ratio"].cpu().numpy())
    assert (dt < 2.0).all() and (dd < 5.0).all(), (dt, dd)                          # eval_align.m's failure thresholds
    fine = reg.register_fpfh(a, b, refine=True)
    for key in ("Rt_ransac", "fitness", "rmse", "num_corr_icp", "nn"):
        assert key in fine, key
    assert torch.equal(fine["Rt_ransac"], res["Rt"]) and bool(fine["valid"].all())
    dt2, dd2 = reg.transform_errors(moved["T"], fine["Rt"], fine["valid"])
    print("refined: dt", dt2, "ddeg", dd2, "fitness", fine["fitness"].cpu().numpy())
    assert (dt2 <= dt).all() and (dd2 <= dd).all(), (dt, dt2, dd, dd2)
    # keypoints: 512 of the points spread over each cloud, and the same ids given by the caller (-1 padded)
    few = reg.register_fpfh(a, b, keypoints=512)
    assert few["match"].shape == (3, 512) and few["anchor_ids"].shape == (3, 512)
    exp = (torch.arange(512, device=dev) * N // 512).to(torch.int32)
    assert torch.equal(few["anchor_ids"][1], exp) and torch.equal(few["positive_ids"][2], exp)
    assert (few["num_corr"].cpu().numpy() == 512).all()
    ids = torch.full((3, 600), -1, dtype=torch.int32, device=dev)
    ids[:, :512] = exp
    mine = reg.register_fpfh(a, b, keypoint_ids=ids)
    assert (mine["num_corr"].cpu().numpy() == 512).all() and torch.equal(mine["match"][:, :512], few["match"])
    for r in (few, mine):
        kdt, kdd = reg.transform_errors(moved["T"], r["Rt"], r["valid"])
        print("512 keypoints: dt", kdt, "ddeg", kdd)      # (printed, not asserted: the two keypoint sets share few points)
    assert torch.equal(mine["valid"], few["valid"])
    # counts: the third pair cut to its first 1024 anchor rows still registers
    nv = (torch.tensor([N, N, 1024], dtype=torch.int32, device=dev), torch.full((3,), N, dtype=torch.int32, device=dev))
    cut = reg.register_fpfh(a, b, num_valid=nv)
    assert cut["num_corr"].cpu().numpy().tolist() == [N, N, 1024] and torch.equal(cut["match"][:2], res["match"][:2])
