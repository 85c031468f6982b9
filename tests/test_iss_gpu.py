"""GPU: ISS keypoints on the device (dh3d_amd.registration.iss_keypoints -> csrc/iss.hip) against the numpy restatement of
the rule (tests/iss_reference.py), and register_fpfh with the detector in front, end to end.

The fixtures are iss_reference.CASES: clouds of at most 2048 points, run in batches of at most 6 -- the five natural clouds
at 2.0 / 1.5 m (one of them behind a count of 1024 with rows of 100000.0 after it), the same at 12.0 / 9.0 m (boxes of more
than 512 cells: the group walk), a uniform cube at 5.0 / 4.0 m and a lattice whose shells lie at exactly d2 == r^2.

Tolerances.  The counts are integers of a float32 rule stated operation by operation: bit-equal.  The eigenvalues: each
entry of S2 / m is below r_s^2, a float64 sum of m <= 2048 terms errs by at most m * 2^-53 * r_s^2 = 2.3e-13 r_s^2 and the
solve adds a few units of that: 1e-12 r_s^2 (reusing the float32 differences of the membership test moves them by 2e-8
r_s^2).  The saliency's sign is compared where the restatement's decision margin is at least 4e-12 (tests/
test_iss_reference.py shows that this is every row of every fixture; at most 0.5 % of a cloud's rows may be left out), its
value at 1e-12 r_s^2 plus one float32 ulp.  Suppression and selection are exact: bit-equal to the restatement's steps 4 and 5
run on the GPU's own saliency and counts."""
import numpy as np
import pytest
import torch

import iss_reference as ref

pytestmark = pytest.mark.gpu

N = ref.N_DEMO
GROUPS = {  # group -> the cases of one call (one radius pair, at most 6 clouds of one size)
    "small": tuple(c for c in ref.CASE_IDS if c.endswith("-small")),
    "wide": tuple(c for c in ref.CASE_IDS if c.endswith("-wide")),
    "cube": ("cube-5-4",),
    "lattice": ("lattice",),
}
GROUP_OF = {c: g for g, cs in GROUPS.items() for c in cs}
NATURAL = tuple(c for c in ref.CASE_IDS if c != "lattice")
_GPU = {}


def _t(dev, v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _batch(dev, group):
    cases = [ref.case(c) for c in GROUPS[group]]
    x = _t(dev, np.stack([c[0] for c in cases]))
    cnt = _t(dev, np.array([c[1] for c in cases], np.int32))
    return x, cnt, cases[0][2], cases[0][3]


def _gpu(dev, group, M=4096):
    """One call per (group, M), kept as numpy arrays."""
    if (group, M) not in _GPU:
        from dh3d_amd import registration as reg
        x, cnt, r_s, r_n = _batch(dev, group)
        out = reg.iss_keypoints(x, cnt, r_s, r_n, max_keypoints=M, eigenvalues=True)
        _GPU[(group, M)] = {k: v.cpu().numpy() for k, v in out.items()}
    return _GPU[(group, M)]


def _mine(dev, case_id, M=4096):
    g = GROUP_OF[case_id]
    p = GROUPS[g].index(case_id)
    return {k: v[p] for k, v in _gpu(dev, g, M).items()}


@pytest.mark.parametrize("case_id", ref.CASE_IDS)
def test_counts_are_bit_equal(dev, case_id):
    X, n, r_s, r_n, res = ref.case(case_id)
    got = _mine(dev, case_id)
    assert got["num_neighbors"].dtype == np.int32 and got["num_neighbors"].shape == (len(X), 2)
    diff = int((got["num_neighbors"] != res["num_nbr"]).any(axis=1).sum())
    print(case_id, "rows with another count:", diff, "; largest |S|", res["num_nbr"][:, 0].max(), "|T|", res["num_nbr"][:, 1].max())
    assert diff == 0
    assert np.array_equal(got["radii"], np.array([r_s, r_n], np.float32))


@pytest.mark.parametrize("case_id", NATURAL)
def test_eigenvalues(dev, case_id):
    X, n, r_s, r_n, res = ref.case(case_id)
    got = _mine(dev, case_id)
    assert got["eigenvalues"].dtype == np.float64 and got["eigenvalues"].shape == (len(X), 3)
    err = np.abs(got["eigenvalues"][:n] - res["lam"][:n]).max() / r_s ** 2         # (every valid row has m >= 1: itself)
    print(case_id, "max |lam_gpu - lam_ref| / r_s^2 = %.3g" % err)
    assert err <= 1e-12
    assert not got["eigenvalues"][n:].any()


@pytest.mark.parametrize("case_id", NATURAL)
def test_saliency(dev, case_id):
    X, n, r_s, r_n, res = ref.case(case_id)
    s = _mine(dev, case_id)["saliency"]
    assert s.dtype == np.float32 and not s[n:].any() and not np.signbit(s).any()
    sure = res["margin"][:n] >= 4e-12
    print(case_id, "rows left out:", int(n - sure.sum()), "; positive:", int((s > 0).sum()), "of", n)
    assert n - sure.sum() <= 0.005 * n
    assert np.array_equal((s[:n] > 0)[sure], (res["saliency"][:n] > 0)[sure])
    both = (s[:n] > 0) & (res["saliency"][:n] > 0)
    err = np.abs(s[:n][both].astype(np.float64) - res["saliency"][:n][both].astype(np.float64))
    tol = 1e-12 * r_s ** 2 + np.spacing(res["saliency"][:n][both]).astype(np.float64)
    print(case_id, "largest saliency error %.3g; bit-equal rows: %d of %d" % (err.max(), int((err == 0).sum()), int(both.sum())))
    assert (err <= tol).all()


@pytest.mark.parametrize("M", (4096, 16))
@pytest.mark.parametrize("case_id", NATURAL)
def test_selection_is_exact(dev, case_id, M):
    X, n, r_s, r_n, res = ref.case(case_id)
    got = _mine(dev, case_id, M)
    ids, count = ref.keypoints(X, n, r_n, got["saliency"], got["num_neighbors"][:, 1], M)
    print(case_id, "M", M, "keypoints", int(got["count"]), "expected", count)
    assert got["ids"].dtype == np.int32 and got["ids"].shape == (M,)
    assert int(got["count"]) == count and np.array_equal(got["ids"], ids)
    if M == 16 and case_id.endswith("-small"):
        assert count == 16                                                        # more maxima than slots: the 16 most salient


@pytest.mark.parametrize("name", ("global_c", "dso_9000"))
def test_plateaus(dev, name):
    from dh3d_amd import registration as reg
    X, n = ref.cloud(name)
    rng = np.random.default_rng(411)
    sal = rng.integers(0, 4, N).astype(np.float32)                               # plateaus: values in {0, 1, 2, 3}
    odd = rng.choice(N, 150, replace=False)
    sal[odd[:50]], sal[odd[50:100]], sal[odd[100:]] = -1.0, -0.0, np.nan
    s_in = _t(dev, sal[None])
    for M in (4096, 16):
        out = reg.iss_keypoints(_t(dev, X[None]), None, 2.0, 1.5, max_keypoints=M, saliency=s_in)
        assert _same_bits(out["saliency"], s_in) and out["eigenvalues"] is None
        num = out["num_neighbors"][0].cpu().numpy()
        assert np.array_equal(num, ref.case(name + "-small")[4]["num_nbr"])
        key, tie = ref.keypoint_mask(X, n, 1.5, sal, num[:, 1])
        ids, count = ref.select(key, sal, M)
        print(name, "M", M, "keypoints", count, "decided by the tie rule", int(tie.sum()))
        assert tie.sum() >= 100 and count >= 16
        assert int(out["count"][0]) == count and np.array_equal(out["ids"][0].cpu().numpy(), ids)


def test_strided_view_and_one_cloud_alone(dev):
    from dh3d_amd import registration as reg
    x, cnt, r_s, r_n = _batch(dev, "small")
    full = reg.iss_keypoints(x, cnt, r_s, r_n, eigenvalues=True)
    wide = torch.full((x.shape[0], N, 6), 7.0, device=dev)
    wide[:, :, 2:5] = x
    view = reg.iss_keypoints(wide[:, :, 2:5], cnt, r_s, r_n, eigenvalues=True)
    for k in ("ids", "count", "saliency", "num_neighbors", "eigenvalues"):
        assert _same_bits(view[k], full[k]), k
    # one cloud alone, over a workspace filled with 0xFF, equals its row in the batch
    for p in (1, 4):
        one = reg.iss_keypoints(x[p:p + 1], cnt[p:p + 1], r_s, r_n, eigenvalues=True)     # (creates the P = 1 workspace)
        reg._ISS_WS[(x.device, 1, N, 4096)].fill_(0xFF)
        again = reg.iss_keypoints(x[p:p + 1], cnt[p:p + 1], r_s, r_n, eigenvalues=True)
        for k in ("ids", "count", "saliency", "num_neighbors", "eigenvalues"):
            assert _same_bits(one[k], full[k][p:p + 1]) and _same_bits(again[k], full[k][p:p + 1]), (p, k)


def test_empty_and_tiny_clouds_and_a_zero_radius(dev):
    from dh3d_amd import registration as reg
    X = ref.cloud("dso_9000_cut")[0]
    x = _t(dev, np.stack([X] * 5))
    x[4] = _t(dev, ref.cloud("global_c")[0])
    cnt = torch.tensor([0, 1, 4, 1024, N], dtype=torch.int32, device=dev)
    rs = torch.tensor([2.0, 2.0, 2.0, 0.0, float("nan")], device=dev)
    rn = torch.tensor([1.5, 1.5, 1.5, 1.5, 1.5], device=dev)
    out = reg.iss_keypoints(x, cnt, rs, rn, max_keypoints=64, eigenvalues=True)
    assert out["count"].cpu().tolist() == [0] * 5 and bool((out["ids"] == -1).all())
    assert not out["saliency"].any() and not torch.signbit(out["saliency"]).any()
    num = out["num_neighbors"].cpu().numpy()
    assert not num[0].any() and num[1, 0].tolist() == [1, 1] and not num[1, 1:].any()
    assert (num[2, :4] >= 1).all() and not num[2, 4:].any()
    assert not num[3, :, 0].any() and np.array_equal(num[3, :, 1], ref.case("dso_9000_cut-small")[4]["num_nbr"][:, 1])
    assert not num[4, :, 0].any() and np.array_equal(num[4, :, 1], ref.case("global_c-small")[4]["num_nbr"][:, 1])
    # a zero non-max radius: saliencies as ever, no keypoints
    out = reg.iss_keypoints(x[4:], None, 2.0, 0.0, max_keypoints=64)
    assert int(out["count"][0]) == 0 and bool((out["ids"] == -1).all()) and not out["num_neighbors"][0, :, 1].any()
    assert np.array_equal(out["saliency"][0].cpu().numpy() > 0, ref.case("global_c-small")[4]["saliency"] > 0)


def test_radii_tensors_resolution_and_defaults(dev):
    from dh3d_amd import registration as reg
    x, cnt, r_s, r_n = _batch(dev, "small")
    P = x.shape[0]
    full = reg.iss_keypoints(x, cnt, r_s, r_n)
    given = reg.iss_keypoints(x, cnt, torch.full((P,), r_s, device=dev), torch.full((P,), r_n, device=dev))
    for k in ("ids", "count", "saliency", "num_neighbors", "radii"):
        assert _same_bits(given[k], full[k]), k
    res = reg.cloud_resolution(x, cnt)
    assert res.dtype == torch.float32 and res.shape == (P,)
    for p, case_id in enumerate(GROUPS["small"]):
        X, n = ref.case(case_id)[:2]
        d = np.linalg.norm(X[None, :n].astype(np.float64) - X[:n, None].astype(np.float64), axis=2)
        d[np.arange(n), np.arange(n)] = np.inf
        want = d.min(1).mean()
        print(case_id, "resolution", float(res[p]), "numpy", want)
        assert abs(float(res[p]) - want) <= 1e-6 * want
    assert reg.cloud_resolution(x[:2], torch.tensor([0, 1], dtype=torch.int32, device=dev)).cpu().tolist() == [0.0, 0.0]
    auto = reg.iss_keypoints(x, cnt)
    mine = reg.iss_keypoints(x, cnt, res * 6.0, res * 4.0)
    assert _same_bits(auto["radii"], torch.stack((res * 6.0, res * 4.0), 1))
    for k in ("ids", "count", "saliency", "num_neighbors"):
        assert _same_bits(auto[k], mine[k]), k
    assert int(auto["count"].min()) > 0


def test_graph_capture(dev):
    from dh3d_amd import registration as reg
    x, cnt, r_s, r_n = _batch(dev, "small")
    radius = (torch.full((x.shape[0],), r_s, device=dev), torch.full((x.shape[0],), r_n, device=dev))
    # the eager call is the warm-up too: it loads the kernels and creates the workspace of this shape, so the capture
    # allocates nothing but its outputs (no stream of the test's own: the suite's later graph tests see the streams and
    # the freed memory they would see without this test)
    eager = reg.iss_keypoints(x, cnt, *radius, max_keypoints=256, eigenvalues=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gout = reg.iss_keypoints(x, cnt, *radius, max_keypoints=256, eigenvalues=True)
    for _ in range(2):
        for k in ("ids", "count", "num_neighbors"):
            gout[k].fill_(7)
        gout["saliency"].fill_(7.0)
        gout["eigenvalues"].fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        for k in ("ids", "count", "saliency", "num_neighbors", "eigenvalues"):
            assert _same_bits(gout[k], eager[k]), k
    for t in gout.values():                                                         # the graph's pool goes back zeroed
        t.zero_()
    torch.cuda.synchronize()


def test_register_fpfh_with_iss_end_to_end(dev):
    from dh3d_amd import registration as reg
    A, B, T = ref.moved_pairs()
    a, b = _t(dev, A), _t(dev, B)
    kw = {"method": "iss", "salient_radius": 2.0, "non_max_radius": 1.5}
    res = reg.register_fpfh(a, b, keypoints=kw)
    assert bool(res["valid"].all())
    dt, dd = reg.transform_errors(T, res["Rt"], res["valid"])
    ka = reg.iss_keypoints(a, None, 2.0, 1.5)
    kb = reg.iss_keypoints(b, None, 2.0, 1.5)
    print("keypoints", ka["count"].cpu().tolist(), kb["count"].cpu().tolist(), "inlier ratio", res["inlier_ratio"].cpu().numpy())
    print("ransac: dt", dt, "ddeg", dd)
    assert torch.equal(res["anchor_ids"], ka["ids"]) and torch.equal(res["positive_ids"], kb["ids"])
    assert torch.equal(res["num_corr"], ka["count"]) and res["match"].shape == (3, 4096)
    assert (dt < 2.0).all() and (dd < 5.0).all(), (dt, dd)                         # eval_align.m's failure thresholds
    fine = reg.register_fpfh(a, b, keypoints=(kw, dict(kw)), refine=True)
    assert torch.equal(fine["Rt_ransac"], res["Rt"]) and bool(fine["valid"].all())
    dt2, dd2 = reg.transform_errors(T, fine["Rt"], fine["valid"])
    print("refined: dt", dt2, "ddeg", dd2, "fitness", fine["fitness"].cpu().numpy())
    assert (dt2 <= dt).all() and (dd2 <= dd).all(), (dt, dt2, dd, dd2)
    with pytest.raises(ValueError, match="method"):
        reg.register_fpfh(a, b, keypoints={"method": "nope"})
