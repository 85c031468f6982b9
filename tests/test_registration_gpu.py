"""GPU: descriptor matching and batched RANSAC registration (dh3d_amd.registration -> csrc/registration.hip) against the
float64 restatement of the MATLAB loop (tests/registration_reference.py): equal ids, trial counts, inlier masks and
validity, poses within 1e-9; pose recovery on real keypoint geometry; batch independence; graph capture; and the model's
keypoints end to end."""
import math
import os

import numpy as np
import pytest
import torch

import registration_reference as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _unit(rng, shape):
    v = rng.standard_normal(shape)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _rot(yaw, pitch=0.0, roll=0.0):
    cz, sz, cy, sy, cx, sx = (math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll),
                              math.sin(roll))
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return Rz @ Ry @ Rx


def _random_pose(rng):
    R = _rot(rng.uniform(-math.pi, math.pi), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1))
    t = rng.standard_normal(3)
    t = t / np.linalg.norm(t) * rng.uniform(0.0, 10.0)
    return R, t


# ------------------------------------------------------------------------------------------------------------ matching

def test_matching_against_float64_argmin(dev):
    from dh3d_amd import registration as reg
    rng = np.random.default_rng(0)
    M, D = 4096, 128
    counts = [(0, 50), (1, 1), (3, 3), (512, 512), (4096, 4096), (700, 37), (40, 0)]
    P = len(counts)
    a = _unit(rng, (P, M, D))
    b = _unit(rng, (P, M, D))
    # planted duplicates: positive rows 5 and 9 (and 20, 21, 30) equal, anchors close to them
    for p in (3, 4):
        b[p, 9] = b[p, 5]
        b[p, 21] = b[p, 20]
        b[p, 30] = b[p, 20]
        a[p, 0] = _unit(rng, (D,)) * 0.01 + b[p, 5]
        a[p, 1] = _unit(rng, (D,)) * 0.01 + b[p, 20]
        a[p, 2] = b[p, 30]
    # rows as the keypoint maps hold them: [xyz | desc | score], read in place through a column view
    rows_a = torch.from_numpy(np.concatenate([np.zeros((P, M, 3), np.float32), a, np.ones((P, M, 1), np.float32)], -1))
    rows_b = torch.from_numpy(np.concatenate([np.zeros((P, M, 3), np.float32), b, np.ones((P, M, 1), np.float32)], -1))
    rows_a, rows_b = rows_a.to(dev), rows_b.to(dev)
    ac = torch.tensor([c[0] for c in counts], dtype=torch.int32, device=dev)
    bc = torch.tensor([c[1] for c in counts], dtype=torch.int32, device=dev)
    match, dist = reg.match_descriptors(rows_a[:, :, 3:131], ac, rows_b[:, :, 3:131], bc)
    match, dist = match.cpu().numpy(), dist.cpu().numpy()
    for p, (na, nb) in enumerate(counts):
        assert (match[p, na:] == -1).all() and np.isinf(dist[p, na:]).all(), p
        if nb == 0:
            assert (match[p] == -1).all() and np.isinf(dist[p]).all(), p
            continue
        ids, best, rel = ref.match(a[p, :na], b[p, :nb])
        clear = rel > 1e-5
        assert (match[p, :na][clear] == ids[clear]).all(), (p, int((match[p, :na][clear] != ids[clear]).sum()))
        assert ((match[p, :na] >= 0) & (match[p, :na] < nb)).all(), p
        assert na == 0 or np.abs(dist[p, :na] - best).max() < 1e-5, p
    for p in (3, 4):
        assert match[p, 0] == 5 and match[p, 1] == 20 and match[p, 2] == 20, match[p, :3]


# -------------------------------------------------------------------------------------------------------------- RANSAC

def _corr_fixture(rng, n, ratio, noise=0.05, side=40.0):
    """n correspondences, a `ratio` share of them true (5 cm noise), the rest random points of the box."""
    R, t = _random_pose(rng)
    x = rng.random((n, 3)) * side - side / 2
    y = (x - t) @ R + rng.normal(0.0, noise, (n, 3))
    out = rng.random(n) >= ratio
    y[out] = rng.random((int(out.sum()), 3)) * side - side / 2
    return x.astype(np.float32), y.astype(np.float32)


def _clear_fixture(n, ratio, threshold, seed, base):
    """The first fixture (seeds base, base + 1, ...) whose evaluated hypotheses keep 1e-7 from the threshold, an eigen gap
    of 1e-6 and every N_k 1e-9 from an integer: no result of the comparison depends on a last-bit rounding."""
    for s in range(base, base + 50):
        x, y = _corr_fixture(np.random.default_rng(s), n, ratio)
        r = ref.ransac(x, y, threshold=threshold, seed=seed)
        if r["margin"] > 1e-7 and r["gap"] > 1e-6 and r["n_frac"] > 1e-9:
            return x, y, r
    raise AssertionError("no clear fixture for n=%d ratio=%g" % (n, ratio))


def _run_batch(dev, fixtures, M, threshold, seed, perm_seed=0):
    """Pack (x, y) pairs into a [P, M] batch with the positives shuffled behind the match ids; run ransac_rigid."""
    from dh3d_amd import registration as reg
    rng = np.random.default_rng(perm_seed)
    P = len(fixtures)
    ax = np.zeros((P, M, 3), np.float32)
    bx = np.full((P, M, 3), 1e6, np.float32)
    match = np.full((P, M), -1, np.int32)
    cnt = np.zeros(P, np.int32)
    for p, (x, y) in enumerate(fixtures):
        n = len(x)
        perm = rng.permutation(M)[:n]
        ax[p, :n] = x
        bx[p, perm] = y
        match[p, :n] = perm
        cnt[p] = n
    t = lambda v: torch.from_numpy(v).to(dev)
    out = reg.ransac_rigid(t(ax), t(bx), t(match), t(cnt), threshold=threshold, seed=seed)
    return {k: v.cpu().numpy() for k, v in out.items()}


CASES = [(0, 0.5), (2, 0.5), (3, 1.0), (4, 0.75), (10, 0.6), (512, 0.05), (512, 0.3), (512, 0.9), (4096, 0.5),
         (4096, 0.05)]  # (at 4096 x 0.05 every threshold but 1.0 takes 0.2: the restatement's 10001 trials cost seconds)


@pytest.mark.parametrize("threshold,seed", [(1.0, 0), (0.5, 7), (2.0, 2 ** 63 + 5)])
def test_ransac_against_restatement(dev, threshold, seed):
    fixtures, exp = [], []
    for c, (n, ratio) in enumerate(CASES):
        ratio = 0.2 if (n, ratio) == (4096, 0.05) and threshold != 1.0 else ratio
        x, y, r = _clear_fixture(n, ratio, threshold, seed, base=1000 * c + int(threshold * 10))
        fixtures.append((x, y))
        exp.append(r)
    got = _run_batch(dev, fixtures, 4096, threshold, seed)
    for p, r in enumerate(exp):
        n = len(fixtures[p][0])
        what = (p, CASES[p])
        assert got["num_corr"][p] == n, what
        assert got["trials"][p] == r["trials"], (what, got["trials"][p], r["trials"])
        assert got["num_inliers"][p] == r["num_inliers"], (what, got["num_inliers"][p], r["num_inliers"])
        assert bool(got["valid"][p]) == r["valid"], what
        assert (got["inliers"][p, :n] == r["mask"]).all() and not got["inliers"][p, n:].any(), what
        if r["valid"]:
            assert np.abs(got["Rt"][p] - r["Rt"]).max() < 1e-9, (what, np.abs(got["Rt"][p] - r["Rt"]).max())
            assert got["inlier_ratio"][p] == r["num_inliers"] / n
        else:
            assert np.isnan(got["Rt"][p]).all(), what
    assert any(r["trials"] == 10001 for r in exp) and any(r["trials"] == 10 for r in exp)


# ------------------------------------------------------------------------------------------ recovery on real geometry

def _keypoint_pairs(rng, P, M=512, D=128, outlier_max=0.8):
    """Anchor keypoints drawn from the demo cloud's FPS points; positives R^T (x - t) + 5 cm noise, shuffled, with matching
    descriptors except for an outlier share (0 - 80 %) whose anchors get unrelated descriptors."""
    demo = np.load(os.path.join(HERE, "golden", "demo_clouds.npz"))
    pts = demo["local_642"][demo["local_642/fps_idx"]].astype(np.float64)
    rows_a = np.zeros((P, M, 3 + D + 1), np.float32)
    rows_b = np.zeros((P, M, 3 + D + 1), np.float32)
    T = np.zeros((P, 3, 4))
    for p in range(P):
        R, t = _random_pose(rng)
        x = pts[rng.choice(len(pts), M, replace=False)]
        y = (x - t) @ R + rng.normal(0.0, 0.05, (M, 3))
        da = _unit(rng, (M, D))
        db = da + 0.01 * rng.standard_normal((M, D)).astype(np.float32)
        out = rng.random(M) < rng.uniform(0.0, outlier_max)
        da[out] = _unit(rng, (int(out.sum()), D))
        perm = rng.permutation(M)
        rows_a[p, :, :3], rows_a[p, :, 3:3 + D] = x, da
        rows_b[p, perm, :3], rows_b[p, perm, 3:3 + D] = y, db
        T[p] = np.concatenate([R, t[:, None]], axis=1)
    return rows_a, rows_b, T


def test_recovery_on_demo_keypoints(dev):
    from dh3d_amd import registration as reg
    rng = np.random.default_rng(5)
    P, M = 24, 512
    ra, rb, T = _keypoint_pairs(rng, P, M)
    cnt = torch.full((P,), M, dtype=torch.int32, device=dev)
    res = reg.register(torch.from_numpy(ra).to(dev), cnt, torch.from_numpy(rb).to(dev), cnt)
    dt, dd = reg.transform_errors(T, res["Rt"], res["valid"])
    assert (dt < 0.1).all() and (dd < 1.0).all(), (dt.max(), dd.max())
    s = reg.summarize_registration(dt, dd, res["inlier_ratio"], res["trials"])
    assert s["success_rate"] == 100.0 and s["mean_inlier_ratio"] > 0.2


def test_batch_independence(dev):
    """Every pair's outputs are the same alone and inside a P = 64 batch with mixed counts."""
    from dh3d_amd import registration as reg
    rng = np.random.default_rng(6)
    P, M = 64, 512
    ra, rb, _ = _keypoint_pairs(rng, P, M, outlier_max=0.9)
    ca = rng.integers(0, M + 1, P).astype(np.int32)
    cb = rng.integers(0, M + 1, P).astype(np.int32)
    ca[:6] = [0, 1, 2, 3, 4, M]
    cb[6:9] = [0, 1, M]
    A, B = torch.from_numpy(ra).to(dev), torch.from_numpy(rb).to(dev)
    CA, CB = torch.from_numpy(ca).to(dev), torch.from_numpy(cb).to(dev)
    full = reg.register(A, CA, B, CB, seed=3)
    for p in range(P):
        one = reg.register(A[p:p + 1], CA[p:p + 1], B[p:p + 1], CB[p:p + 1], seed=3)
        for k, v in one.items():
            w = full[k][p:p + 1]
            if v.dtype == torch.float64:
                assert torch.equal(v.view(torch.int64), w.view(torch.int64)), (p, k)  # (bit for bit, NaN included)
            elif v.dtype == torch.float32:
                assert torch.equal(v.view(torch.int32), w.view(torch.int32)), (p, k)
            else:
                assert torch.equal(v, w), (p, k)
    assert int(full["valid"].sum()) > 20


def test_graph_capture_replays_on_new_inputs(dev):
    from dh3d_amd import registration as reg
    P, M = 16, 512
    ra, rb, _ = _keypoint_pairs(np.random.default_rng(7), P, M)
    sa, sb = torch.from_numpy(ra).to(dev), torch.from_numpy(rb).to(dev)
    sca = torch.full((P,), M, dtype=torch.int32, device=dev)
    scb = sca.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        reg.register(sa, sca, sb, scb)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gout = reg.register(sa, sca, sb, scb)
    for seed in (8, 9):
        r = np.random.default_rng(seed)
        na, nb, _ = _keypoint_pairs(r, P, M)
        ca = torch.from_numpy(r.integers(M // 2, M + 1, P).astype(np.int32)).to(dev)
        a, b = torch.from_numpy(na).to(dev), torch.from_numpy(nb).to(dev)
        sa.copy_(a)
        sb.copy_(b)
        sca.copy_(ca)
        scb.copy_(ca)
        g.replay()
        eout = reg.register(a, ca, b, ca)
        torch.cuda.synchronize()
        for k in eout:
            e, c = eout[k], gout[k]
            if e.dtype == torch.float64:
                assert torch.equal(e.view(torch.int64), c.view(torch.int64)), k
            else:
                assert torch.equal(e, c), k


# ------------------------------------------------------------------------------------------------------------ end to end

@pytest.fixture(scope="module")
def det_model(dev):
    from dh3d_amd import ConfigFactory
    from dh3d_amd.model import DH3D
    return DH3D(ConfigFactory("detection_config").getconfig()).init_synthetic(0).to(dev).eval().prepare()


def test_register_clouds_end_to_end(dev, det_model):
    from dh3d_amd import registration as reg
    demo = np.load(os.path.join(HERE, "golden", "demo_clouds.npz"))
    X = torch.from_numpy(np.stack([demo["local_268"], demo["local_642"]]).astype(np.float32)).to(dev)
    outs = det_model.forward(X, fetch=("kp_count", "xyz_feat_att_nms"))
    rows, count = outs["xyz_feat_att_nms"].cpu().numpy(), outs["kp_count"].cpu().numpy()
    for p in range(2):
        desc = rows[p, :count[p], 3:131]
        assert count[p] >= 3 and len(np.unique(desc, axis=0)) == count[p]  # no twin descriptors: the tie rule cannot bite
    res = reg.register_clouds(det_model, X, X)
    Rt = res["Rt"].cpu().numpy()
    assert res["valid"].all()
    assert np.abs(Rt[:, :, :3] - np.eye(3)).max() < 1e-9 and np.abs(Rt[:, :, 3]).max() < 1e-6
    assert (res["inlier_ratio"] == 1.0).all() and (res["trials"] == 10).all()
    assert torch.equal(res["match"][0, :count[0]].cpu(), torch.arange(int(count[0]), dtype=torch.int32))
    # local_268 against local_642: register_clouds == forward + register, bit for bit
    A, B = X[:1], X[1:]
    got = reg.register_clouds(det_model, A, B)
    oa = det_model.forward(A, fetch=("kp_count", "xyz_feat_att_nms"))
    ob = det_model.forward(B, fetch=("kp_count", "xyz_feat_att_nms"))
    exp = reg.register(oa["xyz_feat_att_nms"], oa["kp_count"], ob["xyz_feat_att_nms"], ob["kp_count"])
    for k in exp:
        e, g = exp[k], got[k]
        if e.dtype == torch.float64:
            assert torch.equal(e.view(torch.int64), g.view(torch.int64)), k
        else:
            assert torch.equal(e, g), k
