"""GPU: place retrieval (dh3d_amd.retrieval -> csrc/retrieval.hip) against the float64 restatement
(tests/retrieval_reference.py): ids and squared distances bit for bit in both launch regimes (one slice, S slices + merge),
on tie-heavy maps, with a device-side fill level, alone and in a batch, under graph capture, as the evaluation's backend, and
the relocalisation loop of PlaceIndex.localize against registration.register on the single pair."""
import math
import os

import numpy as np
import pytest
import torch

import retrieval_reference as rr

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _unit(rng, shape):
    v = rng.standard_normal(shape)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _random_pose(rng):
    """A rotation (any yaw, pitch and roll within 0.1 rad) and a translation of up to 10 m."""
    yaw, pitch, roll = rng.uniform(-math.pi, math.pi), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)
    cz, sz, cy, sy, cx, sx = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    t = rng.standard_normal(3)
    return Rz @ Ry @ Rx, t / np.linalg.norm(t) * rng.uniform(0.0, 10.0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_equal(got, exp, what=None):
    gi, gd = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert gi.dtype == np.int32 and gd.dtype == np.float64 and gi.shape == exp[0].shape
    assert np.array_equal(gi, exp[0]), what
    assert np.array_equal(_bits(gd), _bits(exp[1])), what


def _search(dev, ref, qry, k, count=None):
    from dh3d_amd import retrieval
    rc = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    return retrieval.search_descriptors_sq(torch.from_numpy(ref).to(dev), torch.from_numpy(qry).to(dev), k, rc)


def _first_split(Q, D, k):
    """The smallest R at which the plan cuts the map into slices for Q queries -- asked of the plan, not guessed."""
    from dh3d_amd import retrieval
    for R in range(1, 8193):
        if retrieval.retrieve_plan(Q, R, D, k)[0] >= 2:
            return R
    raise AssertionError("no split up to R = 8192 for Q = %d" % Q)


@pytest.mark.parametrize("Q,R,D,k", [(1, 1, 4, 1), (1, 5, 4, 8), (17, 33, 8, 5), (16, 256, 256, 25), (40, 5000, 256, 25)])
def test_bit_equal_to_the_restatement(dev, Q, R, D, k):
    rng = np.random.default_rng(Q * 1000 + R)
    ref = rng.standard_normal((R, D)).astype(np.float32)
    qry = rng.standard_normal((Q, D)).astype(np.float32)
    exp = rr.topk(ref, qry, k)
    got = _search(dev, ref, qry, k)
    _assert_equal(got, exp)
    if k > R:
        assert (exp[0][:, R:] == -1).all() and np.isinf(exp[1][:, R:]).all()   # the tail the kernel had to write


def test_column_views_are_read_in_place(dev):
    from dh3d_amd import retrieval
    rng = np.random.default_rng(1)
    Q, R, D, k = 3, 257, 128, 64
    ref = rng.standard_normal((R, 132)).astype(np.float32)
    qry = rng.standard_normal((Q, 132)).astype(np.float32)
    tr, tq = torch.from_numpy(ref).to(dev), torch.from_numpy(qry).to(dev)
    got = retrieval.search_descriptors_sq(tr[:, 3:131], tq[:, 3:131], k)
    _assert_equal(got, rr.topk(ref[:, 3:131], qry[:, 3:131], k))
    idx, dist = retrieval.search_descriptors(tr[:, 3:131], tq[:, 3:131], k)
    assert torch.equal(idx, got[0]) and torch.equal(dist, got[1].sqrt())


@pytest.mark.parametrize("Q", [1, 33])
def test_smallest_split_map(dev, Q):
    from dh3d_amd import retrieval
    D, k = 64, 25
    R = _first_split(Q, D, k)
    assert retrieval.retrieve_plan(Q, R, D, k)[0] >= 2 and retrieval.retrieve_plan(Q, R - 1, D, k)[0] == 1
    rng = np.random.default_rng(R + Q)
    ref = rng.standard_normal((R, D)).astype(np.float32)
    qry = rng.standard_normal((Q, D)).astype(np.float32)
    _assert_equal(_search(dev, ref, qry, k), rr.topk(ref, qry, k))
    _assert_equal(_search(dev, ref[:R - 1], qry, k), rr.topk(ref[:R - 1], qry, k))   # and the last unsplit one


@pytest.mark.parametrize("Q,R", [(5, 200), (5, 1500)])
def test_identical_rows_come_back_in_id_order(dev, Q, R):
    D, k = 16, 25
    ref = np.tile(np.random.default_rng(2).standard_normal((1, D)).astype(np.float32), (R, 1))
    qry = np.random.default_rng(3).standard_normal((Q, D)).astype(np.float32)
    idx, d2 = _search(dev, ref, qry, k)
    assert np.array_equal(idx.cpu().numpy(), np.tile(np.arange(k, dtype=np.int32), (Q, 1)))
    _assert_equal((idx, d2), rr.topk(ref, qry, k))


@pytest.mark.parametrize("Q", [2, 1100])
def test_duplicates_a_tile_and_a_slice_apart(dev, Q):
    """Equal rows at j, j + 256 (the next tile) and j + L (the next slice, L from the plan; for few queries a slice is one
    tile) -- and queries equal to them, so the ties sit at d2 = 0 at the head of the lists."""
    from dh3d_amd import retrieval
    D, k, R = 8, 8, 3584
    S, L = retrieval.retrieve_plan(Q, R, D, k)
    assert S >= 2 and (Q == 2) == (L == 256)     # both layouts are met: a slice of one tile, a slice of several
    rng = np.random.default_rng(4)
    ref = rng.standard_normal((R, D)).astype(np.float32)
    heads = [0, 100, 255, 256 + 31, L + 7]
    for j in heads:
        ref[j + 256] = ref[j]
        ref[j + L] = ref[j]
        ref[j + 2 * L] = ref[j]
    qry = rng.standard_normal((Q, D)).astype(np.float32)
    qry[:len(heads) if Q > len(heads) else Q] = ref[heads[:Q]]
    got = _search(dev, ref, qry, k)
    _assert_equal(got, rr.topk(ref, qry, k))
    idx, d2 = got[0].cpu().numpy(), got[1].cpu().numpy()
    for q, j in enumerate(heads[:Q]):
        twins = sorted({j, j + 256, j + L, j + 2 * L})
        assert idx[q, :len(twins)].tolist() == twins and (d2[q, :len(twins)] == 0.0).all(), (q, j)


def test_near_tie_is_ranked_in_float64(dev):
    ref, qry = rr.near_tie_case()
    idx, d2 = _search(dev, ref, qry, 2)
    assert idx.cpu().numpy()[0].tolist() == [7, 3]                            # float32 ranks would tie and return 3, 7
    assert d2.cpu().numpy()[0].tolist() == [1.0, 1.0 + 2.0 ** -26]
    i32, _ = rr.topk(ref, qry, 2, dtype=np.float32)
    assert i32[0].tolist() == [3, 7]


@pytest.mark.parametrize("count", [0, 1, 700])
def test_ref_count_on_a_capacity_of_1024(dev, count):
    """The live map is rows below the device-side count; the rows beyond it are NaN here, so reading one would show."""
    from dh3d_amd import retrieval
    rng = np.random.default_rng(5)
    cap, D, Q, k = 1024, 32, 9, 25
    assert retrieval.retrieve_plan(Q, cap, D, k)[0] >= 2    # a sliced capacity: slices past the count are empty
    ref = rng.standard_normal((cap, D)).astype(np.float32)
    ref[count:] = np.nan
    qry = rng.standard_normal((Q, D)).astype(np.float32)
    exp = rr.topk(ref[:count], qry, k)
    _assert_equal(_search(dev, ref, qry, k, count), exp)
    if count > 256:                                          # the same on an unsliced capacity (Q large enough)
        many = np.tile(qry, (920, 1))[:8200]
        assert retrieval.retrieve_plan(len(many), cap, D, k)[0] == 1
        got = _search(dev, ref, many, k, count)
        _assert_equal((got[0][:Q], got[1][:Q]), exp)
        _assert_equal((got[0][-Q:], got[1][-Q:]), rr.topk(ref[:count], many[-Q:], k))


def test_each_query_alone_equals_its_row_in_the_batch(dev):
    from dh3d_amd import retrieval
    rng = np.random.default_rng(6)
    Q, R, D, k = 21, 1500, 64, 10
    ref = torch.from_numpy(rng.standard_normal((R, D)).astype(np.float32)).to(dev)
    qry = torch.from_numpy(rng.standard_normal((Q, D)).astype(np.float32)).to(dev)
    idx, d2 = retrieval.search_descriptors_sq(ref, qry, k)
    for q in range(Q):
        i1, d1 = retrieval.search_descriptors_sq(ref, qry[q:q + 1], k)
        assert torch.equal(i1[0], idx[q]) and torch.equal(d1[0].view(torch.int64), d2[q].view(torch.int64)), q


def test_graph_capture_serves_a_changed_map(dev):
    from dh3d_amd import retrieval
    rng = np.random.default_rng(7)
    cap, D, Q, k = 1024, 64, 20, 25
    sref = torch.from_numpy(rng.standard_normal((cap, D)).astype(np.float32)).to(dev)
    sqry = torch.from_numpy(rng.standard_normal((Q, D)).astype(np.float32)).to(dev)
    scount = torch.tensor([300], dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        retrieval.search_descriptors_sq(sref, sqry, k, scount)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gout = retrieval.search_descriptors_sq(sref, sqry, k, scount)
    for seed, count in ((8, 10), (9, 1024), (10, 600)):
        r = np.random.default_rng(seed)
        ref = r.standard_normal((cap, D)).astype(np.float32)
        qry = r.standard_normal((Q, D)).astype(np.float32)
        sref.copy_(torch.from_numpy(ref))
        sqry.copy_(torch.from_numpy(qry))
        scount.fill_(count)
        g.replay()
        torch.cuda.synchronize()
        _assert_equal(gout, rr.topk(ref, qry, k, count), seed)


def test_evaluation_backend_hip_equals_torch_on_device_descriptors(dev):
    """The synthetic-traversal recipe of test_evaluation.py: descriptors out of the HIP forward, retrieved by both backends."""
    from dh3d_amd import ConfigFactory, evaluation as ev
    from dh3d_amd.model import DH3D
    m = DH3D(ConfigFactory("global_config").getconfig()).init_synthetic(7).to(dev).eval().prepare()
    rng = np.random.default_rng(11)
    places, N = 48, 2048
    base = rng.random((places, N, 3), dtype=np.float32) * np.array([40, 40, 6], np.float32)
    base *= (0.5 + rng.random((places, 1, 3))).astype(np.float32)
    for p in range(places):
        c = rng.integers(0, N, 5)
        base[p, : N // 2] = base[p, c[rng.integers(0, 5, N // 2)]] + rng.normal(0, 1.0 + 0.1 * p, (N // 2, 3)).astype(np.float32)
    ref_pos = rng.random((places, 2)) * 3000
    qsel = rng.permutation(places)[:40]
    qry = base[qsel][:, rng.permutation(N)] + rng.normal(0, 0.05, (40, N, 3)).astype(np.float32)
    qry_pos = ref_pos[qsel] + rng.normal(0, 8, (40, 2))
    with torch.no_grad():
        ref_d = m(torch.from_numpy(base).to(dev), fetch=("globaldesc",))["globaldesc"]
        qry_d = m(torch.from_numpy(qry).to(dev), fetch=("globaldesc",))["globaldesc"]
    k = 25
    a = ev.retrieval(ref_d, qry_d, k, backend="hip")
    b = ev.retrieval(ref_d, qry_d, k, backend="torch")
    assert a.is_cuda and a.dtype == torch.int64 and torch.equal(a, b)
    assert np.array_equal(a.cpu().numpy(), rr.topk(ref_d.cpu().numpy(), qry_d.cpu().numpy(), k)[0])
    rp, qp = torch.from_numpy(ref_pos).to(dev), torch.from_numpy(qry_pos).to(dev)
    rec_h, one_h = ev.evaluate_pair(ref_d, rp, qry_d, qp, max_num_nn=k, backend="hip")
    rec_t, one_t = ev.evaluate_pair(ref_d, rp, qry_d, qp, max_num_nn=k)
    assert torch.equal(rec_h, rec_t) and one_h == one_t


# ------------------------------------------------------------------------------------------------------ relocalisation

def _places(rng, P=12, M=64, D=128, G=256):
    """P places of up to M keypoints drawn from the demo cloud's FPS points, unit local and global descriptors."""
    demo = np.load(os.path.join(HERE, "golden", "demo_clouds.npz"))
    pts = demo["local_642"][demo["local_642/fps_idx"]].astype(np.float64)
    rows = np.zeros((P, M, 3 + D + 1), np.float32)
    count = rng.integers(48, M + 1, P).astype(np.int32)
    count[0], count[1] = M, 48
    for p in range(P):
        rows[p, :count[p], :3] = pts[rng.choice(len(pts), count[p], replace=False)]
        rows[p, :count[p], 3:3 + D] = _unit(rng, (count[p], D))
    return rows, count, _unit(rng, (P, G))


def _queries(rng, rows, count, gdesc, sel, D=128):
    """Rigidly moved, noisy, shuffled copies of the places `sel`: y = R^T (x - t) + 5 cm noise (the keypoint noise of
    test_registration_gpu's recovery test), local descriptors + 0.01 noise, global descriptors + 0.02 noise."""
    Q, M = len(sel), rows.shape[1]
    qrows = np.zeros((Q, M, rows.shape[2]), np.float32)
    T = np.zeros((Q, 3, 4))
    for q, p in enumerate(sel):
        n = count[p]
        R, t = _random_pose(rng)
        x = rows[p, :n, :3].astype(np.float64)
        perm = rng.permutation(n)
        qrows[q, perm, :3] = (x - t) @ R + rng.normal(0.0, 0.05, (n, 3))
        qrows[q, perm, 3:3 + D] = rows[p, :n, 3:3 + D] + 0.01 * rng.standard_normal((n, D)).astype(np.float32)
        T[q] = np.concatenate([R, t[:, None]], axis=1)
    qdesc = gdesc[sel] + 0.02 * rng.standard_normal((Q, gdesc.shape[1])).astype(np.float32)
    qdesc /= np.linalg.norm(qdesc, axis=1, keepdims=True)
    return qrows, count[sel].copy(), qdesc.astype(np.float32), T


def _index(dev, rows, count, gdesc, capacity=32):
    from dh3d_amd import retrieval
    index = retrieval.PlaceIndex(dim=gdesc.shape[1], capacity=capacity, device=dev, keypoints=rows.shape[1], row_dim=rows.shape[2])
    half = len(rows) // 2                                    # two appends: the offset comes from the host mirror
    pos = np.arange(2 * len(rows), dtype=np.float64).reshape(-1, 2)
    assert list(index.add(gdesc[:half], pos[:half], rows[:half], count[:half])) == list(range(half))
    index.add(torch.from_numpy(gdesc[half:]).to(dev), pos[half:], torch.from_numpy(rows[half:]).to(dev), count[half:])
    assert len(index) == len(rows) and int(index.count.item()) == len(rows)
    return index


def test_localize_finds_the_place_and_the_pose(dev):
    from dh3d_amd import registration as reg
    rng = np.random.default_rng(12)
    rows, count, gdesc = _places(rng)
    sel = np.array([3, 0, 11, 7, 1, 5, 9, 2])
    qrows, qcount, qdesc, T = _queries(rng, rows, count, gdesc, sel)
    index = _index(dev, rows, count, gdesc)
    tq, tc, td = torch.from_numpy(qrows).to(dev), torch.from_numpy(qcount).to(dev), torch.from_numpy(qdesc).to(dev)
    res = index.localize(td, tq, tc, k=5)
    assert res["place"].cpu().numpy().tolist() == sel.tolist()
    assert (res["rank"] == 0).all() and torch.equal(res["idx"][:, 0], res["place"])
    assert np.array_equal(res["idx"].cpu().numpy(), rr.topk(gdesc, qdesc, 5)[0])
    assert np.array_equal(res["pos"].cpu().numpy(), np.stack([2.0 * sel, 2.0 * sel + 1], axis=1))
    A, AC = torch.from_numpy(rows).to(dev), torch.from_numpy(count).to(dev)
    for q, p in enumerate(sel):                              # the single (place, query) pair, bit for bit
        one = reg.register(A[p:p + 1], AC[p:p + 1], tq[q:q + 1], tc[q:q + 1])
        assert bool(one["valid"][0])
        assert torch.equal(one["Rt"][0].view(torch.int64), res["Rt"][q].view(torch.int64)), q
        assert int(one["num_inliers"][0]) == int(res["num_inliers"][q]) and torch.equal(one["inliers"][0], res["inliers"][q]), q
        assert float(one["inlier_ratio"][0]) == float(res["inlier_ratio"][q])
    dt, dd = reg.transform_errors(T, res["Rt"], res["place"] >= 0)
    assert (dt < 0.1).all() and (dd < 1.0).all(), (dt.max(), dd.max())
    assert (res["num_inliers"].cpu().numpy() > 0.8 * qcount).all()


def test_localize_on_a_small_map_and_on_hopeless_queries(dev):
    rng = np.random.default_rng(13)
    rows, count, gdesc = _places(rng, P=3)
    sel = np.array([2, 0, 1, 2])
    qrows, qcount, qdesc, T = _queries(rng, rows, count, gdesc, sel)
    qcount[3] = 0                                            # no keypoints: no candidate can give a model
    index = _index("cuda", rows, count, gdesc, capacity=8)  # the documented spelling: no device index
    assert index.device == dev and index.kp_rows.device == dev
    res = index.localize(torch.from_numpy(qdesc).to(dev), torch.from_numpy(qrows).to(dev), torch.from_numpy(qcount).to(dev), k=5)
    idx = res["idx"].cpu().numpy()
    assert (idx[:, 3:] == -1).all() and (np.sort(idx[:, :3], axis=1) == np.arange(3)).all()   # fewer places than k
    assert res["place"].cpu().numpy().tolist() == [2, 0, 1, -1]
    assert res["rank"].cpu().numpy().tolist() == [0, 0, 0, -1]
    assert int(res["num_inliers"][3]) == 0 and bool(torch.isnan(res["Rt"][3]).all()) and not bool(res["inliers"][3].any())
    assert bool(torch.isfinite(res["Rt"][:3]).all()) and bool(torch.isnan(res["pos"][3]).all())
    with pytest.raises(ValueError):
        index.add(np.zeros((6, 256), np.float32), None, rows[:1].repeat(6, 0), count[:1].repeat(6))   # 3 + 6 > capacity 8


# ------------------------------------------------------------------------------------------------------------ end to end

def test_relocalize_clouds_end_to_end(dev):
    """Clouds in, place ids and poses out, through both models: the two demo clouds are the map, and the same clouds are
    the queries, so every query is its own place at distance 0 with the identity pose and every keypoint an inlier."""
    from dh3d_amd import ConfigFactory, retrieval
    from dh3d_amd.model import DH3D
    gm = DH3D(ConfigFactory("global_config").getconfig()).init_synthetic(0).to(dev).eval().prepare()
    lm = DH3D(ConfigFactory("detection_config").getconfig()).init_synthetic(0).to(dev).eval().prepare()
    demo = np.load(os.path.join(HERE, "golden", "demo_clouds.npz"))
    X = torch.from_numpy(np.stack([demo["local_268"], demo["local_642"]]).astype(np.float32)).to(dev)
    with torch.no_grad():
        g = gm.forward(X, fetch=("globaldesc",))["globaldesc"]
        o = lm.forward(X, fetch=("kp_count", "xyz_feat_att_nms"))
    M, C = o["xyz_feat_att_nms"].shape[1:]
    index = retrieval.PlaceIndex(dim=g.shape[1], capacity=16, keypoints=M, row_dim=C)       # the default device, "cuda"
    index.add(g, np.array([[10.0, 20.0], [30.0, 40.0]]), kp_rows=o["xyz_feat_att_nms"], kp_count=o["kp_count"])
    with torch.no_grad():
        res = retrieval.relocalize_clouds(gm, lm, index, X, k=5)                             # k > the two places
    assert res["place"].cpu().tolist() == [0, 1] and res["rank"].cpu().tolist() == [0, 0]
    assert (res["idx"][:, 2:] == -1).all() and (res["dist"][:, 0] == 0).all()
    assert torch.equal(res["num_inliers"], o["kp_count"]) and (res["inlier_ratio"] == 1.0).all()
    Rt = res["Rt"].cpu().numpy()
    assert np.abs(Rt[:, :, :3] - np.eye(3)).max() < 1e-9 and np.abs(Rt[:, :, 3]).max() < 1e-6
    assert res["pos"].cpu().tolist() == [[10.0, 20.0], [30.0, 40.0]]
    exp = index.localize(g, o["xyz_feat_att_nms"], o["kp_count"], k=5)      # == forward + localize, bit for bit
    for key in exp:
        e, got = exp[key], res[key]
        if e.dtype == torch.float64:
            assert torch.equal(e.view(torch.int64), got.view(torch.int64)), key
        else:
            assert torch.equal(e, got), key
    with pytest.raises(ValueError):
        retrieval.relocalize_clouds(lm, lm, index, X)         # no globaldesc output
    with pytest.raises(ValueError):
        retrieval.relocalize_clouds(gm, gm, index, X)         # no keypoint outputs
