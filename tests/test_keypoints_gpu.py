"""GPU: batched on-device keypoint NMS (utils.batched_nms -> csrc/keypoints.hip) against utils.single_nms, the per-cloud
yardstick, cloud by cloud and bit for bit; the model's keypoint outputs (kp_count / kp_inds / xyz_feat_att_nms) eagerly,
captured and in a Pipeline with pinned host fetches."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NMS = dict(nms_radius=0.5, min_response_ratio=0.01, max_keypoints=512)


def _cube_batch(rng, B, N, side=12.0, outliers=40):
    xyz = (rng.random((B, N, 3)) * side).astype(np.float32)
    xyz[:, :outliers] += 100.0 + 50.0 * rng.random((B, outliers, 3)).astype(np.float32)  # sparse: muted by remove_noise
    return xyz


def _check_vs_single(xyz, scores, dev, invert=False, **kw):
    """batched_nms on the batch == single_nms per cloud (count, ids, order); rows past count are -1."""
    from dh3d_amd import utils
    args = dict(NMS)
    args.update(kw)
    x = torch.as_tensor(xyz).to(dev)
    s = torch.as_tensor(scores).to(dev)
    count, inds = utils.batched_nms(x, s, invert=invert, **args)
    count, inds = count.cpu(), inds.cpu()
    assert inds.shape == (x.shape[0], args["max_keypoints"]) and count.dtype == torch.int32 and inds.dtype == torch.int32
    for b in range(x.shape[0]):
        sb = (1 - s[b]) if invert else s[b]
        n, idx = utils.single_nms(x[b], sb, **args)
        assert int(count[b]) == n, (b, int(count[b]), n)
        assert inds[b, :n].tolist() == idx.cpu().tolist(), b
        assert bool((inds[b, n:] == -1).all()), b
    return count, inds


def test_uniform_cubes_with_outliers(dev):
    rng = np.random.default_rng(0)
    xyz = _cube_batch(rng, 3, 3000)
    count, _ = _check_vs_single(xyz, rng.random((3, 3000), dtype=np.float32), dev, nms_radius=0.8,
                                min_response_ratio=0.05, max_keypoints=256)
    assert int(count.min()) > 0


def test_inverted_scores_read_in_place(dev):
    """invert=True on a strided column view (xyz_feat_att[:, :, 131]) == single_nms(xyz, 1 - att)."""
    from dh3d_amd import utils
    rng = np.random.default_rng(1)
    xyz = torch.from_numpy(_cube_batch(rng, 2, 2000)).to(dev)
    feat = torch.from_numpy(rng.random((2, 2000, 132), dtype=np.float32)).to(dev)
    col = feat[:, :, 131]
    assert not col.is_contiguous()
    count, inds = utils.batched_nms(xyz, col, invert=True, **NMS)
    for b in range(2):
        n, idx = utils.single_nms(xyz[b], 1 - col[b], **NMS)
        assert int(count[b]) == n and inds[b, :n].tolist() == idx.tolist()


@pytest.fixture(scope="module")
def demo():
    return np.load(os.path.join(HERE, "golden", "demo_clouds.npz"))


def test_demo_clouds(dev, demo):
    """Real density (two 16384-point LiDAR sub-maps, ground plane included) and exact duplicates (dso_9000)."""
    rng = np.random.default_rng(2)
    pair = np.stack([demo["local_268"], demo["local_642"]]).astype(np.float32)
    count, _ = _check_vs_single(pair, rng.random((2, 16384), dtype=np.float32), dev)
    assert int(count.min()) > 0
    dso = demo["dso_9000"].astype(np.float32)[None]
    assert len(np.unique(dso[0], axis=0)) < dso.shape[1]  # the fixture does hold exact duplicates
    _check_vs_single(dso, rng.random((1, dso.shape[1]), dtype=np.float32), dev)


def test_beyond_the_ordered_knn(dev):
    """N > 16384: the brute-force kNN path of batched_knn."""
    rng = np.random.default_rng(3)
    _check_vs_single(_cube_batch(rng, 2, 17000, side=25.0), rng.random((2, 17000), dtype=np.float32), dev)


def test_small_clouds_clip_k(dev):
    rng = np.random.default_rng(4)
    for N in (1, 5, 8, 30, 49):
        xyz = (rng.random((2, N, 3)) * 2).astype(np.float32)
        _check_vs_single(xyz, rng.random((2, N), dtype=np.float32), dev)


def test_quantised_scores_ties(dev):
    """Scores on a 1/16 grid: many exact ties, which exercise the (score, index) order and the first-maximum rule."""
    rng = np.random.default_rng(5)
    xyz = _cube_batch(rng, 3, 4000, side=10.0)
    s = (rng.integers(0, 17, (3, 4000)) / 16.0).astype(np.float32)
    _check_vs_single(xyz, s, dev, max_keypoints=4096)
    _check_vs_single(xyz, s, dev, max_keypoints=100)
    _check_vs_single(xyz, s, dev, max_keypoints=512, invert=True)


def test_all_zero_scores(dev):
    rng = np.random.default_rng(6)
    count, inds = _check_vs_single(_cube_batch(rng, 2, 1000), np.zeros((2, 1000), np.float32), dev)
    assert count.tolist() == [0, 0] and bool((inds == -1).all())


def test_more_and_fewer_survivors_than_m(dev):
    rng = np.random.default_rng(7)
    xyz = _cube_batch(rng, 2, 6000, side=30.0)
    s = rng.random((2, 6000), dtype=np.float32)
    few, _ = _check_vs_single(xyz, s, dev, max_keypoints=4096)
    assert 8 < int(few.max()) < 4096
    many, _ = _check_vs_single(xyz, s, dev, max_keypoints=8)
    assert many.tolist() == [8, 8]
    one, _ = _check_vs_single(xyz, s, dev, max_keypoints=1)
    assert one.tolist() == [1, 1]
    # the edge between "every survivor wins" and the select: M = c + 1 and c take all of cloud 0, c - 1 drops its last
    c = int(few[0])
    for m in (c - 1, c, c + 1):
        edge, _ = _check_vs_single(xyz, s, dev, max_keypoints=m)
        assert int(edge[0]) == min(c, m)


def test_mixed_batch_with_an_all_zero_cloud(dev):
    rng = np.random.default_rng(8)
    xyz = _cube_batch(rng, 3, 2500)
    s = rng.random((3, 2500), dtype=np.float32)
    s[1] = 0.0
    count, _ = _check_vs_single(xyz, s, dev)
    assert int(count[1]) == 0 and int(count[0]) > 0 and int(count[2]) > 0


def _restated(nn, dist, a, R, ratio, M, nb, remove_noise=True):
    """Steps 1-5 of the keypoint rule in numpy on the same neighbours (include/dh3d_hip.h dh3d_keypoint_nms)."""
    N, K = nn.shape
    a = a.astype(np.float32).copy()
    if remove_noise and K > 7:
        a[dist[:, 7] > np.float32(2.0)] = np.float32(0.0)
    a[a == 0] = np.float32(0.0)
    thr = np.float32(a[:nb].max()) * np.float32(ratio) if nb > 0 else np.float32(np.inf)
    outside = (dist > np.float32(R)) | (nn < 0) | (nn >= nb)
    s = np.where(outside, np.float32(0.0), a[np.clip(nn, 0, N - 1)])
    is_max = (s[:, 1:] <= s[:, :1]).all(axis=1)
    keep = [i for i in range(nb) if is_max[i] and a[i] > thr]
    keep.sort(key=lambda i: (a[i], i), reverse=True)
    return keep[:M]


def test_numpy_restatement(dev):
    from dh3d_amd import pm, utils
    rng = np.random.default_rng(9)
    xyz = _cube_batch(rng, 2, 3000, side=10.0)
    s = (rng.integers(0, 33, (2, 3000)) / 32.0).astype(np.float32)
    nv = np.array([3000, 2200], np.int32)
    x = torch.from_numpy(xyz).to(dev)
    nn, dist = utils.batched_knn(x, 50)
    for num_valid in (None, torch.from_numpy(nv).to(dev)):
        count, inds = pm.keypoint_nms(torch.from_numpy(s).to(dev), nn, dist, 0.7, 0.02, 300, num_valid=num_valid)
        for b in range(2):
            nb = 3000 if num_valid is None else int(nv[b])
            exp = _restated(nn[b].cpu().numpy(), dist[b].cpu().numpy(), s[b], 0.7, 0.02, 300, nb)
            assert int(count[b]) == len(exp) and inds[b, :len(exp)].tolist() == exp


def test_far_padding_with_num_valid(dev):
    """get_fixednum_pcd(randsample=False) padding + num_valid == single_nms on the cropped cloud."""
    from dh3d_amd import utils
    rng = np.random.default_rng(10)
    N = 4096
    clouds, nv, scores = [], [], []
    for n in (4096, 3000, 1234, 60):
        c, kept = utils.get_fixednum_pcd((rng.random((n, 3)) * 10).astype(np.float32), N, randsample=False)
        clouds.append(c.astype(np.float32))
        nv.append(kept)
        scores.append(rng.random(N, dtype=np.float32))
    x = torch.from_numpy(np.stack(clouds)).to(dev)
    s = torch.from_numpy(np.stack(scores)).to(dev)
    count, inds = utils.batched_nms(x, s, num_valid=torch.tensor(nv, dtype=torch.int32, device=dev), **NMS)
    for b, n in enumerate(nv):
        k, idx = utils.single_nms(x[b, :n].contiguous(), s[b, :n].contiguous(), **NMS)
        assert int(count[b]) == k and inds[b, :k].tolist() == idx.tolist() and bool((inds[b, k:] == -1).all())


def test_graph_capture_replays_on_new_data(dev):
    from dh3d_amd import utils
    rng = np.random.default_rng(11)
    B, N = 3, 5000
    sx = torch.from_numpy(_cube_batch(rng, B, N)).to(dev)
    ss = torch.from_numpy(rng.random((B, N), dtype=np.float32)).to(dev)
    snv = torch.tensor([N, N - 100, 2000], dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        utils.batched_nms(sx, ss, num_valid=snv, **NMS)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gc, gi = utils.batched_nms(sx, ss, num_valid=snv, **NMS)
    for seed in (12, 13):
        r = np.random.default_rng(seed)
        x = torch.from_numpy(_cube_batch(r, B, N)).to(dev)
        s = torch.from_numpy((r.integers(0, 9, (B, N)) / 8.0).astype(np.float32)).to(dev)
        nv = torch.tensor([N - seed, N, 3333], dtype=torch.int32, device=dev)
        sx.copy_(x)
        ss.copy_(s)
        snv.copy_(nv)
        g.replay()
        ec, ei = utils.batched_nms(x, s, num_valid=nv, **NMS)
        torch.cuda.synchronize()
        assert torch.equal(gc, ec) and torch.equal(gi, ei)
        assert int(ec.min()) > 0


def test_gather_rows_any_c(dev):
    from dh3d_amd import pm
    rng = np.random.default_rng(14)
    for C in (1, 3, 131, 132, 200):
        src = torch.from_numpy(rng.standard_normal((2, 300, C)).astype(np.float32)).to(dev)
        inds = torch.from_numpy(rng.integers(0, 300, (2, 16)).astype(np.int32)).to(dev)
        count = torch.tensor([16, 5], dtype=torch.int32, device=dev)
        out = pm.gather_rows(src, inds, count)
        for b, n in enumerate((16, 5)):
            assert torch.equal(out[b, :n], src[b, inds[b, :n].long()])
            assert bool((out[b, n:] == 0).all())


# ------------------------------------------------------------------ the model's keypoint outputs

KP = ("kp_count", "kp_inds", "xyz_feat_att_nms")


@pytest.fixture(scope="module")
def det_model(dev):
    from dh3d_amd import ConfigFactory
    from dh3d_amd.model import DH3D
    return DH3D(ConfigFactory("detection_config").getconfig()).init_synthetic(0).to(dev).eval().prepare()


def _model_batch(seed, B=2, N=4096, pad=(0, 700)):
    from dh3d_amd import utils
    rng = np.random.default_rng(seed)
    clouds, nv = [], []
    for p in pad[:B]:
        c, kept = utils.get_fixednum_pcd((rng.random((N - p, 3)) * 9).astype(np.float32), N, randsample=False)
        clouds.append(c.astype(np.float32))
        nv.append(kept)
    return np.stack(clouds), np.array(nv, np.int32)


def _check_model_outs(outs, xyz_feat_att, num_valid=None):
    from dh3d_amd import utils
    count, inds, rows = outs["kp_count"], outs["kp_inds"], outs["xyz_feat_att_nms"]
    M = 512
    assert inds.shape == (xyz_feat_att.shape[0], M) and rows.shape == (xyz_feat_att.shape[0], M, 132)
    for b in range(xyz_feat_att.shape[0]):
        n_b = xyz_feat_att.shape[1] if num_valid is None else int(num_valid[b])
        res = xyz_feat_att[b, :n_b]
        k, idx = utils.single_nms(res[:, 0:3].contiguous(), 1 - res[:, -1], 0.5, 0.01, M)
        assert k > 0 and int(count[b]) == k and inds[b, :k].tolist() == idx.tolist()
        assert torch.equal(rows[b, :k], xyz_feat_att[b, idx])
        assert bool((rows[b, k:] == 0).all()) and bool((inds[b, k:] == -1).all())


def test_model_keypoint_outputs(dev, det_model):
    pts, nv = _model_batch(20)
    x = torch.from_numpy(pts).to(dev)
    with torch.no_grad():
        full = det_model(x, fetch=("xyz_feat_att",) + KP)
        _check_model_outs(full, full["xyz_feat_att"])
        only = det_model(x, fetch=("kp_count", "xyz_feat_att_nms"))
        assert set(only) >= {"kp_count", "xyz_feat_att_nms"}
        assert torch.equal(only["kp_count"], full["kp_count"])
        assert torch.equal(only["xyz_feat_att_nms"], full["xyz_feat_att_nms"])
        nvt = torch.from_numpy(nv).to(dev)
        padded = det_model(x, fetch=("xyz_feat_att",) + KP, num_valid=nvt)
        _check_model_outs(padded, padded["xyz_feat_att"], nv)
        # nothing changes for a forward that does not ask for keypoints
        plain = det_model(x)
        assert not set(KP) & set(plain)
        assert torch.equal(plain["xyz_feat_att"], full["xyz_feat_att"])


def test_model_keypoints_graphed(dev, det_model):
    pts, nv = _model_batch(21)
    x = torch.from_numpy(pts).to(dev)
    nvt = torch.from_numpy(nv).to(dev)
    with torch.no_grad():
        f = det_model.graphed(x, outputs=("xyz_feat_att",) + KP, example_num_valid=nvt)
        for seed in (22, 23):
            p2, nv2 = _model_batch(seed, pad=(seed * 10, 300))
            x2, nv2t = torch.from_numpy(p2).to(dev), torch.from_numpy(nv2).to(dev)
            got = {k: v.clone() for k, v in f(x2, num_valid=nv2t).items()}
            ref = det_model(x2, fetch=("xyz_feat_att",) + KP, num_valid=nv2t)
            for k in KP + ("xyz_feat_att",):
                assert torch.equal(got[k], ref[k]), k
            _check_model_outs(got, got["xyz_feat_att"], nv2)


def test_model_keypoints_pipeline_pinned_fetch(dev, det_model):
    """Depth-2 Pipeline, pinned host batches in and only the keypoints out (fetch_to pinned buffers), slot by slot."""
    pts, nv = _model_batch(30)
    outputs = ("xyz_feat_att",) + KP
    with torch.no_grad():
        pipe = det_model.pipeline(torch.from_numpy(pts).to(dev), depth=2, outputs=outputs,
                                  example_num_valid=torch.from_numpy(nv).to(dev))
        batches = [_model_batch(31 + i, pad=(50 * i, 400 + i)) for i in range(4)]
        hosts = [(torch.from_numpy(p).pin_memory(), torch.from_numpy(n).pin_memory()) for p, n in batches]
        tickets, bufs = [], []
        for hp, hn in hosts:
            if len(tickets) == 2:
                tickets[-2].event.synchronize()
            fetch_to = {"kp_count": torch.empty((2,), dtype=torch.int32).pin_memory(),
                        "kp_inds": torch.empty((2, 512), dtype=torch.int32).pin_memory(),
                        "xyz_feat_att_nms": torch.empty((2, 512, 132), dtype=torch.float32).pin_memory(),
                        "xyz_feat_att": torch.empty((2, 4096, 132), dtype=torch.float32).pin_memory()}
            tickets.append(pipe.submit(hp, num_valid=hn, fetch_to=fetch_to))
            bufs.append(fetch_to)
        for t in tickets:
            t.event.synchronize()
        for (p, n), got in zip(batches, bufs):
            ref = det_model(torch.from_numpy(p).to(dev), fetch=outputs, num_valid=torch.from_numpy(n).to(dev))
            # the slot's own map: its keypoints are single_nms's on it, its rows are its rows
            _check_model_outs({k: v.to(dev) for k, v in got.items()}, got["xyz_feat_att"].to(dev), n)
            if torch.equal(got["xyz_feat_att"].to(dev), ref["xyz_feat_att"]):
                for k in KP:
                    assert torch.equal(got[k].to(dev), ref[k]), k
            else:  # steps in flight may round the descriptors in another association (engine.py): within 2e-6
                assert float((got["xyz_feat_att"].to(dev) - ref["xyz_feat_att"]).abs().max()) < 1e-5
