"""GPU: prepare_clouds against the numpy restatement (tests/prepare_reference.py) -- torch.equal on points, num_valid and
counts, cloud by cloud, on ragged batches of the real clouds, a synthetic street at three target sizes (crop and pad), the tie
cases, empty / single-point / all-outlier clouds, each stage switched off, B = 1 and 32, Nraw = 131072, sentinel-filled
outputs over a dirty workspace, and replays of a captured graph with other sizes.  The centroid is held to the bound of any
summation order, m * 2^-52 * max|coordinate|, and the kept set must be the restatement's selection from the centroid the op
returned.  Then the chain prepare_clouds -> DH3D.forward(num_valid) -> batched_nms against the same chain on a host-prepared
batch."""
import os

import numpy as np
import pytest
import torch

import prepare_reference as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REAL = ("local_268", "local_642", "dso_9000", "global_a", "global_b", "global_c")


@pytest.fixture(scope="module")
def real():
    d = np.load(os.path.join(GOLDEN, "demo_clouds.npz"))
    return [np.ascontiguousarray(d[k], np.float32) for k in REAL]


def _batch(clouds, dev, nraw=None):
    """raw [B, Nraw, 3] with NaN rows behind every cloud (never to be read) and num_raw."""
    nraw = max([c.shape[0] for c in clouds] + [1]) if nraw is None else nraw
    raw = np.full((len(clouds), nraw, 3), np.nan, np.float32)
    for b, c in enumerate(clouds):
        raw[b, :c.shape[0]] = c
    num = np.array([c.shape[0] for c in clouds], np.int32)
    return torch.from_numpy(raw).to(dev), torch.from_numpy(num).to(dev)


def _check(outs, clouds, targetnum, **kw):
    points, num_valid, counts, centroid = [t.cpu().numpy() for t in outs]
    B = len(clouds)
    assert points.shape == (B, targetnum, 3) and points.dtype == np.float32
    assert num_valid.shape == (B,) and num_valid.dtype == np.int32
    assert counts.shape == (B, 3) and counts.dtype == np.int32 and centroid.shape == (B, 3) and centroid.dtype == np.float64
    for b, c in enumerate(clouds):
        exp = R.prepare_cloud(c, targetnum, centroid=centroid[b], **kw)
        print("cloud %d: counts %s (expected %s), num_valid %d (expected %d)"
              % (b, counts[b].tolist(), exp["counts"].tolist(), num_valid[b], exp["num_valid"]))
        assert np.array_equal(counts[b], exp["counts"]), (b, counts[b], exp["counts"])
        assert num_valid[b] == exp["num_valid"], (b, num_valid[b], exp["num_valid"])
        m = int(exp["counts"][2])
        if m > 0:
            bound = m * 2.0 ** -52 * float(np.abs(exp["stage2"]).max())
            err = float(np.abs(centroid[b] - exp["centroid"]).max())
            print("cloud %d: centroid |err| %.3e, bound %.3e" % (b, err, bound))
            assert err <= bound, (b, err, bound)
        else:
            assert (centroid[b] == 0).all()
        assert torch.equal(torch.from_numpy(points[b]), torch.from_numpy(exp["points"])), \
            (b, int((points[b] != exp["points"]).any(axis=1).sum()))
    return points, num_valid, counts, centroid


def _run(clouds, targetnum, dev, nraw=None, **kw):
    from dh3d_amd import utils
    raw, num = _batch(clouds, dev, nraw)
    outs = utils.prepare_clouds(raw, num, targetnum, **kw)
    torch.cuda.synchronize()
    again = utils.prepare_clouds(raw, num, targetnum, **kw)
    for a, o in zip(again, outs):
        assert torch.equal(a, o)                       # run to run
    return _check(outs, clouds, targetnum, **kw)


def test_ragged_batch_of_the_real_clouds(dev, real):
    _, nv, counts, _ = _run(real, 8192, dev)
    assert counts[0].tolist() == [16384, 14698, 14614] and counts[2].tolist() == [9000, 7687, 7201]
    assert nv.tolist() == [8192, 8192, 7201, 3718, 3542, 7121]        # two cropped, four padded
    _run(real[::-1], 4096, dev)
    _run(real, 16384, dev, sortby_dis=False)


@pytest.mark.parametrize("targetnum", [8192, 16384, 65536])
def test_street_scene(dev, targetnum):
    scene = R.street_scene()
    _, nv, counts, _ = _run([scene], targetnum, dev)
    assert counts[0, 0] == 60300 and 16384 < counts[0, 2] < 65536
    assert nv[0] == min(targetnum, counts[0, 2])                      # 8192, 16384: the crop; 65536: the pad


@pytest.mark.parametrize("name", sorted(R.tie_cases()))
def test_tie_cases(dev, name):
    pts, kw = R.tie_cases()[name]
    kw = dict(kw)
    _run([pts], kw.pop("targetnum"), dev, **kw)


def test_tie_cases_in_one_batch_do_not_mix(dev):
    """A cloud's result does not depend on the batch: the cases that share their arguments, side by side with filler."""
    cases = R.tie_cases()
    rng = np.random.default_rng(5)
    filler = (rng.random((3000, 3), dtype=np.float32) * np.float32(8.0))
    clouds = [cases["duplicates"][0], filler, cases["crowded_voxels"][0], np.zeros((0, 3), np.float32), filler[:1]]
    _run(clouds, 512, dev)


def test_empty_single_and_all_outlier_clouds(dev):
    rng = np.random.default_rng(6)
    lone = (rng.random((40, 3), dtype=np.float32) * np.float32(400.0))           # 40 points, metres apart: all outliers
    clouds = [np.zeros((0, 3), np.float32), np.array([[1.0, 2.0, 3.0]], np.float32), lone,
              rng.random((500, 3), dtype=np.float32) * np.float32(3.0)]
    points, nv, counts, _ = _run(clouds, 256, dev)
    assert nv[:3].tolist() == [0, 0, 0] and counts[:3].tolist() == [[0, 0, 0], [1, 1, 0], [40, 40, 0]]
    assert (points[:3] == R.PAD).all() and nv[3] > 0
    _run(clouds, 256, dev, radius=None)                                           # now the single point survives
    _run([np.zeros((0, 3), np.float32)], 8, dev, nraw=1)


def test_each_stage_switched_off(dev, real):
    clouds = [real[2], real[3]]
    _run(clouds, 4096, dev, voxel_size=None)
    _run(clouds, 4096, dev, radius=None)
    _run(clouds, 4096, dev, voxel_size=None, radius=None)
    _run(clouds, 16384, dev, voxel_size=None, radius=None)
    _run(clouds, 4096, dev, voxel_size=0.5, radius=2.0, nb_points=16)


def test_batch_of_1_and_of_32(dev, real):
    _run([real[5]], 4096, dev)
    rng = np.random.default_rng(8)
    base = real[0]
    clouds = [np.ascontiguousarray(base[rng.permutation(base.shape[0])[:int(n)]]) for n in rng.integers(0, 6000, 32)]
    clouds[7] = clouds[7][:0]
    _run(clouds, 2048, dev)


def test_nraw_131072(dev):
    rng = np.random.default_rng(9)
    big = np.stack([rng.uniform(-60, 60, 131072), rng.uniform(-60, 60, 131072), rng.normal(0, 0.3, 131072)], axis=1)
    big = np.ascontiguousarray(big, np.float32)
    _, nv, counts, _ = _run([big, big[:70000]], 65536, dev)
    assert counts[0, 0] == 131072 and counts[0, 1] < 131072 and nv[0] == 65536
    _run([big], 16384, dev, voxel_size=None, radius=None)


def test_void_cloud_beyond_the_keys(dev):
    from dh3d_amd import utils
    wide = np.array([[0, 0, 0], [1e6, 0, 0], [3, 3, 3]], np.float32)              # 5e6 cells of 0.2 on x
    ok = np.random.default_rng(10).random((300, 3), dtype=np.float32)
    points, nv, counts, _ = _run([wide, ok], 64, dev)
    assert counts[0].tolist() == [3, -1, -1] and nv[0] == 0 and nv[1] > 0
    raw, num = _batch([wide, ok], dev)
    with pytest.raises(ValueError, match="2\\^21"):
        utils.prepare_clouds(raw, num, 64, check=True)
    utils.prepare_clouds(raw[1:], num[1:], 64, check=True)


def test_sentinel_outputs_and_dirty_workspace(dev, real):
    from dh3d_amd import _lib as L
    clouds = [real[3], R.tie_cases()["crowded_voxels"][0], np.zeros((0, 3), np.float32)]
    raw, num = _batch(clouds, dev)
    B, N, T = raw.shape[0], raw.shape[1], 4000
    lib = L.lib()
    nbytes = lib.dh3d_prepare_clouds_workspace(B, N, T)
    results = []
    for fill in (0xFF, 0x00, 0x5A):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
        points = torch.full((B, T, 3), -7.0, dtype=torch.float32, device=dev)
        nv = torch.full((B,), -7, dtype=torch.int32, device=dev)
        counts = torch.full((B, 3), -7, dtype=torch.int32, device=dev)
        cen = torch.full((B, 3), -7.0, dtype=torch.float64, device=dev)
        L.check(lib.dh3d_prepare_clouds(B, N, T, L.ptr(raw), L.ptr(num), 0.2, 1.0, 4, 1, L.ptr(points), L.ptr(nv), L.ptr(counts),
                                        L.ptr(cen), L.ptr(ws), nbytes, L.stream_ptr()), "prepare_clouds")
        torch.cuda.synchronize()
        assert not bool((points == -7.0).any()) and not bool((nv == -7).any()) and not bool((counts == -7).any())
        assert not bool((cen == -7.0).any())
        results.append(_check((points, nv, counts, cen), clouds, T))
    for r in results[1:]:
        for a, o in zip(r, results[0]):
            assert np.array_equal(a, o)


def test_graph_replay_with_other_sizes(dev, real):
    from dh3d_amd import utils
    N, T = 16384, 8192
    sets = [[real[0], real[2]], [real[3], real[1]], [real[5][:1], real[4]], [real[0], real[2]]]
    raw, num = _batch(sets[0], dev, N)

    def run():
        return utils.prepare_clouds(raw, num, T)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run()
    for clouds in sets[1:]:
        r2, n2 = _batch(clouds, dev, N)
        raw.copy_(r2); num.copy_(n2)
        for o in outs:
            o.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        _check(outs, clouds, T)
        eager = run()
        for o, e in zip(outs, eager):
            assert torch.equal(o, e)


def test_prepare_forward_nms_chain(dev, real):
    """prepare_clouds -> DH3D.forward(num_valid) -> batched_nms on the device equals the chain fed with the restatement's
    host-prepared batch."""
    from dh3d_amd import ConfigFactory, utils
    from dh3d_amd.model import DH3D
    model = DH3D(ConfigFactory("detection_config").getconfig()).init_synthetic(0).to(dev).eval().prepare()
    clouds, T = [real[0], real[2]], 8192
    raw, num = _batch(clouds, dev)
    nms = dict(nms_radius=0.5, min_response_ratio=0.01, max_keypoints=512)

    def chain(points, num_valid):
        with torch.no_grad():
            outs = model(points, fetch=("xyz_feat_att",), num_valid=num_valid)
            xfa = outs["xyz_feat_att"]
            count, inds = utils.batched_nms(xfa[:, :, 0:3].contiguous(), xfa[:, :, 131], num_valid=num_valid, invert=True, **nms)
        return xfa, count, inds

    points, num_valid, counts, centroid = utils.prepare_clouds(raw, num, T)
    got = chain(points, num_valid)
    host = [R.prepare_cloud(c, T, centroid=centroid[b].cpu().numpy()) for b, c in enumerate(clouds)]
    hp = torch.from_numpy(np.stack([h["points"] for h in host])).to(dev)
    hn = torch.tensor([h["num_valid"] for h in host], dtype=torch.int32, device=dev)
    assert hn.tolist() == [8192, 7201]
    exp = chain(hp, hn)
    for a, e, name in zip(got, exp, ("xyz_feat_att", "kp_count", "kp_inds")):
        assert torch.equal(a, e), name
    assert int(got[1].min()) > 0
