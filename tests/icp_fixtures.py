"""What the GPU tests of the three ICP rules share (test_icp_gpu, test_icp_plane_gpu, test_gicp_gpu): the bit comparison of
result dicts and the PlaceIndex scene of their test_localize_* tests."""
import os

import numpy as np
import torch

import icp_reference as ir

HERE = os.path.dirname(os.path.abspath(__file__))


def _bits_equal(a, b):
    if a.dtype == torch.float64:
        return torch.equal(a.view(torch.int64), b.view(torch.int64))  # (bit for bit, NaN included)
    return torch.equal(a, b)


def _assert_same(got, exp, what):
    assert set(got) == set(exp), what
    for k in exp:
        assert _bits_equal(got[k], exp[k]), (what, k)


def _place_rows(rng, pts, M=64, D=128):
    rows = np.zeros((M, 3 + D + 1), np.float32)
    d = rng.standard_normal((M, D))
    rows[:, :3] = pts[rng.choice(len(pts), M, replace=False)]
    rows[:, 3:3 + D] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return rows


def place_scene(names, N):
    """Places and one query for PlaceIndex.localize: N-point subsets of the demo clouds `names` with 64 keypoint rows each
    (count 64, 60, 64, ...) and unit global descriptors g; the query is a moved copy of place 1 by the pose T (5 cm noise
    on the keypoints, 2 cm on the cloud, both shuffled).  Returns a dict of numpy arrays: clouds, rows, count, g, T, qrows
    [1, 64, row_dim], qcloud [1, N, 3]."""
    rng = np.random.default_rng(24)
    demo = np.load(os.path.join(HERE, "golden", "demo_clouds.npz"))
    clouds = np.stack([demo[k][rng.permutation(len(demo[k]))[:N]] for k in names]).astype(np.float32)
    rows = np.stack([_place_rows(rng, c) for c in clouds])
    count = np.array([64, 60, 64][:len(names)], np.int32)
    g = rng.standard_normal((len(names), 256)).astype(np.float32)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    R, tr = ir.rotation((0.1, 0.2, 1.0), 0.6), np.array([3.0, -2.0, 0.5])
    n = count[1]
    qrows = np.zeros((1, 64, rows.shape[2]), np.float32)
    perm = rng.permutation(n)
    qrows[0, perm, :3] = (rows[1, :n, :3].astype(np.float64) - tr) @ R + rng.normal(0.0, 0.05, (n, 3))
    qrows[0, perm, 3:131] = rows[1, :n, 3:131] + 0.01 * rng.standard_normal((n, 128)).astype(np.float32)
    qcloud = ((clouds[1].astype(np.float64) - tr) @ R + rng.normal(0.0, 0.02, (N, 3)))[rng.permutation(N)][None].astype(np.float32)
    return dict(clouds=clouds, rows=rows, count=count, g=g, T=np.concatenate([R, tr[:, None]], axis=1), qrows=qrows, qcloud=qcloud)


def place_index(dev, s):
    """A PlaceIndex over place_scene's places, clouds included."""
    from dh3d_amd import retrieval
    index = retrieval.PlaceIndex(dim=256, capacity=8, device=dev, keypoints=64, row_dim=s["rows"].shape[2],
                                 points=s["clouds"].shape[1])
    index.add(s["g"], None, s["rows"], s["count"], cloud=s["clouds"])
    return index
