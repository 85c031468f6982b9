"""GPU parity of the full-cloud kNN (pm.knn_grid, csrc/knn.hip dh3d_knn_grid) in every launch plan it makes, on crowded,
uniform and mixed batches.  The plan depends on the query groups G = B * ceil(N / 64) (pm.knn_grid_plan, the launcher's
own function); inside a plan each cloud goes one of two ways by the crowded flag the sort writes (cells[:, 4106]):

  code 4  G <= 1280         knn_grid_kernel<4, 4>: crowded clouds on the pruned scan, four waves per group, same launch
  code 2  1281 <= G <= 4096 knn_grid_kernel<4, 2>: two groups per workgroup, two waves each (odd ceil(N / 64): half of
                            the last workgroup has no group)
  code 0  G > 4096          knn_grid_kernel<4, 0> for the uniform clouds, then knn_sorted_kernel<4 | 8> gated on the flag

Every case names its plan code, grid drop and per-cloud flags and asserts them before comparing anything, so a later
threshold change cannot quietly move a case out of the regime it covers.  Outputs are pre-filled with a sentinel: a cloud
that neither launch serves fails even where the allocator hands back a block holding a previous correct answer."""
import zlib

import numpy as np
import pytest
import torch

from test_ops_gpu import _knn_clouds

pytestmark = pytest.mark.gpu

NN_SENTINEL = -7
DIST_SENTINEL = 0x7FC00BAD  # a quiet NaN no kernel writes
CROWDED = {"scene": 1, "scene_lattice": 1, "scene_duplicates": 1, "clusters": 1, "one_point": 1,
           "uniform": 0, "lattice": 0, "duplicates": 0}


def _cloud(kind, N, rng):
    if kind == "scene_lattice":  # a scene on a 1/64 lattice: exact distance ties on the pruned scan
        return (np.round(_knn_clouds("scene", 1, N, rng)[0] * 64) / 64).astype(np.float32)
    if kind == "scene_duplicates":  # a scene with every point twice: distance-0 ties on the pruned scan
        p = _knn_clouds("scene", 1, N, rng)[0]
        p[N // 2:] = p[: N - N // 2]
        return p
    return _knn_clouds(kind, 1, N, rng)[0]


def _batch(key, kinds, N):
    rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
    return np.ascontiguousarray(np.stack([_cloud(k, N, rng) for k in kinds]))


def _cyc(B, *kinds):
    return tuple(kinds[b % len(kinds)] for b in range(B))


def _tail(B, kind, last):
    return (kind,) * (B - 1) + (last,)


# id: (N, K, per-cloud kinds (B = their number), expected plan code, expected grid drop D)
CASES = {
    # <4,4>: the control, a mixed batch (G 768)
    "c4_mixed_6x8192": (8192, 8, _cyc(6, "scene", "uniform"), 4, 0),
    # <4,2>: the shipped global batch (G 2048) and the cfg4 training batch (G 1408) on crowded data
    "c2_scene_32x4096_k8": (4096, 8, _cyc(32, "scene"), 2, 0),
    "c2_scene_22x4096_k5": (4096, 5, _cyc(22, "scene"), 2, 0),
    # <4,2> with odd ceil(N / 64): ngq 63 (G 1512) and 125 (G 1500); crowded, then mixed with degenerate clouds
    "c2_odd_scene_24x4031_k3": (4031, 3, _cyc(24, "scene"), 2, 0),
    "c2_odd_ties_12x8000_k4": (8000, 4, _cyc(12, "scene", "scene_lattice", "scene_duplicates", "one_point"), 2, 0),
    "c2_odd_mixed_24x4031_k8": (4031, 8, _cyc(24, "scene", "uniform", "one_point", "lattice"), 2, 0),
    # <4,2> mixed: alternating, and all uniform but the last cloud
    "c2_mixed_32x4096_k8": (4096, 8, _cyc(32, "scene", "uniform"), 2, 0),
    "c2_last_crowded_32x4096_k4": (4096, 4, _tail(32, "uniform", "scene"), 2, 0),
    # the thresholds' edges: G 1280 / 1281 (ngq 61, odd) / 4096 / 4097
    "edge_1280_20x4096_k8": (4096, 8, _cyc(20, "scene", "uniform"), 4, 0),
    "edge_1281_21x3904_k1": (3904, 1, _cyc(21, "scene", "uniform"), 2, 0),
    "edge_4096_64x4096_k5": (4096, 5, _cyc(64, "scene", "uniform", "scene_duplicates", "duplicates"), 2, 0),
    "edge_4097_241x1088_k8": (1088, 8, _cyc(241, "clusters", "uniform", "one_point", "lattice"), 0, 2),
    # the gated pair: knn_sorted_kernel<4> (K <= 4) and <8> (K 5..8) behind the gate (G 5120), a drop-2 grid (G 4800)
    "g_mixed_40x8192_k4": (8192, 4, _cyc(40, "scene", "uniform"), 0, 0),
    "g_ties_40x8192_k5": (8192, 5, _cyc(40, "scene_lattice", "lattice", "scene_duplicates", "duplicates", "one_point",
                                        "uniform"), 0, 0),
    "g_drop2_300x1000_k3": (1000, 3, _cyc(300, "clusters", "uniform"), 0, 2),
    # either launch leaves every cloud to the other (G 4224 / 4160)
    "g_all_crowded_33x8192_k1": (8192, 1, _cyc(33, "scene"), 0, 0),
    "g_all_uniform_65x4096_k8": (4096, 8, _cyc(65, "uniform"), 0, 0),
}


def _flags(kinds):
    return [CROWDED[k] for k in kinds]


def _oracle_clouds(flags):
    """the first crowded and the first uniform cloud of the batch (the CPU oracle's share of a case)"""
    return sorted({flags.index(f) for f in (0, 1) if f in flags})


def _knn_grid_checked(srt, gbox, cells, K):
    """pm.knn_grid into outputs pre-filled with the sentinel; asserts no sentinel survives"""
    from dh3d_amd import pm
    B, N = srt.shape[:2]
    nn = torch.full((B, N, K), NN_SENTINEL, dtype=torch.int32, device=srt.device)
    dist = torch.full((B, N, K), DIST_SENTINEL, dtype=torch.int32, device=srt.device).view(torch.float32)
    got = pm.knn_grid(srt, gbox, cells, K, out=(nn, dist))
    assert got[0] is nn and got[1] is dist
    assert not bool((nn == NN_SENTINEL).any()), "knn_grid left ids unwritten"
    assert not bool((dist.view(torch.int32) == DIST_SENTINEL).any()), "knn_grid left distances unwritten"
    return nn, dist


def test_cases_cover_every_plan_and_regime():
    """The CASES table reaches every plan the launcher makes for K <= 8, with a crowded cloud and a mixed batch in each,
    odd ceil(N / 64) under code 2, both widths of the gated kernel, and every K of {1, 3, 4, 5, 8} on crowded clouds of
    the two new regimes (host only: the plan query needs no GPU)."""
    from dh3d_amd import pm
    seen = set()
    for name, (N, K, kinds, code, drop) in CASES.items():
        B = len(kinds)
        assert pm.knn_grid_plan(B, N, K) == (code, drop), name
        fl = _flags(kinds)
        if 0 < sum(fl) < B:
            seen.add((code, "mixed"))
        if not any(fl):
            continue
        seen |= {(code, "crowded"), ("K", code, K)}
        if ((N + 63) // 64) % 2:
            seen.add(("odd", code))
        if code == 0:
            seen.add(("gated", 4 if K <= 4 else 8))
    want = {(c, w) for c in (0, 2, 4) for w in ("crowded", "mixed")} | {("odd", 2), ("gated", 4), ("gated", 8)}
    want |= {("K", c, k) for c in (0, 2) for k in (1, 3, 4, 5, 8)}  # (every K on crowded clouds of the new regimes)
    assert want <= seen, sorted(map(str, want - seen))
    codes = {pm.knn_grid_plan(B, N, K)[0] for B in (1, 20, 21, 64, 65, 300) for N in (64, 1000, 4096, 8192, 16384)
             for K in (1, 8)}
    assert codes == {0, 2, 4}


@pytest.mark.parametrize("case", list(CASES))
def test_knn_grid_regime_bit_equal_to_brute_force_and_oracle(dev, oracle, case):
    """ids and distance bits == pm.knn_xyz (pinned to the oracle elsewhere) on every cloud, == oracle.knn_bruteforce on
    a crowded and a uniform cloud of the batch, and no sentinel left anywhere."""
    from dh3d_amd import pm
    N, K, kinds, code, drop = CASES[case]
    B = len(kinds)
    assert pm.knn_grid_plan(B, N, K) == (code, drop)
    pts = _batch((case, B, N, K), kinds, N)
    t = torch.from_numpy(pts).to(dev)
    srt, gbox, cells = pm.spatial_sort_cells(t)
    flags = (cells[:, 4106] != 0).int().cpu().tolist()
    assert flags == _flags(kinds), (case, flags)
    nn, dist = _knn_grid_checked(srt, gbox, cells, K)
    nn_b, d_b = pm.knn_xyz(t, K)
    bad = (nn != nn_b).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, (case, "clouds whose ids differ from knn_xyz", bad, [kinds[b] for b in bad])
    assert torch.equal(dist.view(torch.int32), d_b.view(torch.int32)), case
    nn, dist = nn.cpu().numpy(), dist.cpu().numpy()
    for b in _oracle_clouds(flags):
        nn_o, d_o = oracle.knn_bruteforce(np.ascontiguousarray(pts[b:b + 1].transpose(0, 2, 1)), K)
        assert np.array_equal(nn[b], nn_o[0]), (case, b, kinds[b])
        assert np.array_equal(dist[b].view(np.uint32), d_o[0].view(np.uint32)), (case, b, kinds[b])


def test_knn_grid_shipped_scene_batch_vs_float64(dev):
    """32 x 4096 scenes (code 2): ids == a float64 cdist + argsort on every row whose first nine float64 distances are
    further apart than a few float32 ulps (test_ops_gpu.test_knn_config_size_vs_the_references_own_checker's rule)."""
    from scipy.spatial.distance import cdist
    from dh3d_amd import pm
    N, K, kinds, code, _ = CASES["c2_scene_32x4096_k8"]
    pts = _batch(("f64", len(kinds), N, K), kinds, N)
    assert pm.knn_grid_plan(len(kinds), N, K)[0] == code
    srt, gbox, cells = pm.spatial_sort_cells(torch.from_numpy(pts).to(dev))
    assert bool((cells[:, 4106] != 0).all())
    nn, dist = _knn_grid_checked(srt, gbox, cells, K)
    nn, dist = nn.cpu().numpy(), dist.cpu().numpy()
    for b in (0, 13, 31):
        p64 = pts[b].astype(np.float64)
        d = cdist(p64, p64, "euclidean")
        order = np.argsort(d, axis=1, kind="stable")[:, :9]
        exp_d = np.take_along_axis(d, order, 1)
        gap = np.diff(exp_d, axis=1)
        clear = (gap > 4 * np.finfo(np.float32).eps * np.maximum(exp_d[:, 1:], 1.0)).all(1)
        assert clear.mean() > 0.99, (b, clear.mean())
        assert np.array_equal(nn[b][clear], order[clear, :K]), b
        assert np.abs(dist[b] - exp_d[:, :K]).max() < 2e-6, b


THREE_NN_CASES = {  # id: (N, m, per-cloud kinds)
    "scene_32x4096_m512": (4096, 512, _cyc(32, "scene")),
    "mixed_32x4096_m512": (4096, 512, _cyc(32, "scene", "uniform")),
    "scene_22x4096_m512": (4096, 512, _cyc(22, "scene")),
}


@pytest.mark.parametrize("case", list(THREE_NN_CASES))
def test_three_nn_sorted_shipped_batches(dev, oracle, case):
    """The box-pruned three_nn_sorted (128 <= m <= kNNChunk = 1024 and both boxes given: csrc/pointnet2.hip) at the shipped
    batch sizes, its per-cloud group rotation (g + 37 b) % groups across 22 / 32 clouds, on samples the FPS kernel takes
    from each cloud as the model does: ids and distance bits == ops.three_nn, and == oracle.three_nn on a few clouds."""
    from dh3d_amd import ops, pm
    N, m, kinds = THREE_NN_CASES[case]
    assert 128 <= m <= 1024  # the pruned kernel's range
    B = len(kinds)
    pts = _batch(("three_nn", case, B, N, m), kinds, N)
    t = torch.from_numpy(pts).to(dev)
    idx = ops.farthest_point_sample(m, t)
    ts = torch.gather(t, 1, idx.long()[:, :, None].expand(B, m, 3)).contiguous()
    d0, i0 = ops.three_nn(t, ts)
    s1, g1 = pm.spatial_sort(t)
    s2, g2 = pm.spatial_sort(ts)
    d1, i1 = pm.three_nn_sorted(s1, g1, s2, g2)
    bad = (i0 != i1).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, (case, "clouds whose ids differ from three_nn", bad)
    assert torch.equal(d0.view(torch.int32), d1.view(torch.int32)), case
    xs = ts.cpu().numpy()
    d1, i1 = d1.cpu().numpy(), i1.cpu().numpy()
    for b in (0, 1, B - 1):
        de, ie = oracle.three_nn(pts[b:b + 1], xs[b:b + 1])
        assert np.array_equal(i1[b], ie[0]), (case, b)
        assert np.array_equal(d1[b].view(np.uint32), de[0].view(np.uint32)), (case, b)


def test_global_forward_32x4096_scenes_knn_ids(dev):
    """The model's own dispatch: a global-config forward on 32 x 4096 scene clouds (full-cloud kNN on knn_grid code 2, all
    clouds crowded) -- knn_inds == pm.knn_xyz, and the sampled set's ids == the brute-force kNN of the FPS picks."""
    from test_parity_fullsize_gpu import _build
    from dh3d_amd import pm
    B, N = 32, 4096
    m = _build("global_config", dev, seed=41)
    K = m.knn_num
    assert K <= 8 and pm.knn_grid_plan(B, N, K)[0] == 2
    pts = _batch(("global_forward", B, N), _cyc(B, "scene"), N)
    t = torch.from_numpy(pts).to(dev)
    assert bool((pm.spatial_sort_cells(t)[2][:, 4106] != 0).all())
    with torch.no_grad():
        outs = m(t, fetch=("globaldesc", "knn_inds", "sampled_knn_inds", "fps_inds"))
    geo = m._last_geo
    assert geo.cells is not None and geo._lv["_path"]["knn"] == "grid_fps"  # both kNNs went to knn_grid
    nn_b, _ = pm.knn_xyz(t, K)
    assert torch.equal(outs["knn_inds"], nn_b)
    idx = outs["fps_inds"]
    xs = torch.gather(t, 1, idx.long()[:, :, None].expand(B, idx.shape[1], 3)).contiguous()
    nn_s, _ = pm.knn_xyz(xs, K)
    assert torch.equal(outs["sampled_knn_inds"], nn_s)
