"""GPU parity of the sampled-level dispatcher (backbones.compute_level / finish_level): FPS -> sampled coordinates ->
the sampled set's kNN -> three_nn back to the full cloud, built the way the model builds it (Geometry, optionally
Morton-ordered with or without the cell table), against the CPU oracle at every dilate and on each side of every
threshold the dispatcher chooses a kernel by.  Every case also names the paths it must take (lv["_path"]), so a
later change to a threshold cannot quietly drop a path from the suite."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cloud(kind, B, N, seed):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return rng.random((B, N, 3), dtype=np.float32)
    if kind == "blob":  # a dense blob plus a sparse rest (test_ops_gpu.test_fps_sorted_identical)
        xyz = rng.random((B, N, 3), dtype=np.float32)
        xyz[:, : N // 3] = xyz[:, : N // 3] * 0.02 + 0.5
        return xyz
    if kind == "dup":  # every point twice, shuffled: zero distances and tied picks
        base = rng.random((B, (N + 1) // 2, 3), dtype=np.float32)
        return np.ascontiguousarray(np.repeat(base, 2, 1)[:, :N][:, rng.permutation(N)])
    if kind == "lattice":  # integer lattice points: exact distance ties everywhere
        s = int(np.ceil(N ** (1.0 / 3.0))) + 1
        g = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float32)] * 3, indexing="ij"), -1).reshape(-1, 3)
        return np.stack([g[rng.choice(len(g), N, replace=False)] for _ in range(B)])
    raise ValueError(kind)


def _edge_n(ordered):
    """Largest N whose dilate-2 level (m = N // 2) still fits the LDS budget of the ordered FPS output (ordered=True) or
    of the plain sorted kernel's coordinate table -- from the library's own query."""
    from dh3d_amd import pm
    hi = 8192 if ordered else 12288
    fit = [n for n in range(4096, hi + 1) if pm.fps_sorted_fits(n, n // 2, ordered=ordered)]
    assert fit and fit[-1] < hi, "the dilate-2 boundary moved out of the ordered range"
    return fit[-1]


# id: (B, N, dilate, knn, sort, fps_contract, cloud, (fps path, kNN path, three_nn path), extras)
#   sort: None (no Geometry.ordered), "sort" (records + boxes), "cells" (+ the cell table)
#   N = "ordered_edge" / "table_edge" (+1): the exact LDS boundary at dilate 2, from pm.fps_sorted_fits
CASES = {
    # the shipped shapes (bench local and global): ordered FPS, the FPS-written cell table from 16384 sampled points
    "local_8x8192_d8": (8, 8192, 8, 8, "cells", None, "uniform", ("ordered", "brute", "sorted"), {"walk_plan"}),
    "global_32x4096_d8": (32, 4096, 8, 8, "cells", None, "uniform", ("ordered", "grid_fps", "sorted"), set()),
    "16x8192_d8_blob": (16, 8192, 8, 8, "cells", None, "blob", ("ordered", "grid_fps", "sorted"), set()),
    "cfg5_4x16384_d8": (4, 16384, 8, 8, "cells", None, "uniform", ("sorted_cloud", "brute", "sorted"), set()),
    # N = 8192 at dilates 2, 3, 4 (8: above)
    "8192_d2": (2, 8192, 2, 8, "cells", None, "uniform", ("sorted", "grid", "sorted"), set()),
    "8192_d3_nocells": (2, 8192, 3, 8, "sort", None, "dup", ("ordered", "grid", "sorted"), set()),  # m = 2730: m % 64 != 0
    "8192_d4_lattice": (8, 8192, 4, 8, "cells", None, "lattice", ("ordered", "grid_fps", "sorted"), set()),
    # N = 12288 at dilates 2, 3, 4, 8: the coordinate table fits up to m = 3564
    "12288_d2_k16": (1, 12288, 2, 16, "sort", None, "uniform", ("sorted_cloud", "sorted", "sorted"), set()),
    "12288_d3": (2, 12288, 3, 8, "sort", None, "blob", ("sorted_cloud", "grid", "sorted"), set()),
    "12288_d4": (2, 12288, 4, 8, "sort", None, "uniform", ("sorted", "grid", "sorted"), set()),
    "12288_d8": (2, 12288, 8, 8, "cells", None, "lattice", ("sorted", "brute", "sorted"), set()),
    "13000_d8": (2, 13000, 8, 8, "sort", None, "uniform", ("sorted_cloud", "brute", "sorted"), set()),
    # the exact LDS boundaries (largest fitting N at dilate 2 and one point more)
    "ordered_edge": (5, "ordered_edge", 2, 8, "cells", None, "uniform", ("ordered", "grid_fps", "sorted"), set()),
    "ordered_edge+1": (5, "ordered_edge+1", 2, 8, "cells", None, "uniform", ("sorted", "grid", "sorted"), set()),
    "table_edge": (2, "table_edge", 2, 8, "sort", None, "uniform", ("sorted", "grid", "sorted"), set()),
    "table_edge+1": (2, "table_edge+1", 2, 8, "sort", None, "blob", ("sorted_cloud", "grid", "sorted"), set()),
    # the any-N op
    "small_2000_d4": (4, 2000, 4, 8, "sort", None, "uniform", ("any_n", "brute", "sorted"), set()),
    "contract0_8192": (2, 8192, 8, 8, "cells", 0, "blob", ("any_n", "brute", "sorted"), set()),
    "contract1_4096": (2, 4096, 8, 8, "sort", 1, "dup", ("any_n", "brute", "sorted"), set()),
    "unsorted_8192": (2, 8192, 8, 8, None, None, "uniform", ("any_n", "brute", "plain"), set()),
    "big_20000_d8": (1, 20000, 8, 8, None, None, "uniform", ("any_n", "grid", "plain"), set()),
    "npoint_17000": (1, 34000, 2, 8, None, None, "uniform", ("any_n", "brute", "plain"), set()),
    # three_nn on the plain kernel below 256 sampled points (a sorted cloud all the same)
    "m128_sorted": (4, 4096, 32, 8, "sort", None, "uniform", ("ordered", "brute", "plain"), set()),
}


@pytest.mark.parametrize("case", list(CASES))
def test_level_matches_oracle(dev, oracle, case):
    from dh3d_amd import backbones as bb
    from dh3d_amd import pm
    B, N, dilate, knn, sort, contract, kind, want, extras = CASES[case]
    if isinstance(N, str):
        N = _edge_n(N.startswith("ordered")) + N.endswith("+1")
    xyz = _cloud(kind, B, N, seed=N * 31 + dilate * 7 + B)
    t = T(xyz, dev)
    geo = bb.Geometry(t, knn, fps_contract=contract)
    if sort is not None:
        geo.ordered(cells=sort == "cells")
    lv = geo.level(dilate, knn, finish=False)
    if "walk_plan" in extras:
        lv["_want_walk_plan"] = True
    lv = geo.finish(lv)
    torch.cuda.synchronize()
    m = N // dilate

    idx = oracle.farthest_point_sample(m, xyz, contract=contract != 0)
    assert np.array_equal(lv["idx"].cpu().numpy(), idx), "FPS ids"
    xyz_s = np.take_along_axis(xyz, idx[:, :, None].astype(np.int64), 1)
    assert np.array_equal(lv["xyz_s"].cpu().numpy(), xyz_s), "sampled coordinates"
    nn, _ = oracle.knn_bruteforce(np.ascontiguousarray(xyz_s.transpose(0, 2, 1)), knn)
    assert np.array_equal(lv["nbr_s"].cpu().numpy(), nn), "sampled set's kNN ids"
    d3, i3 = oracle.three_nn(xyz, xyz_s)
    assert np.array_equal(lv["nn3_idx"].cpu().numpy(), i3), "three_nn ids"
    assert np.array_equal(lv["nn3_dist"].cpu().numpy().view(np.int32), d3.view(np.int32)), "three_nn distance bits"

    got = (lv["_path"]["fps"], lv["_path"]["knn"], lv["_path"]["nn3"])
    assert got == want, "dispatch moved: %s takes %s, expected %s" % (case, got, want)
    assert ("_ordered_s" in lv) == (sort is not None and (want[0] == "ordered" or want[1] in ("grid", "sorted")))
    if "walk_plan" in extras:  # finish_level's global-tail branch: the plan behind three_nn, as built directly
        again = pm.walk_plan(lv["nn3_idx"], lv["nn3_dist"], geo.sorted[0], m)
        assert torch.equal(lv["walk_plan"], again)


def _randomise_bn(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, buf in module.named_buffers():
            if name.endswith("mean_EMA"):
                buf.copy_(0.1 * torch.randn(buf.shape, generator=g))
            elif name.endswith("variance_EMA"):
                buf.copy_(0.5 + torch.rand(buf.shape, generator=g))
        for name, p in module.named_parameters():
            if name.endswith("gamma"):
                p.copy_(0.75 + 0.5 * torch.rand(p.shape, generator=g))


def test_flex_conv_dilate_block_at_dilate_2(dev):
    """flex_conv_dilate (core/backbones.py:58-101) at dilate 2 on 8192-point clouds, Morton-ordered with the cell table as
    the model orders them: the level falls back from the ordered FPS output (m = 4096 does not fit beside the coordinate
    table) and the block's up-sampling / concat conv run on it -- against oracle/model_np."""
    from dh3d_amd import backbones as bb
    from oracle import model_np
    torch.manual_seed(5)
    B, N = 2, 8192
    blk = bb.FlexConvDilate(64, [128, 128], dilate=2, knn=8)
    _randomise_bn(blk, 6)
    blk = blk.to(dev).eval()
    rng = np.random.default_rng(2024)
    xyz = _cloud("blob", B, N, 2025)
    feat = rng.standard_normal((B, N, 64)).astype(np.float32)
    geo = bb.Geometry(T(xyz, dev), 8)
    geo.ordered(cells=True)
    with torch.no_grad():
        got = blk(geo, T(feat, dev)).cpu().numpy()
    lv = geo.levels[(2, 8)]
    assert (lv["_path"]["fps"], lv["_path"]["knn"], lv["_path"]["nn3"]) == ("sorted", "grid", "sorted")
    w = {"blk/" + k.replace(".", "/").replace("mean_EMA", "mean/EMA").replace("variance_EMA", "variance/EMA"):
         v.detach().cpu().numpy() for k, v in blk.state_dict().items()}
    _, ref = model_np.flex_conv_dilate(xyz, feat, 2, 8, [128, 128], "blk", w, 1e-5)
    assert got.shape == ref.shape == (B, N, 128)
    assert np.allclose(got, ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max()), float(np.abs(got - ref).max())
