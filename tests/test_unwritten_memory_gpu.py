"""GPU: no result depends on memory nobody wrote.  Every buffer dh3d_amd uses comes from torch.empty / torch.empty_like /
Tensor.new_empty, so tests/poisoned_alloc.py can make all of them start from chosen garbage: each case below runs four
times -- plain, and with every allocation pre-filled by the "nan", "pos" and "neg" poisons -- and the four runs must
agree:

  * bit for bit where the operator has no floating-point atomics;
  * where results are summed by atomics, within the tolerance that operator's OWN test uses (named at each checker), and
    with no NaN or infinity under a poison where the plain run has none.

That covers an output tail nobody wrote, a tile's padding rows read by a reduction, a workspace segment read before it
is written, and an accumulator documented as "zeroed by the CALLER" (include/dh3d_hip.h) that a wrapper takes from
torch.empty instead of pm.zeros: the three poisons then give three different answers.  No element is masked out:
include/dh3d_hip.h declares none undefined.

A case is a function that builds its fixed inputs OUTSIDE the poisoned context and returns the call to make inside it
(and, for atomics-summed outputs, {output index: checker}).  A new wrapper is covered by adding a case.  Shapes are the
smallest at which each kernel takes each of its paths: ragged row counts (no multiple of 32 / 64 / 128 / 256), two or
more clouds, per-cloud counts below the capacity.

Below the operators: the whole inference forward of the three configs (eager and through a captured graph), the two
trainers' steps (eager, the capture, replays) against unpoisoned twins, and the recorded situation of an earlier
graph's pool going back to the allocator with 7.0 in it ahead of the two-shape trainer sequence.
"""
import copy

import numpy as np
import pytest
import torch

from poisoned_alloc import KINDS, poisoned

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ comparing runs
def _flat(o, prefix="out"):
    """Nested tuples / lists / dicts of tensors -> [(name, tensor or None)] in a fixed order."""
    if o is None or isinstance(o, torch.Tensor):
        return [(prefix, o)]
    if isinstance(o, dict):
        return [x for k in sorted(o) for x in _flat(o[k], "%s[%r]" % (prefix, k))]
    if isinstance(o, (tuple, list)):
        return [x for i, v in enumerate(o) for x in _flat(v, "%s[%d]" % (prefix, i))]
    return [(prefix, torch.as_tensor(o))]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().reshape(-1).view(torch.uint8),
                                                                     b.contiguous().reshape(-1).view(torch.uint8))


def _agree(name, runs, atomic=None):
    """runs: {kind: call's outputs}, kind None = the plain run; atomic: {flat output index, or the key of a call that returns
    a dict of tensors: checker(got, plain)}."""
    plain = _flat(runs[None])
    atomic = {("out[%r]" % k if isinstance(k, str) else k): v for k, v in (atomic or {}).items()}
    for kind in KINDS:
        got = _flat(runs[kind])
        assert [n for n, _ in got] == [n for n, _ in plain], (name, kind)
        for i, ((nm, a), (_, b)) in enumerate(zip(got, plain)):
            assert (a is None) == (b is None), (name, kind, nm)
            if b is None:
                continue
            check = atomic.get(i, atomic.get(nm))
            if check is not None:
                fa, fb = torch.isfinite(a), torch.isfinite(b)
                assert torch.equal(fa, fb), "%s under %r: %s has NaN / inf where the plain run has none" % (name, kind, nm)
                try:
                    check(a.detach().cpu().numpy(), b.detach().cpu().numpy())
                except AssertionError as e:
                    raise AssertionError("%s under %r: %s beyond its bound: %s" % (name, kind, nm, e))
            else:
                if not _same_bits(a, b):
                    fa, fb = a.reshape(-1), b.reshape(-1)
                    bad = (fa.contiguous().view(torch.uint8).reshape(fa.numel(), -1)
                           != fb.contiguous().view(torch.uint8).reshape(fb.numel(), -1)).any(1).nonzero().reshape(-1)
                    at = [int(i) for i in bad[:4]]
                    raise AssertionError("%s under %r: %s %s differs from the plain run in %d of %d elements; flat indices %s: "
                                         "got %s, plain %s" % (name, kind, nm, tuple(a.shape), bad.numel(), a.numel(), at,
                                                               [fa[i].item() for i in at], [fb[i].item() for i in at]))


def _run_four(name, call, atomic=None):
    runs = {}
    for kind in (None,) + KINDS:
        with poisoned(kind):
            out = call()
            torch.cuda.synchronize()
        runs[kind] = out
    _agree(name, runs, atomic)


# checkers for atomics-summed outputs: each is the assertion of that operator's own test
def max_scaled(a, b):       # tests/test_backward_gpu.py test_flex_conv_bwd_factorised_vs_oracle: 1e-4 of the largest entry
    assert float(np.abs(a - b).max()) <= 1e-4 * float(np.abs(b).max())


def deconv_close(a, b):     # tests/test_flex_deconv_gpu.py: FlexDeconv's weight gradients
    assert np.allclose(a, b, rtol=1e-3, atol=1e-3)


def interp_bwd_close(a, b):  # tests/test_training_gpu.py test_three_interpolate_sorted_backward_matches_the_drop_in_op
    assert float(np.abs(a - b).max()) <= 2e-5 * float(np.abs(b).max())


def ops_close(rtol, atol):  # tests/test_ops_gpu.py `close` (the reference's criterion) at the values its tests pass
    def check(a, b):
        assert np.allclose(a, b, rtol=rtol, atol=atol)
    return check


FLEX_POOL_GRAD = ops_close(1e-5, 1e-5)          # test_flex_pool_exact_and_known_answer
POINTSET_GRAD_F, POINTSET_GRAD_W = ops_close(1e-3, 1e-4), ops_close(1e-3, 1e-3)   # test_conv_pointset_fwd_bwd
GATHER_GRAD = ops_close(1e-5, 1e-5)             # test_group_point_and_interpolate_vs_reference_twin_golden


def agree(tol):             # tests/test_training_gpu.py `agree`: norm-wise within tol, single entries within 10 tol
    def check(a, b):
        a, b = a.astype(np.float64), b.astype(np.float64)
        rel = float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))
        assert rel <= tol, rel
        assert float(np.abs(a - b).max()) <= 10 * tol * float(np.abs(b).max()) + 1e-7, float(np.abs(a - b).max())
    return check


# test_commuted_attention_head_matches_the_materialised_one: att < 2e-6, gradients agree at 2e-3 / 2e-2, EMA allclose
ATT_OUT, ATT_GRAD, EMA_CLOSE = (lambda a, b: _assert(float(np.abs(a - b).max()) < 2e-6)), agree(2e-3), ops_close(1e-5, 1e-6)
# test_commuted_netvlad_assignment_matches_the_materialised_one: V, asum at 2e-5, gradients at 2e-4
NV_OUT, NV_GRAD = agree(2e-5), agree(2e-4)
# test_bn_train_kernels_match_torch: y allclose(1e-5, 1e-5), gradients within 2e-5 of the largest entry + 1e-7
BN_OUT = ops_close(1e-5, 1e-5)


def BN_GRAD(a, b):
    assert float(np.abs(a.astype(np.float64) - b).max()) <= 2e-5 * float(np.abs(b).max()) + 1e-7


def _assert(ok):
    assert ok


def global_tail_close(a, b):  # tests/test_pm_gpu.py test_global_tail_equals_upsample_attention_netvlad
    assert float(np.abs(a - b).max()) <= 2e-6 * float(np.abs(b).max()) + 1e-7


def colsum_close(mag):      # tests/test_backward_gpu.py test_transpose_and_colsum: mag = the column sums of |x|
    def check(a, b):
        assert np.all(np.abs(a.astype(np.float64) - b) <= 2e-6 * mag)
    return check


def gemm_close(mag):        # tests/test_backward_gpu.py test_gemm_tn_vs_fp64 / test_gemm_nn_vs_fp64: mag = |A| |B|
    def check(a, b):
        assert np.all(np.abs(a.astype(np.float64) - b) <= 2e-6 * mag + 1e-6)
    return check


# ------------------------------------------------------------------------------------------------ shared inputs
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(dev, g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def _rand(dev, g, *shape):
    return torch.rand(*shape, generator=g).to(dev)


_CACHE = {}


def _cloud(dev, B, N, K=8, seed=0):
    """xyz [B,N,3], nbr [B,N,K] (exact kNN), and the sort's records / boxes / cell table -- computed once per shape."""
    key = ("cloud", B, N, K, seed)
    if key not in _CACHE:
        from dh3d_amd import pm
        xyz = _rand(dev, _g(1000 * B + N + seed), B, N, 3)
        nbr, _ = pm.knn_xyz(xyz, K)
        srt, gbox, cells = pm.spatial_sort_cells(xyz)
        _CACHE[key] = dict(xyz=xyz, nbr=nbr, srt=srt, gbox=gbox, cells=cells)
    return _CACHE[key]


def _level(dev, B, N, m, seed=0):
    """The cloud, m FPS picks of it with their own sort, and three_nn of every point against the picks."""
    key = ("level", B, N, m, seed)
    if key not in _CACHE:
        from dh3d_amd import ops, pm
        c = dict(_cloud(dev, B, N, 8, seed))
        idx = ops.farthest_point_sample(m, c["xyz"])
        xyz_s = torch.gather(c["xyz"], 1, idx.long()[:, :, None].expand(-1, -1, 3)).contiguous()
        d3, i3 = ops.three_nn(c["xyz"], xyz_s)
        srt_s, gbox_s, cells_s = pm.spatial_sort_cells(xyz_s)
        c.update(idx=idx, xyz_s=xyz_s, d3=d3, i3=i3, srt_s=srt_s, gbox_s=gbox_s, cells_s=cells_s, nbr_s=pm.knn_xyz(xyz_s, 8)[0])
        _CACHE[key] = c
    return _CACHE[key]


def _ep(dev, g, D):
    """(pre_bias, scale, shift) of a folded BatchNorm epilogue."""
    return _randn(dev, g, D, scale=0.1), (0.5 + torch.rand(D, generator=g)).to(dev), _randn(dev, g, D, scale=0.1)


def _flex_w(dev, g, Din, Dout):
    return _randn(dev, g, 3, Din, Dout, scale=Din ** -0.5), _randn(dev, g, Din, Dout, scale=(8 * Din) ** -0.5)


CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


# ------------------------------------------------------------------------------------------------ pm.py: geometry
@case
def knn_xyz(dev):
    from dh3d_amd import pm
    x = _cloud(dev, 2, 333)["xyz"]
    return lambda: pm.knn_xyz(x, 8)


@case
def spatial_sort(dev):
    from dh3d_amd import pm
    x = _cloud(dev, 2, 333)["xyz"]
    return lambda: (pm.spatial_sort(x), pm.spatial_sort_cells(x))


@case
def knn_grid_and_sorted(dev):
    from dh3d_amd import pm
    c = _cloud(dev, 3, 1000)
    return lambda: (pm.knn_grid(c["srt"], c["gbox"], c["cells"], 8), pm.knn_sorted(c["srt"], c["gbox"], 8),
                    pm.knn_sorted(c["srt"], c["gbox"], 12))


@case
def knn_grid_crowded(dev):
    """Half of one cloud inside one cell: the crowded flag is set and the pruned scan serves that cloud."""
    from dh3d_amd import pm
    x = _rand(dev, _g(5), 2, 1001, 3)
    x[0, :600] = x[0, :600] * 0.01
    srt, gbox, cells = pm.spatial_sort_cells(x)
    return lambda: pm.knn_grid(srt, gbox, cells, 8)


@case
def ball_queries(dev):
    from dh3d_amd import ops, pm
    g = _g(11)
    x1, x2 = _rand(dev, g, 2, 333, 3), _rand(dev, g, 2, 70, 3)
    radii = (_rand(dev, g, 2, 70) * 0.3 - 0.02).contiguous()      # some radii <= 0: no hits
    return lambda: (pm.ball_query_scan(0.2, 9, x1, x2), pm.ball_query_scan(radii, 9, x1, x2),
                    pm.ball_query_grid(0.2, 9, x1, x2), pm.ball_query_grid(radii, 9, x1, x2),
                    ops.query_ball_point(0.01, 5, x1, x2), ops.query_ball_point2(radii, 5, x1, x2))


@case
def select_top_k_and_knn_point(dev):
    from dh3d_amd import ops, pm
    g = _g(12)
    d = _rand(dev, g, 2, 5, 70)
    x1, x2 = _rand(dev, g, 2, 333, 3), _rand(dev, g, 2, 70, 3)
    f1, f2 = _randn(dev, g, 2, 130, 5), _randn(dev, g, 2, 33, 5)
    return lambda: (pm.select_top_k(3, d), pm.knn_point(8, x1, x2), pm.knn_point(70, x1, x2), pm.knn_point(4, f1, f2),
                    ops.knn_point(3, x1, x2), ops.select_top_k(70, d))


@case
def prob_sample(dev):
    from dh3d_amd import ops, pm, utils
    from dh3d_amd.pairs import seed_tensor
    g = _g(13)
    w, r = _rand(dev, g, 2, 333), _rand(dev, g, 2, 70)
    count = torch.tensor([333, 200], dtype=torch.int32, device=dev)
    seed = seed_tensor(7, dev)
    return lambda: (pm.prob_sample(w, r), ops.prob_sample(w, r), pm.prob_sample_seeded(w, 70, count, seed),
                    pm.prob_sample_seeded(w, 70, None, seed), utils.sample_by_weight(w, 33, count=count, seed=3))


@case
def prepare_clouds(dev):
    from dh3d_amd import pm
    raw = _rand(dev, _g(500), 2, 500, 3)
    num_raw = torch.tensor([500, 463], dtype=torch.int32, device=dev)
    return lambda: (pm.prepare_clouds(raw, num_raw, 256, voxel_size=0.5, radius=0.3, nb_points=2),
                    pm.prepare_clouds(raw, num_raw, 256, voxel_size=None, radius=0.3, nb_points=2, sortby_dis=False),
                    pm.prepare_clouds(raw, num_raw, 600, voxel_size=0.05, radius=None))


@case
def keypoint_nms_and_gather_rows(dev):
    from dh3d_amd import pm
    g = _g(300)
    B, N, K, M = 2, 300, 8, 16
    pts = _rand(dev, g, B, N, 3)
    dist, nn = torch.cdist(pts, pts).topk(K, dim=2, largest=False)
    dist, nn = dist.contiguous(), nn.to(torch.int32).contiguous()
    score = _rand(dev, g, B, N)
    nv = torch.tensor([300, 211], dtype=torch.int32, device=dev)
    rows = _randn(dev, g, B, N, 12)

    def call():
        count, inds = pm.keypoint_nms(score, nn, dist, 0.1, 0.2, M, num_valid=nv)
        c2, i2 = pm.keypoint_nms(score, nn, dist, 0.3, 0.9, M, remove_noise=False, invert=True)
        return count, inds, c2, i2, pm.gather_rows(rows, inds, count), pm.gather_rows(rows, i2, c2)
    return call


@case
def fps(dev):
    from dh3d_amd import ops, pm
    c = _cloud(dev, 2, 1001)
    big = _rand(dev, _g(17000), 1, 16500, 3)           # beyond the sort's range: the any-N kernel with its scratch row
    return lambda: (pm.fps_sorted(c["srt"], c["gbox"], 125), pm.fps_sorted(c["srt"], c["gbox"], 125, with_xyz=True),
                    pm.fps_sorted(c["srt"], c["gbox"], 125, with_xyz=True, xyz=c["xyz"]),
                    pm.fps_sorted_ordered(c["srt"], c["gbox"], 137, cells=c["cells"]),
                    pm.fps_sorted_ordered(c["srt"], c["gbox"], 125),
                    ops.farthest_point_sample(125, c["xyz"]), ops.farthest_point_sample(125, c["xyz"], contract=0),
                    ops.farthest_point_sample(33, big))


@case
def three_nn(dev):
    from dh3d_amd import ops, pm
    lv = _level(dev, 2, 1100, 137)
    return lambda: (pm.three_nn_sorted(lv["srt"], lv["gbox"], lv["srt_s"], lv["gbox_s"]),
                    pm.three_nn_sorted(lv["srt"], lv["gbox"], lv["srt_s"], lv["gbox_s"], cells2=lv["cells_s"]),
                    ops.three_nn(lv["xyz"], lv["xyz_s"]))


@case
def level_of_the_model(dev):
    """backbones.Geometry: the sampled level the model builds (FPS, the sampled set's kNN, three_nn), all dispatch paths
    of compute_level / finish_level at a ragged N."""
    from dh3d_amd import backbones as bb
    x = _cloud(dev, 2, 4100)["xyz"]

    def call():
        geo = bb.Geometry(x, 8)
        geo.ordered(cells=True)
        lv = geo.level(8, 8)
        return {k: v for k, v in lv.items() if torch.is_tensor(v)}
    return call


# ------------------------------------------------------------------------------------------------ pm.py: packing
@case
def pack_weights(dev):
    from dh3d_amd import pm
    g = _g(21)
    W = _randn(dev, g, 96, 128)
    theta, bias = _flex_w(dev, g, 32, 64)
    return lambda: (pm.pack_weight(W), pm.pack_weight_x3(W), pm.pack_flex_weight(theta, bias),
                    pm.pack_flex_weight_x3(theta, bias))


# ------------------------------------------------------------------------------------------------ pm.py: flex operators
@case
def flex_conv(dev):
    from dh3d_amd import pm
    g = _g(31)
    c = _cloud(dev, 2, 999)
    f = _randn(dev, g, 2, 999, 32)
    theta, bias = _flex_w(dev, g, 32, 64)
    wp = pm.pack_flex_weight(theta, bias)
    pb, sc, sh = _ep(dev, g, 64)
    c12 = _cloud(dev, 2, 300, K=12)
    f12 = _randn(dev, g, 2, 300, 128)
    wp12 = pm.pack_flex_weight(*_flex_w(dev, g, 128, 128))
    return lambda: (pm.flex_conv(f, c["xyz"], c["nbr"], wp, 64), pm.flex_conv(f, c["xyz"], c["nbr"], wp, 64, pre_bias=pb,
                                                                            scale=sc, shift=sh, act=pm.ACT_RELU),
                    pm.flex_conv(f12, c12["xyz"], c12["nbr"], wp12, 128))


@case
def flex_conv_remap(dev):
    from dh3d_amd import pm
    g = _g(32)
    lv = _level(dev, 2, 1001, 125)
    feat = _randn(dev, g, 2, 1001, 64)
    wp = pm.pack_flex_weight(*_flex_w(dev, g, 64, 128))
    return lambda: pm.flex_conv(feat, lv["xyz_s"], lv["nbr_s"], wp, 128, remap=lv["idx"])


@case
def flex_conv_x6(dev):
    from dh3d_amd import pm
    g = _g(33)
    a, b = _cloud(dev, 3, 1000), _cloud(dev, 1, 96)
    fa, fb = _randn(dev, g, 3, 1000, 32), _randn(dev, g, 1, 96, 64)
    w32, w64 = pm.pack_flex_weight_x3(*_flex_w(dev, g, 32, 64)), pm.pack_flex_weight_x3(*_flex_w(dev, g, 64, 64))
    pb, sc, sh = _ep(dev, g, 64)
    return lambda: (pm.flex_conv_x6(fa, a["xyz"], a["nbr"], w32, 64, pre_bias=pb, scale=sc, shift=sh, act=pm.ACT_RELU),
                    pm.flex_conv_x6(fa, a["xyz"], a["nbr"], w32, 64, reserve_cus_per_xcd=31),
                    pm.flex_conv_x6(fb, b["xyz"], b["nbr"], w64, 64, reserve_cus_per_xcd=31),
                    pm.flex_conv_x6(fb, b["xyz"], b["nbr"], w64, 64))


@case
def flex_conv_tile_x6(dev):
    from dh3d_amd import pm
    g = _g(34)
    c = _cloud(dev, 3, 45)
    f64, f128 = _randn(dev, g, 3, 45, 64), _randn(dev, g, 3, 45, 128)
    w_64_128 = pm.pack_flex_weight_x3(*_flex_w(dev, g, 64, 128))
    w_128_256 = pm.pack_flex_weight_x3(*_flex_w(dev, g, 128, 256))
    wpost = pm.pack_weight(_randn(dev, g, 256, 64, scale=1 / 16))
    pb, sc, sh = _ep(dev, g, 256)
    c12 = _cloud(dev, 2, 300, K=12)
    f12 = _randn(dev, g, 2, 300, 128)
    w12 = pm.pack_flex_weight_x3(*_flex_w(dev, g, 128, 128))
    return lambda: (pm.flex_conv_tile_x6(f64, c["xyz"], c["nbr"], w_64_128, 128),
                    pm.flex_conv_tile_x6(f128, c["xyz"], c["nbr"], w_128_256, 256, pre_bias=pb, scale=sc, shift=sh,
                                         act=pm.ACT_RELU, wpost_packed=wpost, Dpost=64),
                    pm.flex_conv_tile_x6(f12, c12["xyz"], c12["nbr"], w12, 128))


@case
def flex_pool_avg_pointset(dev):
    from dh3d_amd import pm
    g = _g(35)
    c = _cloud(dev, 2, 1234)
    f = _randn(dev, g, 2, 1234, 32)
    theta, bias = _randn(dev, g, 3, 32, scale=0.5), _randn(dev, g, 32, scale=0.1)
    pb, sc, sh = _ep(dev, g, 32)
    kw = dict(pre_bias=pb, scale=sc, shift=sh, act=pm.ACT_RELU)
    return lambda: (pm.flex_pool(f, c["nbr"]), pm.flex_pool(f, c["nbr"], want_argmax=True), pm.flex_avg(f, c["nbr"], 0.125),
                    pm.conv_pointset_xyz(c["xyz"], c["nbr"], theta, bias, **kw),
                    pm.conv_pointset_pool_xyz(c["xyz"], c["nbr"], theta, bias, **kw))


# ------------------------------------------------------------------------------------------------ pm.py: dense rows
@case
def linear(dev):
    from dh3d_amd import pm
    g = _g(41)
    x1, x2, res = _randn(dev, g, 777, 128), _randn(dev, g, 777, 64), _randn(dev, g, 777, 128)
    W = _randn(dev, g, 192, 128, scale=1 / 14)
    pb, sc, sh = _ep(dev, g, 128)
    kw = dict(x2=x2, pre_bias=pb, scale=sc, shift=sh, act=pm.ACT_RELU, residual=res)
    xw = _randn(dev, g, 333, 256)
    Ww = _randn(dev, g, 256, 192, scale=1 / 16)
    return lambda: (pm.linear(x1, pm.pack_weight(W), 128, **kw), pm.linear_x6(x1, pm.pack_weight_x3(W), 128, **kw),
                    pm.linear(xw, pm.pack_weight(Ww), 192), pm.linear_x6(x1[:1], pm.pack_weight_x3(W[:128].contiguous()), 128))


@case
def se_res(dev):
    from dh3d_amd import pm
    g = _g(42)
    outs = []
    for C, (B, N) in ((64, (2, 1000)), (128, (3, 333))):
        c = _cloud(dev, B, N)
        x, pool = _randn(dev, g, B, N, C), _randn(dev, g, B, N, C)
        W1, b1 = _randn(dev, g, C, C // 4, scale=1 / 8), _randn(dev, g, C // 4)
        W2, b2 = _randn(dev, g, C // 4, C, scale=1 / 4), _randn(dev, g, C)
        Wc, (bc, sc, sh) = _randn(dev, g, C, C, scale=1 / 8), _ep(dev, g, C)
        outs.append((c, x, pool, W1, b1, W2, b2, Wc, bc, sc, sh))

    def call():
        res = []
        for c, x, pool, W1, b1, W2, b2, Wc, bc, sc, sh in outs:
            packed = pm.se_res_pack(W1, b1, W2)
            res += [pm.se_res(x, pool, W1, b1, W2, b2), pm.se_res_packed(x, pool, *packed, b2),
                    pm.se_res_pool_packed(x, c["nbr"], *packed, b2),
                    pm.se_res_pool_conv(x, c["nbr"], *packed, b2, pm.pack_weight(Wc), bc, sc, sh)]
        return res
    return call


@case
def interpolate_l2norm_heads(dev):
    from dh3d_amd import pm
    g = _g(43)
    lv = _level(dev, 1, 1001, 125)
    pts = _randn(dev, g, 1, 125, 128)
    x, pre = _randn(dev, g, 501, 128), _randn(dev, g, 501, 3)
    x[3] = 0
    h = _randn(dev, g, 301, 256)
    W, wfc = _randn(dev, g, 256, 1024, scale=1 / 16), _randn(dev, g, 1024, scale=1 / 32)
    pb, sc, sh = _ep(dev, g, 1024)
    kw = dict(pre_bias=pb, scale=sc, shift=sh)
    return lambda: (pm.three_interpolate_idw(pts, lv["i3"], lv["d3"]), pm.l2norm_concat(x, 1e-8, prefix=pre),
                    pm.l2norm_concat(x, 1e-8), pm.idw_weights(lv["d3"]),
                    pm.mlp_head(h, pm.pack_weight(W), 1024, wfc, 0.125, **kw),
                    pm.mlp_head_x6(h, pm.pack_weight_x3(W), 1024, wfc, 0.125, **kw))


@case
def upsample_linear(dev):
    from dh3d_amd import pm
    g = _g(44)
    lv = _level(dev, 1, 1001, 125)
    n, m = 1001, 125
    pts, x2, x3 = _randn(dev, g, 1, m, 128), _randn(dev, g, 1, n, 64), _randn(dev, g, 1, n, 64)
    res = _randn(dev, g, 1, n, 128)
    W, Ws = _randn(dev, g, 192, 128, scale=1 / 14), _randn(dev, g, 64, 128, scale=1 / 8)
    e1, e2 = _ep(dev, g, 128), _ep(dev, g, 128)
    w3, wst = pm.pack_weight_x3(W), pm.pack_weight_x3(torch.cat([W, Ws], 0).contiguous())
    kw = dict(x2=x2, pre_bias=e1[0], scale=e1[1], shift=e1[2], act=pm.ACT_RELU, residual=res)
    i3, d3, fine = lv["i3"], lv["d3"], lv["xyz"]
    cw, part = _randn(dev, g, 1, m, 128), _randn(dev, g, 1, n, 128)
    return lambda: (pm.upsample_linear_x6(pts, i3, d3, w3, 128, **kw),
                    pm.upsample_linear_x6(pts, i3, d3, w3, 128, l2cat=(fine, 1e-8), **kw),
                    pm.upsample_linear_shortcut_x6(pts, i3, d3, wst, 128, x2, x3, e1 + (pm.ACT_RELU,), e2 + (pm.ACT_RELU,)),
                    pm.upsample_linear_shortcut_x6(pts, i3, d3, wst, 128, x2, x3, e1 + (pm.ACT_RELU,), e2 + (pm.ACT_RELU,),
                                                   l2cat=(fine, 1e-8)),
                    pm.interp_combine(cw, i3, d3, partial=part, pre_bias=e1[0], scale=e1[1], shift=e1[2], act=pm.ACT_RELU,
                                      residual=res),
                    pm.interp_combine(cw, i3, d3, partial=part, pre_bias=e1[0], scale=e1[1], shift=e1[2], act=pm.ACT_RELU,
                                      residual=res, l2cat=(fine, 1e-8)))


@case
def local_tail_fused(dev):
    from dh3d_amd import pm
    g = _g(45)
    B, N, M = 2, 1056, 132                       # N % 32 == 0 (the kernel's rule), no multiple of 64
    lv = _level(dev, B, N, M)
    x1, x2, cw = _randn(dev, g, B, N, 64), _randn(dev, g, B, N, 64), _randn(dev, g, B, M, 128)
    ws, wl = pm.pack_weight_x3(_randn(dev, g, 64, 128, scale=1 / 8)), pm.pack_weight_x3(_randn(dev, g, 64, 128, scale=1 / 8))
    e1, e2 = _ep(dev, g, 128), _ep(dev, g, 128)
    return lambda: (pm.local_tail_fused(x1, x2, ws, wl, e1, e2, cw, lv["i3"], lv["d3"], lv["xyz"], 1e-8),
                    pm.local_tail_fused(x1, x2, ws, wl, e1, e2, cw, lv["i3"], lv["d3"], None, 0.0))


def _head_weights(dev, g, C=256, Hd=1024):
    from dh3d_amd import pm
    W = _randn(dev, g, C, Hd, scale=C ** -0.5)
    slices = torch.cat([pm.pack_weight_x3(W[:, j:j + 256].contiguous()) for j in range(0, Hd, 256)])
    return slices, _randn(dev, g, Hd, scale=Hd ** -0.5), _ep(dev, g, Hd)


@case
def interp_head(dev):
    from dh3d_amd import pm
    g = _g(46)
    lv = _level(dev, 2, 1001, 125)
    coarse = _randn(dev, g, 2, 125, 256)
    slices, wfc, (pb, sc, sh) = _head_weights(dev, g)
    kw = dict(pre_bias=pb, scale=sc, shift=sh, act=pm.ACT_RELU)
    return lambda: (pm.interp_head(coarse, lv["i3"], lv["d3"], slices, 1024, wfc, 0.2, **kw),
                    pm.interp_head(coarse, lv["i3"], lv["d3"], slices, 1024, wfc, 0.2, order=lv["srt"], **kw))


def _vlad_weights(dev, g, D=256, Cl=64, O=256):
    from dh3d_amd import pm
    Wc = _randn(dev, g, D, Cl, scale=1 / 16)
    return dict(wc=pm.pack_weight(Wc), W2=_randn(dev, g, D, Cl, scale=1 / 16), Wh=_randn(dev, g, D * Cl, O, scale=1 / 8),
                Wg=_randn(dev, g, O, O, scale=1 / 16), cs=(0.5 + torch.rand(Cl, generator=g)).to(dev),
                ch=_randn(dev, g, Cl, scale=0.1), s1=(0.5 + torch.rand(O, generator=g)).to(dev), h1=_randn(dev, g, O, scale=0.1),
                s2=(0.5 + torch.rand(O, generator=g)).to(dev), h2=_randn(dev, g, O, scale=0.1))


@case
def netvlad(dev):
    from dh3d_amd import pm
    g = _g(47)
    B, N = 2, 100
    x, att = _randn(dev, g, B, N, 256), _rand(dev, g, B, N, 1)
    w = _vlad_weights(dev, g)
    flat = _randn(dev, g, B, 256 * 64, scale=0.01)

    def call():
        vlad = pm.netvlad_aggregate(x, att, w["wc"], w["cs"], w["ch"], w["W2"])
        return (vlad, pm.netvlad_head(flat, w["Wh"], w["s1"], w["h1"], w["Wg"], w["s2"], w["h2"], l2_eps=1e-8),
                pm.netvlad_head(flat, w["Wh"], w["s1"], w["h1"], None, None, None),
                pm.netvlad_fused(x, att, w["wc"], w["cs"], w["ch"], w["W2"], w["Wh"], w["s1"], w["h1"], w["Wg"], w["s2"],
                                 w["h2"], l2_eps=1e-8))
    return call


@case
def global_tail(dev):
    """The walk's accumulators (A', asum) are summed by f32 atomics: the descriptors within test_pm_gpu.py's own bound,
    the attention weights and the slot tables bit for bit.  Both ways of getting the accumulator: cleared by the launcher
    (accum None: a torch.empty here) and the caller's zeroed one."""
    from dh3d_amd import pm
    g = _g(48)
    B, n, m = 2, 1001, 125
    lv = _level(dev, B, n, m)
    coarse = _randn(dev, g, B, m, 256)
    slices, wfc, (pb, sc, sh) = _head_weights(dev, g)
    w = _vlad_weights(dev, g)
    args = lambda: (coarse, lv["i3"], lv["d3"], lv["srt"], slices, 1024, wfc, 0.2, (pb, sc, sh, pm.ACT_RELU), w["wc"], w["cs"],
                    w["ch"], w["W2"], w["Wh"], w["s1"], w["h1"], w["Wg"], w["s2"], w["h2"])

    def call():
        plan = pm.walk_plan(lv["i3"], lv["d3"], lv["srt"], m)
        d0, att0 = pm.global_tail(*args(), l2_eps=1e-8, want_att=True)
        accum = torch.zeros((pm.global_tail_accum_size(B, m),), dtype=torch.float32, device=dev)
        d1, att1 = pm.global_tail(*args(), l2_eps=1e-8, want_att=True, accum=accum, plan=plan)
        d2 = pm.global_tail(*args(), plan=pm.walk_plan(lv["i3"], lv["d3"], None, m))
        return plan, att0, att1, d0, d1, d2
    return call, {3: global_tail_close, 4: global_tail_close, 5: global_tail_close}


# ------------------------------------------------------------------------------------------------ pm.py: backward / training
@case
def flex_conv_bwd(dev):
    from dh3d_amd import pm
    g = _g(51)
    c = _cloud(dev, 2, 300)
    f, go = _randn(dev, g, 2, 300, 32), _randn(dev, g, 2, 300, 64)
    theta, bias = _flex_w(dev, g, 32, 64)
    c5 = _cloud(dev, 2, 100, K=5)
    f5, go5 = _randn(dev, g, 2, 100, 16), _randn(dev, g, 2, 100, 24)
    t5, b5 = _flex_w(dev, g, 16, 24)
    call = lambda: (pm.flex_conv_bwd(f, c["xyz"], c["nbr"], theta, bias, go),
                    pm.flex_conv_bwd(f5, c5["xyz"], c5["nbr"], t5, b5, go5, center_rank0=True),
                    pm.flex_conv_bwd(f, c["xyz"], c["nbr"], theta, bias, go, need_grad_features=False))
    return call, {i: max_scaled for i in (0, 1, 2, 3, 4, 5, 7, 8)}


def _gemm_shapes(tn):
    """(unsplit, split) reduction lengths of a 68 x 60 product, chosen by dh3d_gemm_is_split."""
    from dh3d_amd import _lib as L
    ks = (44, 72, 1000, 4100, 18000)
    split = [bool(L.lib().dh3d_gemm_is_split(1 if tn else 0, 68, 60, k, 1)) for k in ks]
    assert not split[0] and any(split), (tn, split)
    return ks[0], ks[split.index(True)]


def _gemm_case(dev, tn, arena):
    from dh3d_amd import pm
    g = _g(52 + tn)
    M, N = 68, 60
    ins, atomic = [], {}
    for j, K in enumerate(_gemm_shapes(tn)):
        A = _randn(dev, g, *((K, M) if tn else (M, K)))
        Bm = _randn(dev, g, K, N)
        C0, bias = _randn(dev, g, M, N), _randn(dev, g, N)
        A64 = A.double().cpu().numpy().T if tn else A.double().cpu().numpy()
        mag = np.abs(A64) @ np.abs(Bm.double().cpu().numpy())
        ins.append((A, Bm, C0, bias))
        if j == 1:   # the split reduction adds its partials with atomics; the unsplit product has none: bit for bit
            # (the accumulate form adds onto C0: test_backward_gpu.py widens mag by it; the bias form is never split)
            atomic.update({3 * j: gemm_close(mag), 3 * j + 1: gemm_close(mag + np.abs(C0.cpu().numpy()))})
            if tn:
                atomic[3 * j + 2] = gemm_close(mag)
    fn = pm.gemm_tn if tn else pm.gemm_nn

    def products():
        out = []
        for A, Bm, C0, bias in ins:
            out += [fn(A, Bm), fn(A, Bm, out=C0.clone(), accumulate=True),
                    fn(A, Bm) if tn else fn(A, Bm, bias=bias)]
        return [o.clone() for o in out]      # (an arena view is valid until the next begin())

    def call():
        if not arena:
            return products()
        za = pm.ZeroArena(fixed_bytes=1 << 20, device=dev)
        with pm.zero_arena(za):
            za.begin(dev)
            out = products()
        assert za.off > 0                    # the split product took its accumulator from the arena
        return out
    return call, atomic


@case
def gemm_tn(dev):
    return _gemm_case(dev, True, False)


@case
def gemm_tn_in_zero_arena(dev):
    return _gemm_case(dev, True, True)


@case
def gemm_nn(dev):
    return _gemm_case(dev, False, False)


@case
def gemm_nn_in_zero_arena(dev):
    return _gemm_case(dev, False, True)


@case
def gemm_batched_colsum_transpose(dev):
    from dh3d_amd import pm
    g = _g(54)
    A, Bm, Dm, bias = _randn(dev, g, 3, 130, 36), _randn(dev, g, 3, 36, 20), _randn(dev, g, 3, 130, 20), _randn(dev, g, 3, 20)
    x = _randn(dev, g, 3, 129, 65)
    xi = torch.randint(0, 1 << 30, (2, 8, 513), generator=g, dtype=torch.int32).to(dev)
    rows = _randn(dev, g, 1001, 100)
    acc = _randn(dev, g, 100)
    few = _randn(dev, g, 200, 36)                 # one row chunk: no atomics meet
    call = lambda: (pm.gemm_nn_batched(A, Bm, bias=bias), pm.gemm_nn_batched(A, Bm), pm.transpose_last2(x),
                    pm.transpose_last2(xi), pm.colsum(few), pm.gemm_tn_batched(A, Dm), pm.colsum(rows),
                    pm.colsum(rows, out=acc.clone(), accumulate=True))
    # the reduction over 130 rows is split and 1001 rows are four row chunks: summed by atomics
    mag_tn = (A.double().abs().transpose(1, 2) @ Dm.double().abs()).cpu().numpy()
    mag_cs = rows.double().abs().sum(0).cpu().numpy()
    return call, {5: gemm_close(mag_tn), 6: colsum_close(mag_cs), 7: colsum_close(mag_cs + acc.double().abs().cpu().numpy())}


@case
def bn_rows(dev):
    """The element-wise and finalize kernels of training-mode BatchNorm on rows (the column sums in front of them add
    float64 partials with atomics and are covered by the trainers' steps below)."""
    from dh3d_amd import pm
    g = _g(55)
    R, C = 777, 64
    x, dy, res = _randn(dev, g, R, C), _randn(dev, g, R, C), _randn(dev, g, R, C)
    gamma, beta = (0.5 + torch.rand(C, generator=g)).to(dev), _randn(dev, g, C, scale=0.1)
    s1 = x.double().sum(0)
    s2 = (x.double() ** 2).sum(0)
    cnt = torch.full((1,), float(R), dtype=torch.float64, device=dev)
    rm0, rv0 = _randn(dev, g, C, scale=0.1), (0.5 + torch.rand(C, generator=g)).to(dev)
    part = torch.stack([s1, s2]).reshape(2, 1, C).repeat(1, 3, 1).contiguous() / 3.0
    part3 = torch.cat([part, part[:1]], 0).contiguous()
    rowscale, colvec = _randn(dev, g, R), _randn(dev, g, C)
    hb = torch.full((1,), 0.2, device=dev)

    def call():
        rm, rv = rm0.clone(), rv0.clone()
        st = pm.bn_finalize(s1, s2, cnt, gamma, beta, 1e-5, 0.9, rm, rv)
        rm2, rv2 = rm0.clone(), rv0.clone()
        st2 = pm.bn_finalize_parts(part, cnt, gamma, beta, 1e-3, 0.999, rm2, rv2, unbiased=False)
        k = pm.bn_bwd_finalize(s1, s2, cnt, st[0], st[1], gamma)
        k2, grads = pm.bn_bwd_finalize_parts(part3, cnt, st[0], st[1], gamma)
        return (st, rm, rv, st2, rm2, rv2, k, k2, grads,
                pm.scale_shift_act(x, st[2], st[3], True), pm.scale_shift_act(x, st[2], st[3], False, residual=res),
                pm.bn_bwd_apply(x, st[2], st[3], k[0], k[1], True, dy=dy),
                pm.bn_bwd_apply(x, st[2], st[3], k[0], k[1], True, rowscale=rowscale, colvec=colvec),
                pm.row_logit_sigmoid(x, st[2], st[3], colvec, hb))
    return call


@case
def small_training_rows(dev):
    from dh3d_amd import pm
    g = _g(56)
    v, gt, dy = _randn(dev, g, 7, 256), _randn(dev, g, 7, 256), _randn(dev, g, 7, 256)
    s, da = _randn(dev, g, 192, 64), _randn(dev, g, 192, 64)
    s200 = _randn(dev, g, 200, 64)
    sc, sh = (0.5 + torch.rand(64, generator=g)).to(dev), _randn(dev, g, 64, scale=0.1)
    att, att200 = _rand(dev, g, 192), _rand(dev, g, 200)
    x, dxn = _randn(dev, g, 5, 256), _randn(dev, g, 5, 256)
    return lambda: (pm.context_gate(v, gt), pm.context_gate_bwd(v, gt, dy), pm.netvlad_assign_rows(s, sc, sh, att, rows_per_cloud=64),
                    pm.netvlad_assign_rows(s200, sc, sh, att200), pm.netvlad_assign_rows_bwd(s, sc, sh, att, da),
                    pm.l2norm_rows_bwd(x, dxn, 1e-8))


# ------------------------------------------------------------------------------------------------ ops.py: drop-in operators
def _grads(outs, leaves, seed):
    """Fixed upstream gradients for the floating outputs -> the leaves' gradients."""
    outs = [o for o in (outs if isinstance(outs, (tuple, list)) else [outs]) if o.is_floating_point() and o.requires_grad]
    g = _g(seed)
    gos = [torch.randn(o.shape, generator=g).to(o.device) for o in outs]
    return torch.autograd.grad(outs, leaves, grad_outputs=gos, allow_unused=True)


def _leaves(*ts):
    return [t.detach().clone().requires_grad_(True) for t in ts]


def _ref_layout(dev, B, N, K, Din, Dout, seed, hub=False):
    g = _g(seed)
    pos = _rand(dev, g, B, 3, N)
    nbr = torch.zeros((B, K, N), dtype=torch.int32) if hub else torch.randint(0, N, (B, K, N), generator=g, dtype=torch.int32)
    theta, bias = _flex_w(dev, g, Din, Dout)
    return dict(f=_randn(dev, g, B, Din, N), pos=pos, nbr=nbr.to(dev), theta=theta, bias=bias)


@case
def ops_flex_convolution(dev):
    """Every dispatch path of the reference-layout operator: the factorisation in two launches (8 -> 12), the persistent
    bf16x6 kernel (32 -> 64, K = 8), the fused f32 kernel (64 -> 128, K = 9), the reference formulation (Din = 6) and
    float64; forward and backward."""
    from dh3d_amd import ops
    cs = [_ref_layout(dev, 2, 70, 3, 8, 12, 61), _ref_layout(dev, 1, 65, 8, 32, 64, 62), _ref_layout(dev, 2, 70, 9, 64, 128, 63),
          _ref_layout(dev, 2, 70, 3, 6, 10, 64)]
    c64 = {k: (v.double() if v.is_floating_point() else v) for k, v in _ref_layout(dev, 2, 70, 3, 6, 10, 65).items()}

    def call():
        res = []
        for c in cs + [c64]:
            f, t, b = _leaves(c["f"], c["theta"], c["bias"])
            out = ops.flex_convolution(f, c["pos"], c["nbr"], t, b)
            res += [out.detach()] + list(_grads(out, [f, t, b], 7))
        return res
    atomic = {4 * j + i: max_scaled for j in range(5) for i in (1, 2, 3)}
    return call, atomic


@case
def ops_flex_convolution_transpose(dev):
    from dh3d_amd import ops
    cs = [_ref_layout(dev, 2, 70, 3, 8, 12, 66), _ref_layout(dev, 2, 70, 3, 8, 12, 67, hub=True)]

    def call():
        res = []
        for c in cs:
            f, t, b = _leaves(c["f"], c["theta"], c["bias"])
            out = ops.flex_convolution_transpose(f, c["pos"], c["nbr"], t, b)
            res += [out.detach()] + list(_grads(out, [f, t, b], 8))
        return res
    return call, {4 * j + i: deconv_close for j in range(2) for i in (2, 3)}


@case
def ops_flex_pooling_and_pointset(dev):
    """flex_pooling and convolution_pointset, forward (bit for bit) and backward (atomics: test_ops_gpu.py's bounds)."""
    from dh3d_amd import ops
    c = _ref_layout(dev, 2, 70, 3, 8, 8, 68)
    g = _g(69)
    theta, bias = _randn(dev, g, 8, 12, scale=0.3), _randn(dev, g, 12, scale=0.1)

    def call():
        (f,) = _leaves(c["f"])
        out, arg = ops.flex_pooling(f, c["nbr"])
        f2, t, b = _leaves(c["f"], theta, bias)
        cp = ops.convolution_pointset(f2, c["nbr"], t, b)
        return [out.detach(), arg, cp.detach()] + list(_grads(out, [f], 9)) + list(_grads(cp, [f2, t, b], 10))
    return call, {3: FLEX_POOL_GRAD, 4: POINTSET_GRAD_F, 5: POINTSET_GRAD_W, 6: POINTSET_GRAD_W}


@case
def ops_pointnet2(dev):
    """knn_bruteforce, group_point / gather_point (distinct indices: every scatter target receives one addend, the sum
    is exact) and three_interpolate with its atomics-summed backward."""
    from dh3d_amd import ops
    g = _g(70)
    lv = _level(dev, 2, 1001, 125)
    pos = lv["xyz"].transpose(1, 2).contiguous()
    x = _randn(dev, g, 2, 1001, 20)
    y = _randn(dev, g, 2, 125, 36)
    w = torch.softmax(_randn(dev, g, 2, 1001, 3), dim=2).contiguous()
    ball = torch.stack([torch.randperm(1001, generator=g)[:4 * 33].reshape(33, 4) for _ in range(2)]).to(torch.int32).to(dev)

    def call():
        (xl, yl) = _leaves(x, y)
        grp = ops.group_point(xl, ball)
        gat = ops.gather_point(lv["xyz"], lv["idx"])
        up = ops.three_interpolate(yl, lv["i3"], w)
        return ([ops.knn_bruteforce(pos, 8), grp.detach(), gat, up.detach()] + list(_grads(grp, [xl], 11))
                + list(_grads(up, [yl], 12)))
    return call, {6: GATHER_GRAD}


# ------------------------------------------------------------------------------------------------ train_ops.py
def _model(dev, preset, seed=3):
    from dh3d_amd import ConfigFactory
    from dh3d_amd.model import DH3D
    return DH3D(ConfigFactory(preset).getconfig()).init_synthetic(seed).to(dev).eval()


def _copies(mod, n=4):
    """Fresh copies of a module whose moving averages the call updates in place: one per run."""
    return [copy.deepcopy(mod) for _ in range(n)]


@case
def train_ops_local_nodes(dev):
    """The nodes of the local training step that have no atomics: relu, se_gate, flex_pool's forward, add_channel_bias,
    l2_normalize_rows, pairwise_sqdist, conv_pointset, forward and backward.  flex_pool's scatter adds with atomics:
    FlexPoolGrad's bound of test_ops_gpu.py."""
    from dh3d_amd import pm, train_ops as T
    g = _g(80)
    c = _cloud(dev, 2, 333)
    x, z = _randn(dev, g, 2, 333, 64), _randn(dev, g, 2, 333, 64)
    bias = _randn(dev, g, 64)
    A, Bm = _randn(dev, g, 2, 36, 128), _randn(dev, g, 2, 44, 128)
    theta, pbias = _randn(dev, g, 3, 32, scale=0.5), _randn(dev, g, 32, scale=0.1)
    # the upstream gradients _grads will draw for add_channel_bias (output 3) and conv_pointset (output 6): their column
    # sums over 666 rows (three row chunks) and S^T dOut (a split reduction) are summed by atomics
    go_ab = torch.randn((2, 333, 64), generator=_g(23)).double().abs().reshape(-1, 64)
    go_cp = torch.randn((2, 333, 32), generator=_g(26)).double().abs().reshape(-1, 32)
    xyz64, nb = c["xyz"].double().cpu(), c["nbr"].long().cpu()
    nbx = torch.gather(xyz64.unsqueeze(1).expand(-1, 333, -1, -1), 2, nb.unsqueeze(-1).expand(-1, -1, -1, 3))
    S = (nbx - nbx[:, :, :1]).sum(2).reshape(-1, 3)

    def call():
        xl, zl, bl, Al, Bl, tl, pl = _leaves(x, z, bias, A, Bm, theta, pbias)
        r = T.relu(xl)
        sg = T.se_gate(xl, zl)
        fp = T.flex_pool(xl, c["nbr"])
        ab = T.add_channel_bias(xl, bl)
        l2 = T.l2_normalize_rows(xl.reshape(-1, 64), 1e-8)
        pd = T.pairwise_sqdist(Al, Bl)
        cp = T.conv_pointset_xyz(c["xyz"], c["nbr"], tl, pl)
        outs = [r, sg, fp, ab, l2, pd, cp]
        res = [o.detach() for o in outs]
        for i, (o, lv) in enumerate(zip(outs, ([xl], [xl, zl], [xl], [xl, bl], [xl], [Al, Bl], [tl, pl]))):
            res += list(_grads(o, lv, 20 + i))
        return res
    # 7 forwards, then: relu dx (7), se_gate dx dz (8, 9), flex_pool dx (10), add_channel_bias dx db (11, 12),
    # l2 dx (13), pairwise dA dB (14, 15), conv_pointset dtheta dbias (16, 17)
    return call, {10: FLEX_POOL_GRAD, 12: colsum_close(go_ab.sum(0).numpy()), 16: gemm_close((S.abs().T @ go_cp).numpy()),
                  17: colsum_close(go_cp.sum(0).numpy())}


@case
def train_ops_linear(dev):
    """train_ops.linear at a split and an unsplit row count: y, dx, dW, db (the split dW is summed by atomics)."""
    from dh3d_amd import train_ops as T
    g = _g(81)
    ks = _gemm_shapes(True)
    ins, atomic = [], {}
    for j, R in enumerate(ks):
        x, W, b = _randn(dev, g, R, 68), _randn(dev, g, 68, 60, scale=1 / 8), _randn(dev, g, 60)
        go = torch.randn((R, 60), generator=_g(30 + j)).double().numpy()
        ins.append((x, W, b))
        atomic[4 * j + 2] = gemm_close(np.abs(x.double().cpu().numpy()).T @ np.abs(go))

    def call():
        res = []
        for j, (x, W, b) in enumerate(ins):
            xl, Wl, bl = _leaves(x, W, b)
            y = T.linear(xl, Wl, bl)
            res += [y.detach()] + list(_grads(y, [xl, Wl, bl], 30 + j))
        return res
    return call, atomic


@case
def train_ops_global_small(dev):
    """vlad_normalize (its aux rows are a scratch of the call), quadruplet_loss, context_gate, batch_norm_train's one-launch
    form for <= 64 rows (dh3d_bn_small_*): forward and backward."""
    from dh3d_amd import train_ops as T
    g = _g(82)
    m = _model(dev, "global_config")
    nv = m._netvlad
    bns = _copies(nv.bn)
    V, asum = _randn(dev, g, 2, 64, 256), _rand(dev, g, 2, 64)     # (two clouds: two addends commute, dW2 is exact)
    desc = torch.nn.functional.normalize(_randn(dev, g, 2 * (2 + 2 + 3), 256), dim=1)
    v, gt = _randn(dev, g, 7, 256), _randn(dev, g, 7, 256)
    mask = torch.tensor([1, 1, 0, 1, 1, 1, 1], dtype=torch.bool, device=dev)

    def call():
        bn = bns.pop()
        Vl, al, W2l, dl, vl, gl, xl = _leaves(V, asum, nv.cluster_weights2, desc, v, gt, v)
        vn = T.vlad_normalize(Vl, al, W2l)
        ql = T.quadruplet_loss(dl, 2, 2, 3)
        cg = T.context_gate(vl, gl)
        bt = T.batch_norm_train(xl, bn, False, mask=mask, rows_per_cloud=1)
        res = [vn.detach(), ql.detach(), cg.detach(), bt.detach(), bn.moving_mean.clone(), bn.moving_variance.clone()]
        res += list(_grads(vn, [Vl, al, W2l], 40)) + list(_grads(ql, [dl], 41)) + list(_grads(cg, [vl, gl], 42))
        res += list(_grads(bt, [xl, bn.gamma, bn.beta], 43))
        return res
    return call


# ---- the masked (padding-cloud) paths: a single-process trainer never passes a mask, so the steps below do not take them
MASKED = (3, 1001, 125)      # clouds, fine points (ragged), sampled points; the middle cloud is padding


def _masked_level(dev):
    Bt, N, M = MASKED
    lv = _level(dev, Bt, N, M)
    return lv, torch.tensor([True, False, True], device=dev)


@case
def bn_sums_with_mask(dev):
    """bn_colstats, both forms of bn_bwd_sums (float64 partials added with atomics: test_bn_train_kernels_match_torch's
    gradient bound) and sigmoid_bwd (dlogit per row, bit for bit; its sum likewise) with a padding cloud."""
    from dh3d_amd import pm
    g = _g(57)
    clouds, rpc, C = 3, 333, 64
    R = clouds * rpc
    mask = torch.tensor([True, False, True], device=dev)
    x, dy = _randn(dev, g, R, C), _randn(dev, g, R, C)
    gamma, beta = (0.5 + torch.rand(C, generator=g)).to(dev), _randn(dev, g, C, scale=0.1)
    mean, rstd = _randn(dev, g, C, scale=0.1), (0.5 + torch.rand(C, generator=g)).to(dev)
    rowscale, colvec = _randn(dev, g, R), _randn(dev, g, C)
    datt, att = _randn(dev, g, R), _rand(dev, g, R)

    def call():
        s1, s2 = pm.bn_colstats(x, mask, rpc)
        t1, t2 = pm.bn_colstats(x)
        dlogit, tot = pm.sigmoid_bwd(datt, att, mask, rpc)
        return dict(s1=s1.clone(), s2=s2.clone(), t1=t1.clone(), t2=t2.clone(),
                    S=pm.bn_bwd_sums(x, mean, rstd, gamma, beta, True, dy=dy, mask=mask, rows_per_cloud=rpc).clone(),
                    S_rank1=pm.bn_bwd_sums(x, mean, rstd, gamma, beta, True, rowscale=rowscale, colvec=colvec, mask=mask,
                                           rows_per_cloud=rpc).clone(),
                    dlogit=dlogit, tot=tot, dx=pm.bn_bwd_apply(x, gamma, beta, mean, rstd, True, dy=dy, mask=mask,
                                                               rows_per_cloud=rpc))
    return call, {k: BN_GRAD for k in ("s1", "s2", "t1", "t2", "S", "S_rank1", "tot")}


@case
def interp_bn_walks_with_mask(dev):
    """The commuted attention head's four walks (csrc/interp_train.hip) with a padding cloud, both layouts of G: the per-row
    attention bit for bit, the per-cloud partials and the scattered dG (atomics) at the commuted head's own bounds."""
    from dh3d_amd import pm
    g = _g(58)
    lv, mask = _masked_level(dev)
    Bt, N, M = MASKED
    i3, d3, order = lv["i3"], lv["d3"], lv["srt"]
    outs = {}
    ins = []
    for tag, Hd, sliced in (("rows", 256, False), ("slices", 512, True)):
        G = _randn(dev, g, Bt * M, Hd)
        if sliced:
            G = G.reshape(Bt * M, Hd // 256, 256).transpose(0, 1).contiguous()
        sc, sh = (0.5 + torch.rand(Hd, generator=g)).to(dev), _randn(dev, g, Hd, scale=0.3)
        mean, rstd = _randn(dev, g, Hd, scale=0.1), (0.5 + torch.rand(Hd, generator=g)).to(dev)
        gamma, beta = (0.5 + torch.rand(Hd, generator=g)).to(dev), _randn(dev, g, Hd, scale=0.1)
        wfc, k2, k3 = _randn(dev, g, Hd, scale=Hd ** -0.5), _randn(dev, g, Hd, scale=0.01), _randn(dev, g, Hd, scale=0.01)
        dlogit = _randn(dev, g, Bt * N) * mask.repeat_interleave(N).float()
        ins.append((tag, G, sc, sh, mean, rstd, gamma, beta, wfc, k2, k3, dlogit))
    bfc = torch.full((1,), 0.2, device=dev)

    def call():
        out = {}
        for tag, G, sc, sh, mean, rstd, gamma, beta, wfc, k2, k3, dlogit in ins:
            s1, s2 = pm.interp_bn_colstats(G, i3, d3, order, mask)
            out.update({tag + "_part": pm.interp_bn_colstats(G, i3, d3, order, mask, parts=True).clone(),
                        tag + "_s1": s1, tag + "_s2": s2,
                        tag + "_att": pm.interp_head_rows(G, i3, d3, order, sc, sh, wfc, bfc),
                        tag + "_att_index_order": pm.interp_head_rows(G, i3, d3, None, sc, sh, wfc, bfc),
                        tag + "_bsums": pm.interp_bn_bwd_sums(G, i3, d3, order, dlogit, wfc, mean, rstd, gamma, beta, mask,
                                                              parts=True).clone(),
                        tag + "_S": pm.interp_bn_bwd_sums(G, i3, d3, order, dlogit, wfc, mean, rstd, gamma, beta, mask),
                        tag + "_dG": pm.interp_bn_bwd_apply(G, i3, d3, order, dlogit, wfc, sc, sh, k2, k3, mask).clone()})
        return out
    atomic = {t + k: ATT_GRAD for t in ("rows", "slices") for k in ("_part", "_s1", "_s2", "_bsums", "_S", "_dG")}
    return call, atomic


@case
def nv_commuted_walks_with_mask(dev):
    """The commuted NetVLAD assignment's four walks and interp_scatter_scaled (csrc/netvlad_train.hip) with a padding cloud:
    every per-point output (s, rinv, p, dz, datt, t2, q -- zero rows for the padding cloud) bit for bit; the per-cloud
    partials, asum and the scattered rows (atomics) at the commuted node's own bounds."""
    from dh3d_amd import pm
    g = _g(59)
    lv, mask = _masked_level(dev)
    Bt, N, M = MASKED
    i3, d3, order = lv["i3"], lv["d3"], lv["srt"]
    c = _randn(dev, g, Bt * M, 256)
    cw = pm.gemm_nn(c, _randn(dev, g, 256, 64, scale=1 / 16))
    E = _randn(dev, g, Bt * M, 64)
    att, dasum = _rand(dev, g, Bt * N), _randn(dev, g, Bt, 64)
    sc, sh = (0.5 + torch.rand(64, generator=g)).to(dev), _randn(dev, g, 64, scale=0.3)
    mean, rstd = _randn(dev, g, 64, scale=0.1), (0.5 + torch.rand(64, generator=g)).to(dev)
    k2, k3 = _randn(dev, g, 64, scale=0.01), _randn(dev, g, 64, scale=0.01)
    dc0 = _randn(dev, g, Bt * M, 256)

    def call():
        out = {}
        for tag, od in (("", order), ("index_order_", None)):
            s, rinv, part = pm.nv_commuted_fwd_stats(c, cw, i3, d3, od, mask, parts=True)
            p, asum, Ap = pm.nv_commuted_fwd_assign(s, rinv, att, sc, sh, i3, d3, od, M, mask)
            dz, datt, t2, bpart = pm.nv_commuted_bwd_sums(E, p, s, att, rinv, dasum, mean, rstd, i3, d3, od, mask, parts=True)
            q, dcw = pm.nv_commuted_bwd_apply(dz, s, rinv, t2, sc, k2, k3, i3, d3, od, M, mask)
            dc = pm.interp_scatter_scaled(c, q, i3, d3, od, dc0.clone(), mask)
            vals = dict(s=s, rinv=rinv, part=part.clone(), p=p, asum=asum.clone(), Ap=Ap.clone(), dz=dz, datt=datt, t2=t2,
                        bpart=bpart.clone(), q=q, dcw=dcw.clone(), dc=dc)
            out.update({tag + k: v for k, v in vals.items()})
        _, _, m1, m2 = pm.nv_commuted_fwd_stats(c, cw, i3, d3, order, mask)
        out.update(sum=m1, sumsq=m2)
        return out
    atomic = {"sum": NV_GRAD, "sumsq": NV_GRAD}
    for tag in ("", "index_order_"):
        atomic.update({tag + "asum": NV_OUT, tag + "Ap": NV_OUT})
        atomic.update({tag + k: NV_GRAD for k in ("part", "bpart", "dcw", "dc")})
    return call, atomic


@case
def train_ops_batch_norm_rows_with_mask(dev):
    """batch_norm_train above 64 rows (_BatchNormTrain: column sums, finalize, apply, backward sums, backward apply) with a
    padding cloud, forward and backward, at test_bn_train_kernels_match_torch's bounds."""
    from dh3d_amd import backbones as bb, train_ops as T
    g = _g(84)
    clouds, rpc, C = 3, 333, 64
    mask = torch.tensor([True, False, True], device=dev)
    x = (_randn(dev, g, clouds * rpc, C) * 2 + 0.5).contiguous()
    bn0 = bb.TPBatchNorm(C).to(dev)
    with torch.no_grad():
        bn0.gamma.copy_((0.5 + torch.rand(C, generator=g)).to(dev))
        bn0.beta.copy_(_randn(dev, g, C))
    bns = _copies(bn0)

    def call():
        bn = bns.pop()
        (xl,) = _leaves(x)
        y = T.batch_norm_train(xl, bn, True, False, mask, rpc)
        dx, dgamma, dbeta = _grads(y, [xl, bn.gamma, bn.beta], 45)
        return dict(y=y.detach(), dx=dx, dgamma=dgamma, dbeta=dbeta, mean_EMA=bn.mean_EMA.clone(),
                    variance_EMA=bn.variance_EMA.clone())
    return call, dict(y=BN_OUT, dx=BN_GRAD, dgamma=BN_GRAD, dbeta=BN_GRAD, mean_EMA=EMA_CLOSE, variance_EMA=EMA_CLOSE)


@case
def train_ops_attention_heads_with_mask(dev):
    """attention_head on materialised rows and attention_head_commuted, with a padding cloud, forward and backward, at
    test_commuted_attention_head_matches_the_materialised_one's bounds."""
    from dh3d_amd import ops, pm, train_ops as T
    lv, mask = _masked_level(dev)
    Bt, N, M = MASKED
    m = _model(dev, "global_config")
    conv0, fcw0 = m.globalatt.detec_conv0, m.globalatt.detec_conv_fc
    with torch.no_grad():
        conv0.bn.gamma.copy_((0.5 + torch.rand(conv0.cout, generator=_g(1))).to(dev))
        conv0.bn.beta.copy_(0.3 * torch.randn(conv0.cout, generator=_g(2)).to(dev))
    mods = _copies(torch.nn.ModuleList([conv0, fcw0]), 8)
    coarse = _randn(dev, _g(7), Bt, M, 256)
    up = ops.three_interpolate(coarse, lv["i3"], pm.idw_weights(lv["d3"])).reshape(Bt * N, 256).contiguous()
    wgt = _randn(dev, _g(9), Bt * N) * mask.repeat_interleave(N).float()

    def one(commuted):
        conv, fcw = mods.pop()
        (xl,) = _leaves(coarse.reshape(Bt * M, 256) if commuted else up)
        if commuted:
            att = T.attention_head_commuted(xl, conv, fcw.W, fcw.b, lv["i3"], lv["d3"], lv["srt"], False, mask)
        else:
            att = T.attention_head(xl, conv, fcw.W, fcw.b, False, mask, N)
        gs = torch.autograd.grad([att], [xl, conv.W, conv.bn.gamma, conv.bn.beta, fcw.W, fcw.b], grad_outputs=[wgt])
        tag = "commuted_" if commuted else "rows_"
        out = {tag + "att": att.detach(), tag + "mean_EMA": conv.bn.mean_EMA.clone(), tag + "variance_EMA": conv.bn.variance_EMA.clone()}
        out.update({tag + "d" + k: v for k, v in zip(("x", "W", "gamma", "beta", "wfc", "bfc"), gs)})
        return out

    def call():
        out = one(True)
        out.update(one(False))
        return out
    atomic = {}
    for tag in ("commuted_", "rows_"):
        atomic.update({tag + "att": ATT_OUT, tag + "mean_EMA": EMA_CLOSE, tag + "variance_EMA": EMA_CLOSE})
        atomic.update({tag + "d" + k: ATT_GRAD for k in ("x", "W", "gamma", "beta", "wfc", "bfc")})
    return call, atomic


@case
def train_ops_netvlad_assign_with_mask(dev):
    """netvlad_assign on materialised rows (192 rows a cloud: asum rides along; 1001: summed afterwards) and
    netvlad_assign_commuted, with a padding cloud, forward and backward, at
    test_commuted_netvlad_assignment_matches_the_materialised_one's bounds."""
    from dh3d_amd import ops, pm, train_ops as T
    lv, mask = _masked_level(dev)
    Bt, N, M = MASKED
    m = _model(dev, "global_config")
    nv = m._netvlad
    with torch.no_grad():
        nv.cluster_bn.gamma.copy_((0.5 + torch.rand(64, generator=_g(1))).to(dev))
        nv.cluster_bn.beta.copy_(0.3 * torch.randn(64, generator=_g(2)).to(dev))
    bns = _copies(nv.cluster_bn, 12)
    coarse = _randn(dev, _g(7), Bt, M, 256)
    up = ops.three_interpolate(coarse, lv["i3"], pm.idw_weights(lv["d3"])).contiguous()
    att = _rand(dev, _g(8), Bt * N)
    live = mask.float()
    dV = _randn(dev, _g(11), Bt, 64, 256) * live[:, None, None]
    dA = _randn(dev, _g(12), Bt, 64) * live[:, None]

    def one(tag):
        bn = bns.pop()
        if tag == "commuted_":
            xl, al, Wl = _leaves(coarse, att, nv.cluster_weights)
            V, asum = T.netvlad_assign_commuted(xl, al, Wl, bn, lv["i3"], lv["d3"], lv["srt"], False, mask)
        else:
            n = 192 if tag == "rows192_" else N
            xl, al, Wl = _leaves(up[:, :n].contiguous(), att.reshape(Bt, N)[:, :n].reshape(-1), nv.cluster_weights)
            V, asum = T.netvlad_assign(xl, al, Wl, bn, False, mask)
        gs = torch.autograd.grad([V, asum], [xl, al, Wl, bn.gamma, bn.beta], grad_outputs=[dV, dA])
        out = {tag + "V": V.detach(), tag + "asum": asum.detach(), tag + "moving_mean": bn.moving_mean.clone(),
               tag + "moving_variance": bn.moving_variance.clone()}
        out.update({tag + "d" + k: v for k, v in zip(("x", "att", "Wc", "gamma", "beta"), gs)})
        return out

    def call():
        out = {}
        for tag in ("commuted_", "rows192_", "rows_"):
            out.update(one(tag))
        return out
    atomic = {}
    for tag in ("commuted_", "rows192_", "rows_"):
        atomic.update({tag + "V": NV_OUT, tag + "asum": NV_OUT, tag + "moving_mean": EMA_CLOSE, tag + "moving_variance": EMA_CLOSE})
        atomic.update({tag + "d" + k: NV_GRAD for k in ("x", "att", "Wc", "gamma", "beta")})
    return call, atomic


# ------------------------------------------------------------------------------------------------ registration.py
def _pair_clouds(dev, P=2, Na=700, Nb=650, seed=90):
    g = _g(seed)
    a = (_rand(dev, g, P, Na, 3) * 10).contiguous()
    ang = 0.05
    R = torch.tensor([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], dtype=torch.float32, device=dev)
    b = ((a[:, :Nb] - torch.tensor([0.1, -0.05, 0.02], device=dev)) @ R).contiguous()
    Rt = torch.zeros((P, 3, 4), dtype=torch.float64, device=dev)
    Rt[:, :, :3] = torch.eye(3, dtype=torch.float64, device=dev)
    return a, b, Rt


@case
def registration_match_ransac(dev):
    from dh3d_amd import registration as reg
    g = _g(91)
    P, Ma, Mb = 3, 70, 65
    rows_a = torch.cat([_rand(dev, g, P, Ma, 3) * 10, torch.nn.functional.normalize(_randn(dev, g, P, Ma, 128), dim=2),
                        _rand(dev, g, P, Ma, 1)], 2).contiguous()
    rows_b = rows_a[:, :Mb].clone()
    rows_b[:, :, :3] += 0.5
    ca = torch.tensor([70, 40, 0], dtype=torch.int32, device=dev)       # counts below the capacity, an empty pair
    cb = torch.tensor([65, 33, 5], dtype=torch.int32, device=dev)
    return lambda: reg.register(rows_a, ca, rows_b, cb, threshold=0.2, max_trials=200, seed=5)


@case
def registration_icp(dev):
    from dh3d_amd import registration as reg
    a, b, Rt = _pair_clouds(dev)
    ca = torch.tensor([700, 555], dtype=torch.int32, device=dev)
    cb = torch.tensor([650, 401], dtype=torch.int32, device=dev)
    valid = torch.tensor([True, True], device=dev)
    kw = dict(valid=valid, anchor_count=ca, positive_count=cb, max_dist=1.0, iterations=3)
    return lambda: (reg.refine_icp(a, b, Rt, path=1, **kw), reg.refine_icp(a, b, Rt, path=2, **kw),
                    reg.refine_icp_plane(a, b, Rt, **kw), reg.refine_icp_gicp(a, b, Rt, **kw))


@case
def registration_normals_fpfh_iss(dev):
    from dh3d_amd import registration as reg
    a, _, _ = _pair_clouds(dev, Na=700)
    nv = torch.tensor([700, 555], dtype=torch.int32, device=dev)
    ids = torch.tensor([[0, 5, 699, -1, 17], [554, 555, 3, 2, 1]], dtype=torch.int32, device=dev)
    return lambda: (reg.estimate_normals(a, nv, k=16), reg.compute_fpfh(a, num_valid=nv, k=16, max_dist=2.0),
                    reg.compute_fpfh(a, num_valid=nv, k=16, ids=ids), reg.cloud_resolution(a, nv),
                    reg.iss_keypoints(a, nv, 2.0, 1.5, max_keypoints=64, eigenvalues=True),
                    reg.iss_keypoints(a, nv, max_keypoints=300))


@case
def registration_fpfh_end_to_end(dev):
    """register_fpfh: FPFH on both clouds, ISS keypoints, matching, RANSAC and the dense refinement, in one call."""
    from dh3d_amd import registration as reg
    a, b, _ = _pair_clouds(dev, P=2, Na=700, Nb=650, seed=93)
    nv = (torch.tensor([700, 555], dtype=torch.int32, device=dev), torch.tensor([650, 401], dtype=torch.int32, device=dev))
    kp = {"method": "iss", "salient_radius": 2.0, "non_max_radius": 1.5, "max_keypoints": 128}
    return lambda: (reg.register_fpfh(a, b, num_valid=nv, keypoints=kp, k=16, refine={"iterations": 2}, threshold=0.3,
                                      max_trials=200, seed=3),
                    reg.register_fpfh(a, b, num_valid=nv, k=16, refine={"method": "plane", "iterations": 2}, threshold=0.3,
                                      max_trials=200, seed=3))


@case
def train_ops_three_interpolate_sorted(dev):
    """The Morton-order backward of three_interpolate (one atomic per block, row and channel): test_training_gpu.py's bound."""
    from dh3d_amd import pm, train_ops as T
    g = _g(83)
    lv = _level(dev, 2, 1001, 125)
    y = _randn(dev, g, 2, 125, 256)
    w = pm.idw_weights(lv["d3"])

    def call():
        (yl,) = _leaves(y)
        up = T.three_interpolate_sorted(yl, lv["i3"], w, lv["srt"])
        return [up.detach()] + list(_grads(up, [yl], 44))
    return call, {1: interp_bwd_close}


@case
def place_index_localize(dev):
    """retrieval.PlaceIndex: search and localize (retrieval, Q * k registrations, the vote, the winner's dense refinement)
    on a half-filled map."""
    from dh3d_amd import retrieval
    g = _g(97)
    n, M, N = 5, 40, 300
    desc = torch.nn.functional.normalize(_randn(dev, g, n, 256), dim=1)
    cloud = (_rand(dev, g, n, N, 3) * 10).contiguous()
    rows = torch.cat([cloud[:, :M], torch.nn.functional.normalize(_randn(dev, g, n, M, 128), dim=2), _rand(dev, g, n, M, 1)], 2)
    kc = torch.tensor([40, 33, 40, 12, 40], dtype=torch.int32, device=dev)
    index = retrieval.PlaceIndex(dim=256, capacity=9, device=dev, keypoints=M, row_dim=132, points=N)
    index.add(desc, pos=torch.rand(n, 2, generator=g, dtype=torch.float64), kp_rows=rows, kp_count=kc, cloud=cloud)
    q = [1, 3, 4]
    qd, qr, qc = (desc[q] + 0.01).contiguous(), rows[q].clone(), kc[q].clone()
    qr[:, :, :3] += 0.25
    qcloud = (cloud[q] + 0.25).contiguous()
    return lambda: (index.search(qd, 7), index.localize(qd, qr, qc, k=3, threshold=0.2, max_trials=100, seed=2),
                    index.localize(qd, qr, qc, k=3, threshold=0.2, max_trials=100, seed=2, refine={"iterations": 2},
                                   query_cloud=qcloud))


# ------------------------------------------------------------------------------------------------ retrieval / scancontext / pairs / tuples
@case
def retrieval_and_scan_context(dev):
    from dh3d_amd import retrieval, scancontext as scx
    g = _g(95)
    ref, qry = _randn(dev, g, 333, 256), _randn(dev, g, 7, 256)
    cnt = torch.tensor([300], dtype=torch.int32, device=dev)
    pts = (torch.randn(3, 1001, 3, generator=g) * torch.tensor([20.0, 20.0, 1.0])).to(dev).contiguous()
    nv = torch.tensor([1001, 640, 0], dtype=torch.int32, device=dev)

    def call():
        sc = scx.scan_context(pts, nv)
        cand = retrieval.search_descriptors_sq(sc["ring_key"], sc["ring_key"], 3)[0]
        return (retrieval.search_descriptors(ref, qry, 5), retrieval.search_descriptors_sq(ref, qry, 64, ref_count=cnt), sc,
                scx.scan_context_distance(sc["desc"], sc["desc"], cand, map_count=torch.tensor([2], dtype=torch.int32, device=dev)))
    return call


@case
def pairs_and_tuples(dev):
    from dh3d_amd import pairs, tuples
    g = _g(96)
    src = (_rand(dev, g, 2, 700, 3) * 10).contiguous()
    nv = torch.tensor([700, 301], dtype=torch.int32, device=dev)
    pos = (torch.rand(70, 2, generator=g, dtype=torch.float64) * 60).to(dev)
    cnt = torch.tensor([65], dtype=torch.int32, device=dev)
    desc = _randn(dev, g, 70, 64)

    def call():
        n_pos, n_neg = tuples.tuple_counts(pos, cnt)
        q, ok = tuples.draw_queries(n_pos, n_neg, 5, 2, 3, count=cnt, seed=4)
        return (pairs.resample_clouds(src, nv, 512, seed=1), pairs.resample_clouds(src, nv, 200, seed=1),
                pairs.augment_clouds(src, ("Jitter", "Scale", "RotateSmall", "Shift", "Rotate1D"), seed=2),
                pairs.make_local_pairs(src, nv, numpts=512, sample_nodes=64, seed=3),
                pairs.make_global_batch(src, nv, numpts=333, seed=3), n_pos, n_neg, q, ok,
                tuples.sample_tuples(pos, q, 2, 3, count=cnt, seed=4),
                tuples.sample_tuples(pos, q, 2, 3, count=cnt, desc=desc, num_hard=2, pool_fraction=0.5, seed=4))
    return call


# ------------------------------------------------------------------------------------------------ one operator at a time
@pytest.mark.parametrize("name", sorted(CASES))
def test_operator_does_not_depend_on_unwritten_memory(dev, name):
    built = CASES[name](dev)
    call, atomic = built if isinstance(built, tuple) else (built, None)
    torch.cuda.synchronize()
    _run_four(name, call, atomic)


# ------------------------------------------------------------------------------------------------ whole steps: inference
INFER_B, INFER_N = 2, 4100


def _fetch_names(model):
    names = set(model.OUTPUT_NAMES)
    if not model.config.detection:
        names -= set(model.KEYPOINT_OUTPUTS)
    return tuple(sorted(names))


def _forward_outputs(outs):
    return {k: v.clone() for k, v in outs.items() if torch.is_tensor(v)}


@pytest.mark.parametrize("preset", ["basic_config", "detection_config", "global_config"])
def test_inference_forward_does_not_depend_on_unwritten_memory(dev, preset):
    """forward() with every fetch name the model offers, plain and under each poison, and through a captured graph whose
    capture (the fills with it: every replay poisons again) ran under a poison.  Bit for bit -- but the global
    descriptor, whose walk sums A' with f32 atomics, within pm.global_tail's own bound (test_pm_gpu.py)."""
    model = _model(dev, preset, seed=0).prepare()
    names = _fetch_names(model)
    pts = _rand(dev, _g(4100), INFER_B, INFER_N, 3)
    nv = torch.tensor([INFER_N, INFER_N - 700], dtype=torch.int32, device=dev) if model.config.detection else None
    runs = {}
    with torch.no_grad():
        for kind in (None,) + KINDS:
            with poisoned(kind):
                runs[kind] = _forward_outputs(model(pts, fetch=names, num_valid=nv))
                torch.cuda.synchronize()
        atomic = {i: global_tail_close for i, (n, _) in enumerate(_flat(runs[None])) if "globaldesc" in n}
        assert {"knn_inds", "feat", "xyz_feat", "fps_inds", "nn3_inds"} <= set(runs[None]), sorted(runs[None])
        assert ("globaldesc" in runs[None]) == bool(model.config.extract_global)
        assert ("kp_inds" in runs[None]) == bool(model.config.detection)
        _agree("forward[%s]" % preset, runs, atomic)
        for kind in ("nan", "pos"):
            with poisoned(kind):
                f = model.graphed(pts, outputs=names, example_num_valid=nv)
                replays = []
                for _ in range(2):
                    replays.append(_forward_outputs(f(pts, num_valid=nv)))
                    torch.cuda.synchronize()
            for i, got in enumerate(replays):
                keys = sorted(set(got) & set(runs[None]))
                assert keys == sorted(got), (sorted(got), sorted(runs[None]))
                _agree("graphed forward[%s] under %r, replay %d" % (preset, kind, i),
                       {k: ({n: runs[None][n] for n in keys} if k is None else got) for k in (None,) + KINDS},
                       {j: global_tail_close for j, n in enumerate(keys) if n == "globaldesc"})
            del f


# ------------------------------------------------------------------------------------------------ whole steps: trainers
class _Poisoned(object):
    """A trainer whose every step runs inside poisoned(kind); everything else is the trainer's."""

    def __init__(self, trainer, kind):
        self.__dict__.update(_trainer=trainer, _kind=kind)

    def step(self, *args, **kw):
        with poisoned(self._kind):
            return self._trainer.step(*args, **kw)

    def __getattr__(self, name):
        return getattr(self._trainer, name)


def _finite_grads(trainer, step):
    """_grad_errors keeps its worst entry with max(): a NaN error never compares greater and would drop out."""
    names = {id(p): n for n, p in trainer.model.named_parameters()}
    for p in trainer.params:
        assert p.grad is None or bool(torch.isfinite(p.grad).all()), (step, names[id(p)])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("preset", ["basic_config", "detection_config"])
def test_local_trainer_steps_do_not_depend_on_unwritten_memory(dev, preset, kind):
    """Three eager steps, the capture and two replays of a LocalTrainer that is built and stepped inside poisoned(kind)
    against an unpoisoned eager twin: losses, every gradient and the moving averages by test_local_training_gpu.py's own
    _step_both and bounds."""
    import test_local_training_gpu as LT
    from dh3d_amd.training import LocalTrainer
    batches = [tuple(LT._T(a, dev) for a in LT._pairs(seed=s, n=2048, m=128)) for s in (92, 93)]
    ma, mb = LT._build(dev, preset, seed=12), LT._build(dev, preset, seed=12)
    with poisoned(kind):
        graphed = _Poisoned(LocalTrainer(ma, graph_step=True, start_lr=1e-8), kind)
    eager = LocalTrainer(mb, graph_step=False, start_lr=1e-8)
    eager.keep_grads = True
    report = []
    for i in range(6):
        dl, (err, name) = LT._step_both(graphed, eager, batches[i % 2])
        _finite_grads(graphed, i)
        report.append((i, round(err, 6), name, "%.2g" % dl))
    assert len(graphed._graphs) == 1 and not eager._graphs
    ema = LT._ema_error(graphed.model, eager.model)
    print("poisoned(%r) %s trainer vs plain eager twin: per-step worst gradient error" % (kind, preset), report, "EMA", ema)
    for i, err, name, _ in report:
        assert err <= LT.TOL_REPLAY, (i, name, err)
    assert ema[0] <= LT.TOL_EMA, ema


@pytest.mark.parametrize("kind", KINDS)
def test_quadruplet_trainer_steps_do_not_depend_on_unwritten_memory(dev, kind):
    """One eager step and one replayed step of a QuadrupletTrainer under poisoned(kind) against a plain eager twin at the
    smallest batch of test_training_gpu.py (7 x 1024), at its vanishing rate.  Bounds: that file's
    test_trainer_zero_arena_and_input_buffer (loss 1e-4 relative; gradients 5e-3 of the tensor's largest entry + 1e-6)."""
    import test_training_gpu as GT
    from dh3d_amd.training import QuadrupletTrainer
    batch = torch.rand(7, 1024, 3, generator=_g(11)).to(dev)
    ma, mb = GT._build(dev, seed=51, B=1, P=2, Ng=3), GT._build(dev, seed=51, B=1, P=2, Ng=3)
    with poisoned(kind):
        tr = QuadrupletTrainer(ma, start_lr=1e-8, graph_step=True)
    twin = QuadrupletTrainer(mb, start_lr=1e-8, graph_step=False)
    twin.keep_grads = True
    for i in range(4):     # steps 1-3 eager, step 4 captured and replayed
        with poisoned(kind):
            la = tr.step(batch)
            got = [None if p.grad is None else p.grad.detach().clone() for p in tr.params]
        lb = twin.step(batch)
        assert bool(tr._graphs) == (i == 3)
        assert np.isfinite(la) and abs(la - lb) <= 1e-4 * max(1.0, abs(lb)), (i, la, lb)
        for p, x, y in zip(tr.params, got, twin.last_grads):
            assert (x is None) == (y is None)
            if y is not None:
                assert torch.isfinite(x).all(), i
                assert float((x - y).abs().max()) <= 5e-3 * float(y.abs().max()) + 1e-6, (i, tuple(p.shape))


# ------------------------------------------------------------------------------------------------ the recorded situation
def test_two_shape_trainer_after_a_dropped_graph_left_sevens_in_its_pool(dev):
    """What the ISS commit recorded: a small graph of a library call is captured after a warm-up on a side stream of the
    test's own, its outputs are filled with 7.0, the graph is dropped -- its pool goes back to the allocator holding
    sevens -- and then the two-shape twin sequence of test_local_trainer_graphs_of_two_shapes_match_eager_steps runs.
    Every step's loss and gradients must match the eager twin's (that file's _step_both and bounds)."""
    import test_iss_gpu as TI
    import test_local_training_gpu as LT
    from dh3d_amd import registration as reg
    x, cnt, r_s, r_n = TI._batch(dev, "small")
    radius = (torch.full((x.shape[0],), r_s, device=dev), torch.full((x.shape[0],), r_n, device=dev))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        reg.iss_keypoints(x, cnt, *radius, max_keypoints=256, eigenvalues=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gout = reg.iss_keypoints(x, cnt, *radius, max_keypoints=256, eigenvalues=True)
    g.replay()
    torch.cuda.synchronize()
    for t in gout.values():
        if torch.is_tensor(t):
            t.fill_(7)
    torch.cuda.synchronize()
    del g, gout
    small = [tuple(LT._T(a, dev) for a in LT._pairs(seed=s, n=2048, m=128)) for s in (96, 97)]
    large = [tuple(LT._T(a, dev) for a in LT._pairs(seed=s, n=4096, m=128)) for s in (98, 99)]
    order = [small[0]] * 4 + [large[0]] * 4 + [small[1], large[1], small[0], large[0]]
    graphed, eager = LT._twins(dev, "basic_config", 14, start_lr=1e-8)
    report = []
    for i, b in enumerate(order):
        dl, (err, name) = LT._step_both(graphed, eager, b)
        _finite_grads(graphed, i)
        report.append((round(err, 6), name, "%.2g" % dl))
        if i >= 3:
            junk = torch.full((1 << 22,), 1e30, device=dev)
            del junk
    assert len(graphed._graphs) == 2, list(graphed._graphs)
    print("two captured shapes after a dropped graph's sevens: per-step worst gradient error", report)
    for i, (err, name, _) in enumerate(report):
        assert err <= LT.TOL_REPLAY, (i, name, err)
