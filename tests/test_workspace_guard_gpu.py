"""GPU: no entry point writes past the workspace size it asks for.  Each of them runs once over a buffer of need + 4096
bytes filled with a byte pattern, told workspace_bytes = need, at the smallest shape that puts every segment of its
layout (csrc/workspace.h) in use: the tail must come back untouched, and the outputs must equal a second run over a
workspace twice as large that starts from zero bytes instead (a segment read before it is written shows) -- bit for
bit where the op has no f32 atomics, within the op's own test's tolerance for the gradients that are summed by atomics
(flex_conv: tests/test_backward_gpu.py, 1e-4 of the largest entry; FlexDeconv's weight gradients:
tests/test_flex_deconv_gpu.py, rtol = atol = 1e-3)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TAIL = 4096
PATTERN = 0xA5


def f32(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def guarded(dev, query, shape, launch, atomic=()):
    """launch(ws_ptr, ws_bytes) -> output tensors; atomic: {output index: check(got, expected)} for the summed ones."""
    from dh3d_amd import _lib
    need = getattr(_lib.lib(), query)(*shape)
    assert need > 0, (query, shape)
    small = torch.full((need + TAIL,), PATTERN, dtype=torch.uint8, device=dev)
    # the second workspace starts from other bytes: an output that depends on what a workspace held before the call
    # differs between the two runs
    large = torch.zeros((2 * need,), dtype=torch.uint8, device=dev)
    got = launch(small.data_ptr(), need)
    exp = launch(large.data_ptr(), 2 * need)
    torch.cuda.synchronize()
    assert bool((small[need:] == PATTERN).all()), "%s%s wrote past its %d bytes" % (query, shape, need)
    assert len(got) == len(exp)
    for i, (a, b) in enumerate(zip(got, exp)):
        if i in atomic:
            atomic[i](a.cpu().numpy(), b.cpu().numpy())
        else:
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (query, shape, "output %d" % i)


def max_scaled(a, b):  # tests/test_backward_gpu.py
    assert float(np.abs(a - b).max()) <= 1e-4 * float(np.abs(b).max())


def deconv_close(a, b):  # tests/test_flex_deconv_gpu.py
    assert np.allclose(a, b, rtol=1e-3, atol=1e-3)


def flex_case(dev, B, N, K, Din, Dout, hub=False):
    """Reference-layout operands: two clouds, N no tile multiple; hub: every edge of a cloud points at its point 0."""
    rng = np.random.default_rng(N + K + Din)
    nbr = np.zeros((B, K, N), np.int32) if hub else rng.integers(0, N, (B, K, N)).astype(np.int32)
    return dict(f=f32(rng, B, Din, N).to(dev), theta=f32(rng, 3, Din, Dout, scale=0.3).to(dev),
                bias=f32(rng, Din, Dout, scale=0.1).to(dev), nbr=torch.from_numpy(nbr).to(dev),
                pos=torch.from_numpy(rng.random((B, 3, N), dtype=np.float32)).to(dev), top=f32(rng, B, Dout, N).to(dev))


def new(dev, *shape, dtype=torch.float32):
    return torch.full(shape, -7, dtype=dtype, device=dev)


@pytest.mark.parametrize("B,N,K,Din,Dout", [(2, 70, 3, 8, 12), (1, 64, 8, 32, 64), (2, 70, 9, 64, 128)],
                         ids=["factorised", "bf16x6", "fused_f32"])
def test_flex_conv_fwd(dev, B, N, K, Din, Dout):
    from dh3d_amd import _lib as L
    c = flex_case(dev, B, N, K, Din, Dout)

    def launch(ws, nbytes):
        out = new(dev, B, Dout, N)
        L.check(L.lib().dh3d_flex_conv_fwd_ws(L.ptr(c["f"]), L.ptr(c["theta"]), L.ptr(c["bias"]), L.ptr(c["nbr"]),
                                              L.ptr(c["pos"]), B, N, K, 3, Din, Dout, L.ptr(out), ws, nbytes,
                                              L.stream_ptr()), "flex_conv_fwd_ws")
        return [out]

    guarded(dev, "dh3d_flex_conv_fwd_workspace_bytes", (B, N, K, 3, Din, Dout), launch)


def test_flex_conv_bwd(dev):
    from dh3d_amd import _lib as L
    B, N, K, Din, Dout = 2, 70, 3, 8, 12
    c = flex_case(dev, B, N, K, Din, Dout)

    def launch(ws, nbytes):
        gf, gt, gb = new(dev, B, Din, N), new(dev, 3, Din, Dout), new(dev, Din, Dout)
        L.check(L.lib().dh3d_flex_conv_bwd_ws(L.ptr(c["f"]), L.ptr(c["theta"]), L.ptr(c["bias"]), L.ptr(c["nbr"]),
                                              L.ptr(c["pos"]), L.ptr(c["top"]), B, N, K, 3, Din, Dout, L.ptr(gf),
                                              L.ptr(gt), L.ptr(gb), ws, nbytes, L.stream_ptr()), "flex_conv_bwd_ws")
        return [gf, gt, gb]

    guarded(dev, "dh3d_flex_conv_bwd_workspace_bytes", (B, N, K, 3, Din, Dout), launch,
            atomic={0: max_scaled, 1: max_scaled, 2: max_scaled})


def test_flex_conv_pm_bwd(dev):
    from dh3d_amd import _lib as L
    B, N, K, Din, Dout = 2, 70, 3, 8, 12
    c = flex_case(dev, B, N, K, Din, Dout)
    f, xyz, nbr, g = [c[k].transpose(1, 2).contiguous() for k in ("f", "pos", "nbr", "top")]

    def launch(ws, nbytes):
        gf, gt, gb = new(dev, B, N, Din), new(dev, 3, Din, Dout), new(dev, Din, Dout)
        L.check(L.lib().dh3d_flex_conv_pm_bwd(L.ptr(f), L.ptr(xyz), L.ptr(nbr), L.ptr(c["theta"]), L.ptr(c["bias"]),
                                              L.ptr(g), B, N, K, Din, Dout, 1, ws, nbytes, L.ptr(gf), L.ptr(gt),
                                              L.ptr(gb), L.stream_ptr()), "flex_conv_pm_bwd")
        return [gf, gt, gb]

    guarded(dev, "dh3d_flex_conv_pm_bwd_workspace_bytes", (B, N, Din, Dout), launch,
            atomic={0: max_scaled, 1: max_scaled, 2: max_scaled})


def test_flex_pool_fwd(dev):
    from dh3d_amd import _lib as L
    B, N, K, D = 2, 70, 3, 8
    c = flex_case(dev, B, N, K, D, D)

    def launch(ws, nbytes):
        out, arg = new(dev, B, D, N), new(dev, B, D, N, dtype=torch.int32)
        L.check(L.lib().dh3d_flex_pool_fwd_ws(L.ptr(c["f"]), L.ptr(c["nbr"]), B, N, K, D, L.ptr(out), L.ptr(arg), ws,
                                              nbytes, L.stream_ptr()), "flex_pool_fwd_ws")
        return [out, arg]

    guarded(dev, "dh3d_flex_pool_fwd_workspace_bytes", (B, N, K, D), launch)


@pytest.mark.parametrize("hub", [False, True], ids=["random", "hub"])
def test_flex_deconv(dev, hub):
    """hub: the in-degree of point 0 is N * K = 210 (forward) and N = 70 (the backward's rank-0 lists), both above the 64
    entries one lane sums, so the partial rows -- the last segment of the inverted lists' layout -- are in use."""
    from dh3d_amd import _lib as L
    B, N, K, Din, Dout = 2, 70, 3, 8, 12
    c = flex_case(dev, B, N, K, Din, Dout, hub=hub)

    def fwd(ws, nbytes):
        out = new(dev, B, Dout, N)
        L.check(L.lib().dh3d_flex_deconv_fwd_ws(L.ptr(c["f"]), L.ptr(c["theta"]), L.ptr(c["bias"]), L.ptr(c["nbr"]),
                                                L.ptr(c["pos"]), B, N, K, 3, Din, Dout, L.ptr(out), ws, nbytes,
                                                L.stream_ptr()), "flex_deconv_fwd_ws")
        return [out]

    def bwd(ws, nbytes):
        gf, gt, gb = new(dev, B, Din, N), new(dev, 3, Din, Dout), new(dev, Din, Dout)
        L.check(L.lib().dh3d_flex_deconv_bwd_ws(L.ptr(c["f"]), L.ptr(c["theta"]), L.ptr(c["bias"]), L.ptr(c["nbr"]),
                                                L.ptr(c["pos"]), L.ptr(c["top"]), B, N, K, 3, Din, Dout, L.ptr(gf),
                                                L.ptr(gt), L.ptr(gb), ws, nbytes, L.stream_ptr()), "flex_deconv_bwd_ws")
        return [gf, gt, gb]

    guarded(dev, "dh3d_flex_deconv_fwd_workspace_bytes", (B, N, K, 3, Din, Dout), fwd)
    guarded(dev, "dh3d_flex_deconv_bwd_workspace_bytes", (B, N, K, 3, Din, Dout), bwd,
            atomic={1: deconv_close, 2: deconv_close})


def test_keypoint_nms(dev):
    from dh3d_amd import _lib as L
    B, N, K, M = 2, 300, 8, 16
    rng = np.random.default_rng(300)
    pts = torch.from_numpy(rng.random((B, N, 3), dtype=np.float32)).to(dev)
    dist, nn = torch.cdist(pts, pts).topk(K, dim=2, largest=False)
    dist, nn = dist.contiguous(), nn.to(torch.int32).contiguous()
    score = torch.from_numpy(rng.random((B, N), dtype=np.float32)).to(dev)

    def launch(ws, nbytes):
        count, inds = new(dev, B, dtype=torch.int32), new(dev, B, M, dtype=torch.int32)
        L.check(L.lib().dh3d_keypoint_nms(L.ptr(score), 1, 0, L.ptr(nn), L.ptr(dist), None, B, N, K, 0.1, 0.2, M, 1,
                                          L.ptr(count), L.ptr(inds), ws, nbytes, L.stream_ptr()), "keypoint_nms")
        return [count, inds]

    guarded(dev, "dh3d_keypoint_nms_workspace_bytes", (B, N, M), launch)


def test_prepare_clouds(dev):
    """Voxels of edge 0.5 over 500 points of the unit cube hold about 60 points each (the member lists and the large-voxel
    records are in use); both stages on."""
    from dh3d_amd import _lib as L
    B, N, target = 2, 500, 256
    raw = torch.from_numpy(np.random.default_rng(500).random((B, N, 3), dtype=np.float32)).to(dev)
    num_raw = torch.tensor([N, N - 37], dtype=torch.int32, device=dev)

    def launch(ws, nbytes):
        points, num_valid, counts = new(dev, B, target, 3), new(dev, B, dtype=torch.int32), new(dev, B, 3, dtype=torch.int32)
        centroid = new(dev, B, 3, dtype=torch.float64)
        L.check(L.lib().dh3d_prepare_clouds(B, N, target, L.ptr(raw), L.ptr(num_raw), 0.5, 0.3, 2, 1, L.ptr(points),
                                            L.ptr(num_valid), L.ptr(counts), L.ptr(centroid), ws, nbytes,
                                            L.stream_ptr()), "prepare_clouds")
        return [points, num_valid, counts, centroid]

    guarded(dev, "dh3d_prepare_clouds_workspace", (B, N, target), launch)


@pytest.fixture(scope="module")
def vlad(dev):
    """NetVLAD operands at B = 2, N = 100 (D = 256, Cl = 64, O = 256); m = 100 sampled rows for the tail."""
    rng = np.random.default_rng(100)
    B, N, D, Cl, O = 2, 100, 256, 64, 256
    c = dict(x=f32(rng, B, N, D), att=torch.from_numpy(rng.random((B, N), dtype=np.float32)), wc=f32(rng, D * Cl, scale=0.1),
             cl_scale=f32(rng, Cl, scale=0.1) + 1, cl_shift=f32(rng, Cl, scale=0.1), W2=f32(rng, D, Cl, scale=0.1),
             Wh=f32(rng, D * Cl, O, scale=0.01), s1=f32(rng, O, scale=0.1) + 1, b1=f32(rng, O, scale=0.1),
             Wg=f32(rng, O, O, scale=0.05), s2=f32(rng, O, scale=0.1) + 1, b2=f32(rng, O, scale=0.1),
             flat=f32(rng, B, D * Cl, scale=0.01), apart=torch.from_numpy(rng.random((B, N, Cl), dtype=np.float32)),
             asum=torch.from_numpy(rng.random((B, Cl), dtype=np.float32)) * N)
    return {k: v.to(dev) for k, v in c.items()}, (B, N, D, Cl, O)


def test_netvlad_aggregate(dev, vlad):
    from dh3d_amd import _lib as L
    c, (B, N, D, Cl, O) = vlad

    def launch(ws, nbytes):
        out = new(dev, B, D * Cl)
        L.check(L.lib().dh3d_netvlad_aggregate_fwd(L.ptr(c["x"]), L.ptr(c["att"]), L.ptr(c["wc"]), L.ptr(c["cl_scale"]),
                                                   L.ptr(c["cl_shift"]), L.ptr(c["W2"]), B, N, D, Cl, ws, nbytes,
                                                   L.ptr(out), L.stream_ptr()), "netvlad_aggregate")
        return [out]

    guarded(dev, "dh3d_netvlad_workspace_bytes", (B, N, D, Cl), launch)


def test_netvlad_head(dev, vlad):
    from dh3d_amd import _lib as L
    c, (B, N, D, Cl, O) = vlad

    def launch(ws, nbytes):
        out = new(dev, B, O)
        L.check(L.lib().dh3d_netvlad_head_fwd(L.ptr(c["flat"]), L.ptr(c["Wh"]), L.ptr(c["s1"]), L.ptr(c["b1"]),
                                              L.ptr(c["Wg"]), L.ptr(c["s2"]), L.ptr(c["b2"]), B, D * Cl, O, 1e-12, ws,
                                              nbytes, L.ptr(out), L.stream_ptr()), "netvlad_head")
        return [out]

    guarded(dev, "dh3d_netvlad_head_workspace_bytes", (B, D * Cl, O), launch)


def test_netvlad_tail(dev, vlad):
    from dh3d_amd import _lib as L
    c, (B, m, D, Cl, O) = vlad

    def launch(ws, nbytes):
        out = new(dev, B, O)
        L.check(L.lib().dh3d_netvlad_tail_assign_fwd(L.ptr(c["apart"]), L.ptr(c["x"]), L.ptr(c["asum"]), m, L.ptr(c["W2"]),
                                                     L.ptr(c["Wh"]), L.ptr(c["s1"]), L.ptr(c["b1"]), L.ptr(c["Wg"]),
                                                     L.ptr(c["s2"]), L.ptr(c["b2"]), B, D, Cl, O, 1e-12, ws, nbytes,
                                                     L.ptr(out), L.stream_ptr()), "netvlad_tail_assign")
        return [out]

    guarded(dev, "dh3d_netvlad_tail_workspace_bytes", (B, D, Cl, O), launch)


def test_netvlad_fused(dev, vlad):
    from dh3d_amd import _lib as L
    c, (B, N, D, Cl, O) = vlad

    def launch(ws, nbytes):
        out = new(dev, B, O)
        L.check(L.lib().dh3d_netvlad_fused_fwd(L.ptr(c["x"]), L.ptr(c["att"]), L.ptr(c["wc"]), L.ptr(c["cl_scale"]),
                                               L.ptr(c["cl_shift"]), L.ptr(c["W2"]), L.ptr(c["Wh"]), L.ptr(c["s1"]),
                                               L.ptr(c["b1"]), L.ptr(c["Wg"]), L.ptr(c["s2"]), L.ptr(c["b2"]), B, N, D,
                                               Cl, O, 1e-12, ws, nbytes, L.ptr(out), L.stream_ptr()), "netvlad_fused")
        return [out]

    guarded(dev, "dh3d_netvlad_fused_workspace_bytes", (B, N, D, Cl, O), launch)
