"""GPU: flex_convolution_transpose (FlexDeconv) on both paths -- the reference formulation (section A, FAST_PATH off) and
the inverted-list form (section A', FAST_PATH on) -- against the float64 restatement of tests/flex_deconv_reference.py."""
import os

import numpy as np
import pytest
import torch

from flex_deconv_reference import flex_deconv, flex_deconv_grad, neighbourhood

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def close(a, b, rtol=1e-4, atol=1e-6):
    return np.allclose(a, b, rtol=rtol, atol=atol)


def close_sum(a, b, rtol=1e-4, k=2e-6):
    """The reference criterion with the absolute floor scaled to the output magnitude (as tests/test_ops_gpu.py)."""
    return np.allclose(a, b, rtol=rtol, atol=max(1e-6, k * float(np.abs(b).max())))


@pytest.fixture(params=[True, False], ids=["fast", "reference"])
def path(request):
    from dh3d_amd import ops
    old = ops.FAST_PATH
    ops.FAST_PATH = request.param
    yield request.param
    ops.FAST_PATH = old


def served(B, N, K, Din, Dout):
    from dh3d_amd import _lib
    return _lib.lib().dh3d_flex_deconv_fwd_workspace_bytes(B, N, K, 3, Din, Dout) > 0


def case(rng, B, N, K, Din, Dout, kind="knn", dev=None, pos=None, nbr=None):
    pos = rng.random((B, 3, N), dtype=np.float32) if pos is None else pos
    if nbr is None:
        if kind == "knn":  # the library's kNN (bit-exact to the reference's), as [B, K, N]
            from dh3d_amd import ops
            nn_, _ = ops.knn_bruteforce(T(pos, dev), K)
            nbr = np.ascontiguousarray(nn_.cpu().numpy().transpose(0, 2, 1))
        else:
            nbr = neighbourhood(kind, B, N, K, rng)
    lim = np.sqrt(6.0 / (Din + Dout))
    return dict(features=rng.standard_normal((B, Din, N)).astype(np.float32), position=pos, neighborhood=nbr,
                theta=rng.uniform(-lim, lim, (3, Din, Dout)).astype(np.float32),
                bias=rng.uniform(-0.1, 0.1, (Din, Dout)).astype(np.float32),
                topdiff=rng.standard_normal((B, Dout, N)).astype(np.float32))


def run(c, dev, backward=True):
    from dh3d_amd import ops
    f = T(c["features"], dev).requires_grad_()
    th = T(c["theta"], dev).requires_grad_()
    bi = T(c["bias"], dev).requires_grad_()
    out = ops.flex_convolution_transpose(f, T(c["position"], dev), T(c["neighborhood"], dev), th, bi)
    if not backward:
        return out.detach().cpu().numpy(), None
    out.backward(T(c["topdiff"], dev))
    return out.detach().cpu().numpy(), (f.grad.cpu().numpy(), th.grad.cpu().numpy(), bi.grad.cpu().numpy())


def check(c, out, grads, fwd_check=close_sum):
    args = (c["features"], c["position"], c["neighborhood"], c["theta"], c["bias"])
    exp = flex_deconv(*args)
    assert out.shape == exp.shape
    assert fwd_check(out, exp), float(np.abs(out - exp).max())
    if grads is None:
        return
    gf, gt, gb = flex_deconv_grad(*args, c["topdiff"])
    # summation / atomics order differs from the restatement: 1e-3 relative, as flex_conv's gradients are checked
    assert close(grads[0], gf, 1e-3, 1e-4), float(np.abs(grads[0] - gf).max())
    assert close(grads[1], gt, 1e-3, 1e-3), float(np.abs(grads[1] - gt).max())
    assert close(grads[2], gb, 1e-3, 1e-3), float(np.abs(grads[2] - gb).max())


def test_reference_test_case(dev, path):
    """The reference's own test case (B=2, N=32, K=4, Din=2, Dout=6; tests/golden/fake_pointcloud.npz) -- a shape A' does
    not serve, so both settings run section A."""
    c = dict(np.load(os.path.join(G, "fake_pointcloud.npz")))
    out, grads = run(c, dev)
    check(c, out, grads, close)


@pytest.mark.parametrize("B,N,K,Din,Dout", [(4, 1024, 8, 32, 64), (4, 1024, 8, 64, 64), (8, 8192, 8, 32, 64),
                                            (8, 8192, 8, 64, 64), (4, 1024, 8, 48, 96), (2, 1000, 16, 32, 64),
                                            (1, 20000, 8, 32, 32)])
def test_knn_shapes(dev, path, B, N, K, Din, Dout):
    assert served(B, N, K, Din, Dout)
    c = case(np.random.default_rng(B * 7 + N + Din), B, N, K, Din, Dout, dev=dev)
    check(c, *run(c, dev))


def test_demo_cloud(dev, path):
    """A LiDAR cloud in metres (local_268, 16384 points) with its stored kNN lists: in-degree median 8, max 18."""
    d = np.load(os.path.join(G, "demo_clouds.npz"))
    pos = np.ascontiguousarray(d["local_268"].T[None])
    nbr = np.ascontiguousarray(d["local_268/knn"].T[None]).astype(np.int32)
    c = case(np.random.default_rng(268), 1, 16384, 8, 32, 64, pos=pos, nbr=nbr)
    check(c, *run(c, dev))


@pytest.mark.parametrize("kind", ["random", "dup", "hub", "hub0", "holes"])
def test_neighbourhood_edge_cases(dev, path, kind):
    """Lists whose centre is not the point, repeated ids, a hub target (in-degree >= N: the chunked sums), a hub centre
    (every point's rank 0 is point 0: the backward's rank-0 lists are skewed), points no list names (exactly 0)."""
    B, N, K, Din, Dout = 2, 2048, 8, 32, 64
    c = case(np.random.default_rng(11), B, N, K, Din, Dout, kind=kind)
    out, grads = run(c, dev)
    check(c, out, grads)
    if kind == "holes":
        named = np.zeros((B, N), bool)
        for b in range(B):
            named[b, np.unique(c["neighborhood"][b])] = True
        assert (~named).any()
        assert not out.transpose(0, 2, 1)[~named].any()


@pytest.mark.parametrize("kind", ["knn", "random"])
def test_f64_gradcheck(dev, kind):
    from dh3d_amd import ops
    c = dict(np.load(os.path.join(G, "fake_pointcloud.npz")))
    nbr = c["neighborhood"] if kind == "knn" else neighbourhood("random", 2, 32, 4, np.random.default_rng(5))
    f = T(c["features"].astype(np.float64), dev).requires_grad_()
    th = T(c["theta"].astype(np.float64), dev).requires_grad_()
    bi = T(c["bias"].astype(np.float64), dev).requires_grad_()
    p = T(c["position"].astype(np.float64), dev)
    nb = T(nbr, dev)
    out = ops.flex_convolution_transpose(f, p, nb, th, bi)
    exp = flex_deconv(c["features"].astype(np.float64), c["position"].astype(np.float64), nbr,
                      c["theta"].astype(np.float64), c["bias"].astype(np.float64))
    np.testing.assert_allclose(out.detach().cpu().numpy(), exp, rtol=1e-10, atol=1e-10)
    assert torch.autograd.gradcheck(lambda a, t, b: ops.flex_convolution_transpose(a, p, nb, t, b), (f, th, bi),
                                    nondet_tol=1e-12)


def test_fast_path_is_reproducible(dev):
    """A': the output and grad_features are bitwise equal across calls on the hub neighbourhood (fixed list order, no
    atomics; grad_theta / grad_bias come from the split-K GEMM's atomics and are not compared)."""
    from dh3d_amd import ops
    assert ops.FAST_PATH
    c = case(np.random.default_rng(12), 2, 4096, 8, 32, 64, kind="hub")
    o1, g1 = run(c, dev)
    o2, g2 = run(c, dev)
    assert np.array_equal(o1, o2)
    assert np.array_equal(g1[0], g2[0])


def test_graph_capture(dev):
    """A' forward + backward captured on one stream and replayed equals eager: nothing in them synchronises or allocates
    outside torch's allocator."""
    from dh3d_amd import ops
    assert ops.FAST_PATH
    c = case(np.random.default_rng(13), 4, 1024, 8, 32, 64, kind="random")
    f = T(c["features"], dev).requires_grad_()
    th = T(c["theta"], dev).requires_grad_()
    bi = T(c["bias"], dev).requires_grad_()
    p, nb, g = T(c["position"], dev), T(c["neighborhood"], dev), T(c["topdiff"], dev)

    def step():
        out = ops.flex_convolution_transpose(f, p, nb, th, bi)
        return (out,) + torch.autograd.grad(out, (f, th, bi), g)

    eager = [t.detach().clone() for t in step()]           # warm-up and the eager result
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    graph.replay()
    torch.cuda.synchronize()
    # output and grad_features: bitwise; grad_theta / grad_bias: up to the split-K GEMM's atomics order
    assert torch.equal(static[0], eager[0]) and torch.equal(static[1], eager[1])
    for a, b in zip(static[2:], eager[2:]):
        a, b = a.detach().cpu().numpy(), b.cpu().numpy()
        assert np.allclose(a, b, rtol=1e-5, atol=1e-6 * float(np.abs(b).max())), float(np.abs(a - b).max())


@pytest.mark.parametrize("data_format", ["simple", "expanded"])
def test_layer(dev, data_format):
    from dh3d_amd import layers
    rng = np.random.default_rng(14)
    c = case(rng, 2, 1024, 8, 32, 64, dev=dev)
    x, p, nb = T(c["features"], dev), T(c["position"], dev), T(c["neighborhood"], dev)
    if data_format == "expanded":
        x, p, nb = x.unsqueeze(2), p.unsqueeze(2), nb.unsqueeze(2)
    torch.manual_seed(0)
    y = layers.flex_convolution_transpose(x, p, nb, 64, activation=torch.relu, data_format=data_format)
    torch.manual_seed(0)
    layer = layers.FlexConvolutionTranspose(32, 64, activation=torch.relu, data_format=data_format).to(dev)
    with torch.no_grad():
        layer.position_bias.copy_(T(c["bias"], dev))
        layer.feature_bias.copy_(T(rng.uniform(-1, 1, (64, 1)).astype(np.float32), dev))
    z = layer(x, p, nb)
    assert y.shape == z.shape == ((2, 64, 1, 1024) if data_format == "expanded" else (2, 64, 1024))
    theta = layer.position_theta.detach().cpu().numpy()
    exp0 = flex_deconv(c["features"], c["position"], c["neighborhood"], theta, np.zeros((32, 64), np.float32))
    exp = flex_deconv(c["features"], c["position"], c["neighborhood"], theta, c["bias"])
    exp = np.maximum(exp + layer.feature_bias.detach().cpu().numpy()[None], 0.0)
    if data_format == "expanded":
        y, z = y.squeeze(2), z.squeeze(2)
    assert close_sum(y.detach().cpu().numpy(), np.maximum(exp0, 0.0))
    assert close_sum(z.detach().cpu().numpy(), exp)
