"""flex_conv_x6<32,64> (eight producer lanes per point, the two producer groups alternating tiles) against two references:

* `<64,64>` on the same features zero-padded to 64 channels, with theta and bias zero-padded on the input-channel axis, bit
  for bit.  The padded channels give S = 0 and three zero bf16 planes; their k-blocks add exact +0 to accumulators that
  start at +0; the non-zero k-blocks meet each accumulator chain in the same order, and both kernels split K at the
  boundary between components 1 and 2.  The 64-channel instantiation keeps sixteen lanes per point and eight producers
  per tile, so it is an independent device reference for the 32-channel producer mapping.
* the float64 closed form  out[n] = sum_k f[nbr_k] @ (bias + dx_k theta_x + dy_k theta_y + dz_k theta_z)  at the tolerance
  tests/test_pm_gpu.py uses for this kernel, with and without the epilogue operands.

Shapes: the smallest at which the tile schedule takes another path (see SHAPES)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K, DIN, DOUT = 8, 32, 64
# (B, N, reserve_cus_per_xcd) on a 256-CU device
SHAPES = [
    (1, 32, 0),      # one tile: the second producer group never produces
    (1, 64, 0),      # two tiles in two workgroups
    (2, 1024, 31),   # 8 workgroups x 8 tiles: the steady state, both groups alternating
    (2, 1024, 30),   # 16 workgroups x 4 tiles
    (3, 1000, 31),   # R = 3000, R % 32 = 24: ragged instantiation, tiles straddling clouds, odd tile counts
    (1, 96, 31),     # three tiles in three workgroups of one tile each, the others with none
]


@functools.lru_cache(maxsize=None)
def _weights():
    g = torch.Generator().manual_seed(3264)
    theta = torch.randn(3, DIN, DOUT, generator=g) / DIN ** 0.5
    bias = torch.randn(DIN, DOUT, generator=g) / (8 * DIN) ** 0.5
    ep = (torch.randn(DOUT, generator=g), 0.5 + torch.rand(DOUT, generator=g), torch.randn(DOUT, generator=g))
    return theta, bias, ep


@functools.lru_cache(maxsize=None)
def _cloud(B, N, ids):
    """(f, xyz, nbr) on the host; ids: 'knn', 'self' (every neighbour the point itself) or 'zero' (every neighbour point 0)."""
    from dh3d_amd import pm
    g = torch.Generator().manual_seed(1000 * B + N)
    xyz = torch.rand(B, N, 3, generator=g)
    f = torch.randn(B, N, DIN, generator=g)
    if ids == "knn":
        nbr = pm.knn_xyz(xyz.cuda(), K)[0].cpu()
    elif ids == "self":
        nbr = torch.arange(N, dtype=torch.int32).view(1, N, 1).expand(B, N, K).contiguous()
    else:
        nbr = torch.zeros(B, N, K, dtype=torch.int32)
    return f, xyz, nbr


@functools.lru_cache(maxsize=None)
def _closed_form(B, N, ids):
    """float64 [B,N,DOUT] from the float32 inputs"""
    f, xyz, nbr = (t.numpy() for t in _cloud(B, N, ids))
    theta, bias, _ = _weights()
    theta, bias = theta.numpy().astype(np.float64), bias.numpy().astype(np.float64)
    b = np.arange(B)[:, None, None]
    fk = f.astype(np.float64)[b, nbr]                                                      # [B,N,K,DIN]
    d = xyz.astype(np.float64)[b, nbr] - xyz.astype(np.float64)[:, :, None, :]             # [B,N,K,3]
    out = fk.sum(2) @ bias
    for c in range(3):
        out += (fk * d[..., c:c + 1]).sum(2) @ theta[c]
    return out


def _run(dev, B, N, ids, reserve, din, epilogue):
    """flex_conv_x6 at `din` input channels: 32 as is, 64 = features, theta and bias zero-padded on the input-channel axis"""
    from dh3d_amd import pm
    f, xyz, nbr = _cloud(B, N, ids)
    theta, bias, ep = _weights()
    if din != DIN:
        f = torch.cat([f, torch.zeros(B, N, din - DIN)], 2)
        theta = torch.cat([theta, torch.zeros(3, din - DIN, DOUT)], 1)
        bias = torch.cat([bias, torch.zeros(din - DIN, DOUT)], 0)
    assert pm.flex_x6_supported(din, DOUT, K)
    wp3 = pm.pack_flex_weight_x3(theta.contiguous().to(dev), bias.contiguous().to(dev))
    kw = dict(pre_bias=ep[0].to(dev), scale=ep[1].to(dev), shift=ep[2].to(dev), act=pm.ACT_RELU) if epilogue else {}
    return pm.flex_conv_x6(f.contiguous().to(dev), xyz.to(dev), nbr.to(dev), wp3, DOUT, reserve_cus_per_xcd=reserve, **kw)


def _check(dev, B, N, ids, reserve):
    exp = _closed_form(B, N, ids)
    _, _, ep = _weights()
    fb, sc, sh = (t.numpy().astype(np.float64) for t in ep)
    for epilogue in (False, True):
        got = _run(dev, B, N, ids, reserve, DIN, epilogue)
        again = _run(dev, B, N, ids, reserve, DIN, epilogue)
        padded = _run(dev, B, N, ids, reserve, 64, epilogue)
        torch.cuda.synchronize()
        assert torch.equal(got, again), "two launches on the same inputs differ"
        assert torch.equal(got, padded), "<32,64> differs from <64,64> on zero-padded channels"
        a = got.cpu().numpy()
        atol = 1e-4 * np.abs(exp).max()
        if epilogue:
            assert np.allclose(a, np.maximum((exp + fb) * sc + sh, 0), rtol=1e-4, atol=atol)
        else:
            assert float(np.abs(a - exp).max() / (np.abs(exp).max() + 1e-30)) < 2e-6
            assert np.allclose(a, exp, rtol=1e-4, atol=atol)


@pytest.mark.parametrize("B,N,reserve", SHAPES)
def test_din32_equals_padded_din64_and_closed_form(dev, B, N, reserve):
    _check(dev, B, N, "knn", reserve)


@pytest.mark.parametrize("ids", ["self", "zero"])
def test_din32_hand_made_ids(dev, ids):
    """every neighbour the point itself (all offsets 0: S_x = S_y = S_z = 0) / every neighbour point 0 of the cloud"""
    _check(dev, 2, 1024, ids, 31)
