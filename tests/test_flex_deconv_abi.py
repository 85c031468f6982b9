"""CPU: the FlexDeconv (flex_convolution_transpose) entry points exist, reject bad arguments with status codes, size their
workspaces by the A' shape rule; the Python op and layer have the reference's interface; the float64 restatement the GPU
tests compare with agrees with the operator's definition written as loops."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from flex_deconv_reference import flex_deconv, flex_deconv_grad, flex_deconv_loops, neighbourhood

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dh3d_flex_deconv_fwd", "dh3d_flex_deconv_bwd", "dh3d_flex_deconv_fwd_f64", "dh3d_flex_deconv_bwd_f64",
         "dh3d_flex_deconv_fwd_workspace_bytes", "dh3d_flex_deconv_fwd_ws", "dh3d_flex_deconv_bwd_workspace_bytes",
         "dh3d_flex_deconv_bwd_ws")


def test_symbols_declared_bound_and_exported():
    from dh3d_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dh3d_hip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(handle, name), name


def test_bad_arguments_are_status_codes():
    from dh3d_amd import _lib
    lib = _lib.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    for fwd in (lib.dh3d_flex_deconv_fwd, lib.dh3d_flex_deconv_fwd_f64):
        assert fwd(z, one, one, one, one, 1, 32, 4, 3, 2, 6, one, z) == 1          # null features
        assert fwd(one, one, one, one, one, 1, 32, 0, 3, 2, 6, one, z) == 1        # K <= 0
        assert fwd(one, one, one, one, one, 1, 32, 4, 5, 2, 6, one, z) == 2        # Dp > kMaxDp
    for bwd in (lib.dh3d_flex_deconv_bwd, lib.dh3d_flex_deconv_bwd_f64):
        assert bwd(one, one, one, one, one, one, 1, 32, 4, 3, 2, 6, z, one, one, z) == 1
        assert bwd(one, one, one, one, one, one, 1, 32, -1, 3, 2, 6, one, one, one, z) == 1
        assert bwd(one, one, one, one, one, one, 1, 32, 4, 5, 2, 6, one, one, one, z) == 2
    assert lib.dh3d_flex_deconv_fwd_ws(one, one, one, one, one, 8, 8192, 8, 3, 64, 64, one, z, 1 << 30, z) == 1
    assert lib.dh3d_flex_deconv_fwd_ws(one, one, one, one, one, 1, 32, 4, 3, 2, 6, one, one, 1 << 30, z) == 2
    assert lib.dh3d_flex_deconv_fwd_ws(one, one, one, one, one, 8, 8192, 8, 3, 64, 64, one, one, 16, z) == 1
    assert lib.dh3d_flex_deconv_bwd_ws(one, one, one, one, one, one, 1, 32, 0, 3, 64, 64, one, one, one, one,
                                       1 << 30, z) == 1
    assert lib.dh3d_flex_deconv_bwd_ws(one, one, one, one, one, one, 1, 32, 4, 2, 64, 64, one, one, one, one,
                                       1 << 30, z) == 2


def test_workspace_bytes_follow_the_shape_rule():
    from dh3d_amd import _lib
    lib = _lib.lib()
    for fn in (lib.dh3d_flex_deconv_fwd_workspace_bytes, lib.dh3d_flex_deconv_bwd_workspace_bytes):
        assert fn(2, 32, 4, 3, 2, 6) == 0          # the reference test's Din = 2, Dout = 6
        assert fn(8, 8192, 8, 2, 64, 64) == 0      # Dp != 3
        assert fn(8, 8192, 8, 3, 64, 66) == 0      # Dout % 4
        assert fn(8, 8192, 0, 3, 64, 64) == 0
        assert fn(8, 8192, 8, 3, 64, 64) > 0
        assert fn(8, 8192, 8, 3, 32, 64) > 0
        assert fn(4096, 1 << 20, 8, 3, 256, 256) == 0   # buffers beyond 32-bit extents


def test_op_rejects_cpu_tensors():
    from dh3d_amd import ops
    assert "flex_convolution_transpose" in ops.__all__
    f = torch.zeros(1, 4, 16)
    with pytest.raises(ValueError):
        ops.flex_convolution_transpose(f, torch.zeros(1, 3, 16), torch.zeros(1, 4, 16, dtype=torch.int32),
                                       torch.zeros(3, 4, 8), torch.zeros(4, 8))


@pytest.mark.parametrize("data_format", ["simple", "expanded"])
def test_layer_parameters(data_format):
    from dh3d_amd import layers
    assert "FlexConvolutionTranspose" in layers.__all__ and "flex_convolution_transpose" in layers.__all__
    layer = layers.FlexConvolutionTranspose(32, 64, data_format=data_format)
    shapes = {n: tuple(p.shape) for n, p in layer.named_parameters()}
    assert shapes == {"position_theta": (3, 32, 64), "position_bias": (32, 64), "feature_bias": (64, 1)}
    assert not layer.position_bias.detach().any() and not layer.feature_bias.detach().any()
    assert float(layer.position_theta.detach().abs().max()) <= np.sqrt(6.0 / (32 + 64))
    nobias = layers.FlexConvolutionTranspose(8, 16, dp=2, use_feature_bias=False, data_format=data_format)
    assert {n: tuple(p.shape) for n, p in nobias.named_parameters()} == {"position_theta": (2, 8, 16),
                                                                        "position_bias": (8, 16)}


@pytest.mark.parametrize("kind", ["knn", "random", "dup", "hub", "hub0", "holes"])
def test_restatement_matches_the_loops(kind):
    rng = np.random.default_rng(3)
    B, N, K, Dp, Din, Dout = 2, 20, 5, 3, 3, 4
    f = rng.standard_normal((B, Din, N))
    p = rng.standard_normal((B, Dp, N))
    th, bi = rng.standard_normal((Dp, Din, Dout)), rng.standard_normal((Din, Dout))
    nb = neighbourhood(kind, B, N, K, rng, p)
    out = flex_deconv(f, p, nb, th, bi)
    np.testing.assert_allclose(out, flex_deconv_loops(f, p, nb, th, bi), rtol=1e-12, atol=1e-12)
    if kind == "holes":
        named = np.zeros((B, N), bool)
        for b in range(B):
            named[b, np.unique(nb[b])] = True
        assert (~named).any() and not out.transpose(0, 2, 1)[~named].any()
    # the gradients: the operator is linear in f, in theta and in bias, so <out, g> = <f, grad_f> = <theta, grad_theta>
    # + <bias, grad_bias>; and one entry of each by a finite difference of the loops
    g = rng.standard_normal((B, Dout, N))
    gf, gt, gb = flex_deconv_grad(f, p, nb, th, bi, g)
    dot = float((out * g).sum())
    assert abs(dot - float((f * gf).sum())) < 1e-9 * max(1.0, abs(dot))
    assert abs(dot - float((th * gt).sum() + (bi * gb).sum())) < 1e-9 * max(1.0, abs(dot))
    e = np.zeros_like(f)
    e[1, 2, nb[1, 0, 7]] = 1.0
    assert abs(float((flex_deconv_loops(e, p, nb, th, bi) * g).sum()) - gf[1, 2, nb[1, 0, 7]]) < 1e-9
    et = np.zeros_like(th)
    et[2, 1, 3] = 1.0
    lin = float((flex_deconv_loops(f, p, nb, et, np.zeros_like(bi)) * g).sum())
    assert abs(lin - gt[2, 1, 3]) < 1e-9 * max(1.0, abs(lin))
