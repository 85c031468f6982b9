"""No GPU: pins tests/dense_reference.py, the float64 yardstick of the dense matrix-pipe kernels, and proves that the
selection and single-product probes built on it are sharp -- the bf16x3 split is exact, six chunk products in any order are within 2^-20 of the float64
product, and losing any one of them is not."""
import numpy as np
import pytest

import dense_reference as D

N_PROD = 1 << 20


def _wide(rng, shape):
    """normal x exp(uniform(-8, 8)): the draw of the single-product probes."""
    return (rng.standard_normal(shape) * np.exp(rng.uniform(-8, 8, shape))).astype(np.float32)


@pytest.fixture(scope="module")
def products():
    rng = np.random.default_rng(20)
    x, w = _wide(rng, N_PROD), _wide(rng, N_PROD)
    exact = x.astype(np.float64) * w.astype(np.float64)
    assert np.abs(exact).min() > 2.0 ** -100
    return x, w, exact


def test_split3_is_exact_bit_for_bit():
    rng = np.random.default_rng(1)
    a = np.concatenate([_wide(rng, 1 << 18), np.float32([0.0, 1.0, -1.0, 1 + 2.0 ** -9, 2.0 ** -6, -2.0 ** 6]),
                        np.ldexp(rng.uniform(1, 2, 4096), rng.integers(-60, 60, 4096)).astype(np.float32)])
    c1, c2, c3 = D.split3(a)
    for c in (c1, c2, c3):                                     # every chunk is a bf16: low 16 bits clear
        assert not np.any(c.view(np.uint32) & np.uint32(0xFFFF))
    s = (c1 + c2).astype(np.float32) + c3
    assert np.array_equal(s.view(np.uint32), a.view(np.uint32))
    assert np.array_equal(c1.astype(np.float64) + c2 + c3, a.astype(np.float64))


def test_single_product_bound_is_two_to_the_minus_twenty():
    assert D.SINGLE_PRODUCT_BOUND == 2.0 ** -20 == 16 * 2.0 ** -24


@pytest.mark.parametrize("order", [D.SIX, D.SIX[::-1], ((2, 2), (1, 1), (3, 1), (1, 2), (1, 3), (2, 1))],
                         ids=["descending", "ascending", "mixed"])
def test_six_products_in_any_order_are_within_the_bound(products, order):
    x, w, exact = products
    rel = np.abs(D.six_products(x, w, order) - exact) / np.abs(exact)
    assert rel.max() <= D.SINGLE_PRODUCT_BOUND, rel.max() / 2.0 ** -24


@pytest.mark.parametrize("dropped", D.SIX, ids=["c%dd%d" % p for p in D.SIX])
def test_one_product_removed_is_ten_times_over_the_bound(products, dropped):
    x, w, exact = products
    keep = tuple(p for p in D.SIX if p != dropped)
    assert len(keep) == 5
    rel = np.abs(D.six_products(x, w, keep) - exact) / np.abs(exact)
    assert rel.max() >= 10 * D.SINGLE_PRODUCT_BOUND, rel.max() / 2.0 ** -24


def test_second_order_probe_value_needs_c2d2():
    v = np.float32(1 + 2.0 ** -9)
    want = np.float32(1 + 2.0 ** -8 + 2.0 ** -18)
    assert float(want) == 1 + 2.0 ** -8 + 2.0 ** -18          # exact in f32
    assert D.six_products(v, v) == want
    assert D.six_products(v, v, tuple(p for p in D.SIX if p != (2, 2))) != want


def test_one_hot_rows_give_the_weight_back_exactly():
    rng = np.random.default_rng(3)
    W = _wide(rng, (96, 128))
    v, T = D.linear(np.eye(96, dtype=np.float32), W)
    assert np.array_equal(v, W.astype(np.float64)) and np.array_equal(T, np.abs(W.astype(np.float64)))
    W = _wide(rng, (64, 1024))
    s, _ = D.linear_slices(np.eye(64, dtype=np.float32), W, 4)
    assert s.shape == (4, 64, 256)
    for i in range(4):                                         # slice i = the columns 256 i .. 256 i + 255, row r = W[r]
        assert np.array_equal(s[i], W[:, 256 * i:256 * (i + 1)].astype(np.float64))


def _ep(rng, n, act, mask=7):
    v = [rng.standard_normal(n).astype(np.float32) if mask >> i & 1 else None for i in range(3)]
    return (v[0], v[1], v[2], act)


def _geom(rng, B, n, m):
    idx = rng.integers(0, m, (B, n, 3)).astype(np.int32)
    dist = (rng.random((B, n, 3)) * 1e-2).astype(np.float32)
    dist[:, ::5] = 0
    return idx, dist


def _plain_interp(rows, idx, dist):
    d = np.maximum(dist.astype(np.float64), np.float64(np.float32(1e-10)))
    w = (1 / d) / (1 / d).sum(-1, keepdims=True)
    out = np.zeros(idx.shape[:2] + (rows.shape[-1],))
    for b in range(idx.shape[0]):
        for t in range(3):
            out[b] += w[b, :, t, None] * rows[b, idx[b, :, t]].astype(np.float64)
    return out


def _act(v, act):
    return {0: lambda a: a, 1: lambda a: np.maximum(a, 0), 2: lambda a: 1 / (1 + np.exp(-a))}[act](v)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("mask", range(8))
def test_linear_is_bias_scale_shift_act_then_residual(act, mask):
    rng = np.random.default_rng(10 * mask + act)
    x1, x2 = rng.standard_normal((9, 8)).astype(np.float32), rng.standard_normal((9, 4)).astype(np.float32)
    W, res = rng.standard_normal((12, 6)).astype(np.float32), rng.standard_normal((9, 6)).astype(np.float32)
    ep = _ep(rng, 6, act, mask)
    r = D.linear(x1, W, x2=x2, ep=ep, residual=res)
    v = np.concatenate([x1, x2], 1).astype(np.float64) @ W
    if ep[0] is not None: v = v + ep[0]
    if ep[1] is not None: v = v * ep[1]
    if ep[2] is not None: v = v + ep[2]
    assert np.allclose(r[0], _act(v, act) + res, rtol=1e-13, atol=1e-13)
    assert len(r) == (3 if act == 2 else 2) and np.all(r[1] >= 0)
    if act == 2:
        assert np.array_equal(r[2], np.ones_like(r[0]))


def test_value_and_T_functions_agree_with_plain_numpy():
    rng = np.random.default_rng(5)
    B, n, m, C = 2, 11, 5, 8
    idx, dist = _geom(rng, B, n, m)
    pts = rng.standard_normal((B, m, C)).astype(np.float32)
    up = _plain_interp(pts, idx, dist)
    v, T = D.three_interpolate_idw(pts, idx, dist)
    assert np.allclose(v, up, rtol=1e-13, atol=1e-14) and np.all(T >= np.abs(v) - 1e-12)
    x2, x3 = rng.standard_normal((B, n, 4)).astype(np.float32), rng.standard_normal((B, n, 4)).astype(np.float32)
    W, Wsc = rng.standard_normal((C + 4, 6)).astype(np.float32), rng.standard_normal((4, 6)).astype(np.float32)
    res, pre = rng.standard_normal((B, n, 6)).astype(np.float32), rng.standard_normal((B, n, 3)).astype(np.float32)
    ep, ep2 = _ep(rng, 6, 1), _ep(rng, 6, 1)
    main = np.maximum((np.concatenate([up, x2], -1) @ W.astype(np.float64) + ep[0]) * ep[1] + ep[2], 0)
    v, _ = D.upsample_linear(pts, idx, dist, W, x2=x2, ep=ep, residual=res)
    assert np.allclose(v, main + res, rtol=1e-13, atol=1e-13)
    sc = np.maximum((x3.astype(np.float64) @ Wsc + ep2[0]) * ep2[1] + ep2[2], 0)
    v, T = D.upsample_linear(pts, idx, dist, W, x2=x2, ep=ep, shortcut=(x3, Wsc, ep2), l2=(pre, 1e-8))
    y = main + sc
    want = np.concatenate([pre, y / np.sqrt(np.maximum((y * y).sum(-1, keepdims=True), 1e-8))], -1)
    assert np.allclose(v, want, rtol=1e-13, atol=1e-13) and np.array_equal(v[..., :3], pre) and not T[..., :3].any()
    # interp_combine and the fused local tail
    cw, part = rng.standard_normal((B, m, 6)).astype(np.float32), rng.standard_normal((B, n, 6)).astype(np.float32)
    y = np.maximum((_plain_interp(cw, idx, dist) + part + ep[0]) * ep[1] + ep[2], 0) + res
    v, _ = D.interp_combine(cw, idx, dist, partial=part, ep=ep, residual=res)
    assert np.allclose(v, y, rtol=1e-13, atol=1e-13)
    Wl = rng.standard_normal((4, 6)).astype(np.float32)
    y = np.maximum((_plain_interp(cw, idx, dist) + x2.astype(np.float64) @ Wl + ep[0]) * ep[1] + ep[2], 0) + sc
    v, _ = D.local_tail_fused(x3, x2, Wsc, Wl, ep2[:3], ep[:3], cw, idx, dist, None, 0.0)
    assert np.allclose(v, y, rtol=1e-13, atol=1e-13)
    v, _ = D.local_tail_fused(x3, x2, Wsc, Wl, ep2[:3], ep[:3], cw, idx, dist, pre, 1e-8)
    assert np.allclose(v[..., 3:], y / np.sqrt(np.maximum((y * y).sum(-1, keepdims=True), 1e-8)), rtol=1e-13, atol=1e-13)


def test_heads_and_slices_agree_with_plain_numpy():
    rng = np.random.default_rng(6)
    B, n, m, C, H = 2, 7, 4, 8, 512
    idx, dist = _geom(rng, B, n, m)
    coarse = rng.standard_normal((B, m, C)).astype(np.float32)
    W = (rng.standard_normal((C, H)) / 3).astype(np.float32)
    wfc = (rng.standard_normal(H) / 20).astype(np.float32)
    ep = _ep(rng, H, 1)
    up = _plain_interp(coarse, idx, dist)
    want = 1 / (1 + np.exp(-(np.maximum((up @ W.astype(np.float64) + ep[0]) * ep[1] + ep[2], 0) @ wfc + 0.2)))
    a, Ta, Sa = D.interp_head(coarse, idx, dist, W, wfc, 0.2, ep)
    assert a.shape == (B, n, 1) and np.allclose(a[..., 0], want, rtol=1e-12, atol=1e-13) and np.all(Sa == 1)
    b, _, _ = D.mlp_head(up.astype(np.float32), W, wfc, 0.2, ep)
    assert np.allclose(a, b, atol=1e-6)
    s, _ = D.linear_slices(coarse.reshape(-1, C), W, 2)
    full = coarse.reshape(-1, C).astype(np.float64) @ W
    assert np.array_equal(s[0], full[:, :256]) and np.array_equal(s[1], full[:, 256:])
    # a sigmoid hidden layer: S counts it through |w_fc| / 4
    _, _, S = D.mlp_head(up.astype(np.float32), W, wfc, 0.0, _ep(rng, H, 2))
    assert np.allclose(S, 1 + np.abs(wfc).sum() / 4)


@pytest.mark.parametrize("C", [64, 128])
def test_se_family_agrees_with_plain_numpy(C):
    rng = np.random.default_rng(C)
    B, N, K = 2, 9, 4
    x = rng.standard_normal((B, N, C)).astype(np.float32)
    nbr = rng.integers(0, N, (B, N, K)).astype(np.int32)
    W1, b1 = (rng.standard_normal((C, C // 4)) / 8).astype(np.float32), rng.standard_normal(C // 4).astype(np.float32)
    W2, b2 = (rng.standard_normal((C // 4, C)) / 4).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    pool = np.stack([x[b][nbr[b]].max(1) for b in range(B)])
    p, _ = D.flex_pool(x, nbr)
    assert np.array_equal(p, pool)
    g = 1 / (1 + np.exp(-(np.maximum(pool.astype(np.float64) @ W1 + b1, 0) @ W2 + b2)))
    want = np.maximum(x + x * g, 0)
    y, Ty, Sy = D.se_res_pool(x, nbr, W1, b1, W2, b2)
    assert np.allclose(y, want, rtol=1e-13, atol=1e-14) and np.array_equal(Sy, np.where(x > 0, np.abs(x), 0))
    Wc, ep = (rng.standard_normal((C, C)) / 8).astype(np.float32), _ep(rng, C, 1)
    (y2, _, _), (z, Tz, Sz) = D.se_res_pool_conv(x, nbr, W1, b1, W2, b2, Wc, ep)
    assert np.array_equal(y2, y)
    assert np.allclose(z, np.maximum((want @ Wc + ep[0]) * ep[1] + ep[2], 0), rtol=1e-12, atol=1e-13)
    assert np.all(Tz >= 0) and np.all(Sz >= 0)


def test_relu_gate_and_l2_clamp_near_their_thresholds():
    # a ReLU input within rounding of 0 keeps its T (either branch is right); one firmly below has T = 0
    x = np.float32([[1.0, -1.0]])
    W = np.float32([[1.0, 1.0], [1.0 + 2.0 ** -23, 0.5]])
    v, T = D.linear(x, W, ep=(None, None, None, D.ACT_RELU))
    assert v[0, 0] == 0 and T[0, 0] > 2 and v[0, 1] == 0.5
    v, T = D.linear(x, np.float32([[1.0], [3.0]]), ep=(None, None, None, D.ACT_RELU))
    assert v[0, 0] == 0 and T[0, 0] == 0
    # l2: an all-zero row stays 0 with T = 0; a row of norm 1e-7 under eps = 1e-12 is scaled by 1e6
    z = np.zeros((3, 4), np.float32)
    z[1] = 5e-8
    v, T = D.l2norm_concat(z, 1e-12, prefix=np.ones((3, 2), np.float32))
    assert not v[0, 2:].any() and not T[0].any() and np.allclose(v[1, 2:], 5e-2) and np.array_equal(v[:, :2], np.ones((3, 2)))
    # that row is firmly below the clamp: the reciprocal root is a constant, T = |x| rinv + |x| rinv with no T(sum x^2) term
    assert np.all(np.isfinite(T[1])) and not T[1, :2].any() and np.allclose(T[1, 2:], 2 * 5e-2, rtol=1e-12)
    # a row above the clamp carries it: T(sum x^2) / (2 sum x^2) = 1 more unit; so does one within GATE_TOL of the clamp
    z[2] = 0.5
    _, T = D.l2norm_concat(z, 1e-12)
    assert np.allclose(T[2], 3 * 0.5, rtol=1e-12)
    e = np.full((1, 4), 0.5, np.float32)
    for eps, units in ((1.0 + 1e-5, 3), (1.0 + 3e-5, 2)):      # sum x^2 = 1, T of it = 2: ambiguous below eps = 1 + 2e-5
        v, T = D.l2norm_concat(e, eps)
        assert np.allclose(T, units * np.abs(v), rtol=1e-4)   # (3 is 2 + 1 / eps)
    # the gate's tolerance is max(GATE_TOL, the relative bound of its input): y = -a T(y) is shut for a = 1.5e-5 behind a
    # short sum ((0 + 16) 2^-24 < GATE_TOL < a), open behind a 512-term sum ((512 + 16) 2^-24 > a), open for a = 0.5e-5
    for a, ktot, live in ((1.5e-5, 0, False), (1.5e-5, 512, True), (0.5e-5, 0, True)):
        y, Ty, _ = D.epilogue(np.float64([-a * 4.0]), np.float64([4.0]), (None, None, None, D.ACT_RELU), ktot)
        assert y[0] == 0 and Ty[0] == (4.0 if live else 0.0), (a, ktot)
