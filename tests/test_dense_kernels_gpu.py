"""GPU: the dense matrix-pipe kernels (csrc/dense.hip, csrc/dense_x6.hip, csrc/dense_tail.hip) against the float64
restatements of tests/dense_reference.py, with inputs built so that the expected value is exact or has an a-priori bound.

(a) exact selection probes (==): one-hot rows give W back, an identity block in W gives x back, and (1 + 2^-9)^2 needs
    the c2 d2 chunk product -- on linear, linear_x6 (general path, Dout 128 / 256, and the C1 = 64 kernel) and
    linear_slices (2 and 4 slices);
(b) single-product probes on the same paths: one nonzero per row, |got - x w| <= 2^-20 |x w| (derived and pinned in
    tests/test_dense_reference.py: with any one chunk product lost the error is more than ten times that);
(c) the option matrix: every subset of {pre_bias, scale, shift}, every activation, every optional operand present and
    absent, |got - ref| <= (Ktot + 16) 2^-24 T (+ A_SIG behind a sigmoid), and the documented refusals;
(d) row counts 1 .. 257 around every tile height into a NaN-filled buffer (rows past R stay NaN bit for bit), tiles that
    span two or three clouds, degenerate idx / dist rows, the l2 clamp;
(e) the squeeze-excite family on kNN lists, on lists with repeated ids, and with a saturated gate;
(f) test_zz_report_worst_ratios prints the worst |got - ref| / bound per kernel.

A_SIG, the absolute allowance of the device sigmoid 1 / (1 + __expf(-v)): test_sigmoid_allowance_is_measured runs it on
pre-activations that are exact (one-hot rows, so the bound before the sigmoid is 0) over v in [-30, 30] and prints the
worst |got - sigmoid64(v)|.  Measured on an MI355X, 2026-10-17: 8.711e-08.  A_SIG = 4 x that, rounded up to one digit
= 4e-7, under the 1e-6 it must not exceed (a missing shift or a wrong column is O(0.1)).

Worst |got - ref| / bound per kernel over (c) (d) (e), from test_zz_report_worst_ratios of that run (with A_SIG = 4e-7):
  interp_combine 0.2250            three_interpolate_idw 0.1980      upsample_linear_shortcut_x6 0.1328
  linear_x6_d128 0.0433            upsample_linear_x6_d256 0.0418    linear_x6_k64 0.0410
  linear 0.0403                    upsample_linear_x6_d128 0.0402    linear_x6_d256 0.0255
  local_tail_fused 0.0236          se_res 0.0144                     se_res_pool_conv/y 0.0129
  se_res_pool_conv/conv_c64 0.0127 se_res_packed_c64 0.0126          se_res_pool_packed_c64 0.0120
  upsample_linear_l2cat_x6 0.0099  upsample_linear_shortcut_x6_l2cat 0.0079
  se_res_packed_c128 0.0061        l2norm_concat 0.0060              se_res_pool_packed_c128 0.0056
  se_res_pool_conv/conv_c128 0.0047  mlp_head_x6 0.0010  mlp_head 0.0008  interp_head_gather 0.0004
  interp_head_lds_staged 0.0002
single_product/*, worst relative error / 2^-20 over (b):
  linear 0.0617   linear_x6_d128 0.3795   linear_x6_d256 0.4450   linear_x6_k64 0.3940   linear_slices_2 0.4012
  linear_slices_4 0.5029 (row 35, k 35, column 434)
Every sum bound is spent to under a quarter.  The single-product figures sit near 0.5 by construction: 2^-20 is 16 x 2^-24
where the analytic worst case is 13 and the numpy emulation of the six products gives 7.3 on the linear_slices_4 probe
itself (0.46); the kernel's 8.05 there is that plus the matrix pipe's own rounding of its partial sums, and one lost
third-order product is 160 or more.

Entry points of the three files this file does not reach: dh3d_pack_flex_weight (flex_conv's operand, with the flex
tests), dh3d_interp_head_sorted_fwd_dev (the trainers' variant of the staged head: tests/test_commuted_walks_gpu.py),
dh3d_walk_plan / dh3d_walk_plan_bytes / dh3d_global_walk_planned_fwd (the planned global walk) and, outside them, every
netvlad_* entry point -- those are tests/test_netvlad_kernels_gpu.py's.  dh3d_pack_weight and dh3d_pack_weight_x3 are reached
through every probe of (a): a wrong fragment order moves a column or a k.
"""
import numpy as np
import pytest
import torch

import dense_reference as D

pytestmark = pytest.mark.gpu

A_SIG = 4e-7             # 4 x the measured 8.711e-08, rounded up to one digit (see above)

NAN = float("nan")
PAD = 8                  # sentinel rows behind every caller-owned output
R_EDGES = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257]
ACTS = (D.ACT_NONE, D.ACT_RELU, D.ACT_SIGMOID)

_WORST = {}


# ------------------------------------------------------------------------------------------------------------ helpers
def _L():
    from dh3d_amd import _lib as L
    return L


def _pm():
    from dh3d_amd import pm
    return pm


def _raw(name, *args):
    L = _L()
    L.check(getattr(L.lib(), name)(*[L.ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args]
                                   + [L.stream_ptr()]), name)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _nanbuf(rows, width, dev):
    return torch.full((rows + PAD, width), NAN, dtype=torch.float32, device=dev)


def _take(buf, rows):
    """The first `rows` rows of a sentinel buffer; the rows behind them must still hold the fill, bit for bit."""
    fill = torch.full((1,), NAN, dtype=torch.float32).view(torch.int32).item()
    tail = buf[rows:].view(torch.int32)
    assert bool((tail == fill).all()), "rows past R were written: %s" % (
        torch.nonzero(tail != fill)[:4].tolist(),)
    return _np(buf[:rows])


def _check(kernel, case, got, ref, ktot):
    """|got - ref| <= (Ktot + 16) 2^-24 T (+ A_SIG S); records the worst ratio of `kernel`."""
    v, T = ref[0], ref[1]
    S = ref[2] if len(ref) == 3 else None
    got = np.asarray(got, np.float64).reshape(v.shape)
    assert np.isfinite(got).all(), "%s %s: non-finite output" % (kernel, case)
    b = D.bound(T, ktot, S, A_SIG)
    err = np.abs(got - v)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / b)
    w = float(ratio.max())
    if w > _WORST.get(kernel, (0.0, ""))[0]:
        _WORST[kernel] = (w, case)
    _WORST.setdefault(kernel, (0.0, case))
    if not w <= 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError("%s %s: element %s got %.9g ref %.9g |diff| %.3g bound %.3g (ratio %.3g)"
                             % (kernel, case, i, got[i], v[i], err[i], b[i], w))


def _full_mantissa(rng, shape):
    """mixed sign, magnitude 2^-6 .. 2^6, all 24 significand bits in use (the lowest one set)."""
    mant = rng.integers(0, 1 << 22, shape).astype(np.uint32) << np.uint32(1) | np.uint32(1)
    expo = rng.integers(127 - 6, 127 + 6, shape).astype(np.uint32) << np.uint32(23)
    sign = rng.integers(0, 2, shape).astype(np.uint32) << np.uint32(31)
    return (sign | expo | mant).view(np.float32)


def _wide(rng, shape):
    return (rng.standard_normal(shape) * np.exp(rng.uniform(-8, 8, shape))).astype(np.float32)


def _gauss(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def _weight(rng, K, Dout, spread):
    W = rng.standard_normal((K, Dout)) / np.sqrt(K)
    if spread:
        W = W * 2.0 ** rng.uniform(-10, 10, Dout)
    return W.astype(np.float32)


def _mkep(rng, n, mask, act, spread=False):
    """(pre_bias, scale, shift, act) as numpy: bit 0 / 1 / 2 of mask = pre_bias / scale / shift present."""
    sp = (lambda: 2.0 ** rng.uniform(-10, 10, n)) if spread else (lambda: 1.0)
    pb = (rng.standard_normal(n) * sp()).astype(np.float32) if mask & 1 else None
    sc = ((0.5 + rng.random(n)) * rng.choice([-1.0, 1.0], n) * sp()).astype(np.float32) if mask & 2 else None
    sh = (rng.standard_normal(n) * sp()).astype(np.float32) if mask & 4 else None
    return (pb, sc, sh, act)


def _dev_ep(ep, dev):
    return tuple(_t(v, dev) for v in ep[:3]) + (ep[3],)


def _epkw(ep, dev):
    d = _dev_ep(ep, dev)
    return dict(pre_bias=d[0], scale=d[1], shift=d[2], act=d[3])


def _raw_ep(ep, dev, keep):
    d = _dev_ep(ep, dev)
    keep.extend(d[:3])
    return _L().make_epilogue(*d)


def _geom(rng, B, n, m, edges=True):
    """idx / dist [B, n, 3] with the degenerate rows of (d): equal ids, ids m - 1, distances 0 0 0, one zero and two large."""
    idx = rng.integers(0, m, (B, n, 3)).astype(np.int32)
    dist = (rng.random((B, n, 3)) * 1e-2).astype(np.float32)
    if edges:
        idx[:, 0::7, 1:] = idx[:, 0::7, :1]
        idx[:, 1::7, :] = m - 1
        dist[:, 2::7, :] = 0.0
        dist[:, 3::7, :] = np.float32([0.0, 5.0, 9.0])
        dist[:, 4::7, 1] = 0.0
    return idx, dist


def _coarse(rng, B, m, C):
    """coarse rows; cloud b sits around the constant b + 1, so a gather that crosses clouds is O(1) wrong."""
    return (0.25 * rng.standard_normal((B, m, C)) + (np.arange(B)[:, None, None] + 1.0)).astype(np.float32)


def _walk_records(rng, B, n):
    """[B, n, 4] records (x, y, z, bits(original index)) of a random walk order, as spatial_sort writes them."""
    rec = rng.random((B, n, 4), dtype=np.float32)
    rec[..., 3] = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int32).view(np.float32)
    return rec


def _unsupported(fn):
    with pytest.raises(ValueError, match="unsupported shape"):
        fn()


# ------------------------------------------------------------------------------------- (a) (b): the four GEMM paths
PATHS = {
    "linear": ("linear", 64, 32, 128),
    "linear_x6_d128": ("x6", 64, 32, 128),
    "linear_x6_d256": ("x6", 128, 64, 256),
    "linear_x6_k64": ("x6", 64, 0, 128),
    "linear_slices_2": ("slices", 64, 0, 512),
    "linear_slices_4": ("slices", 96, 0, 1024),
}


def _run_path(path, x, W, dev):
    """x [R, K], W [K, Dout] numpy f32 -> out [R, Dout] numpy f32, no epilogue, no residual."""
    pm = _pm()
    kind, C1, C2, Dout = PATHS[path]
    xt, Wt = _t(x, dev), _t(W, dev)
    x1 = xt[:, :C1].contiguous()
    x2 = xt[:, C1:].contiguous() if C2 else None
    if kind == "linear":
        return _np(pm.linear(x1, pm.pack_weight(Wt), Dout, x2=x2))
    if kind == "x6":
        return _np(pm.linear_x6(x1, pm.pack_weight_x3(Wt), Dout, x2=x2))
    ns, R = Dout // 256, x.shape[0]
    wp = torch.cat([pm.pack_weight_x3(Wt[:, j:j + 256].contiguous()) for j in range(0, Dout, 256)])
    out = torch.full((ns * R + PAD, 256), NAN, dtype=torch.float32, device=dev)
    _raw("dh3d_linear_slices_pm_x6_fwd", x1, C1, wp, R, ns, out)
    return _take(out, ns * R).reshape(ns, R, 256).transpose(1, 0, 2).reshape(R, Dout)


def _first_diff(got, want):
    r, c = np.argwhere(got != want)[0]
    return "row %d column %d: got %.9g want %.9g" % (r, c, got[r, c], want[r, c])


@pytest.mark.parametrize("path", list(PATHS))
def test_exact_selection_probes(dev, path):
    _, C1, C2, Dout = PATHS[path]
    K = C1 + C2
    rng = np.random.default_rng(K + Dout)
    # one-hot rows: row r selects W[r, :]; every k in one launch
    W = _full_mantissa(rng, (K, Dout))
    got = _run_path(path, np.eye(K, dtype=np.float32), W, dev)
    assert np.array_equal(got, W), "one-hot x (row = k): " + _first_diff(got, W)
    # the mirror: an identity block in W at column offset off selects x[:, k] into column (k + off) % Dout
    x = _full_mantissa(rng, (130, K))
    for off in sorted(set(list(range(0, Dout, K)) + [Dout - K])):
        Wi = np.zeros((K, Dout), np.float32)
        Wi[np.arange(K), (np.arange(K) + off) % Dout] = 1.0
        want = np.zeros((130, Dout), np.float32)
        want[:, (np.arange(K) + off) % Dout] = x
        got = _run_path(path, x, Wi, dev)
        assert np.array_equal(got, want), "identity block at column offset %d: %s" % (off, _first_diff(got, want))
    # second order: (1 + 2^-9)^2 = 1 + 2^-8 + 2^-18 exactly, and only with c2 d2
    v = np.float32(1 + 2.0 ** -9)
    got = _run_path(path, np.eye(K, dtype=np.float32) * v, np.full((K, Dout), v, np.float32), dev)
    want = np.full((K, Dout), np.float32(1 + 2.0 ** -8 + 2.0 ** -18), np.float32)
    assert np.array_equal(got, want), "second-order probe (row = k): " + _first_diff(got, want)


@pytest.mark.parametrize("path", list(PATHS))
def test_single_product_probes(dev, path):
    _, C1, C2, Dout = PATHS[path]
    K = C1 + C2
    rng = np.random.default_rng(7 * K + Dout)
    R = 2 * K + 1
    x = np.zeros((R, K), np.float32)
    x[np.arange(R), np.arange(R) % K] = _wide(rng, R)
    W = _wide(rng, (K, Dout))
    exact = x[np.arange(R), np.arange(R) % K].astype(np.float64)[:, None] * W[np.arange(R) % K].astype(np.float64)
    assert np.abs(exact).min() >= 2.0 ** -100           # the draw leaves nothing to exclude
    got = _run_path(path, x, W, dev).astype(np.float64)
    rel = np.abs(got - exact) / np.abs(exact)
    r, c = np.unravel_index(int(np.argmax(rel)), rel.shape)
    key = "single_product/" + path
    _WORST[key] = (float(rel.max() / D.SINGLE_PRODUCT_BOUND), "row %d k %d column %d" % (r, r % K, c))
    assert rel.max() <= D.SINGLE_PRODUCT_BOUND, "row %d (k = %d) column %d: got %.9g exact %.9g, %.1f x 2^-24" % (
        r, r % K, c, got[r, c], exact[r, c], rel.max() / 2.0 ** -24)


def test_sigmoid_allowance_is_measured(dev):
    """The device sigmoid on exact pre-activations (one-hot rows: the bound before the sigmoid is 0) over [-30, 30]."""
    pm = _pm()
    K, Dout = 64, 128
    v = np.linspace(-30, 30, K * Dout).astype(np.float32)
    rng = np.random.default_rng(0)
    rng.shuffle(v)
    W = v.reshape(K, Dout)
    eye = _t(np.eye(K, dtype=np.float32), dev)
    want = D.sigmoid(W)
    a = _np(pm.linear(eye, pm.pack_weight(_t(W, dev)), Dout, act=pm.ACT_SIGMOID))
    b = _np(pm.linear_x6(eye, pm.pack_weight_x3(_t(W, dev)), Dout, act=pm.ACT_SIGMOID))
    sel = np.zeros(Dout, np.float32)
    sel[5] = 1.0                                         # logit = W[k, 5] exactly
    c = _np(pm.mlp_head(eye, pm.pack_weight(_t(W, dev)), Dout, _t(sel, dev), 0.0, act=pm.ACT_NONE))[:, 0]
    worst = max(np.abs(a - want).max(), np.abs(b - want).max(), np.abs(c - want[:, 5]).max())
    print("\nsigmoid: worst |got - sigmoid64(v)| over exact v in [-30, 30] = %.3e  (A_SIG = %.1e)" % (worst, A_SIG))
    assert A_SIG <= 1e-6
    assert worst <= A_SIG


# ------------------------------------------------------------------------------------- case builders for (c) (d) (e)
# Every builder makes its inputs, the float64 reference and one launch: through the pm wrapper, or -- sentinel=True -- on
# the C entry point with a caller-owned NaN-filled output.  Returns (got, ref, Ktot).
def _b_linear(dev, rng, R, o, sentinel, x6=False, shape=(64, 32, 128)):
    pm = _pm()
    C1, C2, Dout = shape
    if not o.get("x2", True):
        C1, C2 = C1 + C2, 0
    x1, x2 = _gauss(rng, R, C1), (_gauss(rng, R, C2) if C2 else None)
    W = _weight(rng, C1 + C2, Dout, o.get("spread"))
    ep = _mkep(rng, Dout, o["mask"], o["act"], o.get("spread"))
    res = _gauss(rng, R, Dout) if o.get("res") else None
    ref = D.linear(x1, W, x2=x2, ep=ep, residual=res)
    Wt = _t(W, dev)
    wp = pm.pack_weight_x3(Wt) if x6 else pm.pack_weight(Wt)
    if not sentinel:
        fn = pm.linear_x6 if x6 else pm.linear
        got = _np(fn(_t(x1, dev), wp, Dout, x2=_t(x2, dev), residual=_t(res, dev), **_epkw(ep, dev)))
    else:
        keep = []
        buf = _nanbuf(R, Dout, dev)
        _raw("dh3d_linear_pm_x6_fwd" if x6 else "dh3d_linear_pm_fwd", _t(x1, dev), C1, _t(x2, dev), C2, wp, R, Dout,
             _raw_ep(ep, dev, keep), _t(res, dev), buf)
        got = _take(buf, R)
    return got, ref, C1 + C2


def _b_upsample(dev, rng, geo, o, sentinel, Dout=128):
    """upsample_linear_x6 (plain / l2cat) and, with o['shortcut'], upsample_linear_shortcut_x6."""
    pm = _pm()
    B, n, m = geo
    C1, C2, C3 = 64, 32, 32
    idx, dist = _geom(rng, B, n, m)
    pts = _coarse(rng, B, m, C1)
    sc = o.get("shortcut")
    x2 = _gauss(rng, B, n, C2) if (o.get("x2", True) or sc) else None
    K = C1 + (C2 if x2 is not None else 0)
    W = _weight(rng, K, Dout, o.get("spread"))
    ep = _mkep(rng, Dout, o["mask"], o["act"], o.get("spread"))
    res = _gauss(rng, B, n, Dout) if (o.get("res") and not sc) else None
    l2 = (_gauss(rng, B, n, 3), 1e-12) if o.get("l2") else None
    short = None
    if sc:
        x3, Wsc = _gauss(rng, B, n, C3), _weight(rng, C3, Dout, o.get("spread"))
        ep2 = _mkep(rng, Dout, o.get("mask2", 7), o.get("act2", D.ACT_RELU), o.get("spread"))
        short = (x3, Wsc, ep2)
    if o.get("zero_row") and n > 2:                     # an all-zero output row (eps rule) and one of norm ~1e-7
        assert l2 is not None and o["mask"] == 0 and not sc and res is None
        pts[:] = np.abs(pts)
        x2[:, 0] = 0.0
        idx[:, 0] = 0
        pts[:, 0] = 0.0                                  # point 0 of every cloud: interp and x2 are 0 -> y = 0
        x2[:, 1] = 0.0
        idx[:, 1] = 1
        pts[:, 1] = 1e-8                                 # point 1: y = 1e-8 * column sums of W: norm ~1e-7
    ref = D.upsample_linear(pts, idx, dist, W, x2=x2, ep=ep, residual=res, l2=l2, shortcut=short)
    ktot = K + 3 + (C3 if sc else 0) + (Dout if l2 else 0)
    a = [_t(v, dev) for v in (pts, idx, dist)]
    width = Dout + (3 if l2 else 0)
    buf = _nanbuf(B * n, width, dev) if sentinel else None
    keep = []
    if sc:
        wp = pm.pack_weight_x3(_t(np.concatenate([W, short[1]], 0), dev))
        if not sentinel:
            got = _np(pm.upsample_linear_shortcut_x6(*a, wp, Dout, _t(x2, dev), _t(short[0], dev), _dev_ep(ep, dev),
                                                     _dev_ep(short[2], dev), l2cat=(_t(l2[0], dev), l2[1]) if l2 else None))
        else:
            _raw("dh3d_upsample_linear_shortcut_pm_x6_fwd", *a, B, n, m, C1, _t(x2, dev), C2, _t(short[0], dev), C3, wp,
                 Dout, _raw_ep(ep, dev, keep), _raw_ep(short[2], dev, keep), _t(l2[0], dev) if l2 else None,
                 l2[1] if l2 else 0.0, buf)
    else:
        wp = pm.pack_weight_x3(_t(W, dev))
        C2e = C2 if x2 is not None else 0
        if not sentinel:
            got = _np(pm.upsample_linear_x6(*a, wp, Dout, x2=_t(x2, dev), residual=_t(res, dev),
                                            l2cat=(_t(l2[0], dev), l2[1]) if l2 else None, **_epkw(ep, dev)))
        elif l2:
            _raw("dh3d_upsample_linear_l2cat_pm_x6_fwd", *a, B, n, m, C1, _t(x2, dev), C2e, wp, Dout,
                 _raw_ep(ep, dev, keep), _t(res, dev), _t(l2[0], dev), l2[1], buf)
        else:
            _raw("dh3d_upsample_linear_pm_x6_fwd", *a, B, n, m, C1, _t(x2, dev), C2e, wp, Dout, _raw_ep(ep, dev, keep),
                 _t(res, dev), buf)
    if sentinel:
        got = _take(buf, B * n)
    if l2:
        g = np.asarray(got).reshape(B, n, width)
        assert np.array_equal(g[..., :3], l2[0]), "prefix columns are not copies of the input"
    return got, ref, ktot


def _b_interp_combine(dev, rng, geo, o, sentinel):
    pm = _pm()
    B, n, m = geo
    C = 128
    idx, dist = _geom(rng, B, n, m)
    cw = _coarse(rng, B, m, C)
    if o.get("spread"):
        cw = (cw * 2.0 ** rng.uniform(-10, 10, C)).astype(np.float32)
    part = _gauss(rng, B, n, C) if o.get("partial") else None
    res = _gauss(rng, B, n, C) if o.get("res") else None
    l2 = (_gauss(rng, B, n, 3), 1e-12) if o.get("l2") else None
    ep = _mkep(rng, C, o["mask"], o["act"], o.get("spread"))
    if o.get("zero_row") and n > 2:
        assert l2 is not None and o["mask"] == 0 and res is None and part is None
        idx[:, 0], idx[:, 1] = 0, 1
        cw[:, 0], cw[:, 1] = 0.0, 1e-7 / np.sqrt(C)
    ref = D.interp_combine(cw, idx, dist, partial=part, ep=ep, residual=res, l2=l2)
    a = [_t(v, dev) for v in (cw, idx, dist)]
    width = C + (3 if l2 else 0)
    if not sentinel:
        got = _np(pm.interp_combine(*a, partial=_t(part, dev), residual=_t(res, dev),
                                    l2cat=(_t(l2[0], dev), l2[1]) if l2 else None, **_epkw(ep, dev)))
    else:
        keep = []
        buf = _nanbuf(B * n, width, dev)
        _raw("dh3d_interp_combine_fwd", *a, _t(part, dev), B, n, m, C, _raw_ep(ep, dev, keep), _t(res, dev),
             _t(l2[0], dev) if l2 else None, l2[1] if l2 else 0.0, buf)
        got = _take(buf, B * n)
    if l2:
        assert np.array_equal(np.asarray(got).reshape(B, n, width)[..., :3], l2[0])
    return got, ref, 3 + 1 + (C if l2 else 0)


def _b_local_tail(dev, rng, geo, o, sentinel):
    pm = _pm()
    B, n, m = geo
    idx, dist = _geom(rng, B, n, m)
    cw = _coarse(rng, B, m, 128)
    x1, x2 = _gauss(rng, B, n, 64), _gauss(rng, B, n, 64)
    Ws, Wl = _weight(rng, 64, 128, o.get("spread")), _weight(rng, 64, 128, o.get("spread"))
    e1 = _mkep(rng, 128, o.get("mask2", 7), D.ACT_RELU, o.get("spread"))
    e2 = _mkep(rng, 128, o["mask"], D.ACT_RELU, o.get("spread"))
    pre = _gauss(rng, B, n, 3) if o.get("prefix", True) else None
    ref = D.local_tail_fused(x1, x2, Ws, Wl, e1[:3], e2[:3], cw, idx, dist, pre, 1e-12)
    a = [_t(x1, dev), _t(x2, dev), pm.pack_weight_x3(_t(Ws, dev)), pm.pack_weight_x3(_t(Wl, dev))]
    g = [_t(cw, dev), _t(idx, dev), _t(dist, dev), _t(pre, dev)]
    width = 131 if pre is not None else 128
    if not sentinel:
        got = _np(pm.local_tail_fused(*a, _dev_ep(e1, dev)[:3], _dev_ep(e2, dev)[:3], *g, 1e-12))
    else:
        keep = []
        buf = _nanbuf(B * n, width, dev)
        _raw("dh3d_local_tail_fused_fwd", *a, _raw_ep(e1, dev, keep), _raw_ep(e2, dev, keep), *g, 1e-12, B, n, m, buf)
        got = _take(buf, B * n)
    if pre is not None:
        assert np.array_equal(np.asarray(got).reshape(B, n, width)[..., :3], pre)
    return got, ref, 64 + 3 + 64 + (128 if pre is not None else 0)


def _b_mlp_head(dev, rng, R, o, sentinel, x6=False):
    pm = _pm()
    C, H = 64, 256
    h = _gauss(rng, R, C)
    W = _weight(rng, C, H, o.get("spread"))
    ep = _mkep(rng, H, o["mask"], o["act"], o.get("spread"))
    wfc = (rng.standard_normal(H) / np.sqrt(H)).astype(np.float32)
    ref = D.mlp_head(h, W, wfc, 0.125, ep)
    wp = pm.pack_weight_x3(_t(W, dev)) if x6 else pm.pack_weight(_t(W, dev))
    if not sentinel:
        got = _np((pm.mlp_head_x6 if x6 else pm.mlp_head)(_t(h, dev), wp, H, _t(wfc, dev), 0.125, **_epkw(ep, dev)))
    else:
        keep = []
        buf = _nanbuf(R, 1, dev)
        _raw("dh3d_mlp_head_pm_x6_fwd" if x6 else "dh3d_mlp_head_pm_fwd", _t(h, dev), R, C, wp, H, _raw_ep(ep, dev, keep),
             _t(wfc, dev), 0.125, buf)
        got = _take(buf, R)
    return got, ref, C + H


def _b_interp_head(dev, rng, geo, o, sentinel, staged=False, Hd=512):
    pm = _pm()
    B, n, m = geo
    C = 64
    idx, dist = _geom(rng, B, n, m)
    coarse = _coarse(rng, B, m, C)
    W = _weight(rng, C, Hd, o.get("spread"))
    ep = _mkep(rng, Hd, o["mask"], o["act"], o.get("spread"))
    wfc = (rng.standard_normal(Hd) / np.sqrt(Hd)).astype(np.float32)
    ref = D.interp_head(coarse, idx, dist, W, wfc, 0.2, ep)
    Wt = _t(W, dev)
    wp = torch.cat([pm.pack_weight_x3(Wt[:, j:j + 256].contiguous()) for j in range(0, Hd, 256)])
    order = _t(_walk_records(rng, B, n), dev) if staged else None
    a = [_t(idx, dev), _t(dist, dev)]
    if not sentinel:
        got = _np(pm.interp_head(_t(coarse, dev), *a, wp, Hd, _t(wfc, dev), 0.2, order=order, **_epkw(ep, dev)))
    else:
        keep = []
        H = torch.empty((Hd // 256, B * m, 256), dtype=torch.float32, device=dev)
        _raw("dh3d_linear_slices_pm_x6_fwd", _t(coarse, dev), C, wp, B * m, Hd // 256, H)
        buf = _nanbuf(B * n, 1, dev)
        if staged:
            _raw("dh3d_interp_head_sorted_fwd", H, Hd, *a, order, B, n, m, _raw_ep(ep, dev, keep), _t(wfc, dev), 0.2, buf)
        else:
            _raw("dh3d_interp_head_fwd", H, Hd, *a, B, n, m, _raw_ep(ep, dev, keep), _t(wfc, dev), 0.2, buf)
        got = _take(buf, B * n)
    return got, ref, C + 3 + Hd


def _se_weights(rng, C, saturated=False):
    W1, b1 = (rng.standard_normal((C, C // 4)) / 8).astype(np.float32), _gauss(rng, C // 4)
    W2, b2 = (rng.standard_normal((C // 4, C)) / 4).astype(np.float32), _gauss(rng, C)
    if saturated:                                         # gate pre-activations at +-30
        W2 = (W2 / 64).astype(np.float32)
        b2 = np.where(np.arange(C) % 2 == 0, 30.0, -30.0).astype(np.float32)
    return W1, b1, W2, b2


def _se_lists(rng, B, N, K, kind, dev):
    if kind == "knn":
        return _np(_pm().knn_xyz(_t(rng.random((B, N, 3), dtype=np.float32), dev), K)[0])
    nbr = rng.integers(0, N, (B, N, K)).astype(np.int32)   # repeated ids; the centre is not the point itself
    nbr[:, :, 1] = nbr[:, :, 0]
    nbr[:, ::3, :] = nbr[:, ::3, :1]
    return nbr


def _b_se(dev, rng, geo, o, sentinel, which="pool", C=64):
    """which: 'plain' (se_res), 'packed' (se_res_packed), 'pool' (se_res_pool_packed), 'conv' (se_res_pool_conv)."""
    pm = _pm()
    B, N = geo
    K = o.get("K", 8)
    x = _gauss(rng, B, N, C)
    W1, b1, W2, b2 = _se_weights(rng, C, o.get("saturated"))
    packed = list(pm.se_res_pack(_t(W1, dev), _t(b1, dev), _t(W2, dev))) + [_t(b2, dev)]
    k_se = C + C // 4
    if which in ("plain", "packed"):
        pool = _gauss(rng, B, N, C)
        ref = D.se_res(x, pool, W1, b1, W2, b2)
        if which == "plain":
            got = _np(pm.se_res(_t(x, dev), _t(pool, dev), _t(W1, dev), _t(b1, dev), _t(W2, dev), _t(b2, dev)))
        elif not sentinel:
            got = _np(pm.se_res_packed(_t(x, dev), _t(pool, dev), *packed))
        else:
            buf = _nanbuf(B * N, C, dev)
            _raw("dh3d_se_res_pm_packed_fwd", _t(x, dev), _t(pool, dev), *packed, B * N, C, buf)
            got = _take(buf, B * N)
        return got, ref, k_se
    nbr = _se_lists(rng, B, N, K, o.get("lists", "random"), dev)
    if which == "pool":
        ref = D.se_res_pool(x, nbr, W1, b1, W2, b2)
        if not sentinel:
            got = _np(pm.se_res_pool_packed(_t(x, dev), _t(nbr, dev), *packed))
        else:
            buf = _nanbuf(B * N, C, dev)
            _raw("dh3d_se_res_pool_pm_packed_fwd", _t(x, dev), _t(nbr, dev), B, N, K, *packed, C, buf)
            got = _take(buf, B * N)
        return got, ref, k_se
    Wc = _weight(rng, C, C, o.get("spread"))
    ep = _mkep(rng, C, o["mask"], o["act"], o.get("spread"))
    ref_y, ref_z = D.se_res_pool_conv(x, nbr, W1, b1, W2, b2, Wc, ep)
    wc = pm.pack_weight(_t(Wc, dev))
    if not sentinel:
        d = _dev_ep(ep, dev)
        y, z = pm.se_res_pool_conv(_t(x, dev), _t(nbr, dev), *packed, wc, d[0], d[1], d[2], act=d[3])
        y, z = _np(y), _np(z)
    else:
        keep = []
        by, bz = _nanbuf(B * N, C, dev), _nanbuf(B * N, C, dev)
        _raw("dh3d_se_res_pool_conv_pm_fwd", _t(x, dev), _t(nbr, dev), B, N, K, *packed, C, by, wc,
             _raw_ep(ep, dev, keep), C, bz)
        y, z = _take(by, B * N), _take(bz, B * N)
    return (y, z), (ref_y, ref_z), (k_se, k_se + C)


def _b_l2norm(dev, rng, R, o, sentinel):
    pm = _pm()
    C, P = 128, (3 if o.get("prefix", True) else 0)
    x = _gauss(rng, R, C)
    x[0] = 0.0                                            # the eps rule
    if R > 1:
        x[1] *= np.float32(1e-7) / np.linalg.norm(x[1])   # a row of norm 1e-7, below sqrt(eps)
    pre = _gauss(rng, R, P) if P else None
    ref = D.l2norm_concat(x, 1e-12, prefix=pre)
    if not sentinel:
        got = _np(pm.l2norm_concat(_t(x, dev), 1e-12, prefix=_t(pre, dev)))
    else:
        buf = _nanbuf(R, P + C, dev)
        _raw("dh3d_l2norm_concat_fwd", _t(x, dev), R, C, 1e-12, _t(pre, dev), P, buf)
        got = _take(buf, R)
    if P:
        assert np.array_equal(np.asarray(got)[:, :P], pre)
    assert not np.asarray(got)[0, P:].any()
    return got, ref, C


def _b_interpolate(dev, rng, geo, o, sentinel):
    B, n, m = geo
    idx, dist = _geom(rng, B, n, m)
    pts = _coarse(rng, B, m, 64)
    got = _np(_pm().three_interpolate_idw(_t(pts, dev), _t(idx, dev), _t(dist, dev)))
    return got, D.three_interpolate_idw(pts, idx, dist), 3


def _seed(name, *ints):
    return np.random.default_rng([sum(map(ord, name))] + [int(i) for i in ints])


# ---------------------------------------------------------------------------------------------- (c) the option matrix
def _matrix(acts=ACTS, **flags):
    """every subset of {pre_bias, scale, shift} x every act x every combination of the boolean flags"""
    names = list(flags)
    for mask in range(8):
        for act in acts:
            for bits in range(1 << len(names)):
                o = dict(mask=mask, act=act)
                o.update({nm: bool(bits >> i & 1) for i, nm in enumerate(names)})
                yield o


def _case_id(o):
    return ",".join("%s=%s" % (k, int(v) if isinstance(v, bool) else v) for k, v in sorted(o.items()))


def _sweep(kernel, builder, dev, geo, options, **kw):
    for i, o in enumerate(options):
        got, ref, ktot = builder(dev, _seed(kernel, i), geo, o, False, **kw)
        _check(kernel, _case_id(o), got, ref, ktot)
    # one case with a per-column magnitude spread of 2^+-10 in W and in the epilogue vectors
    o = dict(options[-1], mask=7, act=D.ACT_RELU, spread=True)
    got, ref, ktot = builder(dev, _seed(kernel, 999), geo, o, False, **kw)
    _check(kernel, "spread," + _case_id(o), got, ref, ktot)


def test_options_linear(dev):
    _sweep("linear", _b_linear, dev, 70, list(_matrix(res=0, x2=0)))


@pytest.mark.parametrize("name,shape", [("linear_x6_d128", (64, 32, 128)), ("linear_x6_d256", (128, 64, 256)),
                                        ("linear_x6_k64", (64, 0, 128))])
def test_options_linear_x6(dev, name, shape):
    flags = dict(res=0) if shape[1] == 0 else dict(res=0, x2=0)
    _sweep(name, _b_linear, dev, 150, list(_matrix(**flags)), x6=True, shape=shape)


@pytest.mark.parametrize("Dout", [128, 256])
def test_options_upsample_linear_x6(dev, Dout):
    _sweep("upsample_linear_x6_d%d" % Dout, _b_upsample, dev, (2, 75, 9), list(_matrix(res=0, x2=0)), Dout=Dout)


def test_options_upsample_linear_l2cat(dev):
    opts = list(_matrix(res=0, x2=0))
    for o in opts:
        o["l2"] = True
    _sweep("upsample_linear_l2cat_x6", _b_upsample, dev, (2, 75, 9), opts)
    # Dout 256 has no l2cat store: refused before any launch
    _unsupported(lambda: _b_upsample(dev, _seed("l2cat256"), (1, 40, 5), dict(mask=0, act=0, l2=True), False, Dout=256))
    _unsupported(lambda: _b_upsample(dev, _seed("sc256"), (1, 40, 5), dict(mask=0, act=0, shortcut=True), False, Dout=256))


@pytest.mark.parametrize("l2", [False, True])
def test_options_upsample_linear_shortcut(dev, l2):
    opts = [dict(o, shortcut=True, l2=l2) for o in _matrix()]
    opts += [dict(mask=7, act=D.ACT_RELU, mask2=o["mask"], act2=o["act"], shortcut=True, l2=l2) for o in _matrix()]
    _sweep("upsample_linear_shortcut_x6" + ("_l2cat" if l2 else ""), _b_upsample, dev, (2, 75, 9), opts)


def test_options_interp_combine(dev):
    opts = list(_matrix(partial=0, res=0)) + [dict(o, l2=True) for o in _matrix(partial=0, res=0)]
    _sweep("interp_combine", _b_interp_combine, dev, (2, 75, 9), opts)
    # C != 128 is refused before any launch, so stand-in operands do
    _unsupported(lambda: _raw("dh3d_interp_combine_fwd", *[torch.zeros(8, device=dev)] * 3, None, 1, 1, 1, 64, None, None,
                              None, 0.0, torch.zeros(64, device=dev)))


def test_options_local_tail_fused(dev):
    opts = [dict(o, prefix=p) for p in (True, False) for o in _matrix(acts=(D.ACT_RELU,))]
    opts += [dict(mask=7, act=D.ACT_RELU, mask2=mk, prefix=True) for mk in range(8)]
    _sweep("local_tail_fused", _b_local_tail, dev, (2, 96, 9), opts)
    L = _L()
    # z stands in for every operand, the int32 idx included: these calls rely on the entry point checking N % 32 and the
    # two activations before it launches anything.  Should that order ever change, give them real operands first.
    z = torch.zeros(32 * 131, device=dev)
    for acts in ((D.ACT_NONE, D.ACT_RELU), (D.ACT_RELU, D.ACT_SIGMOID)):     # a non-ReLU epilogue is refused
        e1, e2 = L.make_epilogue(None, None, None, acts[0]), L.make_epilogue(None, None, None, acts[1])
        _unsupported(lambda: _raw("dh3d_local_tail_fused_fwd", z, z, z, z, e1, e2, z, z, z, z, 1e-12, 1, 32, 4, z))
    _unsupported(lambda: _raw("dh3d_local_tail_fused_fwd", z, z, z, z, None, None, z, z, z, z, 1e-12, 1, 31, 4, z))


@pytest.mark.parametrize("x6", [False, True], ids=["mlp_head", "mlp_head_x6"])
def test_options_mlp_head(dev, x6):
    _sweep("mlp_head_x6" if x6 else "mlp_head", _b_mlp_head, dev, 150, list(_matrix()), x6=x6)


@pytest.mark.parametrize("staged", [False, True], ids=["gather", "lds_staged"])
def test_options_interp_head(dev, staged):
    acts = (D.ACT_NONE, D.ACT_RELU) if staged else ACTS
    _sweep("interp_head_" + ("lds_staged" if staged else "gather"), _b_interp_head, dev, (2, 150, 20),
           list(_matrix(acts=acts)), staged=staged)
    if staged:                                            # the staged kernel holds ReLU as a clamp: no sigmoid epilogue
        _unsupported(lambda: _b_interp_head(dev, _seed("ihs"), (1, 40, 5), dict(mask=7, act=D.ACT_SIGMOID), False, staged=True))


@pytest.mark.parametrize("C", [64, 128])
def test_options_se_res_pool_conv(dev, C):
    def builder(dev, rng, geo, o, sentinel):
        (y, z), (ry, rz), (ky, kz) = _b_se(dev, rng, geo, o, sentinel, which="conv", C=C)
        _check("se_res_pool_conv/y", _case_id(o), y, ry, ky)
        return z, rz, kz
    _sweep("se_res_pool_conv/conv_c%d" % C, builder, dev, (2, 75), list(_matrix(acts=(D.ACT_NONE, D.ACT_RELU))))
    _unsupported(lambda: _b_se(dev, _seed("sesig"), (1, 40), dict(mask=0, act=D.ACT_SIGMOID), False, which="conv", C=C))


# ----------------------------------------------------------------------------------- (d) row counts and cloud borders
FULL = dict(mask=7, act=D.ACT_RELU, res=True, x2=True, partial=True)
UP_GEOS = [(1, R, 125) for R in R_EDGES] + [(3, n, m) for n in (1, 100, 129) for m in (3, 125)]

ROW_KERNELS = {
    "linear": lambda dev, rng, R: _b_linear(dev, rng, R, FULL, True),
    "linear_x6_d128": lambda dev, rng, R: _b_linear(dev, rng, R, FULL, True, x6=True),
    "linear_x6_d256": lambda dev, rng, R: _b_linear(dev, rng, R, FULL, True, x6=True, shape=(128, 64, 256)),
    "linear_x6_k64": lambda dev, rng, R: _b_linear(dev, rng, R, FULL, True, x6=True, shape=(64, 0, 128)),
    "mlp_head": lambda dev, rng, R: _b_mlp_head(dev, rng, R, FULL, True),
    "mlp_head_x6": lambda dev, rng, R: _b_mlp_head(dev, rng, R, FULL, True, x6=True),
    "l2norm_concat": lambda dev, rng, R: _b_l2norm(dev, rng, R, {}, True),
    "se_res_packed_c64": lambda dev, rng, R: _b_se(dev, rng, (1, R), {}, True, which="packed", C=64),
    "se_res_packed_c128": lambda dev, rng, R: _b_se(dev, rng, (1, R), {}, True, which="packed", C=128),
    "se_res_pool_packed_c64": lambda dev, rng, R: _b_se(dev, rng, (1, R), {}, True, which="pool", C=64),
    "se_res_pool_packed_c128": lambda dev, rng, R: _b_se(dev, rng, (1, R), {}, True, which="pool", C=128),
}

GEO_KERNELS = {
    "upsample_linear_x6_d128": lambda dev, rng, g: _b_upsample(dev, rng, g, FULL, True),
    "upsample_linear_x6_d256": lambda dev, rng, g: _b_upsample(dev, rng, g, FULL, True, Dout=256),
    "upsample_linear_l2cat_x6": lambda dev, rng, g: _b_upsample(dev, rng, g, dict(FULL, l2=True), True),
    "upsample_linear_l2cat_x6/zero_row": lambda dev, rng, g: _b_upsample(
        dev, rng, g, dict(mask=0, act=D.ACT_RELU, x2=True, l2=True, zero_row=True), True),
    "upsample_linear_shortcut_x6": lambda dev, rng, g: _b_upsample(dev, rng, g, dict(FULL, shortcut=True), True),
    "upsample_linear_shortcut_x6_l2cat": lambda dev, rng, g: _b_upsample(dev, rng, g, dict(FULL, shortcut=True, l2=True), True),
    "interp_combine": lambda dev, rng, g: _b_interp_combine(dev, rng, g, FULL, True),
    "interp_combine/l2cat": lambda dev, rng, g: _b_interp_combine(dev, rng, g, dict(FULL, l2=True), True),
    "interp_combine/zero_row": lambda dev, rng, g: _b_interp_combine(
        dev, rng, g, dict(mask=0, act=D.ACT_RELU, l2=True, zero_row=True), True),
    "interp_head_gather": lambda dev, rng, g: _b_interp_head(dev, rng, g, FULL, True),
    "interp_head_lds_staged": lambda dev, rng, g: _b_interp_head(dev, rng, g, FULL, True, staged=True),
    "three_interpolate_idw": lambda dev, rng, g: _b_interpolate(dev, rng, g, FULL, False),
}


@pytest.mark.parametrize("kernel", list(ROW_KERNELS))
def test_row_counts(dev, kernel):
    for R in R_EDGES:
        got, ref, ktot = ROW_KERNELS[kernel](dev, _seed(kernel, R), R)
        _check(kernel.split("/")[0], "R=%d" % R, got, ref, ktot)


@pytest.mark.parametrize("kernel", list(GEO_KERNELS))
def test_row_counts_and_cloud_borders(dev, kernel):
    for g in UP_GEOS:
        got, ref, ktot = GEO_KERNELS[kernel](dev, _seed(kernel, *g), g)
        _check(kernel.split("/")[0], "B=%d,n=%d,m=%d" % g, got, ref, ktot)


@pytest.mark.parametrize("C", [64, 128])
def test_row_counts_se_res_pool_conv(dev, C):
    for B, N in [(1, R) for R in R_EDGES] + [(3, 1), (3, 100), (3, 129)]:
        o = dict(mask=7, act=D.ACT_RELU)
        (y, z), (ry, rz), (ky, kz) = _b_se(dev, _seed("seconv", C, B, N), (B, N), o, True, which="conv", C=C)
        _check("se_res_pool_conv/y", "B=%d,N=%d" % (B, N), y, ry, ky)
        _check("se_res_pool_conv/conv_c%d" % C, "B=%d,N=%d" % (B, N), z, rz, kz)


def test_row_counts_local_tail_fused(dev):
    """N % 32 == 0 is the entry point's contract: the multiples of 32 among the edges, and three clouds per tile."""
    for g in [(1, 32, 125), (1, 64, 125), (1, 128, 3), (3, 32, 3), (3, 96, 125), (3, 160, 125), (1, 256, 125)]:
        for prefix in (True, False):
            got, ref, ktot = _b_local_tail(dev, _seed("tail", *g), g, dict(mask=7, prefix=prefix), True)
            _check("local_tail_fused", "B=%d,n=%d,m=%d" % g, got, ref, ktot)


# --------------------------------------------------------------------------------------- (e) the squeeze-excite family
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("which", ["plain", "packed", "pool", "conv"])
def test_se_family(dev, which, C):
    name = {"plain": "se_res", "packed": "se_res_packed", "pool": "se_res_pool_packed", "conv": "se_res_pool_conv"}[which]
    cases = [((3, 333), dict(lists="knn")), ((2, 1000), dict(lists="random")), ((3, 100), dict(lists="random", K=5)),
             ((2, 300), dict(lists="knn", saturated=True)), ((70, 300), dict(lists="random"))]   # (the last: 64-row tiles at C 128)
    for i, (geo, o) in enumerate(cases):
        o = dict(o, mask=7, act=D.ACT_RELU)
        got, ref, ktot = _b_se(dev, _seed(name, C, i), geo, o, False, which=which, C=C)
        cid = "C=%d,B=%d,N=%d,%s" % (C, geo[0], geo[1], _case_id(o))
        if which == "conv":
            _check("se_res_pool_conv/y", cid, got[0], ref[0], ktot[0])
            _check("se_res_pool_conv/conv_c%d" % C, cid, got[1], ref[1], ktot[1])
        else:
            _check(name + "_c%d" % C if which in ("packed", "pool") else name, cid, got, ref, ktot)


# ------------------------------------------------------------------------------------------------------- (f) the report
def test_zz_report_worst_ratios():
    print("\nworst |got - ref| / bound per kernel (single_product/*: worst relative error / 2^-20):")
    for k in sorted(_WORST):
        print("  %-40s %.4f   %s" % (k, _WORST[k][0], _WORST[k][1]))
    assert all(v[0] <= 1.0 for v in _WORST.values())
