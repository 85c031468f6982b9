"""GPU: the training GEMMs of csrc/gemm.hip kernel by kernel -- gemm_rows_kernel<1..4>, gemm_shortk_kernel, the four
gemm_f32_kernel and the four gemm_x6_kernel instantiations, transpose32_kernel, colsum_kernel -- at the entry points
dh3d_gemm_tn_f32, dh3d_gemm_nn_f32, their batched forms, dh3d_colsum_f32 and dh3d_transpose32, with inputs built so that the
expected value is exact or a single product (tests/gemm_cases.py; tests/test_gemm_cases.py shows from the reference alone
that the probes are sharp where |got - exp| <= 2e-6 |A||B| + 1e-6 is not).  Every case first asserts, through
dh3d_gemm_plan, that it reaches the kernel and the split state it is filed under.

(a)  exact integer products (==): operands in [-8, 8], every kernel, plain / accumulate onto an integer C0 (added exactly
     once) / integer bias (nn) / the arena path (accumulate onto zeros == the plain result, where dh3d_gemm_is_split) /
     batched with different operands per entry; outputs in NaN-filled buffers whose 8 extra rows keep the fill;
(a') the bf16x6 kernels with all three chunks of one operand in use: 20-bit integers against <= 8 entries of +-1 per
     line, at every residue mod 32 and both sides of every chunk boundary (==);
(b)  second order: (1 + 2^-9)^2 = 1 + 2^-8 + 2^-18 exactly, and only with c2 d2 (==);
(c)  single products of full-mantissa values: |got - a b| <= 2^-20 |a b|;
(d)  dense sums of full-mantissa and wide-magnitude operands at one edge shape per instantiation:
     |got - ref| <= (K + 16) 2^-24 T -- for index errors and O(1) faults on realistic data; (b) (c) guard precision;
(e)  colsum (integers ==, one rounding case) and transpose_last2 (== into a sentinel buffer);
(f)  the documented refusals: status, error, output untouched;
(g)  test_zz_report_worst_ratios prints the worst ratios of (d) and (c).

Measured on an MI355X, 2026-10-21, from test_zz_report_worst_ratios.  Worst |got - ref| / bound per kernel instantiation
over (d):
  shortk 0.1599 (68 x 31 x 132, full mantissa, accumulate)      f32_wide_nn 0.1588 (133 x 52 x 68 + bias, wide)
  f32_wide_tn 0.1565 (260 x 49 x 132, wide, accumulate)         f32_narrow_nn_batched 0.1374 (3 x 130 x 36 x 20 + bias)
  f32_wide_tn_batched 0.0821   rows2 0.0614   rows4 0.0433   x6_wide_nn_batched 0.0255   rows1 0.0170   rows3 0.0122
  f32_narrow_nn 0.0091   x6_wide_nn 0.0071   x6_wide_tn_batched 0.0066   f32_narrow_tn 0.0039   x6_narrow_nn 0.0036
  x6_wide_tn 0.0011   x6_narrow_tn 0.0006   colsum 0.0007 (R 1000, C 100)
Worst relative error / 2^-20 over (c):
  x6_narrow_tn 0.3899   x6_wide_nn_batched 0.3898   x6_wide_tn 0.3870   x6_wide_nn 0.3810   x6_narrow_nn 0.3755
No (d) ratio exceeds 0.5; the largest sit on the short reductions, where the 16 of (K + 16) is most of the bound.  The
single-product figures are 6.0 .. 6.2 x 2^-24, where the numpy emulation of the six products gives up to 7.3 and one lost
third-order product 160 or more (tests/test_dense_kernels_gpu.py has the same figures for the forward kernels)."""
import numpy as np
import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 8                  # sentinel rows behind every output
_WORST = {}


# ------------------------------------------------------------------------------------------------------------ helpers
def _L():
    from dh3d_amd import _lib as L
    return L


def _pm():
    from dh3d_amd import pm
    return pm


def _status(name, *args):
    L = _L()
    return getattr(L.lib(), name)(*[L.ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args]
                                  + [L.stream_ptr()])


def _raw(name, *args):
    _L().check(_status(name, *args), name)


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.detach().cpu().numpy()


def _nanbuf(rows, width, dev):
    return torch.full((rows + PAD, width), NAN, dtype=torch.float32, device=dev)


def _fill_bits():
    return torch.full((1,), NAN, dtype=torch.float32).view(torch.int32).item()


def _take(buf, rows):
    """The first `rows` rows of a sentinel buffer; the rows behind them must still hold the fill, bit for bit."""
    tail = buf[rows:].view(torch.int32)
    assert bool((tail == _fill_bits()).all()), "rows past M were written: %s" % (
        torch.nonzero(tail != _fill_bits())[:4].tolist(),)
    return _np(buf[:rows])


def _untouched(buf):
    return bool((buf.view(torch.int32) == _fill_bits()).all())


def _filed(c):
    """the dispatch of this case, asserted; -> (kernel, chunks, kchunk, stage), is_split"""
    ta = int(c.form == "tn")
    plan = _pm().gemm_plan(ta, c.M, c.N, c.K, c.batch, c.bias)
    split = _L().lib().dh3d_gemm_is_split(ta, c.M, c.N, c.K, c.batch)
    moved = G.filed_ok(c, plan, split)
    assert moved is None, "the dispatch table moved this case: %s -> %s" % (G.case_id(c), moved)
    return plan, bool(split)


def _run(c, dev, X, Y, bias=None, C0=None, zeros=False):
    """One launch of the case's entry point on the logical operands X [batch, M, K], Y [batch, K, N] into a sentinel buffer
    -> [batch, M, N].  C0: accumulate onto it; zeros: accumulate onto a zeroed output (the arena path).  batch == 1 goes
    through pm.gemm_nn / pm.gemm_tn with `out` a view of the buffer, the batched forms through the raw symbols."""
    pm = _pm()
    A, B = G.device_operands(c, X, Y)
    rows = c.batch * c.M
    buf = _nanbuf(rows, c.N, dev)
    acc = C0 is not None or zeros
    if acc:
        buf[:rows] = _t(C0.reshape(rows, c.N), dev) if C0 is not None else 0.0
    if c.batch == 1:
        At, Bt = _t(A[0], dev), _t(B[0], dev)
        if c.form == "nn":
            r = pm.gemm_nn(At, Bt, out=buf[:rows], accumulate=acc, bias=_t(None if bias is None else bias[0], dev))
        else:
            r = pm.gemm_tn(At, Bt, out=buf[:rows], accumulate=acc)
        assert r.data_ptr() == buf.data_ptr()
    else:
        assert not acc                                    # (the batched forms have no accumulate)
        if c.form == "nn":
            _raw("dh3d_gemm_nn_f32_batched", _t(A, dev), _t(B, dev), _t(bias, dev), c.batch, c.M, c.K, c.N, buf)
        else:
            _raw("dh3d_gemm_tn_f32_batched", _t(A, dev), _t(B, dev), c.batch, c.K, c.M, c.N, buf)
    return _take(buf, rows).reshape(c.batch, c.M, c.N)


def _run_own_output(c, dev, X, Y, bias=None):
    """The same product through the pm wrapper alone, which allocates the output at its exact size."""
    pm = _pm()
    A, B = G.device_operands(c, X, Y)
    if c.batch > 1:
        if c.form == "nn":
            return _np(pm.gemm_nn_batched(_t(A, dev), _t(B, dev), bias=_t(bias, dev)))
        return _np(pm.gemm_tn_batched(_t(A, dev), _t(B, dev)))
    if c.form == "nn":
        return _np(pm.gemm_nn(_t(A[0], dev), _t(B[0], dev), bias=_t(None if bias is None else bias[0], dev)))[None]
    return _np(pm.gemm_tn(_t(A[0], dev), _t(B[0], dev)))[None]


def _first_diff(got, want):
    i = tuple(np.argwhere(got != want)[0])
    return "%d of %d elements differ, the first at (batch, row, column) %s: got %.9g want %.9g" % (
        int((got != want).sum()), got.size, i, got[i], want[i])


def _same(c, what, got, want):
    want = np.asarray(want).astype(np.float32)
    assert got.shape == want.shape and np.array_equal(got, want), "%s %s: %s" % (G.case_id(c), what, _first_diff(got, want))


# ------------------------------------------------------------------------------------------- (a) exact integer products
@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_exact_integer_products(dev, family):
    for c in G.FAMILIES[family]:
        plan, is_split = _filed(c)
        X, Y, C0, bias, want = G.integer_operands(c, G.rng_of(c))
        if c.bias:
            wb = want + bias.astype(np.int64)[:, None, :]
            _same(c, "with bias", _run(c, dev, X, Y, bias=bias), wb)
            _same(c, "with bias, own output", _run_own_output(c, dev, X, Y, bias=bias), wb)
            continue
        plain = _run(c, dev, X, Y)
        _same(c, "plain", plain, want)
        _same(c, "plain, own output", _run_own_output(c, dev, X, Y), want)
        if c.batch == 1:
            _same(c, "accumulate", _run(c, dev, X, Y, C0=C0), want + C0.astype(np.int64))
            if is_split:                                   # what pm does with its arena: the partials land on zeros
                _same(c, "accumulate onto zeros", _run(c, dev, X, Y, zeros=True), plain)
        if c.form == "nn":                                 # a bias keeps the kernel and forces one chunk
            with_bias = _pm().gemm_plan(0, c.M, c.N, c.K, c.batch, True)
            assert with_bias[:2] == (plan[0], 1), "the dispatch table moved this case: %s + bias -> %s" % (
                G.case_id(c), with_bias)
            _same(c, "with bias", _run(c, dev, X, Y, bias=bias), want + bias.astype(np.int64)[:, None, :])


# ---------------------------------------------------------------------------- (a') (b) (c) the bf16x6 kernels' products
@pytest.mark.parametrize("c", G.X6_PROBE_CASES, ids=G.case_id)
def test_three_chunk_integers(dev, c):
    plan, _ = _filed(c)
    for dense in ("X", "Y"):
        X, Y, want, covered = G.three_chunk_operands(c, plan[2], G.rng_of(c, 2), dense)
        assert covered
        _same(c, "20-bit integers in %s" % dense, _run(c, dev, X, Y), want)


@pytest.mark.parametrize("c", G.X6_PROBE_CASES, ids=G.case_id)
def test_second_order_probe(dev, c):
    plan, _ = _filed(c)
    for sparse in ("X", "Y"):
        X, Y, covered = G.second_order_operands(c, plan[2], sparse)
        assert covered or (sparse == "Y" and c.N < plan[1])
        _same(c, "one 1 + 2^-9 per line of %s" % sparse, _run(c, dev, X, Y),
              np.full((c.batch, c.M, c.N), G.V9_SQUARED, np.float32))


@pytest.mark.parametrize("c", G.X6_PROBE_CASES, ids=G.case_id)
def test_single_product_probes(dev, c):
    plan, _ = _filed(c)
    X, Y, a, rows, covered = G.single_product_operands(c, plan[2], G.rng_of(c, 3))
    assert covered
    exact = a.astype(np.float64)[..., None] * rows.astype(np.float64)
    assert np.abs(exact).min() >= 2.0 ** -100
    got = _run(c, dev, X, Y).astype(np.float64)
    rel = np.abs(got - exact) / np.abs(exact)
    i = np.unravel_index(int(np.argmax(rel)), rel.shape)
    key = "single_product/" + G.instantiation(c) + ("_batched" if c.batch > 1 else "")
    _WORST[key] = (float(rel.max() / G.SINGLE_PRODUCT_BOUND), "%s (batch, row, column) %s" % (G.case_id(c), i))
    print("\n%s: worst relative error %.3f x 2^-24 at %s" % (key, rel.max() / 2.0 ** -24, i))
    assert rel.max() <= G.SINGLE_PRODUCT_BOUND, "%s %s: got %.9g exact %.9g, %.1f x 2^-24" % (
        G.case_id(c), i, got[i], exact[i], rel.max() / 2.0 ** -24)


# ------------------------------------------------------------------------------------------------------ (d) dense sums
def _check(c, what, got, ref, T):
    """|got - ref| <= (K + 16) 2^-24 T; records the worst ratio of the case's kernel instantiation."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), "%s %s: non-finite output" % (G.case_id(c), what)
    b = G.bound(T, c.K)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / b)
    w = float(ratio.max())
    key = G.instantiation(c) + ("_batched" if c.batch > 1 else "")
    if w >= _WORST.get(key, (-1.0, ""))[0]:
        _WORST[key] = (w, "%s %s" % (G.case_id(c), what))
    print("%s %s: worst |got - ref| / bound %.4f" % (G.case_id(c), what, w))
    if not w <= 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError("%s %s: element %s got %.9g ref %.9g |diff| %.3g bound %.3g (ratio %.3g)"
                             % (G.case_id(c), what, i, got[i], ref[i], err[i], b[i], w))


@pytest.mark.parametrize("c", G.DENSE_CASES, ids=G.case_id)
def test_dense_sums(dev, c):
    _filed(c)
    for salt, (name, draw) in enumerate((("full mantissa", G.full_mantissa), ("wide", G.wide))):
        rng = G.rng_of(c, 10 + salt)
        X, Y = draw(rng, (c.batch, c.M, c.K)), draw(rng, (c.batch, c.K, c.N))
        C0, bias = draw(rng, (c.batch, c.M, c.N)), draw(rng, (c.batch, c.N))
        if c.bias:
            _check(c, name + ", bias", _run(c, dev, X, Y, bias=bias), *G.dense_reference(X, Y, bias=bias))
            continue
        _check(c, name, _run(c, dev, X, Y), *G.dense_reference(X, Y))
        if c.batch == 1:
            _check(c, name + ", accumulate", _run(c, dev, X, Y, C0=C0), *G.dense_reference(X, Y, C0=C0))


# ------------------------------------------------------------------------------------- (e) colsum and transpose_last2
COLSUM_R = (1, 3, 255, 256, 257, 1000, 131073)      # 131073: 512 row chunks (the cap) of 257 rows, the last one ragged
COLSUM_C = (1, 63, 64, 65, 100)


def _colsum(dev, x, C0=None):
    Cc = x.shape[1]
    buf = torch.full((Cc + PAD,), NAN, dtype=torch.float32, device=dev)
    if C0 is not None:
        buf[:Cc] = _t(C0, dev)
    r = _pm().colsum(x, out=buf[:Cc], accumulate=C0 is not None)
    assert r.data_ptr() == buf.data_ptr()
    return _take(buf, Cc)


@pytest.mark.parametrize("Cc", COLSUM_C)
def test_colsum_exact(dev, Cc):
    rng = np.random.default_rng(Cc)
    big = rng.integers(-8, 9, (max(COLSUM_R), Cc)).astype(np.float32)       # sums below 2^21: exact in any order
    bigt = _t(big, dev)
    C0 = rng.integers(-1000, 1001, Cc).astype(np.float32)
    for R in COLSUM_R:
        want = big[-R:].astype(np.int64).sum(0)
        x = bigt[-R:]                                       # (rows R back from the end: contiguous, its own row 0)
        got = _colsum(dev, x)
        assert np.array_equal(got, want.astype(np.float32)), "R %d C %d: %s" % (R, Cc, np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(_np(_pm().colsum(x)), want.astype(np.float32)), (R, Cc)
        got = _colsum(dev, x, C0)
        assert np.array_equal(got, (want + C0.astype(np.int64)).astype(np.float32)), "accumulate, R %d C %d" % (R, Cc)


def test_colsum_rounding(dev):
    R, Cc = 1000, 100
    x = G.full_mantissa(np.random.default_rng(1000), (R, Cc))
    got = _colsum(dev, _t(x, dev)).astype(np.float64)
    ref, T = x.astype(np.float64).sum(0), np.abs(x.astype(np.float64)).sum(0)
    ratio = np.abs(got - ref) / G.bound(T, R)
    _WORST["colsum"] = (float(ratio.max()), "R %d C %d column %d" % (R, Cc, int(np.argmax(ratio))))
    assert ratio.max() <= 1.0, ratio.max()


@pytest.mark.parametrize("Bt", [1, 3])
def test_transpose_exact(dev, Bt):
    rng = np.random.default_rng(Bt)
    edge = (1, 31, 32, 33, 65)
    for R in edge:
        for Cc in edge:
            for x in (G.full_mantissa(rng, (Bt, R, Cc)), rng.integers(-2 ** 31, 2 ** 31, (Bt, R, Cc)).astype(np.int32)):
                xt = _t(x, dev)
                buf = torch.full((Bt * R * Cc + PAD,), NAN, dtype=torch.float32, device=dev)
                _raw("dh3d_transpose32", xt, Bt, R, Cc, buf)
                got = _take(buf, Bt * R * Cc).view(x.dtype).reshape(Bt, Cc, R)
                want = x.transpose(0, 2, 1)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (Bt, R, Cc, x.dtype)
                own = _np(_pm().transpose_last2(xt))
                assert own.dtype == x.dtype and np.array_equal(own.view(np.uint32), want.view(np.uint32)), (Bt, R, Cc)


# -------------------------------------------------------------------------------------------------------- (f) refusals
def test_refusals(dev):
    """Each refused call gets real operands of its stated shape (nothing is out of bounds even if a check were missing),
    returns the documented status, raises the library's error through pm, and leaves a NaN-filled output untouched."""
    pm = _pm()
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    UNSUPPORTED, INVALID = 2, 1

    def refused(status, name, args, out, wrapper, match):
        assert _status(name, *args) == status, name
        with pytest.raises(ValueError, match=match):
            wrapper()
        torch.cuda.synchronize()
        assert _untouched(out), name + " wrote its output"

    # nn: K % 4, N % 4
    for M, K, N in ((8, 6, 8), (8, 8, 6), (40, 6, 68), (40, 1000, 6)):
        A, B, out = z(M, K), z(K, N), _nanbuf(M, N, dev)
        assert pm.gemm_plan(0, M, N, K) is None
        refused(UNSUPPORTED, "dh3d_gemm_nn_f32", (A, B, None, M, K, N, 0, out), out,
                lambda: pm.gemm_nn(A, B, out=out[:M]), "unsupported shape")
        Ab, Bb, outb = z(2, M, K), z(2, K, N), _nanbuf(2 * M, N, dev)
        refused(UNSUPPORTED, "dh3d_gemm_nn_f32_batched", (Ab, Bb, None, 2, M, K, N, outb), outb,
                lambda: pm.gemm_nn_batched(Ab, Bb), "unsupported shape")
    # tn: M % 4, N % 4
    for K, M, N in ((8, 6, 8), (8, 8, 6), (70, 6, 68), (1000, 68, 6)):
        A, B, out = z(K, M), z(K, N), _nanbuf(M, N, dev)
        assert pm.gemm_plan(1, M, N, K) is None
        refused(UNSUPPORTED, "dh3d_gemm_tn_f32", (A, B, K, M, N, 0, out), out,
                lambda: pm.gemm_tn(A, B, out=out[:M]), "unsupported shape")
        Ab, Bb, outb = z(2, K, M), z(2, K, N), _nanbuf(2 * M, N, dev)
        refused(UNSUPPORTED, "dh3d_gemm_tn_f32_batched", (Ab, Bb, 2, K, M, N, outb), outb,
                lambda: pm.gemm_tn_batched(Ab, Bb), "unsupported shape")
    # a bias together with accumulate: on the rows kernel, the f32 tiles and a bf16x6 shape
    for M, K, N in ((8, 64, 64), (132, 36, 68), (256, 2048, 128)):
        A, B, bias, out = z(M, K), z(K, N), z(N), _nanbuf(M, N, dev)
        refused(INVALID, "dh3d_gemm_nn_f32", (A, B, bias, M, K, N, 1, out), out,
                lambda: pm.gemm_nn(A, B, out=out[:M], accumulate=True, bias=bias), "invalid argument")


# ------------------------------------------------------------------------------------------------------ (g) the report
def test_zz_report_worst_ratios():
    print("\nworst |got - ref| / bound per kernel instantiation over (d) (single_product/*: worst relative error / 2^-20):")
    for k in sorted(_WORST):
        print("  %-36s %.4f   %s" % (k, _WORST[k][0], _WORST[k][1]))
    assert all(v[0] <= 1.0 for v in _WORST.values())
