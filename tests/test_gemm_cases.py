"""No GPU: pins tests/gemm_cases.py, the cases and probes of tests/test_gemm_kernels_gpu.py -- every case reaches the kernel
it is filed under (dh3d_gemm_plan is host only), the builders keep their exactness preconditions and visit the positions
they promise, and the probes are sharp: a restatement of the bf16x6 kernel with one third-order product removed, c2 d2 or
c1 d3, passes the first-generation check |got - exp| <= 2e-6 |A||B| + 1e-6 at K = 2048 and fails the probes."""
import numpy as np
import pytest

import gemm_cases as G


def _plan(c):
    from dh3d_amd import _lib, pm
    ta = int(c.form == "tn")
    return (pm.gemm_plan(ta, c.M, c.N, c.K, c.batch, c.bias), _lib.lib().dh3d_gemm_is_split(ta, c.M, c.N, c.K, c.batch))


@pytest.mark.parametrize("family", list(G.FAMILIES) + ["dense"])
def test_every_case_is_filed_under_its_kernel(family):
    cases = G.DENSE_CASES if family == "dense" else G.FAMILIES[family]
    for c in cases:
        moved = G.filed_ok(c, *_plan(c))
        assert moved is None, "the dispatch table moved this case: %s -> %s" % (G.case_id(c), moved)


def test_the_case_table_holds_the_edges():
    fam = G.FAMILIES
    assert set(c.kernel for c in fam["rows"]) == {"rows1", "rows2", "rows3", "rows4"}
    assert set(c.M for c in fam["rows"]) == {1, 8, 9, 16, 17, 24, 25, 32}
    assert set(c.K for c in fam["rows"]) == {4, 60, 64, 68, 252, 256, 512}
    assert set(c.N for c in fam["rows"]) == {4, 60, 64, 68, 132}
    assert len(fam["shortk"]) == 100
    for form, Ks in (("tn", {33, 47, 48, 49, 70, 1000, 1001}), ("nn", {20, 36, 52, 1000, 4000})):
        f = [c for c in fam["f32"] if c.form == form and c.batch == 1]
        assert Ks <= set(c.K for c in f) and {4, 124, 128, 132, 260} <= set(c.M for c in f)
        assert {4, 60, 64, 68, 128, 132, 260} <= set(c.N for c in f)
        assert set(c.kernel for c in f) == {"f32_narrow", "f32_wide"} and set(c.split for c in f) == {False, True}
    assert set(G.instantiation(c) for c in fam["x6"]) == {"x6_wide_nn", "x6_narrow_nn", "x6_wide_tn", "x6_narrow_tn"}
    assert set(G.instantiation(c) for c in G.X6_PROBE_CASES) == set(G.instantiation(c) for c in fam["x6"])
    assert any(c.batch > 1 for c in G.X6_PROBE_CASES)
    inst = set(G.instantiation(c) for c in G.DENSE_CASES)
    assert inst == {"rows1", "rows2", "rows3", "rows4", "shortk"} | {"%s_%s_%s" % (p, w, f) for p in ("f32", "x6")
                                                                     for w in ("narrow", "wide") for f in ("nn", "tn")}
    # no shape above roughly 1024 x 4128 x 260 (the narrow tn cases need K = 8192 to reach 2^26 multiply-adds)
    for cases in list(fam.values()) + [G.DENSE_CASES]:
        for c in cases:
            assert c.batch * c.M * c.K * c.N <= 1024 * 4128 * 260, G.case_id(c)


def test_integer_operands_are_exact_in_any_order():
    c = G.case("nn", 129, 4096, 132, "x6_wide", True)
    X, Y, C0, bias, want = G.integer_operands(c, G.rng_of(c))
    assert X.dtype == Y.dtype == np.float32 and np.abs(X).max() == 8 and np.abs(Y).max() == 8
    assert np.array_equal(X, np.rint(X)) and np.array_equal(C0, np.rint(C0)) and np.array_equal(bias, np.rint(bias))
    assert np.array_equal(want[0], X[0].astype(np.int64) @ Y[0].astype(np.int64))
    # integers in [-8, 8] live in the first bf16 chunk alone: this probe cannot see c2, c3
    assert not G.split3(X)[1].any() and not G.split3(X)[2].any()
    # f32 partial sums in a scrambled order still give the integer
    order = G.rng_of(c, 1).permutation(c.K)
    acc = np.zeros((c.M, c.N), np.float32)
    for k0 in range(0, c.K, 512):
        acc += X[0][:, order[k0:k0 + 512]] @ Y[0][order[k0:k0 + 512]]
    assert np.array_equal(acc.astype(np.int64), want[0])
    b = G.case("tn", 64, 1024, 132, "x6_wide", True, batch=8)
    X, Y, _, _, want = G.integer_operands(b, G.rng_of(b))
    assert X.shape == (8, 64, 1024) and not np.array_equal(X[0], X[1]) and not np.array_equal(Y[0], Y[1])
    A, B = G.device_operands(b, X, Y)
    assert A.shape == (8, 1024, 64) and A.flags.c_contiguous and np.array_equal(A[3].T, X[3])


def _kchunk(c):
    return _plan(c)[0][2]


@pytest.mark.parametrize("c", G.X6_PROBE_CASES, ids=G.case_id)
def test_three_chunk_probe_is_exact_and_needs_the_first_order_products(c):
    kc = _kchunk(c)
    for dense, needs in (("X", ((2, 1), (3, 1))), ("Y", ((1, 2), (1, 3)))):
        X, Y, want, covered = G.three_chunk_operands(c, kc, G.rng_of(c, 2), dense)
        assert covered, "positions miss a residue mod 32 or a side of a chunk boundary"
        assert np.abs(want).max() < 2 ** 23 and np.abs(X).max() < 2 ** 20 and np.abs(Y).max() < 2 ** 20
        if c.batch > 1:
            assert not np.array_equal(X[0] != 0, X[1] != 0) or not np.array_equal(Y[0] != 0, Y[1] != 0)
        got = G.emulate_x6(X[-1], Y[-1])
        assert np.array_equal(got, want[-1])
        for drop in needs:
            keep = tuple(p for p in G.KERNEL_ORDER if p != drop)
            assert not np.array_equal(G.emulate_x6(X[-1], Y[-1], keep), want[-1]), drop


@pytest.mark.parametrize("c", G.X6_PROBE_CASES, ids=G.case_id)
def test_second_order_probe_is_exact_and_needs_c2d2(c):
    assert float(G.V9_SQUARED) == 1 + 2.0 ** -8 + 2.0 ** -18 == float(G.V9) ** 2
    kc = _kchunk(c)
    for sparse in ("X", "Y"):
        X, Y, covered = G.second_order_operands(c, kc, sparse)
        # (the mirror has N lines: fewer than the 128 chunks of the narrow tn case, whose chunks the X form visits)
        assert covered or (sparse == "Y" and c.N < -(-c.K // kc)), "positions miss a residue mod 32 or a chunk"
        assert ((X[0] != 0).sum(1) == (1 if sparse == "X" else c.K)).all()
        assert ((Y[0] != 0).sum(0) == (1 if sparse == "Y" else c.K)).all()
        # one product per element: the six chunk products rounded to f32 in the kernel's order, and in any other
        for order in (G.KERNEL_ORDER, G.SIX):
            assert G.six_products(G.V9, G.V9, order) == G.V9_SQUARED
        assert G.six_products(G.V9, G.V9, tuple(p for p in G.KERNEL_ORDER if p != (2, 2))) != G.V9_SQUARED
        got = G.emulate_x6(X[0], Y[0])
        assert np.array_equal(got, np.full((c.M, c.N), float(G.V9_SQUARED)))
        bad = G.emulate_x6(X[0], Y[0], tuple(p for p in G.KERNEL_ORDER if p != (2, 2)))
        assert (bad.astype(np.float32) != G.V9_SQUARED).all()


@pytest.mark.parametrize("c", G.X6_PROBE_CASES, ids=G.case_id)
def test_single_product_probe_bound_and_margin_on_its_own_arrays(c):
    X, Y, a, rows, covered = G.single_product_operands(c, _kchunk(c), G.rng_of(c, 3))
    assert covered
    assert ((X != 0).sum(2) == 1).all() and np.array_equal(X.sum(2), a)
    exact = a.astype(np.float64)[..., None] * rows.astype(np.float64)
    assert np.abs(exact).min() > 2.0 ** -100
    assert np.array_equal(X[0].astype(np.float64) @ Y[0].astype(np.float64), exact[0])
    for order in (G.KERNEL_ORDER, G.SIX, G.SIX[::-1]):
        rel = np.abs(G.six_products(a[..., None], rows, order) - exact) / np.abs(exact)
        assert rel.max() <= G.SINGLE_PRODUCT_BOUND, rel.max() / 2.0 ** -24
    for dropped in G.SIX:
        keep = tuple(p for p in G.KERNEL_ORDER if p != dropped)
        rel = np.abs(G.six_products(a[..., None], rows, keep) - exact) / np.abs(exact)
        assert rel.max() >= 10 * G.SINGLE_PRODUCT_BOUND, (dropped, rel.max() / 2.0 ** -24)


@pytest.mark.parametrize("dropped", [(2, 2), (1, 3)], ids=["c2d2", "c1d3"])
def test_a_lost_third_order_product_passes_the_old_check_and_fails_the_probes(dropped):
    """Gaussian 48 x 2048 x 48, the bf16x6 kernel restated with one product missing: inside 2e-6 |A||B| + 1e-6, and far
    inside the rounding-sum bound (K + 16) 2^-24 T -- while (b) sees c2 d2, (a') sees c1 d3 and (c) sees both, by more than
    ten times its bound."""
    rng = np.random.default_rng(2048)
    X, Y = rng.standard_normal((48, 2048)).astype(np.float32), rng.standard_normal((2048, 48)).astype(np.float32)
    keep = tuple(p for p in G.KERNEL_ORDER if p != dropped)
    exp, mag = G.dense_reference(X[None], Y[None])
    err = np.abs(G.emulate_x6(X, Y, keep) - exp[0])
    old = (err / (2e-6 * mag[0] + 1e-6)).max()
    assert 0.1 < old < 1.0, old                                   # the old test passes
    assert (err / G.bound(mag[0], 2048)).max() < 0.05             # and so does a sum bound
    assert (np.abs(G.emulate_x6(X, Y) - exp[0]) / (2e-6 * mag[0] + 1e-6)).max() < 0.01   # (all six: nothing to see)
    # at K = 256 the same loss is over the old tolerance: short reductions were covered
    err = np.abs(G.emulate_x6(X[:, :256], Y[:256], keep) - X[:, :256].astype(np.float64) @ Y[:256].astype(np.float64))
    assert (err / (2e-6 * (np.abs(X[:, :256]).astype(np.float64) @ np.abs(Y[:256])) + 1e-6)).max() > 1.0
    # the probes, on the smallest bf16x6 probe case's own arrays
    c = G.X6_PROBE_CASES[0]
    kc = _kchunk(c)
    if dropped == (2, 2):
        Xs, Ys, _ = G.second_order_operands(c, kc, "X")
        assert (G.emulate_x6(Xs[0], Ys[0], keep).astype(np.float32) != G.V9_SQUARED).all()
    else:
        Xs, Ys, want, _ = G.three_chunk_operands(c, kc, G.rng_of(c, 2), "Y")
        assert not np.array_equal(G.emulate_x6(Xs[0], Ys[0], keep), want[0])
    _, _, a, rows, _ = G.single_product_operands(c, kc, G.rng_of(c, 3))
    exact = a.astype(np.float64)[..., None] * rows.astype(np.float64)
    rel = np.abs(G.six_products(a[..., None], rows, keep) - exact) / np.abs(exact)
    assert rel.max() >= 10 * G.SINGLE_PRODUCT_BOUND


def test_dense_reference_and_positions():
    rng = np.random.default_rng(4)
    X, Y = G.wide(rng, (2, 5, 7)), G.full_mantissa(rng, (2, 7, 3))
    assert (G.full_mantissa(rng, 1000).view(np.uint32) & 1).all()
    C0, bias = G.wide(rng, (2, 5, 3)), G.wide(rng, (2, 3))
    v, T = G.dense_reference(X, Y, C0=C0)
    for b in range(2):
        assert np.allclose(v[b], X[b].astype(np.float64) @ Y[b] + C0[b], rtol=1e-14)
        assert np.allclose(T[b], np.abs(X[b]).astype(np.float64) @ np.abs(Y[b]) + np.abs(C0[b]), rtol=1e-14)
    v2, T2 = G.dense_reference(X, Y, bias=bias)
    assert np.allclose(v2 - bias[:, None, :], v - C0, rtol=1e-9) and np.all(T2 >= np.abs(v2) * (1 - 1e-12))
    ks, fits = G.probe_positions(2080, 256, 8 * 132)
    assert fits and len(ks) == 8 * 132 and ks.min() == 0 and ks.max() == 2079 and G.positions_cover(ks, 2080, 256)
    assert not G.positions_cover(ks[ks != 255], 2080, 256) and not G.positions_cover(ks[ks % 32 != 7], 2080, 256)
    assert not G.probe_positions(8192, 64, 8 * 16)[1]
    c = G.case("nn", 260, 2080, 132, "x6_wide", True)
    assert G.lines_cover(G.line_positions(c, 256, 260), 2080, 256) and not G.lines_cover(G.line_positions(c, 256, 8), 2080, 256)
