"""GPU: the drop-in flex operators (dh3d_amd/ops.py flex_convolution, flex_pooling, convolution_pointset), forward and every
gradient, on every kernel `ops._run` and csrc/flex_bwd.hip's fast_fwd_kind can choose by shape, against the float64
restatements of tests/flex_ops_reference.py -- on caller-made lists whose rank 0 is not the point (the forward centres on
the point, both backward paths on rank 0), repeated ids, a hub of in-degree N in the partial last tile, ids no list names,
and a cloud a thousand units from the origin.  tests/test_flex_ops_reference.py shows from the reference alone that the
other centre rule or a dropped last neighbour is >= 100 x outside these bounds at every point it touches.

Each float32 case runs twice: ops.FAST_PATH on (the plan the case is filed under, and the factorised backward) and off
(plan 0: the reference formulation of csrc/flex_generic.hip at the same shape).  Errors are in float32 unit roundoffs u of
each sum's own size T (flex_ops_reference: the same sum over |terms|); the float64 twins in float64 roundoffs.
"""
import contextlib

import numpy as np
import pytest
import torch

import flex_ops_reference as R

pytestmark = pytest.mark.gpu
QUANTITIES = ("out", "df", "dtheta", "dbias")


@contextlib.contextmanager
def _fast_path(on):
    from dh3d_amd import ops
    old = ops.FAST_PATH
    ops.FAST_PATH = on
    try:
        yield
    finally:
        ops.FAST_PATH = old


def _report(name, ratios):
    print("%s: worst error ratios %s" % (name, {k: round(v, 3) for k, v in ratios.items()}))


def _leaves(c, dev, *keys):
    return [c[k].to(dev).requires_grad_(True) for k in keys]


def _conv(c, dev):
    """(out, out of a second call, df, dtheta, dbias) of ops.flex_convolution on the case."""
    from dh3d_amd import ops
    f, th, bi = _leaves(c, dev, "f", "theta", "bias")
    p, nbr = c["p"].to(dev), c["nbr"].to(dev)
    out = ops.flex_convolution(f, p, nbr, th, bi)
    again = ops.flex_convolution(f.detach(), p, nbr, th.detach(), bi.detach())
    return (out.detach(), again) + torch.autograd.grad(out, (f, th, bi), c["dout"].to(dev))


def _pointset(c, dev):
    from dh3d_amd import ops
    f, th, bi = _leaves(c, dev, "f", "theta", "bias")
    nbr = c["nbr"].to(dev)
    out = ops.convolution_pointset(f, nbr, th, bi)
    again = ops.convolution_pointset(f.detach(), nbr, th.detach(), bi.detach())
    return (out.detach(), again) + torch.autograd.grad(out, (f, th, bi), c["dout"].to(dev))


def _ratios(got, ref, refs, T, Ts, unit=1.0):
    want, scale = (ref,) + tuple(refs), (T,) + tuple(Ts)
    return {q: R.ulp_ratio(g, w, s) * unit for q, g, w, s in zip(QUANTITIES, (got[0],) + tuple(got[2:]), want, scale)}


def _forward_has_atomics(plan, B, N, Din, Dout):
    """Plan 2's GEMM adds its partial sums with atomics where it splits the reduction; nothing else in a forward does."""
    from dh3d_amd import _lib
    return plan == 2 and bool(_lib.lib().dh3d_gemm_is_split(0, B * N, Dout, 4 * Din, 1))


def _case_id(c):
    return "p%d-%dx%d-k%d-%dto%d-dp%d-%s-%s" % c


# --------------------------------------------------------------------------------------------------- flex_convolution
@pytest.mark.parametrize("case", R.CONV_CASES, ids=_case_id)
def test_flex_convolution_on_every_plan(dev, case):
    from dh3d_amd import _lib
    plan, B, N, K, Din, Dout, Dp, kind, ckind = case
    assert _lib.lib().dh3d_flex_conv_fwd_plan(B, N, K, Dp, Din, Dout) == plan, "the dispatch table moved this case"
    c = R.conv_case(B, N, K, Din, Dout, Dp, kind, ckind)
    args = [c[k] for k in ("f", "p", "nbr", "theta", "bias")]
    ref, T = R.flex_conv(*args)
    refs, Ts = R.flex_conv_grads(*args, c["dout"])
    if kind == "adversarial" and R.adversarial_applies(N, K):
        assert not Ts[0][:, :, list(R.REMOVED)].any()           # no list names them: df must be EXACTLY 0 there
    bad = []
    for fast in (True, False):
        group = plan if fast else 0
        with _fast_path(fast):
            got = _conv(c, dev)
        r = _ratios(got, ref, refs, T, Ts)
        _report("flex_convolution %s %s (plan %d)" % (_case_id(case), "fast" if fast else "reference", group), r)
        if not _forward_has_atomics(group, B, N, Din, Dout):
            assert torch.equal(got[0], got[1]), "two forward calls differ"
        bad += [(group, q, v) for q, v in r.items() if not v <= R.BOUNDS[group][q]]
    assert not bad, bad


@pytest.mark.parametrize("case", R.F64_CONV_CASES, ids=_case_id)
def test_flex_convolution_float64_twins(dev, case):
    _, B, N, K, Din, Dout, Dp, kind, ckind = case
    c = R.conv_case(B, N, K, Din, Dout, Dp, kind, ckind, dtype=torch.float64)
    args = [c[k] for k in ("f", "p", "nbr", "theta", "bias")]
    ref, T = R.flex_conv(*args)
    refs, Ts = R.flex_conv_grads(*args, c["dout"])
    got = _conv(c, dev)
    assert got[0].dtype == got[2].dtype == torch.float64
    r = _ratios(got, ref, refs, T, Ts, unit=R.U / R.U64)
    _report("flex_convolution float64 %s (in float64 roundoffs)" % _case_id(case), r)
    assert torch.equal(got[0], got[1])
    assert all(v <= R.BOUNDS["f64"][q] for q, v in r.items()), r


# ------------------------------------------------------------------------------------------------------- flex_pooling
def _pool(c, dev):
    from dh3d_amd import ops
    f = c["f"].to(dev).requires_grad_(True)
    out, arg = ops.flex_pooling(f, c["nbr"].to(dev))
    (df,) = torch.autograd.grad(out, f, c["dout"].to(dev))
    return out.detach(), arg, df


def _check_pool(c, got, name, unit=1.0):
    B, D, N = c["f"].shape
    val, arg = R.flex_pool(c["f"], c["nbr"])
    assert np.array_equal(got[0].cpu().numpy(), val), "values differ from the rule"
    assert np.array_equal(got[1].cpu().numpy(), arg), "argmax differs from the rule (first k of a tie, id 0 for no candidate)"
    for n in R.POOL_EMPTY:                                       # lists of nothing but -inf / NaN
        assert (arg[:, :, n] == 0).all() and (val[:, :, n] == np.finfo(val.dtype).min).all()
    assert ((arg == N - 1).reshape(B, -1).sum(1) > N).all()     # the hub is the argmax of more than N entries
    din, Tdin, cnt = R.flex_pool_grad(c["dout"], arg)
    r = dict(df=R.ulp_ratio(got[2], din, Tdin) * unit, max_contributions=float(cnt.max()))
    _report(name, r)
    assert r["df"] <= R.BOUNDS["pool"]["df"], r


@pytest.mark.parametrize("B,N,K,D", R.POOL_CASES)
def test_flex_pooling_on_both_paths(dev, B, N, K, D):
    from dh3d_amd import _lib
    assert (_lib.lib().dh3d_flex_pool_fwd_workspace_bytes(B, N, K, D) > 0) == (D % 4 == 0)    # the point-major kernel
    c = R.pool_case(B, N, K, D)
    for fast in (True, False):
        with _fast_path(fast):
            got = _pool(c, dev)
        _check_pool(c, got, "flex_pooling %dx%d k%d d%d %s" % (B, N, K, D, "fast" if fast else "reference"))


def test_flex_pooling_float64_twin(dev):
    c = R.pool_case(*R.F64_POOL_CASE, dtype=torch.float64)
    got = _pool(c, dev)
    assert got[0].dtype == got[2].dtype == torch.float64
    _check_pool(c, got, "flex_pooling float64 %dx%d k%d d%d (in float64 roundoffs)" % R.F64_POOL_CASE, unit=R.U / R.U64)


# ----------------------------------------------------------------------------------------------- convolution_pointset
def _check_pointset(c, got, name, group, unit=1.0):
    args = (c["f"], c["nbr"], c["theta"], c["bias"])
    ref, T = R.conv_pointset(*args)
    refs, Ts = R.conv_pointset_grads(*args, c["dout"])
    r = _ratios(got, ref, refs, T, Ts, unit)
    _report(name, r)
    assert torch.equal(got[0], got[1]), "two forward calls differ"
    assert all(v <= R.BOUNDS[group][q] for q, v in r.items()), r


@pytest.mark.parametrize("case", R.POINTSET_CASES, ids=lambda c: "%dx%d-k%d-%dto%d-%s" % c)
def test_convolution_pointset(dev, case):
    c = R.pointset_case(*case)
    if case[5] == "adversarial":
        assert not R.conv_pointset_grads(c["f"], c["nbr"], c["theta"], c["bias"], c["dout"])[1][0][:, :, list(R.REMOVED)].any()
    for fast in (True, False):
        with _fast_path(fast):
            got = _pointset(c, dev)
        _check_pointset(c, got, "convolution_pointset %s %s" % (case, "fast" if fast else "reference"), "pointset")


def test_convolution_pointset_float64_twin(dev):
    c = R.pointset_case(*R.F64_POINTSET_CASE, dtype=torch.float64)
    got = _pointset(c, dev)
    assert got[0].dtype == got[2].dtype == torch.float64
    _check_pointset(c, got, "convolution_pointset float64 %s (in float64 roundoffs)" % (R.F64_POINTSET_CASE,),
                    "pointset_f64", unit=R.U / R.U64)
