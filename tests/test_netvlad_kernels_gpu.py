"""GPU: the NetVLAD kernels (csrc/netvlad.hip) and the global walk (csrc/dense_x6.hip: dh3d_walk_plan,
dh3d_global_walk_planned_fwd) stage by stage against the float64 restatements of tests/netvlad_reference.py, through the
C entry points, every output in a NaN-filled buffer with sentinel rows behind it, every element compared against an
a-priori bound (tests/test_netvlad_reference.py proves on these very inputs that the listed mistakes exceed it tenfold).

(a) selection probes on dh3d_netvlad_aggregate_fwd: one-hot rows, one-hot assignment, dyadic attention -- every cell (c, d)
    of every cloud carries its own value; once more with a one-hot W2 (its column and its sign);
(b) shapes of the aggregation (netvlad_reference.AGG_SHAPES: every chunking regime, N around the 64-point tile, B around
    the 8 XCDs) on aggregate_fwd and fused_fwd with / without gating, l2_eps 1e-8 / 0 (all four pairs at B = 9, N = 130);
(c) clamps: a zero row, a cloud of zero rows, a cloud with zero attention beside a normal one, saturated logits, rows
    scaled by 2^-70 (under the 1e-12 clamp, as the contract has it), 2^-16 and 2^40 (scale-free);
(d) dh3d_netvlad_head_fwd alone: Kd 8 .. 16384, B 1 .. 33, gating, l2_eps 0 / 1e-8 / 1e-3 with a row the clamp decides,
    one-hot rows that return rows of Wh, and the refusal of Kd % 8 != 0;
(e) the walk: att, apart and asum compared directly; m 1 .. 1024, n 1 .. 300, B 1 .. 9, coherent and overflowing lists,
    order / plan / att present and absent, zero_accum both ways, every attention epilogue, the refusals;
(f) dh3d_netvlad_tail_assign_fwd alone on synthetic operands: m 1 .. 1024, B 1 .. 9, one-hot apart, a zero cloud;
(g) end to end at B = 3, n = 300, m = 40.
Not reached here: csrc/netvlad_train.hip (dh3d_netvlad_assign_rows*, dh3d_netvlad_commuted_*), covered by
tests/test_commuted_walks_gpu.py and the training tests.

Allowances (tests/netvlad_reference.py), measured on an MI355X on 2026-10-18 by test_allowances_are_measured on inputs
whose value before the function is exact; each is four times the worst error measured, rounded up to one digit, and the
test fails if the constant is anything else (under it or above it):
  A_EXP = 3e-7   measured 5.746e-08 relative per (1 + |x|) (the rounding of x log2 e grows with |x|): one-hot rows against
                 integer logits through the walk; 5.311e-08 through dh3d_netvlad_aggregate_fwd.  4 x 5.746e-08 = 2.3e-7.
  A_RSQ = 2e-7   measured 1.045e-07 relative on the selection probes of (a), where three rsqrt follow each other (row,
                 cluster, whole vector).  Assumption: the three errors add evenly, so one rsqrt is charged a third of the
                 measured figure, which also still holds the probe's own roundings: 4 x 1.045e-07 / 3 = 1.4e-7.
tests/test_netvlad_reference.py computes the smallest relative effect of any mutation (0.047, walk_no_rinv) and requires
both allowances ten times under it; they are more than 10^5 times under it.
Selection probes: their bound is |ref| (3 A_RSQ + 61.5 x 2^-24), each sum charged by dense_reference.rel_bound at its
own number of non-zero terms (derived at the test); the change of a norm through the errors of its terms is not charged.

Worst |got - ref| / bound per kernel, MI355X, 2026-10-18 (test_zz_report_worst_ratios prints it; all 66 tests pass, each
under two seconds); none is above 0.5:
  head/onehot            0.3282  (Kd=16384)
  walk/apart             0.0903  (B1 n300 m1024 random Hd1024 planned)
  head                   0.0661  (Kd=8 B=33 gating=0 l2=1e-08)
  aggregate/selection    0.0279  (w2)
  walk/asum              0.0056  (B3 n127 m3 nn Hd256 planned)
  aggregate              0.0028  (B257 N64)
  fused                  0.0024  (zero_att_cloud gating=1 l2=1e-08)
  tail_assign            0.0021  (zero_cloud)
  walk/att               0.0015  (e2e)
  tail_assign/onehot     0.0000  (closed form)
  e2e/out                0.0000  (walk+tail)
test_zz_report_worst_ratios prints the worst |got - ref| / bound per kernel and requires every one of them under 1.
The bounds of `out` behind the 16384-deep projection are the any-order bound of that sum (16400 x 2^-24 of the sum of
absolute terms): they see a wrong cloud, column or clamp, not a lost point; the lost point is seen on vlad, apart and asum.
"""
import numpy as np
import pytest
import torch

import dense_reference as D
import netvlad_reference as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 8
DM, CL, OD = R.DM, R.CL, R.OD
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


def _nanbuf(rows, width, dev):
    return torch.full((rows + PAD, width), NAN, dtype=torch.float32, device=dev)


def _take(buf, rows):
    """The first `rows` rows of a sentinel buffer; the rows behind them must still hold the fill, bit for bit."""
    fill = torch.full((1,), NAN, dtype=torch.float32).view(torch.int32).item()
    tail = buf[rows:].view(torch.int32)
    assert bool((tail == fill).all()), "rows past the output were written: %s" % (torch.nonzero(tail != fill)[:4].tolist(),)
    return buf[:rows].detach().cpu().numpy()


def _check(kernel, case, got, ref, E):
    got = np.asarray(got, np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), "%s %s: non-finite output" % (kernel, case)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / E)
    w = float(ratio.max())
    if w > _WORST.get(kernel, (-1.0, ""))[0]:
        _WORST[kernel] = (w, str(case))
    print("%s %s: worst |got - ref| / bound %.4g" % (kernel, case, w))
    if not w <= 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError("%s %s: element %s got %.9g ref %.9g |diff| %.3g bound %.3g (ratio %.3g)"
                             % (kernel, case, i, got[i], ref[i], err[i], E[i], w))


def _unsupported(fn):
    with pytest.raises(ValueError, match="unsupported shape"):
        fn()


def _ws(nbytes, dev):
    return torch.full((nbytes // 4 + 64,), NAN, dtype=torch.float32, device=dev)


def _aggregate(dev, x, att, Wc, sc, sh, W2):
    B, N, _ = x.shape
    nb = _L().lib().dh3d_netvlad_workspace_bytes(B, N, DM, CL)
    out = _nanbuf(B, DM * CL, dev)
    _raw("dh3d_netvlad_aggregate_fwd", _t(x, dev), _t(att, dev), _pm().pack_weight(_t(Wc, dev)), _t(sc, dev), _t(sh, dev),
         _t(W2, dev), B, N, DM, CL, _ws(nb, dev), nb, out)
    return _take(out, B)


def _fused(dev, x, att, Wc, sc, sh, W2, Wh, s1, h1, Wg, s2, h2, l2_eps):
    B, N, _ = x.shape
    nb = _L().lib().dh3d_netvlad_fused_workspace_bytes(B, N, DM, CL, OD)
    out = _nanbuf(B, OD, dev)
    _raw("dh3d_netvlad_fused_fwd", _t(x, dev), _t(att, dev), _pm().pack_weight(_t(Wc, dev)), _t(sc, dev), _t(sh, dev),
         _t(W2, dev), _t(Wh, dev), _t(s1, dev), _t(h1, dev), _t(Wg, dev), _t(s2, dev), _t(h2, dev), B, N, DM, CL, OD,
         float(l2_eps), _ws(nb, dev), nb, out)
    return _take(out, B)


def _head(dev, vlad, Wh, s1, h1, Wg, s2, h2, l2_eps, Kd=None, slack=0):
    """Kd: the claimed width (vlad / Wh are allocated with `slack` floats more per row for the refusals)."""
    B = vlad.shape[0]
    Kd = vlad.shape[1] if Kd is None else Kd
    nb = _L().lib().dh3d_netvlad_head_workspace_bytes(B, Kd, OD)
    out = _nanbuf(B, OD, dev)
    _raw("dh3d_netvlad_head_fwd", _t(vlad, dev), _t(Wh, dev), _t(s1, dev), _t(h1, dev), _t(Wg, dev), _t(s2, dev),
         _t(h2, dev), B, Kd, OD, float(l2_eps), _ws(nb + 4 * slack, dev), nb, out)
    return _take(out, B)


def _tail(dev, apart, coarse, asum, W2, Wh, s1, h1, Wg, s2, h2, l2_eps, m=None):
    B = coarse.shape[0]
    m = coarse.shape[1] if m is None else m
    nb = _L().lib().dh3d_netvlad_tail_workspace_bytes(B, DM, CL, OD)
    out = _nanbuf(B, OD, dev)
    _raw("dh3d_netvlad_tail_assign_fwd", _t(apart, dev), _t(coarse, dev), _t(asum, dev), m, _t(W2, dev), _t(Wh, dev),
         _t(s1, dev), _t(h1, dev), _t(Wg, dev), _t(s2, dev), _t(h2, dev), B, DM, CL, OD, float(l2_eps), _ws(nb, dev), nb, out)
    return _take(out, B)


def _walk(dev, case, order=True, plan=True, zero_accum=1, want_att=True, m=None, Hd=None, act=None):
    """-> att [B, n] (or None), apart [B, m, 64], asum [B, 64] of dh3d_global_walk_planned_fwd; H and cw come from the
    library's own GEMMs, as pm.global_tail has them.  m / Hd / act: a claimed shape for the refusals (buffers stay valid)."""
    pm, L = _pm(), _L()
    W_att, att_ep, w_fc, b_fc, Wc, sc, sh = case["par"]
    B, n, mm, hd = case["B"], case["n"], case["m"], case["Hd"]
    c = _t(case["coarse"], dev)
    Wt = _t(W_att, dev)
    wp = torch.cat([pm.pack_weight_x3(Wt[:, j:j + 256].contiguous()) for j in range(0, hd, 256)])
    H = torch.empty((hd // 256, B * mm, 256), dtype=torch.float32, device=dev)
    _raw("dh3d_linear_slices_pm_x6_fwd", c, DM, wp, B * mm, hd // 256, H)
    cw = pm.linear(c, pm.pack_weight(_t(Wc, dev)), CL)
    idx, dist = _t(case["idx"], dev), _t(case["dist"], dev)
    srt = None
    if order and n >= 64:
        srt = pm.spatial_sort(_t(case["fine"], dev))[0]
    elif order:                                      # tiny clouds: a random walk order, written as spatial_sort writes it
        rng = R.seed("order", B, n)
        rec = np.concatenate([case["fine"], np.zeros((B, n, 1), np.float32)], -1)
        rec[..., 3] = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int32).view(np.float32)
        rec[..., :3] = np.take_along_axis(case["fine"], rec[..., 3].view(np.int32)[..., None].astype(np.int64), 1)
        srt = _t(rec, dev)
    pl = pm.walk_plan(idx, dist, srt, mm) if plan else None
    keep = []
    ep = None
    if att_ep is not None or act is not None:
        e = list(att_ep) if att_ep is not None else [None, None, None, D.ACT_NONE]
        if act is not None:
            e[3] = act
        d = [_t(v, dev) for v in e[:3]]
        keep.extend(d)
        ep = L.make_epilogue(*d, e[3])
    att = _nanbuf(B, n, dev) if want_att else None
    if zero_accum:                                  # NaN everywhere: the call itself must clear its part
        acc = torch.full((1 + PAD, B * mm * CL + B * CL), NAN, dtype=torch.float32, device=dev)
    else:
        acc = torch.cat([torch.zeros((1, B * mm * CL + B * CL), device=dev),
                         torch.full((PAD, B * mm * CL + B * CL), NAN, dtype=torch.float32, device=dev)])
    _raw("dh3d_global_walk_planned_fwd", H, hd if Hd is None else Hd, c, cw, idx, dist, srt, pl, B, n, mm if m is None else m,
         ep, _t(w_fc, dev), float(b_fc), _t(sc, dev), _t(sh, dev), att, acc, int(zero_accum))
    a = _take(acc, 1)[0]
    return (_take(att, B) if want_att else None), a[:B * mm * CL].reshape(B, mm, CL), a[B * mm * CL:].reshape(B, CL)


def _check_walk(name, case, got, ref):
    if got[0] is not None:
        _check("walk/att", name, got[0], ref[0], ref[1])
    _check("walk/apart", name, got[1], ref[2], ref[3])
    _check("walk/asum", name, got[2], ref[4], ref[5])


# ------------------------------------------------------------------------------------------------- the allowances
def _exp_probe_aggregate(dev):
    """cloud b: x0 = e_{2b}, x1 = e_{2b+1}; Wc[2b] integer logits, Wc[2b+1] = 0 (a = 1/64 exactly): V[c, 2b] / V[c, 2b+1]
    = 64 a[0, c], whatever the two normalisations do."""
    B = 8
    x = np.zeros((B, 2, DM), np.float32)
    Wc = np.zeros((DM, CL), np.float32)
    for b in range(B):
        x[b, 0, 2 * b], x[b, 1, 2 * b + 1] = 1.0, 1.0
        Wc[2 * b] = -((np.arange(CL) * (b + 1)) % 30)
    vl = _aggregate(dev, x, np.ones((B, 2), np.float32), Wc, np.ones(CL, np.float32), np.zeros(CL, np.float32),
                    np.zeros((DM, CL), np.float32)).astype(np.float64).reshape(B, DM, CL)
    worst = 0.0
    for b in range(B):
        l = Wc[2 * b].astype(np.float64)
        xk = l - l.max()
        p = np.exp(xk) / np.exp(xk).sum()
        got = vl[b, 2 * b] / vl[b, 2 * b + 1] / 64.0
        om = (1 + np.abs(xk)) + (p * (1 + np.abs(xk))).sum()
        worst = max(worst, float((np.abs(got / p - 1) / om).max()))
    return worst


def _exp_probe_walk(dev):
    """one point per cloud on one coarse row e_b with dyadic weights: x = e_b, |x| = 1, logits = the integer row b of Wc."""
    B = 8
    case = R.walk_case(B, 1, 3, "nn")
    case["coarse"][:] = 0
    case["coarse"][np.arange(B), 0, np.arange(B)] = 1.0
    case["idx"][:] = 0
    case["dist"][:] = np.float32([1.0, 2.0, 2.0])
    par = list(case["par"])
    Wc = np.zeros((DM, CL), np.float32)
    for b in range(B):
        Wc[b] = -((np.arange(CL) * (b + 1)) % 30)
    par[4], par[5], par[6] = Wc, np.ones(CL, np.float32), np.zeros(CL, np.float32)
    case["par"] = tuple(par)
    att, _, asum = _walk(dev, case)
    worst = 0.0
    for b in range(B):
        l = Wc[b].astype(np.float64)
        xk = l - l.max()
        p = np.exp(xk) / np.exp(xk).sum()
        om = (1 + np.abs(xk)) + (p * (1 + np.abs(xk))).sum()
        worst = max(worst, float((np.abs(asum[b].astype(np.float64) / float(att[b, 0]) / p - 1) / om).max()))
    return worst


def _selection(dev, w2):
    case = R.selection_case(w2=w2)
    ref, _ = R.aggregate(*case)
    got = _aggregate(dev, *case).astype(np.float64)
    return got, ref


def _one_digit_up(v):
    """v rounded up to one significant digit."""
    e = 10.0 ** np.floor(np.log10(v))
    return float(np.ceil(v / e - 1e-9) * e)


def test_allowances_are_measured(dev):
    """A_EXP and A_RSQ ARE four times the measured worst error, rounded up to one digit: neither under it nor above it."""
    e1, e2 = _exp_probe_aggregate(dev), _exp_probe_walk(dev)
    got, ref = _selection(dev, False)
    big = np.abs(ref) > 1e-6
    rs = float((np.abs(got - ref)[big] / np.abs(ref)[big]).max())
    a_exp, a_rsq = _one_digit_up(4 * max(e1, e2)), _one_digit_up(4 * rs / 3)
    print("MEASURED exp: aggregate %.4g, walk %.4g (relative, per 1 + |x|) -> A_EXP = 4 x %.4g, one digit up = %.0e; rsqrt "
          "(three in a row, plus the roundings of the probe): %.4g -> A_RSQ = 4 x %.4g / 3, one digit up = %.0e"
          % (e1, e2, max(e1, e2), a_exp, rs, rs, a_rsq))
    assert abs(R.A_EXP - a_exp) <= 1e-6 * a_exp, "A_EXP %.3g is not four times the measured %.4g, rounded up to one " \
        "digit (%.0e)" % (R.A_EXP, max(e1, e2), a_exp)
    assert abs(R.A_RSQ - a_rsq) <= 1e-6 * a_rsq, "A_RSQ %.3g is not four times the measured %.4g / 3, rounded up to one " \
        "digit (%.0e)" % (R.A_RSQ, rs, a_rsq)


# --------------------------------------------------------------------------------------------- (a) selection probes
@pytest.mark.parametrize("w2", [False, True], ids=["w2_zero", "w2_onehot"])
def test_selection_probes(dev, w2):
    got, ref = _selection(dev, w2)
    case_n = R.selection_case(w2=w2)[0].shape[1]
    assert len(np.unique(ref[0][np.abs(ref[0]) > 1e-6])) > 20 and not np.allclose(ref[0], ref[1], atol=1e-3)
    # Behind a cell, relative: three rsqrt (row, cluster, whole vector), and by dense_reference.bound's rule the sum of
    # a cell (at most ceil(200 / 24) = 9 points), half of the 3-term and of the 24-term sum of squares under the two
    # later rsqrt, and 7 single roundings (x rinv; v rinv and y rinv with the two roundings of either clamp):
    # 25 + 9.5 + 20 + 7 = 61.5 roundings.  Cells of clusters that nothing selects sit at the clamp (1e-10, absolute).
    n_pts, n_intra, n_cells = -(-case_n // 24), 3, 24
    E = np.abs(ref) * (3 * R.A_RSQ + D.rel_bound(n_pts) + 0.5 * D.rel_bound(n_intra) + 0.5 * D.rel_bound(n_cells)
                       + 7 * R.EPS32) + 1e-10
    _check("aggregate/selection", "w2" if w2 else "plain", got, ref, E)


# ------------------------------------------------------------------------------------------- (b) shapes, (c) clamps
def _run_agg_case(dev, name, case, hp_seed, pairs=((True, 1e-8), (False, 0.0))):
    vl, E, f = R.aggregate(*case, detail=True)
    _check("aggregate", name, _aggregate(dev, *case), vl, E)
    for gating, l2 in pairs:
        hp = R.head_params(R.seed("hp", hp_seed, gating), DM * CL, gating)
        ref, Eo = R.head(f["y"], *hp, l2, tot=f["tot"], E_vlad=f["Ey"], E_tot=f["Etot"])
        _check("fused", "%s gating=%d l2=%g" % (name, gating, l2), _fused(dev, *case, *hp, l2), ref, Eo)
    return vl


@pytest.mark.parametrize("shape", R.AGG_SHAPES, ids=lambda s: "B%d_N%d" % s)
def test_aggregate_and_fused_shapes(dev, shape):
    pairs = ((True, 1e-8), (False, 0.0))
    if shape == (9, 130):                           # both axes in full at one shape: more than one chunk, B past the 8 XCDs
        pairs += ((True, 0.0), (False, 1e-8))
    _run_agg_case(dev, "B%d N%d" % shape, R.agg_case(*shape), shape, pairs)


@pytest.mark.parametrize("kind", R.CLAMP_KINDS)
def test_aggregate_clamps(dev, kind):
    case = R.clamp_case(kind)
    vl = _run_agg_case(dev, kind, case, kind)
    if kind == "zero_att_cloud":                    # closed form: vlad = 0, and out = bn1_shift with gating off (exactly)
        assert not vl[0].any()
        hp = R.head_params(R.seed("hp", kind, False), DM * CL, False)
        assert np.array_equal(_fused(dev, *case, *hp, 0.0)[0], hp[2])
        assert not _aggregate(dev, *case)[0].any()


# ---------------------------------------------------------------------------------------------------- (d) the head
@pytest.mark.parametrize("Kd", R.HEAD_KD)
def test_head_widths(dev, Kd):
    for B in R.HEAD_B:
        for gating, l2 in ((True, 0.0), (False, 1e-8), (True, 1e-8)) if B == 33 else ((True, 1e-8),):
            case = R.head_case(Kd, B, gating)
            ref, E = R.head(*case, l2)
            _check("head", "Kd=%d B=%d gating=%d l2=%g" % (Kd, B, gating, l2), _head(dev, *case, l2), ref, E)


@pytest.mark.parametrize("gating", [True, False])
def test_head_l2_clamp_decides(dev, gating):
    case = R.head_case(256, 33, gating, clamp=True)
    ref, E = R.head(*case, 1e-3)
    pre, _ = R.head(*case, 0.0)
    assert (pre[0] ** 2).sum() < 1e-3 < (pre[1:] ** 2).sum(-1).min()
    _check("head", "clamp gating=%d" % gating, _head(dev, *case, 1e-3), ref, E)


@pytest.mark.parametrize("Kd", [8, 136, 1000, 16384])
def test_head_onehot_rows_return_rows_of_wh(dev, Kd):
    B = min(Kd, 33)
    vlad, Wh, s1, h1, _, _, _ = R.head_case(Kd, B, gating=False)
    vlad[:] = 0
    cols = Kd - 1 - np.arange(B) * max(1, (Kd - 1) // 40)       # from the last column down, across the k slices
    vlad[np.arange(B), cols] = 1.0
    ref = Wh[cols].astype(np.float64) * s1 + h1
    E = 3 * R.EPS32 * (np.abs(Wh[cols] * s1.astype(np.float64)) + np.abs(ref))
    _check("head/onehot", "Kd=%d" % Kd, _head(dev, vlad, Wh, s1, h1, None, None, None, 0.0), ref, E)


@pytest.mark.parametrize("Kd", [4, 100, 102, 16380])
def test_head_refuses_widths_that_are_no_multiple_of_8(dev, Kd):
    vlad, Wh, s1, h1, Wg, s2, h2 = R.head_case(Kd + 8, 3)        # slack behind the claimed shape
    _unsupported(lambda: _head(dev, vlad, Wh, s1, h1, Wg, s2, h2, 0.0, Kd=Kd, slack=4096))
    with pytest.raises(ValueError, match="multiple of 8"):
        _pm().netvlad_head(_t(vlad[:, :Kd], dev), _t(Wh[:Kd], dev), _t(s1, dev), _t(h1, dev), _t(Wg, dev), _t(s2, dev),
                           _t(h2, dev))


# ---------------------------------------------------------------------------------------------------- (e) the walk
@pytest.mark.parametrize("shape", R.WALK_SHAPES, ids=lambda s: "B%d_n%d_m%d_%s_Hd%d" % s)
def test_walk_shapes(dev, shape):
    case = R.walk_case(*shape)
    ref = R.walk_ref(case)
    name = "B%d n%d m%d %s Hd%d" % shape
    planned = _walk(dev, case, order=True, plan=True, zero_accum=1)
    _check_walk(name + " planned", case, planned, ref)
    plain = _walk(dev, case, order=True, plan=False, zero_accum=0)
    _check_walk(name + " unplanned", case, plain, ref)
    assert np.array_equal(planned[0], plain[0]), "att differs between the planned and the unplanned walk"


@pytest.mark.parametrize("opt", ["no_order_planned", "no_order_unplanned", "no_att", "act_none", "ep_null"])
def test_walk_options(dev, opt):
    shape = (3, 300, 65, "mixed", 256)
    case = R.walk_case(*shape, act=D.ACT_NONE if opt == "act_none" else D.ACT_RELU, ep=opt != "ep_null")
    ref = R.walk_ref(case)
    got = _walk(dev, case, order=not opt.startswith("no_order"), plan=opt != "no_order_unplanned",
                zero_accum=0 if opt == "no_att" else 1, want_att=opt != "no_att")
    _check_walk(opt, case, got, ref)


def test_walk_refusals(dev):
    case = R.walk_case(1, 40, 1024, "nn")
    case["coarse"] = np.concatenate([case["coarse"], case["coarse"][:, :1]], 1)     # 1025 valid rows
    case["m"] = 1025
    _unsupported(lambda: _walk(dev, case, plan=False))
    _unsupported(lambda: _pm().walk_plan(_t(case["idx"], dev), _t(case["dist"], dev), None, 1025))
    small = R.walk_case(1, 40, 5, "nn", Hd=512)
    _unsupported(lambda: _walk(dev, small, Hd=300))
    _unsupported(lambda: _walk(dev, small, act=D.ACT_SIGMOID))


# ---------------------------------------------------------------------------------------------------- (f) the tail
@pytest.mark.parametrize("m", R.TAIL_M)
def test_tail_assign_rows(dev, m):
    for B in R.TAIL_B if m in (17, 1024) else (9,):
        case = R.tail_case(B, m)
        ref, E = R.tail_assign(*case, 1e-8)
        _check("tail_assign", "B=%d m=%d" % (B, m), _tail(dev, *case, 1e-8), ref, E)


@pytest.mark.parametrize("opt", ["onehot", "zero_cloud", "no_gating"])
def test_tail_assign_options(dev, opt):
    case = R.tail_case(9, 17, gating=opt != "no_gating", zero_cloud=4 if opt == "zero_cloud" else None, onehot=opt == "onehot")
    l2 = 0.0 if opt == "no_gating" else 1e-8
    ref, E, f = R.tail_assign(*case, l2, detail=True)
    got = _tail(dev, *case, l2)
    _check("tail_assign", opt, got, ref, E)
    if opt == "onehot":        # V[b, c] = (1 + c / 64) coarse[b, (c + 3 b) % m], one rounding: the device against the closed form
        apart, coarse, asum, W2 = case[:4]
        rows = (np.arange(CL)[None] + 3 * np.arange(9)[:, None]) % 17
        V = (1 + np.arange(CL) / 64.0)[None, :, None] * coarse.astype(np.float64)[np.arange(9)[:, None], rows]
        f = R._finish(V, R.EPS32 * np.abs(V), asum.astype(np.float64), np.zeros(asum.shape), W2.astype(np.float64),
                      np.float64, ())
        ref, E = R.head(f["y"], *case[4:], l2, tot=f["tot"], E_vlad=f["Ey"], E_tot=f["Etot"])
        _check("tail_assign/onehot", "closed form", got, ref, E)


def test_tail_assign_refuses_m_1025(dev):
    case = R.tail_case(1, 1025)
    _unsupported(lambda: _tail(dev, *case, 0.0))


# --------------------------------------------------------------------------------------------------- (g) end to end
def test_walk_then_tail_end_to_end(dev):
    case = R.walk_case(3, 300, 40, "nn")
    W_att, att_ep, w_fc, b_fc, Wc, sc, sh = case["par"]
    rng = R.seed("e2e")
    W2 = (rng.standard_normal((DM, CL)) / 16).astype(np.float32)
    hp = R.head_params(rng, DM * CL)
    ref = R.walk_ref(case)
    att, apart, asum = _walk(dev, case)
    _check_walk("e2e", case, (att, apart, asum), ref)
    out = _tail(dev, apart, case["coarse"], asum, W2, *hp, 1e-8)
    r1, E1 = R.tail_assign(ref[2], case["coarse"], ref[4], W2, *hp, 1e-8, E_apart=ref[3], E_asum=ref[5])
    _check("e2e/out", "walk+tail", out, r1, E1)
    up, Tup = D.three_interpolate_idw(case["coarse"], case["idx"], case["dist"])
    r2, E2 = R.fused(up, ref[0], Wc, sc, sh, W2, *hp, 1e-8)
    _check("e2e/out", "against fused on the up-sampled map", out, r2, E1 + E2)


def test_zz_report_worst_ratios():
    for k in sorted(_WORST, key=lambda k: -_WORST[k][0]):
        print("WORST %-22s %.4f  (%s)" % (k, _WORST[k][0], _WORST[k][1]))
    assert _WORST and all(v[0] <= 1.0 for v in _WORST.values())
