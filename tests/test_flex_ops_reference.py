"""CPU: the float64 yardstick of the drop-in flex operators (tests/flex_ops_reference.py) is pinned to the C oracle, its
case builders keep their rules, and -- from the reference alone -- the GPU test built on it has the power it claims: the
other centre rule, a dropped last neighbour and a multiply-first coordinate difference all land far outside the bounds the
GPU assertions use."""
import os

import numpy as np
import pytest
import torch

import flex_ops_reference as R

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONV_KEYS = ("f", "p", "nbr", "theta", "bias")


def _np(c, *keys):
    return [c[k].numpy() for k in keys]


def _indegree(nbr):
    """The most list entries that name one point of one cloud."""
    B, K, N = nbr.shape
    return int(max(np.bincount(nbr[b].reshape(-1).numpy(), minlength=N).max() for b in range(B)))


def _check_conv_against_oracle(oracle, c):
    """The oracle evaluates the same sums in float32, in the reference's order: within (number of terms) u T of float64."""
    B, Din, N = c["f"].shape
    Dp, K, Dout = c["p"].shape[1], c["nbr"].shape[1], c["theta"].shape[2]
    ref, T = R.flex_conv(*[c[k] for k in CONV_KEYS])
    got = oracle.flex_convolution(*_np(c, "f", "p", "nbr", "theta", "bias"), True)
    r = dict(out=R.ulp_ratio(torch.from_numpy(got), ref, T) / ((Dp + 1) * K * Din))
    refs, Ts = R.flex_conv_grads(*[c[k] for k in CONV_KEYS], c["dout"])
    gots = oracle.flex_convolution_grad(*_np(c, "f", "p", "nbr", "theta", "bias", "dout"))
    terms = dict(df=_indegree(c["nbr"]) * (Dp + 1) * Dout, dtheta=B * N * K, dbias=B * N * K)
    for name, g, e, t in zip(("df", "dtheta", "dbias"), gots, refs, Ts):
        r[name] = R.ulp_ratio(torch.from_numpy(g), e, t) / terms[name]
    print("flex_conv oracle / (terms u T):", {k: round(v, 4) for k, v in r.items()})
    assert max(r.values()) <= 1.0, r


def test_flex_conv_reference_agrees_with_the_oracle(oracle):
    g = dict(np.load(os.path.join(G, "fake_pointcloud.npz")))
    c = dict(f=g["features"], p=g["position"], nbr=g["neighborhood"].astype(np.int32), theta=g["theta"], bias=g["bias"],
             dout=g["topdiff"])
    _check_conv_against_oracle(oracle, {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in c.items()})
    _check_conv_against_oracle(oracle, R.conv_case(2, 100, 5, 16, 24, lists_kind="knn"))
    # the oracle's gradient centres on rank 0 too: a foreign rank 0 must not part them
    _check_conv_against_oracle(oracle, R.conv_case(2, 100, 5, 16, 24, lists_kind="adversarial"))


def test_conv_pointset_reference_agrees_with_the_oracle(oracle):
    for kind in ("knn", "adversarial", "hub0"):
        c = R.pointset_case(2, 100, 12, 7, 9, lists_kind=kind)
        (B, Din, N), K, Dout = c["f"].shape, c["nbr"].shape[1], c["theta"].shape[1]
        ref, T = R.conv_pointset(c["f"], c["nbr"], c["theta"], c["bias"])
        got = oracle.convolution_pointset(*_np(c, "f", "nbr", "theta", "bias"))
        r = dict(out=R.ulp_ratio(torch.from_numpy(got), ref, T) / (K * Din + 1))
        refs, Ts = R.conv_pointset_grads(c["f"], c["nbr"], c["theta"], c["bias"], c["dout"])
        gots = oracle.convolution_pointset_grad(*_np(c, "f", "nbr", "theta", "dout"))
        rank0 = int(max(np.bincount(c["nbr"][b, 0].numpy(), minlength=N).max() for b in range(B)))
        terms = dict(df=(_indegree(c["nbr"]) + K * rank0) * Dout, dtheta=B * N * K, dbias=B * N)
        for name, g, e, t in zip(("df", "dtheta", "dbias"), gots, refs, Ts):
            r[name] = R.ulp_ratio(torch.from_numpy(g), e, t) / terms[name]
        print("conv_pointset %s oracle / (terms u T):" % kind, {k: round(v, 4) for k, v in r.items()})
        assert max(r.values()) <= 1.0, (kind, r)


def test_flex_pool_reference_is_the_oracles_rule(oracle):
    """Values and argmax equal the oracle's bit for bit, on ties, -inf, NaN and lists of nothing else; the scatter is the
    oracle's within (contributions) u T."""
    c = R.pool_case(2, 257, 8, 5)
    val, arg = R.flex_pool(c["f"], c["nbr"])
    oval, oarg = oracle.flex_pooling(*_np(c, "f", "nbr"))
    assert np.array_equal(val, oval) and np.array_equal(arg, oarg)
    assert not np.isnan(val).any() and np.isfinite(val).all()
    lowest = -np.finfo(np.float32).max
    for n in R.POOL_EMPTY:
        assert (val[:, :, n] == lowest).all() and (arg[:, :, n] == 0).all()
    assert ((val == lowest).sum(), (val == lowest).all(1).sum()) == (2 * 5 * 3, 2 * 3)   # and nowhere else
    B, D, N = val.shape
    cand = c["f"].numpy()[np.arange(B)[:, None, None, None], np.arange(D)[None, :, None, None],
                          c["nbr"].numpy()[:, None, :, :]]                                # [B,D,K,N]
    assert ((cand == val[:, :, None, :]).sum(2) > 1).mean() > 0.3                         # ties on most entries
    hub = (arg == N - 1).reshape(B, -1).sum(1)
    assert (hub > N).all(), hub                                                           # the hub wins > N entries
    din, T, cnt = R.flex_pool_grad(c["dout"], arg)
    got = oracle.flex_pooling_grad(c["dout"].numpy(), arg)
    assert R.ulp_ratio(torch.from_numpy(got), din, T * cnt.clamp(min=1)) <= 1.0
    # double: a list of nothing gives double's lowest
    v64, a64 = R.flex_pool(c["f"].double(), c["nbr"])
    assert np.array_equal(a64, arg) and (v64[:, :, 20] == -np.finfo(np.float64).max).all()
    keep = val != lowest
    assert np.array_equal(v64[keep], val[keep].astype(np.float64))


# ------------------------------------------------------------------------------------------------------- the builders
def test_case_builders_keep_their_rules():
    seen = set()
    for plan, B, N, K, Din, Dout, Dp, kind, ckind in R.CONV_CASES + R.F64_CONV_CASES:
        assert (B * N) % 64 != 0 and (B * N) % 32 != 0                 # ragged: every launch ends in a partial tile
        c = R.conv_case(B, N, K, Din, Dout, Dp, kind, ckind)
        nbr = c["nbr"]
        assert nbr.shape == (B, K, N) and nbr.dtype == torch.int32 and c["p"].shape == (B, Dp, N)
        assert int(nbr.min()) >= 0 and int(nbr.max()) < N
        lo, hi = (1000.0, 1060.0) if ckind == "offset" else (0.0, R.EXTENT)
        assert float(c["p"].min()) >= lo and float(c["p"].max()) <= hi
        seen.add((plan, kind, ckind))
        for group in (plan, 0):                                       # a bound above the number of terms tests nothing
            assert R.BOUNDS[group]["out"] <= (Dp + 1) * K * Din and R.BOUNDS[group]["df"] <= (Dp + 1) * Dout
        if kind != "adversarial":
            if kind == "knn":
                assert not R.foreign(nbr).any()
            continue
        if R.adversarial_applies(N, K):
            assert R.foreign(nbr).float().mean() >= 0.3, (B, N, K)
            assert (nbr[:, K - 1, :] == N - 1).all()                    # the hub, in the partial last tile of its cloud
            assert not any((nbr == r).any() for r in R.REMOVED)
            if K >= 6:
                assert (nbr[:, 3:6, 2::5] == nbr[:, 1:2, 2::5]).all()
        else:                                                           # K = 1 or N = 1: random lists (N = 1: all 0)
            assert K == 1 or N == 1
            gen = torch.Generator().manual_seed(R._seed(B, N, K, Din, Dout, Dp, len(kind), len(ckind)))
            assert torch.equal(nbr, R.lists("random", R.cloud(B, N, Dp, ckind, gen), K, gen))
            assert N > 1 or not nbr.any()
    for plan in (0, 1, 2, 3):                                           # what each plan is promised
        assert {(plan, "knn", "rand"), (plan, "random", "rand"), (plan, "adversarial", "offset")} <= seen
    assert not R.adversarial_applies(1, 1) and not R.adversarial_applies(129, 1) and not R.adversarial_applies(8, 8)
    assert not R.adversarial_applies(9, 2) and R.adversarial_applies(10, 2)
    for B, N, K, Din, Dout, kind in R.POINTSET_CASES:
        nbr = R.pointset_case(B, N, K, Din, Dout, kind)["nbr"]
        assert R.foreign(nbr).float().mean() >= 0.3
        if kind == "hub0":
            assert not nbr[:, 0, :].any()


# --------------------------------------------------------------------------------------------------------- the power
ADVERSARIAL = [c for c in R.CONV_CASES if c[7] == "adversarial" and R.adversarial_applies(c[2], c[3])]


def _per_point(x):
    """[B,C,N] -> [B,N]: the worst entry of each point."""
    return x.max(1).values


@pytest.mark.parametrize("case", ADVERSARIAL, ids=lambda c: "p%d-%dx%d-k%d-%dto%d-dp%d-%s" % (c[:7] + (c[8],)))
def test_wrong_centre_and_dropped_neighbour_are_far_outside_the_bounds(case):
    """What the GPU assertions (`worst ratio <= bound`) would see of the two defects the old suite let through, per point
    whose rank-0 entry is not the point itself -- the worst of that point's own entries, since one entry over the bound
    fails the test: the forward centred on rank 0, and the feature gradient centred on the point (what that point alone
    adds to the rows its list names), each >= 100 x the bound at EVERY such point and >= 1e4 x at the median; a last
    neighbour dropped from one point of the partial last tile moves that point's outputs by > 10 x the bound.  The case
    runs under its own plan and, with FAST_PATH off, under plan 0: the larger bound of the two counts.  Measured over
    the cases: forward >= 6.6e4 at every such point and >= 1.8e6 at the median, df >= 2.5e4 and >= 8.3e5, the dropped
    neighbour >= 2.8e4, against bounds of at most 21.1."""
    plan, B, N, K, Din, Dout, Dp, kind, ckind = case
    c = R.conv_case(B, N, K, Din, Dout, Dp, kind, ckind)
    args = [c[k] for k in CONV_KEYS]
    bound = {q: max(R.BOUNDS[plan][q], R.BOUNDS[0][q]) for q in ("out", "df")}
    far = R.foreign(c["nbr"])
    assert far.float().mean() >= 0.3
    ref, T = R.flex_conv(*args)
    swapped, _ = R.flex_conv(*args, centre_swapped=True)
    fwd = _per_point((swapped - ref).abs() / (R.U * T))[far]
    (_, _, _), (Tdf, _, _) = R.flex_conv_grads(*args, c["dout"])
    shift = R.flex_conv_centre_shift(c["p"], c["nbr"], c["theta"], c["dout"])               # [B,N,Din]
    Trows = R.gather(Tdf.transpose(1, 2).contiguous(), c["nbr"].transpose(1, 2))              # [B,N,K,Din]
    df = (shift.abs().unsqueeze(2) / (R.U * Trows)).amax((2, 3))[far]
    # a row of the partial last tile (of 32 and of 64 points): the hub's neighbour B N - 2 where the tile holds it
    b, n = B - 1, N - (2 if (B * N) % 32 >= 2 else 1)
    assert 0 < B * N - (b * N + n) <= (B * N) % 32 <= (B * N) % 64
    last = R.flex_conv_last_term(*args, b, n)
    drop = float((last.abs() / (R.U * T[b, :, n])).max())
    print("power %s: forward min %.3g median %.3g, df min %.3g median %.3g, dropped neighbour %.3g (in u T)"
          % (case, fwd.min(), fwd.median(), df.min(), df.median(), drop))
    assert float(fwd.min()) >= 100 * bound["out"] and float(fwd.median()) >= 1e4 * bound["out"]
    assert float(df.min()) >= 100 * bound["df"] and float(df.median()) >= 1e4 * bound["df"]
    assert drop > 10 * bound["out"]


@pytest.mark.parametrize("case", R.POINTSET_CASES, ids=lambda c: "%dx%d-k%d-%dto%d-%s" % c)
def test_pointset_wrong_centre_is_far_outside_the_bounds(case):
    """conv_pointset centred on the point itself instead of on rank 0: the forward of every foreign point and the rows
    that take its -K acc."""
    c = R.pointset_case(*case)
    far = R.foreign(c["nbr"])
    args = (c["f"], c["nbr"], c["theta"], c["bias"])
    ref, T = R.conv_pointset(*args)
    swapped, _ = R.conv_pointset(*args, centre_swapped=True)
    fwd = _per_point((swapped - ref).abs() / (R.U * T))[far]
    (rdf, _, _), (Tdf, _, _) = R.conv_pointset_grads(*args, c["dout"])
    (sdf, _, _), _ = R.conv_pointset_grads(*args, c["dout"], centre_swapped=True)
    named = Tdf > 0                                              # (the ids no list names stay exactly 0 under rank 0)
    df = float(((sdf - rdf).abs()[named] / (R.U * Tdf[named])).max())
    bound = R.BOUNDS["pointset"]
    print("pointset power %s: forward min %.3g median %.3g, df worst %.3g" % (case, fwd.min(), fwd.median(), df))
    assert float(fwd.min()) >= 100 * bound["out"] and float(fwd.median()) >= 1e4 * bound["out"]
    assert df >= 1e4 * bound["df"]


# --------------------------------------------------------------------------------------------------- the offset cloud
def _flex_conv_f32(c, expand):
    """float32 numpy evaluation of the forward in the factorised form the fast kernels use.  expand=True multiplies first
    and subtracts afterwards -- Sd = sum_k p[nk,d] f[nk,i] - p[n,d] S0[i], the sum over i of theta . p[nk] f - theta . p[n] f
    -- instead of Sd = sum_k (p[nk,d] - p[n,d]) f[nk,i]."""
    f, p, nb = (np.ascontiguousarray(c[k].numpy().transpose(0, 2, 1)) for k in ("f", "p", "nbr"))
    bi = np.arange(f.shape[0])[:, None, None]
    g, gp = f[bi, nb], p[bi, nb]                                 # [B,N,K,Din], [B,N,K,Dp]
    S0 = g.sum(2, dtype=np.float32)
    if expand:
        Sd = np.einsum("bnkd,bnki->bndi", gp, g) - p[:, :, :, None] * S0[:, :, None, :]
    else:
        Sd = np.einsum("bnkd,bnki->bndi", gp - p[:, :, None, :], g)
    out = S0 @ c["bias"].numpy() + np.einsum("bndi,dio->bno", Sd, c["theta"].numpy())
    assert out.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(out.transpose(0, 2, 1)))


OFFSET = [c for c in R.CONV_CASES if c[8] == "offset"]


@pytest.mark.parametrize("case", OFFSET, ids=lambda c: "p%d-%dx%d-k%d-%dto%d" % c[:6])
def test_offset_cloud_catches_a_multiply_first_kernel(case):
    """Coordinates near 1000 with neighbour distances of a few units: p[nk] - p[n] is exact or nearly so in float32, while
    products taken first round at the size of the coordinates.  T is that of the differences, so on every offset case of
    the GPU test the multiply-first form leaves the largest bound the case runs under (its plan's and plan 0's): the
    worst entry by > 4 x, and the worst entry of the median POINT by > 1 x; the subtract-first float32 form stays inside
    the smallest.  Measured here: multiply first 99 .. 304 u T at the worst entry, 26 .. 46 at the median point's worst
    and 6.7 .. 12.1 at the median ENTRY; subtract first 2.5 .. 3.8 at the worst entry.  The median entry is NOT above
    the bounds of plans 0 and 1 (21.1, 17.4): rounding errors add up like sqrt(3 K Din) and T like 3 K Din, which
    leaves ~1000 / (sqrt(3 K Din) |dp|) ~ 10 however dense the cloud's lists are; what fails the GPU assertion is the
    worst entry."""
    plan, B, N, K, Din, Dout, Dp, kind, ckind = case
    c = R.conv_case(B, N, K, Din, Dout, Dp, kind, ckind)
    ref, T = R.flex_conv(*[c[k] for k in CONV_KEYS])
    r = {}
    for expand in (False, True):
        e = (R.f64(_flex_conv_f32(c, expand)) - ref).abs() / (R.U * T)
        r[expand] = (float(e.median()), float(_per_point(e).median()), float(e.max()))
    print("offset cloud %s, float32 forward in u T (median entry, median point's worst, worst): subtract first %s, "
          "multiply first %s" % (case, r[False], r[True]))
    hi, lo = (f(R.BOUNDS[plan]["out"], R.BOUNDS[0]["out"]) for f in (max, min))
    assert r[True][2] > 4 * hi and r[True][1] > hi
    assert r[False][2] <= lo
