"""GPU: the BatchNorm family and the global head's training kernels of csrc/train.hip, entry point by entry point through
the C ABI, against the float64 restatements of tests/global_training_reference.py evaluated (on the device) on exactly
the f32 inputs the kernel got: |got - ref| <= RTOL * T + 1e-30 everywhere (commuted_reference.RTOL, T the reference's
error scale); counts, gates, masked rows and running buffers at count 0 are compared exactly.  Power: for every reducing
kernel, dropping the last row of a partial chunk from the reference moves some entry -- and some entry of the last
64-column block -- by more than that bound.  The shapes are the smallest at which each launch geometry can still go
wrong (train.hip's launchers): row chunks of 128 up to the 1024-chunk cap, 64-column blocks, the grid caps of the flat
and the row-walking kernels, chunks that straddle clouds, one row per cloud, the 64-row limit of the short form.

The gate-agreement tests place every input within 4 ulp of a site's ReLU threshold and read each pass's gates out
bit for bit: forward, backward apply, backward sums (through sums of powers of two) and the short form must all take
the float64-exact sign of fmaf(x, scale, shift); the commuted sums / apply walks must agree with each other.

Measured on the MI355X: worst |got - ref| / (T + 1e-30 / RTOL) per entry point over all cases (the bound is 1e-5);
test_zz_report_worst_ratios prints the table per output.
    bn_colstats 8.8e-08 (sumsq, R 127, C 1024)          bn_bwd_sums 5.9e-08 (rank-one S1, R 1, C 1024)
    bn_finalize[_parts] 1.1e-07 (run_var)               bn_bwd_finalize[_parts] 2.4e-07 (k2, count 1)
    scale_shift_act 5.9e-08, _res 1.1e-07 (16400 x 1024) bn_bwd_apply 1.1e-07 (both forms, 4097 x 1024)
    bn_small_fwd / _bwd 1.1e-07 (run_var); y 4.1e-08, dx 3.9e-08, dgamma 2.5e-08, dbeta 5.9e-08;
        against the long form on the same input 8.0e-08 (run_var), dx 3.1e-08, dbeta 7.4e-08
    row_logit_sigmoid 8.1e-08   sigmoid_bwd 3.7e-08 (dlogit), 7.9e-09 (sum)   context_gate 6.6e-08 (dv)
    netvlad_assign_rows 5.8e-08 (a), 2.1e-08 (asum)     netvlad_assign_rows_bwd 4.0e-08 (dz), 1.6e-08 (datt)
    l2norm_rows_bwd 5.3e-08     vlad_normalize 7.7e-08 (inv_c), 3.9e-08 (dV), 2.2e-08 (dW2)
    quadruplet_loss 1.8e-08 (loss), 1.2e-07 (grad)
    attention_head node 1.2e-09 (dX), 6.4e-08 (run_mean)   netvlad_assign node 2.2e-09 (datt), 9.9e-08 (run_var)
Gates, of elements within 4 ulp of their threshold: with bn_bwd_sums and the commuted sums walk deciding the gate by
fmaf((x - mean) * rstd, gamma, beta) > 0 (as they did before this module was written), bn_bwd_sums disagreed with the
float64 gate on 121 of 1536 (C 64) and 1679 of 24576 (C 1024) elements in both of its forms, and the commuted sums walk
with the commuted apply walk on 412 of 6144 (Hd 256) and 1859 of 24576 (Hd 1024); forward, bn_bwd_apply and bn_small:
0.  With every pass folding (scale, shift) through dh3d_bn_fold and gating on fmaf(x, scale, shift) > 0: 0 everywhere.
"""
import pytest
import torch

import commuted_reference as CR
import global_training_reference as G

pytestmark = pytest.mark.gpu

NAN = float("nan")
UNSUPPORTED = 2
F64 = torch.float64
_WORST = {}


def _L():
    from dh3d_amd import _lib as L
    return L


def _status(name, *args):
    L = _L()
    return getattr(L.lib(), name)(*[L.ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args]
                                  + [L.stream_ptr()])


def _call(name, *args):
    _L().check(_status(name, *args), name)


def _close(name, got, ref, sel=None, case=""):
    """got (f32 / f64 device tensor) against the E `ref` within RTOL * T; records the worst |got - ref| / T."""
    v, t = ref.v.reshape(got.shape), ref.t.reshape(got.shape)
    got = got.double()
    if sel is not None:
        got, v, t = got[sel], v[sel], t[sel]
    if got.numel() == 0:
        return
    assert bool(torch.isfinite(got).all()), (name, case, "non-finite output")
    dev = (got - v).abs()
    ratio = float((dev / (t + 1e-30 / CR.RTOL)).max())            # (relative to the whole bound: RTOL * T + 1e-30)
    if ratio > _WORST.get(name, (0.0, ""))[0] or name not in _WORST:
        _WORST[name] = (ratio, str(case))
    bad = dev > CR.RTOL * t + 1e-30
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError("%s %s: %d entries off, first at %d: got %.9e ref %.9e T %.3e; worst |got-ref|/T %.2e" % (
            name, case, int(bad.sum()), i, float(got.reshape(-1)[i]), float(v.reshape(-1)[i]), float(t.reshape(-1)[i]),
            ratio))


def _power(name, ref, dropped, case="", last_block=True):
    """Dropping a row moves some entry of `ref` (an E [.., C]) by more than the bound -- in the last 64-column block too."""
    move = (ref.v - dropped.v).abs() / (CR.RTOL * ref.t + 1e-30)
    assert float(move.max()) > 1.0, (name, case, float(move.max()))
    if last_block:
        C = ref.v.shape[-1]
        assert float(move[..., (C - 1) // 64 * 64:].max()) > 1.0, (name, case, "last column block")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _mask(clouds, padding, g):
    m = torch.ones(clouds, dtype=torch.bool)
    if padding == "first":
        m[0] = False
    elif padding == "middle":
        m[clouds // 2] = False
    elif padding == "last":
        m[-1] = False
    elif padding == "all_but_one":
        m[:] = False
        m[clouds // 2] = True
    elif padding == "all":
        m[:] = False
    elif padding == "random":
        m = torch.rand(clouds, generator=g) < 0.6
        m[-1] = True
    return m


# --------------------------------------------------------------------------------- column statistics and backward sums
# (R, C list, rows_per_cloud, padding)
SUMS_CASES = {
    "r1": (1, (4, 60, 64, 68, 1024), 0, None),
    "r127": (127, (4, 60, 64, 68, 1024), 0, None),
    "r128": (128, (4, 60, 64, 68, 1024), 0, None),
    "r129": (129, (4, 60, 64, 68, 1024), 0, None),
    "r777": (777, (4, 60, 64, 68, 1024), 0, None),
    "chunk_cap": (131073, (4,), 0, None),            # 1024 chunks of 129 rows (the last one: 9)
    "straddle_first": (700, (68,), 100, "first"),    # chunks of 117 rows over clouds of 100
    "straddle_middle": (700, (68,), 100, "middle"),
    "straddle_last": (700, (68,), 100, "last"),
    "straddle_all_but_one": (700, (68,), 100, "all_but_one"),
    "straddle_all": (700, (68,), 100, "all"),
    "row_per_cloud": (129, (60,), 1, "random"),
}


def _sums_inputs(R, C, rpc, padding, g, dev):
    x = torch.randn(R, C, generator=g) * 2 + 0.5
    if C > 1:
        x[:, 1] = 30.0 + torch.randn(R, generator=g)           # mean / std = 30: E[x^2] - E[x]^2 cancels 3 digits
    dy = torch.randn(R, C, generator=g)
    rowscale = torch.randn(R, generator=g)
    if R > 1000:                                               # one row of 130k has to show in a sum of 130k terms
        x[-1], dy[-1], rowscale[-1] = 50.0, 50.0, 50.0
    mask = live = None
    if padding is not None:
        mask = _mask((R + rpc - 1) // rpc, padding, g)
        live = G.rows_live(R, mask, rpc)
    return x, dy, rowscale, mask, live


@pytest.mark.parametrize("case", sorted(SUMS_CASES))
def test_colstats_and_bwd_sums_match_float64(dev, case):
    R, Cs, rpc, padding = SUMS_CASES[case]
    g = _gen(sum(map(ord, case)))
    for C in Cs:
        tag = "%s C=%d" % (case, C)
        x, dy, rowscale, mask, live = _sums_inputs(R, C, rpc, padding, g, dev)
        x, dy, rowscale = x.to(dev), dy.to(dev), rowscale.to(dev)
        m8 = None if mask is None else mask.to(torch.uint8).to(dev)
        live = None if live is None else live.to(dev)
        drop = int(live.nonzero()[-1]) if live is not None and bool(live.any()) else R - 1
        x[drop] = x[drop].abs() + 3.0                          # the row that is dropped below: most of its gates are open
        keep = torch.ones(R, dtype=torch.bool, device=dev) if live is None else live.clone()
        keep[drop] = False
        can_drop = live is None or bool(live.any())
        x_in, dy_in, rs_in = x, dy, rowscale
        if live is not None:                                   # a padding cloud's rows are never read
            x_in, dy_in, rs_in = x.clone(), dy.clone(), rowscale.clone()
            x_in[~live], dy_in[~live], rs_in[~live] = NAN, NAN, NAN

        acc = torch.zeros(2, C, dtype=F64, device=dev)
        _call("dh3d_bn_colstats", x_in, R, C, m8, rpc, acc[0], acc[1])
        s1, s2 = G.bn_colstats(x, live)
        _close("bn_colstats.sum", acc[0], s1, case=tag)
        _close("bn_colstats.sumsq", acc[1], s2, case=tag)
        if live is not None and not bool(live.any()):
            assert float(acc.abs().max()) == 0.0
        if can_drop:
            d1, d2 = G.bn_colstats(x, keep)
            _power("bn_colstats.sum", s1, d1, tag)
            _power("bn_colstats.sumsq", s2, d2, tag)

        # backward sums on the statistics of these rows (as f32, folded as every kernel folds them)
        cnt = float(R if live is None else int(live.sum()))
        gamma = (0.5 + torch.rand(C, generator=g)).to(dev)
        beta = (0.3 * torch.randn(C, generator=g)).to(dev)
        st = G.bn_finalize(s1, s2, cnt, gamma, beta, 1e-3, 0.9, True, torch.zeros(C, device=dev), torch.ones(C, device=dev))
        mean, rstd = st["mean"].v.float(), st["rstd"].v.float()
        scale, shift = G.fold(mean, rstd, gamma, beta)
        colvec = torch.randn(C, generator=g).to(dev)
        for relu in (1, 0):
            S = torch.zeros(3, C, dtype=F64, device=dev)
            _call("dh3d_bn_bwd_sums", x_in, dy_in, None, None, R, C, mean, rstd, gamma, beta, relu, m8, rpc, S[0], S[1], None)
            r1, r2, _ = G.bn_bwd_sums(x, mean, rstd, scale, shift, relu, dy=dy, live=live)
            _close("bn_bwd_sums.S1", S[0], r1, case=tag)
            _close("bn_bwd_sums.S2", S[1], r2, case=tag)
            assert float(S[2].abs().max()) == 0.0                      # the dense form leaves S3 alone
            if can_drop and (R > 1 or not relu):
                q1, q2, _ = G.bn_bwd_sums(x, mean, rstd, scale, shift, relu, dy=dy, live=keep)
                _power("bn_bwd_sums.S1", r1, q1, tag, last_block=R > 1)
                if R > 1:                                                      # (one row: xhat = 0)
                    _power("bn_bwd_sums.S2", r2, q2, tag)
            S = torch.zeros(3, C, dtype=F64, device=dev)
            _call("dh3d_bn_bwd_sums", x_in, None, rs_in, colvec, R, C, mean, rstd, gamma, beta, relu, m8, rpc, S[0], S[1],
                  S[2])
            r1, r2, r3 = G.bn_bwd_sums(x, mean, rstd, scale, shift, relu, rowscale=rowscale, colvec=colvec, live=live)
            _close("bn_bwd_sums.rank1.S1", S[0], r1, case=tag)
            _close("bn_bwd_sums.rank1.S2", S[1], r2, case=tag)
            _close("bn_bwd_sums.rank1.S3", S[2], r3, case=tag)
            if live is not None and not bool(live.any()):
                assert float(S.abs().max()) == 0.0
            if can_drop and (R > 1 or not relu):
                q1, q2, q3 = G.bn_bwd_sums(x, mean, rstd, scale, shift, relu, rowscale=rowscale, colvec=colvec, live=keep)
                _power("bn_bwd_sums.rank1.S1", r1, q1, tag, last_block=R > 1)
                _power("bn_bwd_sums.rank1.S3", r3, q3, tag, last_block=R > 1)


# --------------------------------------------------------------------------------------------------- the finalize kernels
def _seq_sum(part):
    """Rows summed in index order, as one thread of the kernel does."""
    a = torch.zeros_like(part[0])
    for p in range(part.shape[0]):
        a = a + part[p]
    return a


@pytest.mark.parametrize("C", [1, 255, 257])
def test_finalize_kernels_match_float64(dev, C):
    g = _gen(40 + C)
    R = 777.0
    gamma, beta = (0.5 + torch.rand(C, generator=g)).to(dev), torch.randn(C, generator=g).to(dev)
    for P in (1, 22):
        for cnt in (0.0, 1.0, 2.0, R):
            for unbiased, mom, eps in ((1, 0.9, 1e-5), (0, 0.999, 1e-3)):
                tag = "C=%d P=%d n=%g unbiased=%d" % (C, P, cnt, unbiased)
                n = max(cnt, 1.0)
                mu = torch.randn(C, generator=g, dtype=F64)
                var = torch.rand(C, generator=g, dtype=F64) + 0.1
                s1, s2 = n * mu, n * (var + mu * mu)
                if cnt == 1.0:
                    s2 = s1 * s1                                       # one row: its variance is 0
                s1[0], s2[0] = 3.0 * n, 9.0 * n * (1 - 1e-15)          # a constant column: the variance rounds below 0
                if cnt == 0.0:
                    s1, s2 = s1 * 0, s2 * 0
                w = torch.rand(P, 1, generator=g, dtype=F64)
                w = w / w.sum()
                part = torch.stack([s1 * w, s2 * w]).to(dev).contiguous()          # [2, P, C]
                cn = torch.full((1,), cnt, dtype=F64, device=dev)
                rm0, rv0 = torch.randn(C, generator=g).to(dev), torch.rand(C, generator=g).to(dev)
                rm, rv = rm0.clone(), rv0.clone()
                out = torch.full((4, C), NAN, device=dev)
                _call("dh3d_bn_finalize_parts", part, P, cn, gamma, beta, eps, mom, unbiased, rm, rv, C, out[0], out[1],
                      out[2], out[3])
                t1, t2 = _seq_sum(part[0]), _seq_sum(part[1])
                ref = G.bn_finalize(G.E(t1).exact(), G.E(t2).exact(), cnt, gamma, beta, eps, mom, unbiased, rm0, rv0)
                for i, k in enumerate(("mean", "rstd", "scale", "shift")):
                    _close("bn_finalize." + k, out[i], ref[k], case=tag)
                sc, sh = G.fold(out[0], out[1], gamma, beta)
                assert torch.equal(sc, out[2]) and torch.equal(sh, out[3]), tag       # folded as the reference folds
                if cnt == 0.0:
                    assert torch.equal(rm, rm0) and torch.equal(rv, rv0), tag          # left alone, bit for bit
                else:
                    _close("bn_finalize.run_mean", rm, ref["run_mean"], case=tag)
                    _close("bn_finalize.run_var", rv, ref["run_var"], case=tag)
                assert float((out[1, 0].double() - G.f32(eps) ** -0.5).abs()) <= 1e-6 * G.f32(eps) ** -0.5, tag
                # the plain entry point on the summed rows: the same bits
                rm2, rv2 = rm0.clone(), rv0.clone()
                out2 = torch.full((4, C), NAN, device=dev)
                _call("dh3d_bn_finalize", t1, t2, cn, gamma, beta, eps, mom, unbiased, rm2, rv2, C, out2[0], out2[1],
                      out2[2], out2[3])
                assert torch.equal(out, out2) and torch.equal(rm, rm2) and torch.equal(rv, rv2), tag

                # backward
                for nk in (2, 3):
                    bp = (torch.randn(nk, P, C, generator=g, dtype=F64) * 5).to(dev)
                    mean, rstd = out[0], out[1]
                    k = torch.full((2, C), NAN, device=dev)
                    grads = torch.full((nk, C), NAN, device=dev)
                    _call("dh3d_bn_bwd_finalize_parts", bp, nk, P, cn, mean, rstd, gamma, C, k[0], k[1], grads)
                    sums = torch.stack([_seq_sum(bp[j]) for j in range(nk)])
                    assert torch.equal(grads, sums.float()), tag                       # the sums themselves, as f32
                    rb = G.bn_bwd_finalize(G.E(sums[0]).exact(), G.E(sums[1]).exact(), cnt, mean, rstd, gamma)
                    _close("bn_bwd_finalize.k2", k[0], rb["k2"], case=tag)
                    _close("bn_bwd_finalize.k3", k[1], rb["k3"], case=tag)
                    k1 = torch.full((2, C), NAN, device=dev)
                    _call("dh3d_bn_bwd_finalize", sums[0].contiguous(), sums[1].contiguous(), cn, mean, rstd, gamma, C,
                          k1[0], k1[1])
                    assert torch.equal(k, k1), tag


# ------------------------------------------------------------------------------------------------- scale_shift_act[_res]
@pytest.mark.parametrize("R,C", [(5, 4), (777, 68), (16400, 1024)])      # 16400 x 256 float4: past the 16384-block cap
def test_scale_shift_act_matches_float64(dev, R, C):
    g = _gen(R + C)
    x = torch.randn(R, C, generator=g).to(dev)
    scale, shift = torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    res = torch.randn(R, C, generator=g).to(dev)
    for relu in (0, 1):
        tag = "%dx%d relu=%d" % (R, C, relu)
        y = torch.full_like(x, NAN)
        _call("dh3d_scale_shift_act", x, R, C, scale, shift, relu, y)
        _close("scale_shift_act", y, G.scale_shift_act(x, scale, shift, relu), case=tag)
        if relu:
            assert torch.equal(y > 0, G.gate(x, scale, shift)), tag
        y2 = torch.full_like(x, NAN)
        _call("dh3d_scale_shift_act_res", x, R, C, scale, shift, relu, res, y2)
        _close("scale_shift_act_res", y2, G.scale_shift_act(x, scale, shift, relu, res), case=tag)
        y3 = torch.full_like(x, NAN)
        _call("dh3d_scale_shift_act_res", x, R, C, scale, shift, relu, None, y3)
        assert torch.equal(y3, y), tag
        xa = x.clone()
        _call("dh3d_scale_shift_act", xa, R, C, scale, shift, relu, xa)               # out aliasing x
        assert torch.equal(xa, y), tag
    assert _status("dh3d_scale_shift_act", x, R, 6, scale, shift, 1, y) == UNSUPPORTED


# ----------------------------------------------------------------------------------------------------------- bn_bwd_apply
# C -> rows per block pass 256 / (C / 4); R just past 4096 passes where the grid-stride loop has to run
@pytest.mark.parametrize("R,C,rpc", [(4096 * 256 + 1, 4, 4099), (100, 64, 7), (37, 256, 5), (4097, 1024, 241)])
def test_bn_bwd_apply_matches_float64(dev, R, C, rpc):
    g = _gen(R % 1000 + C)
    x, dy = torch.randn(R, C, generator=g).to(dev), torch.randn(R, C, generator=g).to(dev)
    rowscale, colvec = torch.randn(R, generator=g).to(dev), torch.randn(C, generator=g).to(dev)
    scale, shift = torch.randn(C, generator=g).to(dev), 0.5 * torch.randn(C, generator=g).to(dev)
    k2, k3 = 0.1 * torch.randn(C, generator=g).to(dev), 0.1 * torch.randn(C, generator=g).to(dev)
    clouds = (R + rpc - 1) // rpc
    for padding in (None, "first", "middle", "last"):
        mask = None if padding is None else _mask(clouds, padding, g).to(dev)
        live = None if mask is None else G.rows_live(R, mask, rpc)
        m8 = None if mask is None else mask.to(torch.uint8)
        x_in, dy_in, rs_in = x.clone(), dy.clone(), rowscale.clone()
        if live is not None:
            x_in[~live], dy_in[~live], rs_in[~live] = NAN, NAN, NAN
        for relu in ((0, 1) if padding in (None, "middle") else (1,)):
            tag = "%dx%d %s relu=%d" % (R, C, padding, relu)
            ref = G.bn_bwd_apply(x, scale, shift, k2, k3, relu, dy=dy, live=live)
            dx = torch.full_like(x, NAN)
            _call("dh3d_bn_bwd_apply", x_in, dy_in, None, None, R, C, scale, shift, k2, k3, relu, m8, rpc, dx)
            _close("bn_bwd_apply", dx, ref, case=tag)
            if live is not None:
                assert float(dx[~live].abs().max()) == 0.0, tag                        # exact zeros, x = NaN there
            for alias in ("x", "dy"):                                                  # in place
                xa, da = x_in.clone(), dy_in.clone()
                _call("dh3d_bn_bwd_apply", xa, da, None, None, R, C, scale, shift, k2, k3, relu, m8, rpc,
                      xa if alias == "x" else da)
                assert torch.equal(xa if alias == "x" else da, dx), (tag, alias)
            ref = G.bn_bwd_apply(x, scale, shift, k2, k3, relu, rowscale=rowscale, colvec=colvec, live=live)
            xa = x_in.clone()
            _call("dh3d_bn_bwd_apply", xa, None, rs_in, colvec, R, C, scale, shift, k2, k3, relu, m8, rpc, xa)
            _close("bn_bwd_apply.rank1", xa, ref, case=tag)
            if live is not None:
                assert float(xa[~live].abs().max()) == 0.0, tag


def test_bn_bwd_apply_refuses_other_widths(dev):
    for C in (320, 2048):
        x = torch.randn(8, C, device=dev)
        v = torch.ones(C, device=dev)
        dx = torch.full_like(x, 7.0)
        assert _status("dh3d_bn_bwd_apply", x, x, None, None, 8, C, v, v, v, v, 1, None, 0, dx) == UNSUPPORTED
        torch.cuda.synchronize()
        assert float((dx - 7.0).abs().max()) == 0.0        # nothing was launched


# ------------------------------------------------------------------------------------------------------- the short form
@pytest.mark.parametrize("R", [1, 2, 63, 64])
def test_bn_small_matches_float64_and_the_long_form(dev, R):
    g = _gen(90 + R)
    for C in (60, 256, 320):
        for padding in (None, "all", "one", "zero"):
            for relu, unbiased, mom, eps in ((1, 1, 0.9, 1e-5), (0, 0, 0.999, 1e-3)):
                tag = "R=%d C=%d live=%s relu=%d" % (R, C, padding, relu)
                x = (torch.randn(R, C, generator=g) * 2 + 0.5).to(dev)
                dy = torch.randn(R, C, generator=g).to(dev)
                gamma, beta = (0.5 + torch.rand(C, generator=g)).to(dev), (0.3 * torch.randn(C, generator=g)).to(dev)
                rm0, rv0 = torch.randn(C, generator=g).to(dev), torch.rand(C, generator=g).to(dev)
                mask = None
                if padding is not None:
                    mask = torch.zeros(R, dtype=torch.bool, device=dev)
                    if padding == "one":
                        mask[R // 2] = True
                    if padding == "all":
                        mask[:] = True
                live = mask
                m8 = None if mask is None else mask.to(torch.uint8)
                x_in, dy_in = x.clone(), dy.clone()
                if live is not None:
                    x_in[~live], dy_in[~live] = NAN, NAN
                lsel = slice(None) if live is None else live
                rm, rv = rm0.clone(), rv0.clone()
                stats, y = torch.full((4, C), NAN, device=dev), torch.full_like(x, NAN)
                _call("dh3d_bn_small_fwd", x_in, R, C, gamma, beta, eps, mom, unbiased, relu, m8, rm, rv, stats, y)
                ref = G.batch_norm_train(x, gamma, beta, eps, mom, bool(unbiased), bool(relu), rm0, rv0, dy, live,
                                         gate32=(stats[2].contiguous(), stats[3].contiguous()))
                for i, k in enumerate(("mean", "rstd", "scale", "shift")):
                    _close("bn_small." + k, stats[i], ref[k], case=tag)
                n = R if live is None else int(live.sum())
                if n == 0:
                    assert torch.equal(rm, rm0) and torch.equal(rv, rv0), tag
                else:
                    _close("bn_small.run_mean", rm, ref["run_mean"], case=tag)
                    _close("bn_small.run_var", rv, ref["run_var"], case=tag)
                _close("bn_small.y", y, ref["y"], sel=lsel, case=tag)
                if relu:
                    assert torch.equal((y > 0)[lsel], G.gate(x, stats[2].contiguous(), stats[3].contiguous())[lsel]), tag
                dx, dgb = torch.full_like(x, NAN), torch.full((2, C), NAN, device=dev)
                _call("dh3d_bn_small_bwd", x_in, dy_in, R, C, gamma, stats, relu, m8, dx, dgb[0], dgb[1])
                _close("bn_small.dx", dx, ref["dx"], case=tag)
                _close("bn_small.dgamma", dgb[0], ref["dgamma"], case=tag)
                _close("bn_small.dbeta", dgb[1], ref["dbeta"], case=tag)
                if live is not None:
                    assert float(dx[~live].abs().max() if bool((~live).any()) else 0.0) == 0.0, tag

                # the long form on the same input: "same arithmetic" -- to RTOL * T of the reference
                acc = torch.zeros(2, C, dtype=F64, device=dev)
                cn = torch.full((1,), float(n), dtype=F64, device=dev)
                _call("dh3d_bn_colstats", x_in, R, C, m8, 1, acc[0], acc[1])
                rm2, rv2, st2 = rm0.clone(), rv0.clone(), torch.full((4, C), NAN, device=dev)
                _call("dh3d_bn_finalize", acc[0], acc[1], cn, gamma, beta, eps, mom, unbiased, rm2, rv2, C, st2[0], st2[1],
                      st2[2], st2[3])
                for i, k in enumerate(("mean", "rstd", "scale", "shift")):
                    _close("bn_small~long." + k, st2[i], G.E(stats[i], ref[k].t), case=tag)
                _close("bn_small~long.run_var", rv2, G.E(rv, ref["run_var"].t + 1e-300), case=tag)
                y2 = torch.full_like(x, NAN)
                _call("dh3d_scale_shift_act", x_in, R, C, st2[2], st2[3], relu, y2)
                if not relu:                                  # (with ReLU a gate may differ where the statistics do)
                    _close("bn_small~long.y", y2, G.E(y, ref["y"].t), sel=lsel, case=tag)
                S = torch.zeros(2, C, dtype=F64, device=dev)
                _call("dh3d_bn_bwd_sums", x_in, dy_in, None, None, R, C, stats[0], stats[1], gamma, beta, relu, m8, 1, S[0],
                      S[1], None)
                _close("bn_small~long.dbeta", S[0], G.E(dgb[1], ref["dbeta"].t), case=tag)
                _close("bn_small~long.dgamma", S[1], G.E(dgb[0], ref["dgamma"].t), case=tag)
                if C == 256:
                    k = torch.full((2, C), NAN, device=dev)
                    _call("dh3d_bn_bwd_finalize", S[0], S[1], cn, stats[0], stats[1], gamma, C, k[0], k[1])
                    dx2 = torch.full_like(x, NAN)
                    _call("dh3d_bn_bwd_apply", x_in, dy_in, None, None, R, C, stats[2], stats[3], k[0], k[1], relu, m8, 1, dx2)
                    _close("bn_small~long.dx", dx2, G.E(dx, ref["dx"].t), case=tag)


def test_bn_small_refuses_more_than_64_rows(dev):
    x = torch.randn(65, 64, device=dev)
    v = torch.ones(64, device=dev)
    stats, y = torch.zeros(4, 64, device=dev), torch.full_like(x, 7.0)
    assert _status("dh3d_bn_small_fwd", x, 65, 64, v, v, 1e-5, 0.9, 1, 1, None, v.clone(), v.clone(), stats, y) == UNSUPPORTED
    assert _status("dh3d_bn_small_bwd", x, x, 65, 64, v, stats, 1, None, y, v.clone(), v.clone()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert float((y - 7.0).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ attention head's passes
@pytest.mark.parametrize("R", [1, 3, 5])
def test_row_logit_sigmoid_matches_float64(dev, R):
    g = _gen(7 + R)
    for C in (4, 256, 260, 1024):
        h = torch.randn(R, C, generator=g).to(dev)
        scale, shift = (0.5 + torch.rand(C, generator=g)).to(dev), (0.5 * torch.randn(C, generator=g)).to(dev)
        w = (torch.randn(C, generator=g) / C ** 0.5).to(dev)
        for b in (0.3, 100.0, -100.0):                          # +-100: saturated, no NaN
            bt = torch.full((1,), b, device=dev)
            att = torch.full((R,), NAN, device=dev)
            _call("dh3d_row_logit_sigmoid", h, R, C, scale, shift, w, bt, att)
            _close("row_logit_sigmoid", att, G.row_logit_sigmoid(h, scale, shift, w, bt), case="R=%d C=%d b=%g" % (R, C, b))
            if b == 100.0:
                assert float(att.min()) == 1.0
            if b == -100.0:
                assert float(att.max()) <= 1e-40
        # power: the last column (past the last full 256-column pass at C = 260) shows in every row
        ref = G.row_logit_sigmoid(h, scale, shift, w, torch.full((1,), 0.3, device=dev))
        h2 = h.clone()
        h2[:, C - 1] = h2[:, C - 1].abs() + 3.0
        w2 = w.clone()
        w2[C - 1] = 0.0
        full, cut = (G.row_logit_sigmoid(h2, scale, shift, ww, torch.full((1,), 0.3, device=dev)) for ww in (w, w2))
        assert float(((full.v - cut.v).abs() / (CR.RTOL * full.t)).min()) > 1.0 or float(w[C - 1].abs()) < 1e-3


@pytest.mark.parametrize("n,rpc", [(1, 1), (1023, 100), (1025, 100), (1024 * 1024 + 5, 4099)])
def test_sigmoid_bwd_matches_float64(dev, n, rpc):
    g = _gen(n % 997)
    datt, att = torch.randn(n, generator=g).to(dev), torch.rand(n, generator=g).to(dev)
    att[0] = 1.0
    if n > 2:
        att[1], att[n // 2] = 0.0, 1.0
        datt[-1] = 1000.0                                        # the last element shows in the sum
        att[-1] = 0.5
    clouds = (n + rpc - 1) // rpc
    for padding in (None, "first", "middle", "last", "all"):
        if padding is not None and clouds == 1 and padding != "all":
            continue
        mask = None if padding is None else _mask(clouds, padding, g).to(dev)
        live = None if mask is None else G.rows_live(n, mask, rpc)
        d_in = datt.clone()
        if live is not None:
            d_in[~live] = NAN
        dl, sm = torch.full((n,), NAN, device=dev), torch.zeros(1, device=dev)
        _call("dh3d_sigmoid_bwd", d_in, att, None if mask is None else mask.to(torch.uint8), rpc, n, dl, sm)
        rd, rs = G.sigmoid_bwd(datt, att, live)
        tag = "n=%d %s" % (n, padding)
        _close("sigmoid_bwd.dlogit", dl, rd, case=tag)
        _close("sigmoid_bwd.sum", sm, rs, case=tag)
        assert float(dl[0]) == 0.0 and (n <= 2 or float(dl[1]) == 0.0), tag           # att exactly 1 and 0
        if live is not None:
            assert float(dl[~live].abs().max() if bool((~live).any()) else 0.0) == 0.0, tag
        if n > 2 and (live is None or bool(live[-1])):
            keep = torch.ones(n, dtype=torch.bool, device=dev) if live is None else live.clone()
            keep[-1] = False
            _power("sigmoid_bwd.sum", G.E(rs.v.reshape(1), rs.t.reshape(1)),
                   G.E(G.sigmoid_bwd(datt, att, keep)[1].v.reshape(1)), tag, last_block=False)


# ---------------------------------------------------------------------------------------------------- NetVLAD assignment
def _assign_inputs(R, g, dev, spread):
    s = torch.randn(R, 64, generator=g)
    scale, shift = 1.0 + 2 * torch.rand(64, generator=g), 0.5 * torch.randn(64, generator=g)
    if spread:                                                   # logits spread to +-60
        scale = scale * 20.0 / 3.0
        s = s.clamp(-3.0, 3.0)
    att = 0.25 + 0.75 * torch.rand(R, generator=g)
    att[::5] = 0.0                                               # att = 0 rows
    return s.to(dev), scale.to(dev), shift.to(dev), att.to(dev)


@pytest.mark.parametrize("spread", [False, True])
def test_netvlad_assign_rows_match_float64(dev, spread):
    g = _gen(21 + spread)
    for R in (1, 63, 64, 65):
        s, scale, shift, att = _assign_inputs(R, g, dev, spread)
        a = torch.full((R, 64), NAN, device=dev)
        _call("dh3d_netvlad_assign_rows", s, R, 64, scale, shift, att, a, None, 0)
        ra, _, _ = G.netvlad_assign_rows(s, scale, shift, att)
        _close("netvlad_assign_rows.a", a, ra, case="R=%d spread=%d" % (R, spread))
        assert float(a[::5].abs().max()) == 0.0
    for rpc, clouds in ((64, 9), (640, 2), (64, 1)):             # clouds beyond eight; ten workgroups per cloud
        R = rpc * clouds
        s, scale, shift, att = _assign_inputs(R, g, dev, spread)
        att[-1] = 0.7
        a, asum = torch.full((R, 64), NAN, device=dev), torch.full((clouds, 64), NAN, device=dev)   # (zeroed by the call)
        _call("dh3d_netvlad_assign_rows", s, R, 64, scale, shift, att, a, asum, rpc)
        ra, rs, _ = G.netvlad_assign_rows(s, scale, shift, att, rpc)
        tag = "rpc=%d clouds=%d spread=%d" % (rpc, clouds, spread)
        _close("netvlad_assign_rows.a", a, ra, case=tag)
        _close("netvlad_assign_rows.asum", asum, rs, case=tag)
        # ... and equal to the per-cloud column sums of the a it wrote
        _close("netvlad_assign_rows.asum~a", asum, G.E(a.double().reshape(clouds, rpc, 64).sum(1), rs.t), case=tag)
        att2 = att.clone()
        att2[-1] = 0.0                                           # the last row of the last cloud dropped
        _power("netvlad_assign_rows.asum", rs, G.netvlad_assign_rows(s, scale, shift, att2, rpc)[1], tag, last_block=False)
    s, scale, shift, att = _assign_inputs(200, g, dev, spread)
    a, asum = torch.full((200, 64), 7.0, device=dev), torch.full((2, 64), 7.0, device=dev)
    assert _status("dh3d_netvlad_assign_rows", s, 200, 64, scale, shift, att, a, asum, 100) == UNSUPPORTED
    torch.cuda.synchronize()
    assert float((a - 7.0).abs().max()) == 0.0 and float((asum - 7.0).abs().max()) == 0.0


@pytest.mark.parametrize("spread", [False, True])
def test_netvlad_assign_rows_bwd_match_float64(dev, spread):
    g = _gen(31 + spread)
    for R in (1, 3, 5, 640):
        s, scale, shift, att = _assign_inputs(R, g, dev, spread)
        da = torch.randn(R, 64, generator=g).to(dev)
        dz, datt = torch.full((R, 64), NAN, device=dev), torch.full((R,), NAN, device=dev)
        _call("dh3d_netvlad_assign_rows_bwd", s, R, 64, scale, shift, att, da, dz, datt)
        rz, rd = G.netvlad_assign_rows_bwd(s, scale, shift, att, da)
        tag = "R=%d spread=%d" % (R, spread)
        _close("netvlad_assign_rows_bwd.dz", dz, rz, case=tag)
        _close("netvlad_assign_rows_bwd.datt", datt, rd, case=tag)
        assert float(dz[::5].abs().max()) == 0.0                 # att = 0: no gradient into the logits
        # power (per row): the outputs sit well above the bound
        assert float((CR.RTOL * rd.t).median()) < 0.1 * float(rd.v.abs().median()) + 1e-30


@pytest.mark.parametrize("n", [1, 255, 257, 22 * 256])
def test_context_gate_matches_float64(dev, n):
    g = _gen(n)
    v, gt, dy = torch.randn(n, generator=g).to(dev), (3 * torch.randn(n, generator=g)).to(dev), torch.randn(n, generator=g).to(dev)
    gt[0] = 100.0
    if n > 1:
        gt[-1] = -100.0
    y = torch.full((n,), NAN, device=dev)
    _call("dh3d_context_gate_fwd", v, gt, n, y)
    ry, rv, rg = G.context_gate(v, gt, dy)
    _close("context_gate.y", y, ry, case=n)
    dv, dg = torch.full((n,), NAN, device=dev), torch.full((n,), NAN, device=dev)
    _call("dh3d_context_gate_bwd", v, gt, dy, n, dv, dg)
    _close("context_gate.dv", dv, rv, case=n)
    _close("context_gate.dg", dg, rg, case=n)


@pytest.mark.parametrize("R", [1, 5])
def test_l2norm_rows_bwd_matches_float64_at_the_global_eps(dev, R):
    g = _gen(60 + R)
    for C in (3, 64, 256, 260):
        x, dxn = torch.randn(R, C, generator=g), torch.randn(R, C, generator=g)
        if R > 1:
            x[1] = 0.0                                           # a zero row
            x[3] *= 1e-7 / x[3].norm()                           # under the clamp: |x|^2 = 1e-14 < 1e-12
        x, dxn = x.to(dev), dxn.to(dev)
        dx = torch.full_like(x, NAN)
        _call("dh3d_l2norm_rows_bwd", x, dxn, R, C, CR.EPS_L2, dx)
        ref = G.l2norm_rows_bwd(x, dxn)
        _close("l2norm_rows_bwd", dx, ref, case="R=%d C=%d" % (R, C))
        assert float((CR.RTOL * ref.t).median()) < 0.1 * float(ref.v.abs().median()) + 1e-30


@pytest.mark.parametrize("B", [1, 9])
def test_vlad_normalize_matches_float64(dev, B):
    g = _gen(70 + B)
    V, asum, W2 = torch.randn(B, 64, 256, generator=g), torch.rand(B, 64, generator=g) * 5, torch.randn(256, 64, generator=g)
    V[0, 5], asum[0, 5] = 0.0, 0.0                               # an empty cluster: norm clamped, no projection term
    V[0, 63], asum[0, 63] = 0.0, 0.0
    if B > 1:
        V[B - 1] = 1e-15 * torch.randn(64, 256, generator=g)     # a cloud whose whole vector is under the clamp
        asum[B - 1] = 0.0
    gr = torch.randn(B, 16384, generator=g)
    V, asum, W2, gr = V.to(dev), asum.to(dev), W2.to(dev), gr.to(dev)
    out, ic, it = torch.full((B, 16384), NAN, device=dev), torch.full((B, 64), NAN, device=dev), torch.full((B,), NAN, device=dev)
    _call("dh3d_vlad_normalize_fwd", V, asum, W2, B, 256, 64, CR.EPS_L2, out, ic, it)
    ref = G.vlad_normalize(V, asum, W2, gr)
    assert bool(ref["clamped_c"][0, 5]) and (B == 1 or bool(ref["clamped_t"][B - 1])) and not bool(ref["clamped_t"][0])
    _close("vlad_normalize.out", out, ref["out"], case=B)
    _close("vlad_normalize.inv_c", ic, ref["inv_c"], case=B)
    _close("vlad_normalize.inv_t", it, ref["inv_t"], case=B)
    dV, das, dW2 = torch.full_like(V, NAN), torch.full_like(asum, NAN), torch.full_like(W2, NAN)    # (dW2 zeroed by the call)
    _call("dh3d_vlad_normalize_bwd", V, asum, W2, gr, B, 256, 64, CR.EPS_L2, dV, das, dW2)
    _close("vlad_normalize.dV", dV, ref["dV"], case=B)
    _close("vlad_normalize.dasum", das, ref["dasum"], case=B)
    _close("vlad_normalize.dW2", dW2, ref["dW2"], case=B)
    assert float((CR.RTOL * ref["dV"].t).median()) < 0.1 * float(ref["dV"].v.abs().median())
    assert _status("dh3d_vlad_normalize_fwd", V, asum, W2, B, 128, 64, CR.EPS_L2, out, ic, it) == UNSUPPORTED


def _quad_desc(B, P, Ng, kind, g):
    D = 256
    desc = torch.randn(B * (2 + P + Ng), D, generator=g) * 0.02
    m1, m2 = 0.5, 0.2
    if kind == "inactive":        # positives next to the query, negatives far: no hinge is active
        desc = desc * 50.0
        desc[B:B + B * P] = desc[:B].repeat_interleave(P, 0) + 0.01 * torch.randn(B * P, D, generator=g)
    if kind == "dups":            # duplicate positives and negatives: the first index takes the gradient
        pos = desc[B:B + B * P].reshape(B, P, D)
        pos[:, 1] *= 0.1
        pos[:, 3] = pos[:, 1]
        neg = desc[B + B * P:B + B * P + B * Ng].reshape(B, Ng, D)
        neg[:, 7] = desc[:B] * 0.5 + desc[-B:] * 0.5 + 0.001
        neg[:, 40] = neg[:, 7]
    if kind == "zero_hinge":      # exactly representable: hinge 1 = 0.5 + 0.25 - 0.75 = 0, hinge 2 < 0
        desc.zero_()
        m1, m2 = 0.5, 0.25
        desc[1, 0] = 0.5
        desc[2, 0], desc[2, 1], desc[2, 2] = 0.5, 0.5, 0.5
        desc[3, 3] = 0.5
    return desc, m1, m2


@pytest.mark.parametrize("B,P,Ng,kind", [(1, 1, 1, "zero_hinge"), (1, 1, 1, "plain"), (3, 8, 64, "dups"),
                                         (3, 8, 64, "plain"), (2, 2, 18, "inactive"), (2, 2, 18, "plain")])
def test_quadruplet_loss_matches_float64(dev, B, P, Ng, kind):
    desc, m1, m2 = _quad_desc(B, P, Ng, kind, _gen(B + P + Ng))
    desc = desc.to(dev)
    loss, grad = torch.full((1,), NAN, device=dev), torch.full_like(desc, NAN)
    _call("dh3d_quadruplet_loss", desc, B, P, Ng, 256, m1, m2, loss, grad)
    rl, rg = G.quadruplet_loss(desc, B, P, Ng, m1, m2)
    tag = "%d,%d,%d %s" % (B, P, Ng, kind)
    _close("quadruplet_loss.loss", loss, rl, case=tag)
    _close("quadruplet_loss.grad", grad, rg, case=tag)
    assert torch.equal(grad != 0, rg.v != 0), tag                # the gradient lands on the same rows: first index on ties
    if kind == "inactive":
        assert float(loss) == 0.0 and float(grad.abs().max()) == 0.0
    if kind == "zero_hinge":
        assert float(loss) == 0.0 and float(grad.abs().max()) > 0.0          # passed at a hinge of exactly 0
    if kind == "dups":
        assert float(grad[B + B * P:].reshape(-1, 256)[40].abs().max()) == 0.0 and float(rg.v[B + B * P + 7].abs().max()) > 0


def test_quadruplet_loss_refuses_more_roles(dev):
    for P, Ng in ((9, 4), (2, 65)):
        desc = torch.randn(2 * (2 + P + Ng), 256, device=dev)
        loss, grad = torch.full((1,), 7.0, device=dev), torch.full_like(desc, 7.0)
        assert _status("dh3d_quadruplet_loss", desc, 2, P, Ng, 256, 0.5, 0.2, loss, grad) == UNSUPPORTED
        torch.cuda.synchronize()
        assert float(loss) == 7.0 and float((grad - 7.0).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------- the composed nodes
@pytest.fixture(scope="module")
def head_inputs(dev):
    g = _gen(101)
    return dict(W=(torch.randn(64, 256, generator=g) / 8).to(dev), b=(0.1 * torch.randn(256, generator=g)).to(dev),
                gamma=(0.5 + torch.rand(256, generator=g)).to(dev), beta=(0.3 * torch.randn(256, generator=g)).to(dev),
                wfc=(torch.randn(256, 1, generator=g) / 16).to(dev), bfc=torch.randn(1, generator=g).to(dev),
                Wc=(torch.randn(256, 64, generator=g) / 4).to(dev), g64=(0.5 + torch.rand(64, generator=g)).to(dev),
                b64=(0.3 * torch.randn(64, generator=g)).to(dev))


@pytest.mark.parametrize("N", [192, 200])
def test_attention_head_node_matches_the_reference_composition(dev, head_inputs, N):
    """(T is chained through the node's ten launches to first order and comes to some hundreds of |value|: these two
    tests check the wiring -- which kernel, which buffer, which mask, which running buffer -- the kernel tests above
    check the digits.)"""
    from dh3d_amd import backbones as bb, pm, train_ops as T
    g = _gen(N)
    K = head_inputs
    X = torch.randn(3 * N, 64, generator=g).to(dev)
    datt = torch.randn(3 * N, generator=g).to(dev)
    mask = torch.tensor([True, False, True], device=dev)
    live = G.rows_live(3 * N, mask, N)
    conv = bb.Conv2D1x1(64, 256).to(dev)
    with torch.no_grad():
        conv.W.copy_(K["W"].reshape(1, 1, 64, 256)); conv.b.copy_(K["b"])
        conv.bn.gamma.copy_(K["gamma"]); conv.bn.beta.copy_(K["beta"])
        conv.bn.mean_EMA.normal_(); conv.bn.variance_EMA.uniform_(0.5, 1.5)
    rm0, rv0 = conv.bn.mean_EMA.clone(), conv.bn.variance_EMA.clone()
    Xp, wfc, bfc = X.clone().requires_grad_(), K["wfc"].clone().requires_grad_(), K["bfc"].clone().requires_grad_()
    att = T.attention_head(Xp, conv, wfc, bfc, False, mask, N)
    att.backward(datt)
    # the node's own pre-activation and folded statistics (the same launches on the same inputs): the gate's f32 tensors
    h32 = pm.gemm_nn(X, K["W"], bias=K["b"])
    acc = torch.zeros(2, 256, dtype=F64, device=dev)
    _call("dh3d_bn_colstats", h32, 3 * N, 256, mask.to(torch.uint8), N, acc[0], acc[1])
    st = torch.empty(4, 256, device=dev)
    cn = torch.full((1,), float(live.sum()), dtype=F64, device=dev)
    _call("dh3d_bn_finalize", acc[0], acc[1], cn, K["gamma"], K["beta"], conv.bn.eps, 0.9, 1, rm0.clone(), rv0.clone(), 256,
          st[0], st[1], st[2], st[3])
    ref = G.attention_head(X, K["W"], K["b"], K["gamma"], K["beta"], K["wfc"], K["bfc"], conv.bn.eps, 0.9, rm0, rv0, datt, live,
                           h32=h32, scale32=st[2].contiguous(), shift32=st[3].contiguous())
    tag = "N=%d" % N
    _close("attention_head.att", att.detach(), ref["att"], sel=live, case=tag)
    _close("attention_head.dX", Xp.grad, ref["dX"], case=tag)
    _close("attention_head.dW", conv.W.grad.reshape(64, 256), ref["dW"], case=tag)
    _close("attention_head.dgamma", conv.bn.gamma.grad, ref["dgamma"], case=tag)
    _close("attention_head.dbeta", conv.bn.beta.grad, ref["dbeta"], case=tag)
    _close("attention_head.dwfc", wfc.grad.reshape(-1), ref["dwfc"], case=tag)
    _close("attention_head.dbfc", bfc.grad, ref["dbfc"], case=tag)
    _close("attention_head.run_mean", conv.bn.mean_EMA, ref["run_mean"], case=tag)
    _close("attention_head.run_var", conv.bn.variance_EMA, ref["run_var"], case=tag)
    assert float(conv.b.grad.abs().max()) == 0.0 and float(Xp.grad[~live].abs().max()) == 0.0


@pytest.mark.parametrize("N", [192, 200])      # N % 64 == 0: asum rides along; else a.sum(1)
def test_netvlad_assign_node_matches_the_reference_composition(dev, head_inputs, N):
    from dh3d_amd import backbones as bb, train_ops as T
    g = _gen(N + 1)
    K = head_inputs
    x = torch.randn(3, N, 256, generator=g).to(dev)
    att = (0.25 + 0.75 * torch.rand(3 * N, generator=g)).to(dev)
    dV, dasum = torch.randn(3, 64, 256, generator=g).to(dev), torch.randn(3, 64, generator=g).to(dev)
    mask = torch.tensor([True, False, True], device=dev)
    dV[1], dasum[1] = 0.0, 0.0                                    # a padding cloud's outputs feed nothing
    bn = bb.SlimBatchNorm(64, fused=False).to(dev)
    with torch.no_grad():
        bn.gamma.copy_(K["g64"]); bn.beta.copy_(K["b64"])
        bn.moving_mean.normal_(); bn.moving_variance.uniform_(0.5, 1.5)
    rm0, rv0 = bn.moving_mean.clone(), bn.moving_variance.clone()
    xp, ap, Wc = x.clone().requires_grad_(), att.clone().requires_grad_(), K["Wc"].clone().requires_grad_()
    V, asum = T.netvlad_assign(xp, ap, Wc, bn, False, mask)
    torch.autograd.backward((V, asum), (dV, dasum))
    ref = G.netvlad_assign(x, att, K["Wc"], K["g64"], K["b64"], bn.eps, 0.999, rm0, rv0, dV, dasum, mask)
    tag = "N=%d" % N
    _close("netvlad_assign.V", V.detach(), ref["V"], sel=mask, case=tag)
    _close("netvlad_assign.asum", asum.detach(), ref["asum"], sel=mask, case=tag)
    _close("netvlad_assign.dx", xp.grad, ref["dx"], sel=mask, case=tag)
    _close("netvlad_assign.datt", ap.grad, ref["datt"], case=tag)
    _close("netvlad_assign.dWc", Wc.grad, ref["dWc"], case=tag)
    _close("netvlad_assign.dgamma", bn.gamma.grad, ref["dgamma"], case=tag)
    _close("netvlad_assign.dbeta", bn.beta.grad, ref["dbeta"], case=tag)
    _close("netvlad_assign.run_mean", bn.moving_mean, ref["run_mean"], case=tag)
    _close("netvlad_assign.run_var", bn.moving_variance, ref["run_var"], case=tag)


# ------------------------------------------------------------------------------------------------------ gate agreement
def _near_threshold(scale, shift, R, g):
    """x [R, C] f32 on the host: every element within +-4 ulp of -shift / scale of its column."""
    thr = (-shift.double().cpu() / scale.double().cpu()).float()
    assert bool((thr != 0).all()) and bool(torch.isfinite(thr).all())
    k = torch.randint(-4, 5, (R, thr.shape[0]), generator=g, dtype=torch.int32)
    return (thr.view(torch.int32)[None, :] + k).view(torch.float32)


def _bits(S, R):
    """S [C] exact sums of 2^r over the open gates -> gates [R, C]."""
    v = S.round().long()
    assert torch.equal(v.double(), S.double())
    return ((v[None, :] >> torch.arange(R, device=S.device)[:, None]) & 1).bool()


@pytest.mark.parametrize("C", [64, 1024])
def test_every_pass_of_a_site_takes_the_same_relu_gate(dev, C):
    g = _gen(500 + C)
    R = 24
    gamma = ((0.5 + torch.rand(C, generator=g)) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)).to(dev)   # both signs
    beta = ((0.2 + torch.rand(C, generator=g)) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)).to(dev)
    mu, var = torch.randn(C, generator=g, dtype=F64), torch.rand(C, generator=g, dtype=F64) + 0.1
    n = 4096.0
    cn = torch.full((1,), n, dtype=F64, device=dev)
    st = torch.empty(4, C, device=dev)
    _call("dh3d_bn_finalize", (n * mu).to(dev), (n * (var + mu * mu)).to(dev), cn, gamma, beta, 1e-5, 0.9, 1,
          torch.zeros(C, device=dev), torch.ones(C, device=dev), C, st[0], st[1], st[2], st[3])
    mean, rstd, scale, shift = (st[i].contiguous() for i in range(4))
    assert bool((scale != 0).all())
    x = _near_threshold(scale, shift, R, g).to(dev)
    want = G.gate(x, scale, shift)
    assert 0.2 < float(want.float().mean()) < 0.8
    pow2 = (2 ** torch.arange(R)).float().to(dev)[:, None].expand(R, C).contiguous()       # (integer powers: exact)
    ones, zeros = torch.ones(R, C, device=dev), torch.zeros(C, device=dev)
    counts = {}
    y = torch.empty_like(x)
    _call("dh3d_scale_shift_act", x, R, C, scale, shift, 1, y)
    counts["forward"] = int(((y > 0) != want).sum())
    dx = torch.empty_like(x)
    _call("dh3d_bn_bwd_apply", x, ones, None, None, R, C, scale, shift, zeros, zeros, 1, None, 0, dx)
    counts["bn_bwd_apply"] = int(((dx != 0) != want).sum())
    S = torch.zeros(2, C, dtype=F64, device=dev)
    _call("dh3d_bn_bwd_sums", x, pow2, None, None, R, C, mean, rstd, gamma, beta, 1, None, 0, S[0], S[1], None)
    counts["bn_bwd_sums"] = int((_bits(S[0], R) != want).sum())
    S3 = torch.zeros(3, C, dtype=F64, device=dev)
    _call("dh3d_bn_bwd_sums", x, None, pow2[:, 0].contiguous(), torch.ones(C, device=dev), R, C, mean, rstd, gamma, beta, 1,
          None, 0, S3[0], S3[1], S3[2])
    counts["bn_bwd_sums rank-one"] = int((_bits(S3[0], R) != want).sum())
    # the short form against its own forward (beta = 0: a nearly constant column sits on its own threshold)
    b0 = torch.zeros(C, device=dev)
    stats, ys = torch.empty(4, C, device=dev), torch.empty_like(x)
    _call("dh3d_bn_small_fwd", x, R, C, gamma, b0, 1e-5, 0.9, 1, 1, None, torch.zeros(C, device=dev),
          torch.ones(C, device=dev), stats, ys)
    dxs, dgb = torch.empty_like(x), torch.empty(2, C, device=dev)
    _call("dh3d_bn_small_bwd", x, pow2, R, C, gamma, stats, 1, None, dxs, dgb[0], dgb[1])
    want_s = G.gate(x, stats[2].contiguous(), stats[3].contiguous())
    counts["bn_small forward"] = int(((ys > 0) != want_s).sum())
    counts["bn_small dbeta"] = int((_bits(dgb[1], R) != want_s).sum())
    print("gate disagreements with the float64 gate, of %d elements within 4 ulp of the threshold: %s" % (R * C, counts))
    assert all(v == 0 for v in counts.values()), counts


@pytest.mark.parametrize("Hd", [256, 1024])
def test_commuted_sums_and_apply_walks_take_the_same_relu_gate(dev, Hd):
    g = _gen(600 + Hd)
    n, m = 24, 32
    gamma = ((0.5 + torch.rand(Hd, generator=g)) * (torch.randint(0, 2, (Hd,), generator=g) * 2 - 1)).to(dev)
    beta = ((0.2 + torch.rand(Hd, generator=g)) * (torch.randint(0, 2, (Hd,), generator=g) * 2 - 1)).to(dev)
    mu, var = torch.randn(Hd, generator=g, dtype=F64), torch.rand(Hd, generator=g, dtype=F64) + 0.1
    cn = torch.full((1,), 4096.0, dtype=F64, device=dev)
    st = torch.empty(4, Hd, device=dev)
    _call("dh3d_bn_finalize", (4096.0 * mu).to(dev), (4096.0 * (var + mu * mu)).to(dev), cn, gamma, beta, 1e-5, 0.9, 1,
          torch.zeros(Hd, device=dev), torch.ones(Hd, device=dev), Hd, st[0], st[1], st[2], st[3])
    mean, rstd, scale, shift = (st[i].contiguous() for i in range(4))
    Grows = torch.zeros(m, Hd)
    Grows[:] = _near_threshold(scale, shift, 1, g)
    Grows[:n] = _near_threshold(scale, shift, n, g)
    Grows = Grows.to(dev).contiguous()
    idx = torch.arange(n, dtype=torch.int32)[:, None].expand(n, 3).reshape(1, n, 3).contiguous().to(dev)   # point i: row i only
    dist = torch.full((1, n, 3), 0.01, device=dev)
    dlogit = (2 ** torch.arange(n)).float().to(dev)
    wfc, zeros = torch.ones(Hd, device=dev), torch.zeros(Hd, device=dev)
    part = torch.zeros(3, 1, Hd, dtype=F64, device=dev)
    _call("dh3d_interp_bn_bwd_sums", Grows, Hd, 1, idx, dist, None, 1, n, m, None, dlogit, wfc, mean, rstd, gamma, beta, part)
    dG = torch.zeros(m, Hd, device=dev)
    _call("dh3d_interp_bn_bwd_apply", Grows, Hd, 1, idx, dist, None, 1, n, m, None, dlogit, wfc, scale, shift, zeros, zeros, dG)
    sums_gate, apply_gate = _bits(part[0, 0], n), dG[:n] != 0
    assert float(dG[n:].abs().max()) == 0.0
    differ = int((sums_gate != apply_gate).sum())
    print("commuted walks: %d of %d gates within a few ulp of the threshold differ between sums and apply (%.0f%% open)" % (
        differ, n * Hd, 100 * float(apply_gate.float().mean())))
    assert 0.1 < float(apply_gate.float().mean()) < 0.9
    assert differ == 0


def test_zz_report_worst_ratios():
    """Prints the worst |got - ref| / T per output over the cases run (informational; run with -s or -rA)."""
    for k in sorted(_WORST):
        print("worst %-36s %.3e  (%s)" % (k, _WORST[k][0], _WORST[k][1]))
