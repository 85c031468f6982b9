"""CPU: the float64 restatements of tests/global_training_reference.py against torch.autograd of the plain float64 graph
at toy sizes -- values and every gradient -- so that the GPU tests compare the kernels with formulas that are themselves
checked.  Padding clouds first / middle / last and a rank of padding clouds only; an empty cluster and clamped norms in
vlad_normalize; duplicate negatives, all-inactive hinges and a hinge of exactly 0 in the quadruplet loss."""
import pytest
import torch

import global_training_reference as G

F64 = torch.float64
TOL = 1e-11


def _close(name, got, ref):
    got = got.v if isinstance(got, G.E) else got
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if got.numel() == 0:
        return
    err = float((got - ref).abs().max())
    assert err <= TOL * (1.0 + float(ref.abs().max())), (name, err)


def _rnd(g, *s):
    return torch.randn(*s, generator=g)     # float32 values, as the kernels get them


def _live(clouds, rpc, padding):
    m = torch.ones(clouds, dtype=torch.bool)
    if padding == "first":
        m[0] = False
    elif padding == "middle":
        m[clouds // 2] = False
    elif padding == "last":
        m[-1] = False
    elif padding == "all":
        m[:] = False
    return None if padding is None else m


def _plain_bn(x, gamma, beta, eps, relu, live):
    xs = x[live]
    n = max(xs.shape[0], 1)
    mean = xs.sum(0) / n
    var = (xs * xs).sum(0) / n - mean * mean
    y = (x - mean) * torch.rsqrt(var + eps) * gamma + beta
    return (torch.relu(y) if relu else y), mean, var


@pytest.mark.parametrize("padding", [None, "first", "middle", "last", "all"])
@pytest.mark.parametrize("relu", [False, True])
def test_batch_norm_site_matches_autograd(padding, relu):
    g = torch.Generator().manual_seed(3)
    clouds, rpc, C = 3, 5, 6
    R = clouds * rpc
    x, dy = _rnd(g, R, C) * 2 + 0.5, _rnd(g, R, C)
    gamma, beta = 0.5 + torch.rand(C, generator=g), _rnd(g, C)
    rm, rv = _rnd(g, C), torch.rand(C, generator=g)
    mask = _live(clouds, rpc, padding)
    live = G.rows_live(R, mask, rpc)
    eps = G.f32(1e-3)
    for unbiased, mom in ((True, 0.9), (False, 0.999)):
        out = G.batch_norm_train(x, gamma, beta, eps, mom, unbiased, relu, rm, rv, dy, None if mask is None else live)
        x2, g2, b2 = (t.double().requires_grad_() for t in (x, gamma, beta))
        y, mean, var = _plain_bn(x2, g2, b2, eps, relu, live)
        gx, gg, gb = torch.autograd.grad((y * dy.double() * live[:, None]).sum(), (x2, g2, b2))
        _close("y", out["y"].v[live], y[live].detach())
        _close("dx", out["dx"], gx)
        _close("dgamma", out["dgamma"], gg)
        _close("dbeta", out["dbeta"], gb)
        n = float(live.sum())
        m = G.f32(mom)
        if n == 0:
            assert torch.equal(out["run_mean"].v, rm.double()) and torch.equal(out["run_var"].v, rv.double())
            assert float(out["run_mean"].t.max()) == 0.0
            assert bool(torch.isfinite(out["rstd"].v).all())
        else:
            uv = var * (n / (n - 1)) if unbiased and n > 1 else var
            _close("run_mean", out["run_mean"], (m * rm.double() + (1 - m) * mean).detach())
            _close("run_var", out["run_var"], (m * rv.double() + (1 - m) * uv).detach())
        # the stand-alone restatements compose to the same site
        st = out
        mean32, rstd32 = st["mean"].v.float(), st["rstd"].v.float()
        sc32, sh32 = G.fold(mean32, rstd32, gamma, beta)
        lv = None if mask is None else live
        S1, S2, _ = G.bn_bwd_sums(x, mean32, rstd32, sc32, sh32, relu, dy=dy, live=lv)
        if n > 0:
            assert float((S1.v - gb).abs().max()) <= 1e-5 * float(S1.t.max()) + 1e-12      # (f32 statistics)
        k = G.bn_bwd_finalize(S1, S2, n, mean32, rstd32, gamma)
        dx = G.bn_bwd_apply(x, sc32, sh32, k["k2"].v.float(), k["k3"].v.float(), relu, dy=dy, live=lv)
        assert float(((dx.v - gx).abs() / (dx.t + 1e-30)).max()) <= 1e-5
        assert float(dx.v[~live].abs().max() if (~live).any() else 0.0) == 0.0


def test_finalize_parts_counts_and_constant_column():
    g = torch.Generator().manual_seed(4)
    C, P = 5, 4
    part1, part2 = torch.randn(P, C, generator=g, dtype=F64), torch.rand(P, C, generator=g, dtype=F64) * 50 + 10
    gamma, beta, rm, rv = (_rnd(g, C) for _ in range(4))
    a = G.bn_finalize(G.E(part1).exact(), G.E(part2).exact(), 7.0, gamma, beta, 1e-5, 0.9, True, rm, rv)
    b = G.bn_finalize(G.E(part1.sum(0)).exact(), G.E(part2.sum(0)).exact(), 7.0, gamma, beta, 1e-5, 0.9, True, rm, rv)
    for k in a:
        _close(k, a[k], b[k].v)
    # a constant column whose variance rounds below zero: clamped, rstd = 1 / sqrt(eps)
    n = 9.0
    s1, s2 = torch.full((C,), 3.0 * n, dtype=F64), torch.full((C,), 9.0 * n * (1 - 1e-15), dtype=F64)
    c = G.bn_finalize(G.E(s1).exact(), G.E(s2).exact(), n, gamma, beta, 1e-5, 0.9, True, rm, rv)
    _close("rstd", c["rstd"], torch.full((C,), G.f32(1e-5), dtype=F64).rsqrt())
    # counts 0 / 1: no division by zero, no Bessel factor
    for cnt in (0.0, 1.0):
        d = G.bn_finalize(G.E(s1 * 0).exact(), G.E(s2 * 0).exact(), cnt, gamma, beta, 1e-5, 0.9, True, rm, rv)
        assert all(bool(torch.isfinite(d[k].v).all()) for k in d)
    S = G.bn_bwd_finalize(G.E(part1).exact(), G.E(part2).exact(), 7.0, rm, rv.abs(), gamma)
    _close("dbeta", S["dbeta"], part1.sum(0))
    _close("dgamma", S["dgamma"], part2.sum(0))


@pytest.mark.parametrize("padding", [None, "first", "middle", "last", "all"])
def test_attention_head_matches_autograd(padding):
    g = torch.Generator().manual_seed(5)
    clouds, rpc, Cin, H = 3, 7, 4, 8
    R = clouds * rpc
    X, W, b = _rnd(g, R, Cin), _rnd(g, Cin, H) / 2, _rnd(g, H)
    gamma, beta, wfc, bfc = 0.5 + torch.rand(H, generator=g), 0.3 * _rnd(g, H), _rnd(g, H, 1), _rnd(g, 1)
    rm, rv, datt = _rnd(g, H), torch.rand(H, generator=g), _rnd(g, R)
    mask = _live(clouds, rpc, padding)
    live = G.rows_live(R, mask, rpc)
    out = G.attention_head(X, W, b, gamma, beta, wfc, bfc, 1e-3, 0.9, rm, rv, datt, None if mask is None else live)
    p = [t.double().requires_grad_() for t in (X, W, b, gamma, beta, wfc, bfc)]
    h = p[0] @ p[1] + p[2]
    y, mean, var = _plain_bn(h, p[3], p[4], G.f32(1e-3), True, live)
    att = torch.sigmoid(y @ p[5].reshape(-1) + p[6])
    grads = torch.autograd.grad((att * datt.double() * live).sum(), p)
    _close("att", out["att"].v[live], att[live].detach())
    for name, gr in zip(("dX", "dW", None, "dgamma", "dbeta", "dwfc", "dbfc"), grads):
        if name:
            _close(name, out[name], gr.reshape(out[name].v.shape))
    assert float(grads[2].abs().max()) <= 1e-12      # a bias in front of a BatchNorm: exact gradient 0
    # the rank-one forms of the kernels' restatements give the same sums
    if float(live.sum()) > 0:
        mean32, rstd32 = out["mean"].v.float(), out["rstd"].v.float()
        sc32, sh32 = G.fold(mean32, rstd32, gamma, beta)
        h32 = out["h"].v.float()
        dl = out["dlogit"].v.float()
        S1, S2, S3 = G.bn_bwd_sums(h32, mean32, rstd32, sc32, sh32, True, rowscale=dl, colvec=wfc.reshape(-1),
                                   live=None if mask is None else live)
        for name, S in (("dbeta", S1), ("dgamma", S2), ("dwfc", S3)):
            assert float(((S.v - out[name].v).abs() / (S.t + 1e-30)).max()) <= 1e-4, name   # (f32 inputs; a flipped gate ~ 1)


@pytest.mark.parametrize("padding", [None, "first", "middle", "last"])
def test_netvlad_assign_matches_autograd(padding):
    g = torch.Generator().manual_seed(6)
    B, N, D = 3, 5, 8
    x, att, Wc = _rnd(g, B, N, D), torch.rand(B * N, generator=g), _rnd(g, D, 64) / 2
    x[1, 2] = 0.0                                   # a row the l2 clamp holds
    gamma, beta = 0.5 + torch.rand(64, generator=g), 0.3 * _rnd(g, 64)
    rm, rv = _rnd(g, 64), torch.rand(64, generator=g)
    dV, dasum = _rnd(g, B, 64, D), _rnd(g, B, 64)
    mask = _live(B, N, padding)
    live = G.rows_live(B * N, mask, N)
    out = G.netvlad_assign(x, att, Wc, gamma, beta, 1e-3, 0.999, rm, rv, dV, dasum, mask)
    p = [t.double().requires_grad_() for t in (x, att, Wc, gamma, beta)]
    x2 = p[0].reshape(B * N, D)
    xn = x2 * torch.rsqrt((x2 * x2).sum(-1, keepdim=True).clamp_min(G.EPS_L2))
    s = xn @ p[2]
    z, mean, var = _plain_bn(s, p[3], p[4], G.f32(1e-3), False, live)
    a = (torch.softmax(z, -1) * p[1][:, None]).reshape(B, N, 64)
    V, asum = a.transpose(1, 2) @ xn.reshape(B, N, D), a.sum(1)
    lc = torch.ones(B, dtype=torch.bool) if mask is None else mask
    _close("V", out["V"].v[lc], V[lc].detach())
    _close("asum", out["asum"].v[lc], asum[lc].detach())
    loss = (V * dV.double() * lc[:, None, None]).sum() + (asum * dasum.double() * lc[:, None]).sum()
    # (padding clouds get no gradient: the caller's dV / dasum are zero there)
    dVm, dam = dV * lc[:, None, None], dasum * lc[:, None]
    out = G.netvlad_assign(x, att, Wc, gamma, beta, 1e-3, 0.999, rm, rv, dVm, dam, mask)
    grads = torch.autograd.grad(loss, p)
    gx = grads[0] * lc[:, None, None]               # x of a padding cloud still feeds nothing
    _close("dx", out["dx"].v[lc], gx[lc])
    for name, gr in zip(("datt", "dWc", "dgamma", "dbeta"), grads[1:]):
        _close(name, out[name], gr)
    n = float(live.sum())
    _close("run_var", out["run_var"], (G.f32(0.999) * rv.double() + (1 - G.f32(0.999)) * var).detach())   # biased


def test_vlad_normalize_matches_autograd_with_empty_cluster_and_clamped_norm():
    g = torch.Generator().manual_seed(7)
    B = 3
    V, asum, W2 = _rnd(g, B, 64, 256), torch.rand(B, 64, generator=g), _rnd(g, 256, 64)
    V[0, 5] = 0.0
    asum[0, 5] = 0.0                                # an empty cluster: u = 0, its norm clamped, no projection term
    V[2] = 1e-15 * _rnd(g, 64, 256)
    asum[2] = 0.0                                   # a cloud whose whole vector is under the clamp
    gr = _rnd(g, B, 16384)
    out = G.vlad_normalize(V, asum, W2, gr)
    assert bool(out["clamped_c"][0, 5]) and bool(out["clamped_t"][2]) and not bool(out["clamped_t"][0])
    p = [t.double().requires_grad_() for t in (V, asum, W2)]
    u = p[0] - p[1][:, :, None] * p[2].t()[None]
    y1 = u * torch.rsqrt((u * u).sum(-1, keepdim=True).clamp_min(G.EPS_L2))
    flat = y1.permute(0, 2, 1).reshape(B, -1)
    y = flat * torch.rsqrt((flat * flat).sum(-1, keepdim=True).clamp_min(G.EPS_L2))
    _close("out", out["out"], y.detach())
    grads = torch.autograd.grad((y * gr.double()).sum(), p)
    for name, gg in zip(("dV", "dasum", "dW2"), grads):
        _close(name, out[name], gg)
    assert float(out["inv_c"].v[0, 5]) == pytest.approx(1e6, rel=1e-6)


def test_context_gate_sigmoid_bwd_and_l2norm_match_autograd():
    g = torch.Generator().manual_seed(8)
    v, gg, dy = _rnd(g, 33), 3 * _rnd(g, 33), _rnd(g, 33)
    gg[:2] = torch.tensor([100.0, -100.0])
    y, dv, dg = G.context_gate(v, gg, dy)
    p = [t.double().requires_grad_() for t in (v, gg)]
    yy = p[0] * torch.sigmoid(p[1])
    gv, g_g = torch.autograd.grad((yy * dy.double()).sum(), p)
    _close("y", y, yy.detach()), _close("dv", dv, gv), _close("dg", dg, g_g)
    att = torch.rand(12, generator=g)
    att[0], att[1] = 0.0, 1.0
    live = torch.tensor([True] * 4 + [False] * 4 + [True] * 4)
    d, s = G.sigmoid_bwd(dy[:12], att, live)
    ref = dy[:12].double() * att.double() * (1 - att.double()) * live
    _close("dlogit", d, ref), _close("sum", s, ref.sum())
    x, dxn = _rnd(g, 5, 7), _rnd(g, 5, 7)
    x[1] = 0.0
    x[3] *= 1e-8                                     # under the clamp
    p = x.double().requires_grad_()
    xn = p * torch.rsqrt((p * p).sum(-1, keepdim=True).clamp_min(G.EPS_L2))
    (gx,) = torch.autograd.grad((xn * dxn.double()).sum(), p)
    _close("l2 dx", G.l2norm_rows_bwd(x, dxn), gx)
    a, asum, _ = G.netvlad_assign_rows(_rnd(g, 6, 64), 1 + torch.rand(64, generator=g), _rnd(g, 64),
                                       torch.rand(6, generator=g), rows_per_cloud=3)
    _close("asum", asum, a.v.reshape(2, 3, 64).sum(1))


def _plain_quadruplet(desc, B, P, Ng, m1, m2):
    D = desc.shape[1]
    q, pos = desc[:B][:, None], desc[B:B + B * P].reshape(B, P, D)
    neg, oth = desc[B + B * P:B + B * P + B * Ng].reshape(B, Ng, D), desc[B + B * P + B * Ng:][:, None]
    best = ((pos - q) ** 2).sum(2).min(1).values[:, None]
    trip = torch.clamp(m1 + best - ((neg - q) ** 2).sum(2), min=0).max(1).values.mean()
    second = torch.clamp(m2 + best - ((neg - oth) ** 2).sum(2), min=0).max(1).values.mean()
    return trip + second


@pytest.mark.parametrize("B,P,Ng,kind", [(1, 1, 1, "zero_hinge"), (3, 8, 64, "dups"), (2, 2, 18, "inactive"),
                                         (3, 2, 5, "plain")])
def test_quadruplet_loss_matches_autograd(B, P, Ng, kind):
    g = torch.Generator().manual_seed(9)
    D = 256
    desc = _rnd(g, B * (2 + P + Ng), D) * (0.02 if kind != "inactive" else 1.0)
    m1, m2 = 0.5, 0.2
    if kind == "inactive":      # positives next to the query, negatives far: no hinge is active
        desc[B:B + B * P] = desc[:B].repeat_interleave(P, 0) + 0.01 * _rnd(g, B * P, D)
    if kind == "dups":          # duplicate positives and negatives: the first index takes the gradient
        pos = desc[B:B + B * P].reshape(B, P, D)
        pos[:, 3] = pos[:, 1]
        pos[:, 1] *= 0.1
        pos[:, 3] = pos[:, 1]
        neg = desc[B + B * P:B + B * P + B * Ng].reshape(B, Ng, D)
        neg[:, 40] = neg[:, 7]
        neg[:, 7] = desc[:B] * 0.5 + desc[-B:] * 0.5 + 0.001     # close to both: the hardest negative, twice
        neg[:, 40] = neg[:, 7]
    if kind == "zero_hinge":    # exactly representable: |pos - q|^2 = 0.25, |neg - q|^2 = 0.75 = |neg - o|^2 - 0.3 + ...
        desc.zero_()
        m1, m2 = 0.5, 0.25
        desc[1, 0] = 0.5                      # pos: d = 0.25
        desc[2, 0], desc[2, 1] = 0.5, 0.5     # neg: |neg - q|^2 = 0.5 ... hinge1 = 0.5 + 0.25 - 0.5 > 0
        desc[2, 2] = 0.5                      # |neg - q|^2 = 0.75: hinge1 = 0 exactly
        desc[3, 3] = 0.5                      # other: |neg - o|^2 = 1.0; hinge2 = 0.25 + 0.25 - 1.0 < 0
    loss, grad = G.quadruplet_loss(desc, B, P, Ng, m1, m2)
    d = desc.double().requires_grad_()
    ref = _plain_quadruplet(d, B, P, Ng, G.f32(m1), G.f32(m2))
    (gd,) = torch.autograd.grad(ref, d)
    _close("loss", loss, ref.detach())
    _close("grad", grad, gd)
    if kind == "inactive":
        assert float(loss.v) == 0.0 and float(grad.v.abs().max()) == 0.0
    if kind == "zero_hinge":
        assert float(loss.v) == 0.0 and float(grad.v.abs().max()) > 0.0      # the gradient passes at a hinge of 0
    if kind == "dups":
        assert float(grad.v[B + B * P:].reshape(-1, D)[40].abs().max()) == 0.0   # the second copy gets nothing
