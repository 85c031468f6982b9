"""CPU: the float64 restatements of the commuted training walks (tests/commuted_reference.py), put together the way
train_ops' _AttentionHeadCommuted / _NetVLADAssignCommuted put the kernels together, equal torch autograd of the
materialised graphs -- conv -> BN_train -> ReLU -> fc -> sigmoid on interp(coarse) for the attention head,
l2_normalize -> Wc -> BN_train -> softmax * att -> (V, asum) on interp(c) for NetVLAD -- in float64.  Includes padding
clouds (no statistics, zero gradients), duplicate neighbours, zero distances and rows held by the l2 clamp."""
import pytest
import torch

import commuted_reference as R

F64 = torch.float64


def _geometry(g, B, n, m, extras=True):
    idx = torch.stack([torch.stack([torch.randperm(m, generator=g)[:3] for _ in range(n)]) for _ in range(B)])
    dist = torch.rand(B, n, 3, generator=g, dtype=F64) * 10.0 ** torch.randint(-3, 3, (B, n, 3), generator=g)
    if extras:
        idx[:, 0, :] = idx[:, 0, :1]          # duplicates: one row three times
        dist[:, 1, 0] = 0.0                   # a zero distance (the 1e-10 clamp)
        dist[:, 2, :] = 0.0                   # three zero distances
    return idx.to(torch.int32), dist


def _mask(B, which):
    live = torch.ones(B, dtype=torch.bool)
    if which == "first":
        live[0] = False
    elif which == "last":
        live[-1] = False
    return live


@pytest.mark.parametrize("padding", ["none", "first", "last"])
def test_attention_head_restatement_is_autograd_of_the_materialised_graph(padding):
    g = torch.Generator().manual_seed(11)
    B, n, m, Cin, Hd, eps = 3, 40, 9, 8, 12, 1e-3
    idx, dist = _geometry(g, B, n, m)
    live = _mask(B, padding)
    w = R.idw_weights(dist)
    C = torch.randn(B, m, Cin, generator=g, dtype=F64, requires_grad=True)
    W = torch.randn(Cin, Hd, generator=g, dtype=F64, requires_grad=True)
    b = torch.randn(Hd, generator=g, dtype=F64)
    gamma = (0.5 + torch.rand(Hd, generator=g, dtype=F64)).requires_grad_()
    beta = (0.3 * torch.randn(Hd, generator=g, dtype=F64)).requires_grad_()
    wfc = torch.randn(Hd, generator=g, dtype=F64, requires_grad=True)
    bfc = torch.randn(1, generator=g, dtype=F64, requires_grad=True)
    wgt = torch.randn(B, n, generator=g, dtype=F64)

    # materialised: only the live clouds' rows exist for the batch norm; the loss never sees a padding cloud
    up, _ = R.interp(C, idx, w)
    hpre = up[live] @ W + b
    mu, var = hpre.reshape(-1, Hd).mean(0), hpre.reshape(-1, Hd).var(0, unbiased=False)
    y = torch.relu((hpre - mu) * torch.rsqrt(var + eps) * gamma + beta)
    att_m = torch.sigmoid(y @ wfc + bfc)
    loss = (att_m * wgt[live]).sum()
    gC, gW, gg, gb, gwfc, gbfc = torch.autograd.grad(loss, [C, W, gamma, beta, wfc, bfc])

    # commuted, as train_ops does it
    with torch.no_grad():
        G = C @ W + b
        cnt = float(live.sum()) * n
        part, _ = R.interp_bn_colstats(G, idx, w, live)
        mean, rstd, scale, shift = R.bn_coeffs(part[0].sum(0), part[1].sum(0), cnt, gamma, beta, eps)
        att, _ = R.interp_head_rows(G, idx, w, scale, shift, wfc, float(bfc))
        assert torch.allclose(att[live], att_m, rtol=1e-12, atol=1e-14)
        dlogit = torch.where(live[:, None], wgt * att * (1 - att), torch.zeros(()).to(F64))   # sigmoid_bwd
        S, _ = R.interp_bn_bwd_sums(G, idx, w, dlogit, wfc, mean, rstd, gamma, beta, live)
        S = S.sum(1)
        k2, k3 = R.bn_bwd_coeffs(S[0], S[1], cnt, mean, rstd, scale)
        dG, _ = R.interp_bn_bwd_apply(G, idx, w, dlogit, wfc, scale, shift, k2, k3, live)
        dC, dW = dG @ W.t(), C.reshape(-1, Cin).t() @ dG.reshape(-1, Hd)
    for name, got, ref in (("dC", dC, gC), ("dW", dW, gW), ("dgamma", S[1], gg), ("dbeta", S[0], gb),
                           ("dwfc", S[2], gwfc), ("dbfc", dlogit.sum().reshape(1), gbfc)):
        err = float((got - ref).abs().max())
        assert err <= 1e-10 * float(ref.abs().max()) + 1e-13, (name, err)
    if padding != "none":
        assert float(dC[~live].abs().max()) == 0.0


def _netvlad_case(g, padding, clamp):
    B, n, m, D, K = 3, 48, 10, 16, 8
    idx, dist = _geometry(g, B, n, m)
    c = torch.randn(B, m, D, generator=g, dtype=F64)
    if clamp:   # two coarse rows of norm 7e-7; some points take all three neighbours there: |x|^2 <= 4.9e-13 < 1e-12
        c[:, :2] *= 7e-7 / c[:, :2].norm(dim=-1, keepdim=True)
        idx[:, 5:9, :] = 0
        idx[:, 9:11, :] = torch.tensor([0, 1, 1], dtype=torch.int32)
    return B, n, m, D, K, idx, dist, c.requires_grad_(), _mask(B, padding)


@pytest.mark.parametrize("padding,clamp", [("none", False), ("first", True), ("last", True), ("none", True)])
def test_netvlad_restatement_is_autograd_of_the_materialised_graph(padding, clamp):
    g = torch.Generator().manual_seed(21 + clamp)
    B, n, m, D, K, idx, dist, c, live = _netvlad_case(g, padding, clamp)
    eps = 1e-3
    w = R.idw_weights(dist)
    Wc = (torch.randn(D, K, generator=g, dtype=F64) / D ** 0.5).requires_grad_()
    gamma = (0.5 + torch.rand(K, generator=g, dtype=F64)).requires_grad_()
    beta = torch.randn(K, generator=g, dtype=F64, requires_grad=True)
    att = torch.rand(B, n, generator=g, dtype=F64, requires_grad=True)
    dV = torch.randn(B, K, D, generator=g, dtype=F64) * live[:, None, None]
    dasum = torch.randn(B, K, generator=g, dtype=F64) * live[:, None]

    # materialised (the batch norm sees the live rows only)
    x, _ = R.interp(c, idx, w)
    xn = x * torch.rsqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=R.EPS_L2))
    s_m = xn @ Wc
    sl = s_m[live].reshape(-1, K)
    mu, var = sl.mean(0), sl.var(0, unbiased=False)
    z = (s_m - mu) * torch.rsqrt(var + eps) * gamma + beta
    a = torch.softmax(z, -1) * att[..., None]
    V_m, asum_m = a.transpose(1, 2) @ xn, a.sum(1)
    loss = ((V_m * dV)[live].sum() + (asum_m * dasum)[live].sum())
    gc, gWc, gg, gb, gatt = torch.autograd.grad(loss, [c, Wc, gamma, beta, att])

    with torch.no_grad():
        cd, Wd = c.detach(), Wc.detach()
        cnt = float(live.sum()) * n
        f = R.nv_fwd_stats(cd, cd @ Wd, idx, w, live)
        assert bool(f["clamped"].any()) == clamp
        mean, rstd, scale, shift = R.bn_coeffs(f["part"][0].sum(0), f["part"][1].sum(0), cnt, gamma, beta, eps)
        fa = R.nv_fwd_assign(f["s"], f["rinv"], att, scale, shift, idx, w, m, live)
        V = fa["Ap"].transpose(1, 2) @ cd
        assert torch.allclose(V[live], V_m[live], rtol=1e-10, atol=1e-12)
        assert torch.allclose(fa["asum"][live], asum_m[live], rtol=1e-12, atol=1e-14)
        E = cd @ dV.transpose(1, 2)
        bs = R.nv_bwd_sums(E, fa["p"], f["s"], att, f["rinv"], dasum, mean, rstd, idx, w, live)
        S1, S2 = bs["part"][0].sum(0), bs["part"][1].sum(0)
        k2, k3 = R.bn_bwd_coeffs(S1, S2, cnt, mean, rstd, scale)
        ba = R.nv_bwd_apply(bs["dz"], f["s"], f["rinv"], bs["t2"], scale, k2, k3, idx, w, m, f["clamped"], live=live)
        dWc = cd.reshape(-1, D).t() @ ba["dcw"].reshape(-1, K)
        dc0 = fa["Ap"] @ dV + ba["dcw"] @ Wd.t()
        dc, _ = R.interp_scatter_scaled(cd, ba["q"], idx, w, dc0, live)
        # the same with q taken at face value on the clamped rows (no zeroing): what a kernel without the rule computes
        ba_raw = R.nv_bwd_apply(bs["dz"], f["s"], f["rinv"], bs["t2"], scale, k2, k3, idx, w, m,
                                torch.zeros_like(f["clamped"]), live=live)
        dc_raw, _ = R.interp_scatter_scaled(cd, ba_raw["q"], idx, w, dc0, live)
    for name, got, ref in (("dc", dc, gc), ("dWc", dWc, gWc), ("dgamma", S2, gg), ("dbeta", S1, gb),
                           ("datt", bs["datt"], gatt)):
        err = float((got - ref).abs().max())
        assert err <= 1e-9 * float(ref.abs().max()) + 1e-13, (name, err)
    if padding != "none":
        assert float(dc[~live].abs().max()) == 0.0 and float(bs["datt"][~live].abs().max()) == 0.0
    if clamp:   # on the coarse rows the clamped points use, q x is |x|^2 / 1e-12 of the true term there: not negligible
        rows = gc[live][:, :2]
        assert float((dc_raw[live][:, :2] - rows).abs().max()) > 0.05 * float(rows.abs().max())


def test_error_scales_bound_a_float32_evaluation():
    """The T of every restatement bounds the deviation of the same formulas evaluated from float32 inputs in float32
    (torch on the CPU): a sanity check that T is an error scale and not merely some positive number."""
    g = torch.Generator().manual_seed(5)
    B, n, m, Hd = 2, 300, 20, 64
    idx, dist = _geometry(g, B, n, m)
    w = R.idw_weights(dist)
    G = torch.randn(B, m, Hd, generator=g)
    h32 = (torch.gather(G, 1, idx.long().reshape(B, -1, 1).expand(-1, -1, Hd)).reshape(B, n, 3, Hd)
           * w.float()[..., None]).sum(2)
    part, T = R.interp_bn_colstats(G, idx, w)
    got = torch.stack([h32.sum(1), (h32 * h32).sum(1)]).double()
    assert bool(((got - part).abs() <= R.RTOL * T).all())
    # and T is not loose: the bound is a small fraction of one point's contribution
    assert float((R.RTOL * T[0]).max()) < 0.1 * float(h32.abs().mean())
