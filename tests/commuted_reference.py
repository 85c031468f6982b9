"""float64 torch restatements of the commuted training walks (csrc/interp_train.hip, csrc/netvlad_train.hip) and the
forward of the attention head on the same rows, the yardstick of tests/test_commuted_*.py.  Written from the contracts
in include/dh3d_hip.h (the interp_bn_* / netvlad_commuted_* / three_interpolate_bwd_sorted / interp_scatter_scaled
block) and the kernels' header comments, not from the kernels.

Layouts (all clouds at once, by ORIGINAL point index): coarse rows G / c / cw / E [B, m, C]; idx / dist / weight
[B, n, 3]; per-point values [B, n] or [B, n, C]; live [B] bool (False: a padding cloud -- no statistics, zero
gradients).  interp(R)[b, i] = sum_t w[b, i, t] R[b, idx[b, i, t]] with the inverse-distance weights of
core/backbones.py:89-100 (distances clamped at 1e-10); interp_t is its adjoint.

Every function returns, next to each output, an error scale T of the same shape: the same sum taken over the absolute
values of its terms, propagated to first order (T(a + b) = T(a) + T(b), T(a b) = T(a) |b| + |a| T(b), T(input) =
|input|).  An f32 kernel that computes the same sums in any order lands within a few hundred ulps of T; the tests
allow RTOL * T.  Where a branch of the kernel is decided by an f32 value within rounding of its threshold (a ReLU gate
whose input is below GATE_TOL of its own scale, a row norm within GATE_TOL of the l2 clamp), either branch is right:
the term it switches is added to T at full size (divided by RTOL, so the bound covers it) and nothing else is forgiven.
"""
import numpy as np
import torch

F64 = torch.float64
RTOL = 1e-5                              # the tests' bound: |got - ref| <= RTOL * T + 1e-30
GATE_TOL = 1e-5                          # |y| below this fraction of T(y): the f32 gate may go either way
DIST_CLAMP = float(np.float32(1e-10))    # fmaxf(d, 1e-10f) of the IDW weights
EPS_L2 = float(np.float32(1e-12))        # tf.nn.l2_normalize's clamp as the kernels hold it


def _f(x):
    return x.to(F64)


def idw_weights(dist):
    """dist [B, n, 3] squared three_nn distances -> w [B, n, 3] = (1/max(d, 1e-10)) / sum_t (1/max(d_t, 1e-10))."""
    r = 1.0 / _f(dist).clamp_min(DIST_CLAMP)
    return r / r.sum(-1, keepdim=True)


def _live(v, live, dims):
    """v with the entries of padding clouds set to exactly 0 (NaN inputs there must not leak)."""
    if live is None:
        return v
    return torch.where(live.reshape((-1,) + (1,) * (dims - 1)), v, torch.zeros((), dtype=v.dtype, device=v.device))


def interp(rows, idx, w, T_rows=None):
    """rows [B, m, C] -> (interp(rows) [B, n, C], T).  T_rows: the error scale of rows (default |rows|)."""
    rows = _f(rows)
    B, n, _ = idx.shape
    C = rows.shape[2]
    ix = idx.long().reshape(B, n * 3, 1).expand(-1, -1, C)
    g = torch.gather(rows, 1, ix).reshape(B, n, 3, C)
    tg = torch.gather(rows.abs() if T_rows is None else _f(T_rows), 1, ix).reshape(B, n, 3, C)
    w = _f(w)[..., None]
    return (g * w).sum(2), (tg * w.abs()).sum(2)


def interp_t(vals, idx, w, m, T_vals=None):
    """Adjoint: vals [B, n, C] -> (out [B, m, C], T): out[b, j] = sum_{(i, t): idx[b, i, t] = j} w[b, i, t] vals[b, i]."""
    vals = _f(vals)
    B, n, C = vals.shape
    ix = idx.long().reshape(B, n * 3, 1).expand(-1, -1, C)
    w = _f(w)[..., None]
    out = torch.zeros(B, m, C, dtype=F64, device=vals.device)
    out.scatter_add_(1, ix, (vals[:, :, None, :] * w).reshape(B, n * 3, C))
    T = torch.zeros_like(out)
    tv = vals.abs() if T_vals is None else _f(T_vals)
    T.scatter_add_(1, ix, (tv[:, :, None, :] * w.abs()).reshape(B, n * 3, C))
    return out, T


def _gate(y, Ty):
    """(y > 0, ambiguous): the f32 value of y may have the other sign where |y| < GATE_TOL * T(y)."""
    return y > 0, y.abs() < GATE_TOL * Ty


# ---------------------------------------------------------------------------------------- attention head (interp_train)
def interp_bn_colstats(G, idx, w, live=None):
    """-> (part [2, B, Hd], T): per-cloud sum_n h and sum_n h^2 of h = interp(G) over the live clouds."""
    h, Th = interp(G, idx, w)
    part = torch.stack([_live(h.sum(1), live, 2), _live((h * h).sum(1), live, 2)])
    T = torch.stack([_live(Th.sum(1), live, 2), _live((2 * h.abs() * Th).sum(1), live, 2)])
    return part, T


def interp_head_rows(G, idx, w, scale, shift, w_fc, b_fc):
    """-> (att [B, n], T): sigmoid(relu(h scale + shift) . w_fc + b_fc), h = interp(G)."""
    h, Th = interp(G, idx, w)
    scale, shift, w_fc = _f(scale), _f(shift), _f(w_fc)
    y = h * scale + shift
    Ty = Th * scale.abs() + shift.abs()
    on, amb = _gate(y, Ty)
    r = torch.where(on, y, torch.zeros_like(y))
    Tr = torch.where(on | amb, Ty, torch.zeros_like(Ty))
    logit = (r * w_fc).sum(-1) + float(b_fc)
    Tl = (Tr * w_fc.abs()).sum(-1) + abs(float(b_fc))
    att = torch.sigmoid(logit)
    return att, att * (1 - att) * Tl + att


def interp_bn_bwd_sums(G, idx, w, dlogit, w_fc, mean, rstd, gamma, beta, live=None):
    """-> (part [3, B, Hd], T): per-cloud S1 = sum dz, S2 = sum dz xhat, S3 = sum dlogit relu(y), with xhat = (h - mean)
    rstd, y = xhat gamma + beta, dz = dlogit w_fc [y > 0] (dh3d_bn_bwd_sums for the rank-one dy = dlogit x w_fc)."""
    h, Th = interp(G, idx, w)
    mean, rstd, gamma, beta, w_fc = _f(mean), _f(rstd), _f(gamma), _f(beta), _f(w_fc)
    dl = _f(dlogit)[..., None]
    xh = (h - mean) * rstd
    Txh = (Th + mean.abs()) * rstd.abs()
    y = xh * gamma + beta
    Ty = Txh * gamma.abs() + beta.abs()
    on, amb = _gate(y, Ty)
    full = dl * w_fc
    zero = torch.zeros_like(y)
    dz = torch.where(on, full, zero)
    flip = torch.where(amb, full.abs() / RTOL, zero)            # a flipped gate moves dz by its full size
    Tdz = torch.where(on, full.abs(), zero) + flip
    S1, T1 = dz.sum(1), Tdz.sum(1)
    S2, T2 = (dz * xh).sum(1), (Tdz * xh.abs() + dz.abs() * Txh).sum(1)
    relu = torch.where(on, y, zero)
    S3, T3 = (dl * relu).sum(1), (dl.abs() * torch.where(on | amb, Ty, zero)).sum(1)
    part = torch.stack([_live(v, live, 2) for v in (S1, S2, S3)])
    T = torch.stack([_live(v, live, 2) for v in (T1, T2, T3)])
    return part, T


def interp_bn_bwd_apply(G, idx, w, dlogit, w_fc, scale, shift, k2, k3, live=None):
    """-> (dG [B, m, Hd], T): interp^T(scale dz - k2 - k3 h), dz = dlogit w_fc [h scale + shift > 0]."""
    m = G.shape[1]
    h, Th = interp(G, idx, w)
    scale, shift, k2, k3, w_fc = _f(scale), _f(shift), _f(k2), _f(k3), _f(w_fc)
    dl = _f(dlogit)[..., None]
    y = h * scale + shift
    Ty = Th * scale.abs() + shift.abs()
    on, amb = _gate(y, Ty)
    zero = torch.zeros_like(y)
    full = scale * dl * w_fc
    dh = torch.where(on, full, zero) - k2 - k3 * h
    Tdh = torch.where(on, full.abs(), zero) + torch.where(amb, full.abs() / RTOL, zero) + k2.abs() + k3.abs() * Th
    dG, T = interp_t(dh, idx, w, m, Tdh)
    return _live(dG, live, 3), _live(T, live, 3)


def three_interpolate_bwd(grad_out, idx, weight, m):
    """-> (grad_points [B, m, C], T): the backward of three_interpolate with explicit weights (tf_interpolate.cpp:131-153)."""
    return interp_t(grad_out, idx, weight, m)


def interp_scatter_scaled(c, q, idx, w, dc0, live=None):
    """-> (dc0 + interp^T(-q x), T), x = interp(c), q [B, n]: the l2-normalisation term of NetVLAD's commuted backward."""
    m = c.shape[1]
    x, Tx = interp(c, idx, w)
    q = _f(q)[..., None]
    d, T = interp_t(-q * x, idx, w, m, q.abs() * Tx)
    return _f(dc0) + _live(d, live, 3), _f(dc0).abs() + _live(T, live, 3)


# ---------------------------------------------------------------------------------------- NetVLAD (netvlad_train)
def nv_fwd_stats(c, cw, idx, w, live=None):
    """-> dict: s [B, n, 64] = rinv interp(cw), rinv [B, n] = rsqrt(max(|x|^2, 1e-12)) with x = interp(c), part [2, B, 64]
    = per-cloud sums / sums of squares of s, and the l2 clamp per point: `clamped` (|x|^2 <= 1e-12) and `clamp_amb`
    (|x|^2 within rounding of 1e-12), each output with its T ("T_s", ...)."""
    x, Tx = interp(c, idx, w)
    ss, Tss = (x * x).sum(-1), (2 * x.abs() * Tx).sum(-1)
    clamped = ss <= EPS_L2
    amb = (ss - EPS_L2).abs() <= GATE_TOL * Tss
    rinv = torch.rsqrt(ss.clamp_min(EPS_L2))
    Tr = rinv * (1 + torch.where(clamped, torch.zeros_like(ss), 0.5 * Tss / ss.clamp_min(EPS_L2)))
    u, Tu = interp(cw, idx, w)
    s = rinv[..., None] * u
    Ts = Tr[..., None] * u.abs() + rinv[..., None] * Tu
    part = torch.stack([_live(s.sum(1), live, 2), _live((s * s).sum(1), live, 2)])
    Tp = torch.stack([_live(Ts.sum(1), live, 2), _live((2 * s.abs() * Ts).sum(1), live, 2)])
    return dict(s=s, T_s=Ts, rinv=rinv, T_rinv=Tr, part=part, T_part=Tp, clamped=clamped, clamp_amb=amb)


def nv_fwd_assign(s, rinv, att, scale, shift, idx, w, m, live=None):
    """-> dict: p [B, n, 64] = softmax(s scale + shift), asum [B, 64] = sum_n p att, Ap [B, m, 64] = interp^T(p att
    rinv), each with its T."""
    s, rinv, att, scale, shift = _f(s), _f(rinv), _f(att), _f(scale), _f(shift)
    z = s * scale + shift
    Tz = (s * scale).abs() + shift.abs()
    p = torch.softmax(z, -1)
    # relative error of p_k: its own exponent's (rounding of z_k and of the exp) and the normaliser's
    Tp = p * (1 + Tz + (p * Tz).sum(-1, keepdim=True))
    a, Ta = p * att[..., None], Tp * att.abs()[..., None]
    asum, Tas = _live(a.sum(1), live, 2), _live(Ta.sum(1), live, 2)
    Ap, TAp = interp_t(a * rinv[..., None], idx, w, m, Ta * rinv.abs()[..., None])
    return dict(p=p, T_p=Tp, asum=asum, T_asum=Tas, Ap=_live(Ap, live, 3), T_Ap=_live(TAp, live, 3))


def nv_bwd_sums(E, p, s, att, rinv, dasum, mean, rstd, idx, w, live=None):
    """-> dict: dz [B, n, 64] (softmax backward of da att, da = rinv interp(E) + dasum), datt [B, n] = sum_k da p (0 on
    padding clouds), t2 [B, n] = sum_k p att interp(E), part [2, B, 64] = per-cloud sums of dz and dz (s - mean) rstd."""
    e, Te = interp(E, idx, w)
    p, s, att, rinv, dasum = _f(p), _f(s), _f(att)[..., None], _f(rinv)[..., None], _f(dasum)[:, None, :]
    mean, rstd = _f(mean), _f(rstd)
    da, Tda = rinv * e + dasum, rinv.abs() * Te + dasum.abs()
    datt, Tdatt = (da * p).sum(-1), (Tda * p.abs()).sum(-1)
    dp, Tdp = da * att, Tda * att.abs()
    inner, Tin = (dp * p).sum(-1, keepdim=True), (Tdp * p.abs()).sum(-1, keepdim=True)
    dz, Tdz = p * (dp - inner), p.abs() * (Tdp + Tin)
    t2, Tt2 = (p * att * e).sum(-1), (p.abs() * att.abs() * Te).sum(-1)
    sh, Tsh = (s - mean) * rstd, (s.abs() + mean.abs()) * rstd.abs()
    part = torch.stack([_live(dz.sum(1), live, 2), _live((dz * sh).sum(1), live, 2)])
    Tp = torch.stack([_live(Tdz.sum(1), live, 2), _live((Tdz * sh.abs() + dz.abs() * Tsh).sum(1), live, 2)])
    return dict(dz=dz, T_dz=Tdz, datt=_live(datt, live, 2), T_datt=_live(Tdatt, live, 2), t2=t2, T_t2=Tt2, part=part,
                T_part=Tp)


def nv_bwd_apply(dz, s, rinv, t2, k1, k2, k3, idx, w, m, clamped, clamp_amb=None, live=None):
    """-> dict: q [B, n] = rinv^2 sum_k ds s + rinv^3 t2 where the row norm is live and 0 where the l2 clamp held it
    (`clamped`: then rinv is a constant and has no gradient), dcw [B, m, 64] = interp^T(rinv ds), with ds = k1 dz - k2 -
    k3 s."""
    dz, s, rinv, t2 = _f(dz), _f(s), _f(rinv), _f(t2)
    k1, k2, k3 = _f(k1), _f(k2), _f(k3)
    ds = k1 * dz - k2 - k3 * s
    Tds = (k1 * dz).abs() + k2.abs() + (k3 * s).abs()
    g, Tg = (ds * s).sum(-1), (Tds * s.abs()).sum(-1)
    qf = rinv ** 2 * g + rinv ** 3 * t2
    Tq = rinv ** 2 * Tg + (rinv ** 3 * t2).abs()
    zero = torch.zeros_like(qf)
    q = torch.where(clamped, zero, qf)
    Tq = torch.where(clamped, zero, Tq)
    if clamp_amb is not None:
        Tq = Tq + torch.where(clamp_amb, qf.abs() / RTOL, zero)
    dcw, Tdcw = interp_t(rinv[..., None] * ds, idx, w, m, rinv.abs()[..., None] * Tds)
    return dict(q=q, T_q=Tq, dcw=_live(dcw, live, 3), T_dcw=_live(Tdcw, live, 3))


# ---------------------------------------------------------------------------------------- BatchNorm glue (host side)
def bn_coeffs(s1, s2, cnt, gamma, beta, eps):
    """Column sums over the live rows -> mean, rstd, scale, shift of the training-mode batch norm (biased variance)."""
    mean = s1 / cnt
    var = s2 / cnt - mean * mean
    rstd = torch.rsqrt(var + eps)
    scale = _f(gamma) * rstd
    return mean, rstd, scale, _f(beta) - mean * scale


def bn_bwd_coeffs(S1, S2, cnt, mean, rstd, scale):
    """(S1, S2) -> k2, k3 of dx = scale dz - k2 - k3 x == gamma rstd (dz - S1/cnt - xhat S2/cnt)."""
    k3 = scale * rstd * S2 / cnt
    return scale * S1 / cnt - k3 * mean, k3
