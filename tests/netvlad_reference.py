"""float64 numpy restatements of the NetVLAD kernels (csrc/netvlad.hip) and of the global walk (csrc/dense_x6.hip,
dh3d_global_walk_planned_fwd), the yardstick of tests/test_netvlad_kernels_gpu.py; tests/test_netvlad_reference.py pins
it.  Written from the contracts in include/dh3d_hip.h and the formulas above VladTail in csrc/dense_x6.hip, not from the
kernels' control flow.

Every function returns (value, E, ...): E is an a-priori bound on |f32 kernel - value|, element by element, computed from
the inputs and the float64 values alone.  (tests/dense_reference.py returns a scale T and leaves the depth factor to
the caller; here stages of different depth follow each other, so each stage multiplies its own (K + 16) 2^-24 in --
`dense_reference.bound` -- and passes an absolute E on.)  The rules:
  sums            (K + 16) 2^-24 T, T the same sum over absolute values, K the number of terms: any order of f32 additions;
  normalisation   y = v rsqrt(max(|v|^2, eps)):  dy <= dv / |v| + |y| (sum_d |y_d| dv_d / |v| + (K + 16) 2^-25 + A_RSQ + 3 2^-24)
                  (sum |y_d| dv_d is the first-order change of |v|, never above |dv|_2; the clamp is continuous);
  softmax         p_k moves by p_k ((1 - p_k) dl_k + sum_{j != k} p_j dl_j) for logit errors dl -- never above p_k 2 max dl;
  exponentials    the device's exp(x), x <= 0, is within A_EXP (1 + |x|) of relative error (the fast exponential takes
                  2^(x log2 e): the product's rounding grows with |x|); a softmax output carries that of its own term plus
                  the p-weighted mean of the others' (the sum);
  rsqrt           relative A_RSQ;
  underflow       every product that can fall under the smallest normal f32 carries 2^-126, absolute.
A_EXP and A_RSQ are the two measured numbers (tests/test_netvlad_kernels_gpu.py, test_allowances_are_measured, and the
header of that file); A_SIG is the sigmoid allowance of tests/test_dense_kernels_gpu.py.

`dt` = numpy.float32 evaluates the same formulas in float32 numpy (test_netvlad_reference.py: the unmutated reference in
f32 must stay under E); `mut` names ONE deliberate mistake (the mutations of test_netvlad_reference.py: each must exceed
E tenfold on the case built to catch it).  The input generators of the two test files are at the end."""
import zlib

import numpy as np

import dense_reference as D

F64 = np.float64
EPS32 = D.EPS32
A_EXP = 3e-7     # four times the measured worst error, one digit up: the header of tests/test_netvlad_kernels_gpu.py
A_RSQ = 2e-7
A_SIG = 4e-7     # tests/test_dense_kernels_gpu.py
CLAMP = 1e-12    # every l2 clamp of the aggregation
TINY = 2.0 ** -126   # a product under the smallest normal f32 may be flushed or rounded to a denormal: absolute, per term
DM, CL, OD = 256, 64, 256


def _a(x, dt):
    return None if x is None else np.asarray(x, dt)


def _softmax(l, El, dt):
    """softmax over the last axis -> (p, relative error bound of p)."""
    x = l - l.max(-1, keepdims=True)
    e = np.exp(x)
    p = e / e.sum(-1, keepdims=True)
    Ex = El + EPS32 * np.abs(x)                                        # the subtraction of the maximum
    prop = (1 - p) * Ex + ((p * Ex).sum(-1, keepdims=True) - p * Ex)
    prop = prop * np.exp(2 * Ex.max(-1, keepdims=True))                # beyond first order, point by point
    ax = 1 + np.abs(x)
    ex = A_EXP * (ax + (p * ax).sum(-1, keepdims=True))
    return p.astype(dt), prop + ex + D.rel_bound(l.shape[-1]) + 3 * EPS32


def normalize(v, Ev, eps, depth, dt=F64):
    """over the last axis -> (y, Ey, ss)."""
    ss = (v * v).sum(-1, keepdims=True)
    nrm = np.sqrt(np.maximum(ss, dt(eps)))
    y = v / nrm
    dn = (np.abs(y) * Ev).sum(-1, keepdims=True)
    Ey = Ev / nrm + np.abs(y) * (dn / nrm + 0.5 * D.rel_bound(depth) + A_RSQ + 3 * EPS32)
    return y, Ey, ss[..., 0]


def _finish(V, EV, asum, Easum, W2, dt, mut):
    """V [B, Cl, D], asum [B, Cl], W2 [D, Cl] -> dict: v (un-normalised V - asum W2), y (intra-normalised, flattened
    d-major), tot (|y|^2 per cloud) and their bounds."""
    W2t = W2.T if "w2_transposed" not in mut else W2.reshape(CL, DM)
    sub = asum[:, :, None] * W2t[None]
    if "no_asum_w2" in mut:
        sub = sub * 0
    v = V - sub
    Ev = EV + Easum[:, :, None] * np.abs(W2t)[None] + 2 * EPS32 * (np.abs(V) + np.abs(sub))
    y, Ey, _ = normalize(v, Ev, CLAMP, DM, dt)
    if "cluster_not_normalized" in mut:
        y[:, 5] = v[:, 5]
    B = V.shape[0]
    if "flatten_c_major" in mut:
        yf, Eyf = y.reshape(B, -1), Ey.reshape(B, -1)
    else:
        yf, Eyf = y.transpose(0, 2, 1).reshape(B, -1), Ey.transpose(0, 2, 1).reshape(B, -1)
    yf, Eyf = np.ascontiguousarray(yf), np.ascontiguousarray(Eyf)
    tot = (yf * yf).sum(-1)
    Etot = (2 * np.abs(yf) * Eyf).sum(-1) + D.rel_bound(DM * CL) * tot
    return dict(v=v, Ev=Ev, y=yf, Ey=Eyf, tot=tot, Etot=Etot, asum=asum, Easum=Easum)


def _whole(f, dt):
    """the whole-vector normalisation of _finish's y -> (vlad, E)."""
    vl, E, _ = normalize(f["y"], f["Ey"], CLAMP, DM * CL, dt)
    return vl, E


def _assign(x, att, Wc, cl_scale, cl_shift, dt, mut):
    """-> xn, its relative bound, a = softmax(bn(xn Wc)) att and its bound."""
    ss = (x * x).sum(-1, keepdims=True)
    rinv = 1 / np.sqrt(np.maximum(ss, dt(CLAMP)))
    r_xn = 0.5 * D.rel_bound(x.shape[-1]) + A_RSQ + EPS32
    xn = x * rinv
    z = xn @ Wc
    Ez = (D.rel_bound(x.shape[-1]) + r_xn) * (np.abs(xn) @ np.abs(Wc))
    sh = cl_shift
    if "cl_shift_swapped" in mut:
        sh = sh.copy()
        sh[[3, 4]] = sh[[4, 3]]
    l = z * cl_scale + sh
    El = Ez * np.abs(cl_scale) + EPS32 * np.abs(l)
    p, rp = _softmax(l, El, dt)
    a = p * att[..., None]
    return xn, r_xn, a, a * (rp + EPS32) + TINY


def aggregate(x, att, Wc, cl_scale, cl_shift, W2, dt=F64, mut=(), detail=False):
    """x [B, N, D], att [B, N], Wc [D, Cl], cl_scale / cl_shift [Cl], W2 [D, Cl] -> vlad [B, D Cl], E (, detail dict with
    v = V - asum W2 [B, Cl, D], asum [B, Cl], y, tot and their bounds)."""
    x, att, Wc, W2 = _a(x, dt), _a(att, dt), _a(Wc, dt), _a(W2, dt)
    cl_scale, cl_shift = _a(cl_scale, dt), _a(cl_shift, dt)
    N = x.shape[1]
    xn, r_xn, a, Ea = _assign(x, att, Wc, cl_scale, cl_shift, dt, mut)
    keep = np.ones(N, bool)
    if "drop_tile_last" in mut:
        keep[63] = False                       # the last point of the first 64-point tile
    if "drop_cloud_last" in mut:
        keep[N - 1] = False
    if "drop_chunk" in mut:
        ch, tiles = mut_chunks(x.shape[0], N), (N + 63) // 64
        keep[64 * (tiles * (ch - 1) // ch):] = False
    a, Ea, xn = a[:, keep], Ea[:, keep], xn[:, keep]
    n = a.shape[1]
    asum = a.sum(1)
    Easum = Ea.sum(1) + D.rel_bound(n) * asum
    V = np.einsum("bnc,bnd->bcd", a, xn)
    EV = np.einsum("bnc,bnd->bcd", Ea + a * r_xn, np.abs(xn)) + D.rel_bound(n) * np.einsum("bnc,bnd->bcd", a, np.abs(xn))
    f = _finish(V, EV, asum, Easum, W2, dt, mut)
    vl, E = _whole(f, dt)
    return (vl, E, f) if detail else (vl, E)


def mut_chunks(B, N):
    """the chunk count the header of csrc/netvlad.hip states: 256 / B, at most 16, at most the tile count, at least 1."""
    return max(1, min(256 // B, 16, (N + 63) // 64))


def head(vlad, Wh, s1, h1, Wg, s2, h2, l2_eps, tot=None, E_vlad=None, E_tot=None, dt=F64, mut=()):
    """h = bn1(vlad Wh [rsqrt(max(tot, 1e-12))]); out = h sigmoid(bn2(h Wg)) (Wg None: h); l2_eps > 0: out
    rsqrt(max(|out|^2, l2_eps)).  vlad [B, Kd] -> out [B, O], E."""
    vlad, Wh, s1, h1 = _a(vlad, dt), _a(Wh, dt), _a(s1, dt), _a(h1, dt)
    Kd = vlad.shape[1]
    E_vlad = np.zeros_like(vlad) if E_vlad is None else E_vlad
    keepk = Kd
    if "drop_k_mod_256" in mut:
        keepk = Kd - Kd % 256
    if "drop_last_8" in mut:
        keepk = Kd - 8
    h0 = vlad[:, :keepk] @ Wh[:keepk]
    E0 = D.rel_bound(Kd) * (np.abs(vlad) @ np.abs(Wh)) + E_vlad @ np.abs(Wh)
    if tot is not None:
        tot = _a(tot, dt)[:, None]
        sc = 1 / np.sqrt(np.maximum(tot, dt(CLAMP)))
        E_tot = np.zeros_like(tot) if E_tot is None else np.asarray(E_tot)[:, None]
        h0 = h0 * sc
        E0 = E0 * sc + np.abs(h0) * (0.5 * E_tot / np.maximum(tot, CLAMP) + A_RSQ + EPS32)
    h = h0 * s1 + h1
    Eh = E0 * np.abs(s1) + EPS32 * np.abs(h)
    v, Ev = h, Eh
    if Wg is not None:
        Wg, s2, h2 = _a(Wg, dt), _a(s2, dt), _a(h2, dt)
        hg = h0 if "gate_before_bn1" in mut else h
        g0 = hg @ Wg
        g = g0 * s2 + h2
        Eg = (D.rel_bound(Wg.shape[0]) * (np.abs(h) @ np.abs(Wg)) + Eh @ np.abs(Wg)) * np.abs(s2) + EPS32 * np.abs(g)
        sg = _a(D.sigmoid(g), dt)
        Esg = Eg / 4 + sg * (A_EXP * (1 + np.abs(g)) + 3 * EPS32)
        v = h * sg
        Ev = Eh * sg + np.abs(h) * Esg + EPS32 * np.abs(v)
    if l2_eps > 0:
        v, Ev, _ = normalize(v, Ev, CLAMP if "l2_eps_1e12" in mut else l2_eps, v.shape[-1], dt)
    return v, Ev


def fused(x, att, Wc, cl_scale, cl_shift, W2, Wh, s1, h1, Wg, s2, h2, l2_eps, dt=F64, mut=(), use_tot=True):
    """head(aggregate(...)); use_tot: the whole-vector factor applied behind the projection, as dh3d_netvlad_fused_fwd
    documents (the same function)."""
    vl, E, f = aggregate(x, att, Wc, cl_scale, cl_shift, W2, dt, mut, detail=True)
    if not use_tot:
        return head(vl, Wh, s1, h1, Wg, s2, h2, l2_eps, E_vlad=E, dt=dt, mut=mut)
    return head(f["y"], Wh, s1, h1, Wg, s2, h2, l2_eps, tot=f["tot"], E_vlad=f["Ey"], E_tot=f["Etot"], dt=dt, mut=mut)


def _attention(coarse, idx, dist, W_att, att_ep, w_fc, b_fc, dt):
    """sigmoid(act(bn(interp(coarse) W_att + b)) . w_fc + b_fc) [B, n] and its bound (dense_reference.interp_head)."""
    v, T, S = D.interp_head(coarse, idx, dist, W_att, w_fc, b_fc, att_ep)
    E = D.bound(T, np.shape(coarse)[-1] + 3 + np.shape(W_att)[-1], S, A_SIG)[..., 0]
    if dt is F64:
        return v[..., 0], E
    pb, sc, sh, act = att_ep if att_ep is not None else (None, None, None, D.ACT_NONE)
    w = _a(D.idw_weights(dist), dt)[..., None]
    b = np.arange(len(coarse))[:, None, None]
    hid = ((_a(coarse, dt) @ _a(W_att, dt))[b, np.asarray(idx, np.int64)] * w).sum(2)
    hid = hid + _a(pb, dt) if pb is not None else hid
    hid = hid * _a(sc, dt) if sc is not None else hid
    hid = hid + _a(sh, dt) if sh is not None else hid
    hid = np.maximum(hid, 0) if act == D.ACT_RELU else hid
    z = hid @ _a(w_fc, dt) + dt(b_fc)
    return (1 / (1 + np.exp(-z))).astype(dt), E


def walk(coarse, Wc, idx, dist, W_att, att_ep, w_fc, b_fc, cl_scale, cl_shift, dt=F64, mut=(), att=None):
    """coarse [B, m, 256], idx / dist [B, n, 3] -> att [B, n], apart [B, m, 64], asum [B, 64] and their bounds, as
    (att, E_att, apart, E_apart, asum, E_asum).  att given: used instead of the attention head (its bound 0)."""
    c, Wc = _a(coarse, dt), _a(Wc, dt)
    cl_scale, cl_shift = _a(cl_scale, dt), _a(cl_shift, dt)
    B, m, _ = c.shape
    n = np.shape(idx)[1]
    ix = np.asarray(idx, np.int64)
    bb = np.arange(B)[:, None, None]
    if att is None:
        att, E_att = _attention(coarse, idx, dist, W_att, att_ep, w_fc, b_fc, dt)
    else:
        att, E_att = _a(att, dt), np.zeros(np.shape(att))
    d = np.asarray(dist, F64)
    r = 1.0 / np.maximum(d, 1e-12 if "dist_clamp_1e12" in mut else D.DIST_CLAMP)
    w = _a(r / r.sum(-1, keepdims=True), dt)                          # [B, n, 3]
    r_w = 4 * EPS32
    x = (c[bb, ix] * w[..., None]).sum(2)
    Ex = (D.rel_bound(3) + r_w) * (np.abs(c)[bb, ix] * w[..., None]).sum(2)
    ss = (x * x).sum(-1)
    Ess = (2 * np.abs(x) * Ex).sum(-1) + D.rel_bound(c.shape[-1]) * ss
    den = np.maximum(ss, dt(CLAMP))
    rinv = 1 / np.sqrt(den)
    r_inv = 0.5 * Ess / den + A_RSQ
    cw = c @ Wc
    Ecw = D.rel_bound(c.shape[-1]) * (np.abs(c) @ np.abs(Wc))
    mix = (cw[bb, ix] * w[..., None]).sum(2)
    Emix = (Ecw[bb, ix] * w[..., None]).sum(2) + (D.rel_bound(3) + r_w) * (np.abs(cw)[bb, ix] * w[..., None]).sum(2)
    z = mix * rinv[..., None]
    Ez = np.abs(z) * (r_inv[..., None] + 2 * EPS32) + rinv[..., None] * Emix
    l = z * cl_scale + cl_shift
    El = Ez * np.abs(cl_scale) + EPS32 * np.abs(l)
    p, rp = _softmax(l, El, dt)
    a = p * att[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        r_att = np.where(att > 0, E_att / att, 0.0)
    ra = rp + 3 * EPS32 + r_att[..., None]
    Ea = a * ra + TINY
    asum = a.sum(1)
    Easum = Ea.sum(1) + D.rel_bound(n) * asum
    apart, Eap, refs = np.zeros((B, m, CL), dt), np.zeros((B, m, CL)), np.zeros((B, m))
    live = np.ones(n, bool)
    if "walk_drop_last" in mut:
        live[n - 1] = False
    for t in range(3):
        wt = w[..., (t + 1) % 3] if "walk_wrong_slot" in mut else w[..., t]
        cf = wt if "walk_no_rinv" in mut else wt * rinv
        use = live[None, :] & np.ones((B, n), bool)
        if "walk_dup_once" in mut:                                    # a repeated neighbour counted once
            for u in range(t):
                use = use & (ix[..., u] != ix[..., t])
        term = a * (cf * use)[..., None]
        Et = term * (ra + (r_w + r_inv + 2 * EPS32)[..., None]) + 2 * TINY
        for b in range(B):
            np.add.at(apart[b], ix[b, :, t], term[b])
            np.add.at(Eap[b], ix[b, :, t], Et[b])
            np.add.at(refs[b], ix[b, :, t], 1.0)
    Eap = Eap + (refs[..., None] + 16) * EPS32 * apart
    return att, E_att, apart, Eap, asum, Easum


def tail_assign(apart, coarse, asum, W2, Wh, s1, h1, Wg, s2, h2, l2_eps, E_apart=None, E_asum=None, dt=F64, mut=(),
                detail=False):
    """V = apart^T coarse, then the finish of `aggregate` and `head` -> out [B, O], E."""
    ap, c, asum, W2 = _a(apart, dt), _a(coarse, dt), _a(asum, dt), _a(W2, dt)
    m = c.shape[1]
    E_apart = np.zeros(ap.shape) if E_apart is None else E_apart
    E_asum = np.zeros(asum.shape) if E_asum is None else E_asum
    V = np.einsum("bjc,bjd->bcd", ap, c)
    EV = D.rel_bound(m) * np.einsum("bjc,bjd->bcd", np.abs(ap), np.abs(c)) + np.einsum("bjc,bjd->bcd", E_apart, np.abs(c))
    f = _finish(V, EV, asum, E_asum, W2, dt, mut)
    out = head(f["y"], Wh, s1, h1, Wg, s2, h2, l2_eps, tot=f["tot"], E_vlad=f["Ey"], E_tot=f["Etot"], dt=dt, mut=mut)
    return out + (f,) if detail else out


# ================================================================================================ shared generators
def seed(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def bn(rng, n, spread=0.5):
    return ((0.5 + rng.random(n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32), \
        (spread * rng.standard_normal(n)).astype(np.float32)


def head_params(rng, Kd, gating=True):
    """Wh [Kd, O], s1, h1, Wg [O, O] or None, s2, h2."""
    Wh = (rng.standard_normal((Kd, OD)) / np.sqrt(Kd)).astype(np.float32)
    s1, h1 = bn(rng, OD)
    if not gating:
        return Wh, s1, h1, None, None, None
    Wg = (rng.standard_normal((OD, OD)) / np.sqrt(OD)).astype(np.float32)
    s2, h2 = bn(rng, OD)
    return Wh, s1, h1, Wg, s2, h2


def agg_params(rng, peak=3.0):
    """Wc scaled so that the largest assignment of a point is moderately peaked (0.3 .. 0.9 for unit rows), cluster BN,
    W2."""
    Wc = (peak * rng.standard_normal((DM, CL))).astype(np.float32)
    sc, sh = bn(rng, CL)
    W2 = (rng.standard_normal((DM, CL)) / 16).astype(np.float32)
    return Wc, sc, sh, W2


def agg_inputs(rng, B, N):
    """rows of mixed scale; cloud b leans towards feature b so that a cloud mixed up with another is O(1) wrong."""
    x = rng.standard_normal((B, N, DM)) * np.exp(rng.uniform(-3, 3, (B, N, 1)))
    x[np.arange(B), :, np.arange(B) % DM] += 3.0 * np.exp(rng.uniform(-3, 3, (B, N)))
    att = rng.random((B, N)) * 0.9 + 0.05
    return x.astype(np.float32), att.astype(np.float32)


# shapes of the aggregation: (B, N)
AGG_SHAPES = [(2, 1), (2, 63), (2, 64), (2, 65), (2, 200), (2, 1000), (1, 130), (8, 130), (9, 130), (17, 130), (33, 130),
              (257, 64), (16, 320)]


def agg_case(B, N):
    rng = seed("agg", B, N)
    return agg_inputs(rng, B, N) + agg_params(rng)


CLAMP_KINDS = ["zero_row", "zero_cloud", "zero_att_cloud", "saturated", "scaled"]


def clamp_case(kind):
    """the clamps of the aggregation inside a launch of two clouds of 130 points: a zero row in either cloud (one of them
    the last point), a cloud of zero rows, a cloud with zero attention beside a normal one, cluster logits of +-1e4 behind
    the BatchNorm, rows scaled by 2^-70 (under the 1e-12 clamp, as the contract has it), 2^-16 and 2^40 (scale-free)."""
    x, att, Wc, sc, sh, W2 = agg_case(2, 130)
    if kind == "zero_row":
        x[0, 5] = 0
        x[1, 129] = 0
    elif kind == "zero_cloud":
        x[1] = 0
    elif kind == "zero_att_cloud":
        att[0] = 0
    elif kind == "saturated":
        sh[[3, 9]] = np.float32([1e4, -1e4])
    elif kind == "scaled":
        x[:, 0::4] *= np.float32(2.0 ** -70)
        x[:, 1::4] *= np.float32(2.0 ** 40)
        x[:, 2::4] *= np.float32(2.0 ** -16)
    else:
        raise ValueError(kind)
    return x, att, Wc, sc, sh, W2


def selection_case(B=3, N=200, w2=False):
    """selection probe: x[n] = s_n e_{d(n)}, Wc[d, c(d)] = 40, att dyadic: V[c, d] = sum of att over the points of d (before the
    normalisations), every non-zero cell of a cloud another value, every cloud different."""
    rng = seed("sel", B, N, w2)
    nd = 24                                                     # features in use: d = 7 j + 11 b, clusters c(d) = (5 (d % 8) + 3) % 64
    x, att = np.zeros((B, N, DM), np.float32), np.zeros((B, N), np.float32)
    for b in range(B):
        dn = (7 * (np.arange(N) % nd) + 11 * b) % DM
        x[b, np.arange(N), dn] = 2.0 ** rng.integers(-20, 20, N)
        att[b] = (1 + (np.arange(N) % nd) + 32 * (np.arange(N) // nd % 2) + b) / 128.0
    Wc = np.zeros((DM, CL), np.float32)
    Wc[np.arange(DM), (5 * (np.arange(DM) % 8) + 3) % CL] = 40.0     # three features of a cloud per cluster: the
                                                                      # intra-normalisation keeps their ratios
    W2 = np.zeros((DM, CL), np.float32)
    if w2:                                                      # one-hot per cluster: column c holds -(c + 1) / 8 at d = 3 c + 1
        W2[(3 * np.arange(CL) + 1) % DM, np.arange(CL)] = -(np.arange(CL) + 1) / 8.0
    return x, att, Wc, np.ones(CL, np.float32), np.zeros(CL, np.float32), W2


def three_nn(fine, sub):
    """brute force: squared distances and ids of the three nearest rows of sub [B, m, 3] for fine [B, n, 3]."""
    d2 = ((np.asarray(fine, F64)[:, :, None] - np.asarray(sub, F64)[:, None]) ** 2).sum(-1)
    m = d2.shape[-1]
    if m < 3:
        d2 = np.concatenate([d2] * 3, -1)
    ix = np.argsort(d2, -1, kind="stable")[..., :3]
    return np.take_along_axis(d2, ix, -1).astype(np.float32), (ix % m).astype(np.int32)


def walk_geometry(rng, B, n, m, kind):
    """fine cloud [B, n, 3], idx, dist.  kind 'nn': three_nn lists of a random cloud against m of its neighbours (coherent:
    a 128-point block of the Morton order touches few rows); 'random': uniform ids (m >= 200: every block overflows the
    64 staged rows); 'mixed': even clouds 'nn', odd clouds 'random'.  Degenerate rows are planted in either."""
    fine = rng.random((B, n, 3)).astype(np.float32)
    sub = rng.random((B, m, 3)).astype(np.float32)
    dist, idx = three_nn(fine, sub)
    if kind != "nn":
        ri = rng.integers(0, m, (B, n, 3)).astype(np.int32)
        rd = (rng.random((B, n, 3)) * 1e-2 + 1e-4).astype(np.float32)
        sel = np.ones(B, bool) if kind == "random" else (np.arange(B) % 2 == 1)
        idx[sel], dist[sel] = ri[sel], rd[sel]
    k = np.arange(n)
    idx[:, k % 11 == 3, 1:] = idx[:, k % 11 == 3, :1]                 # all three the same coarse row
    idx[:, k % 11 == 5, 2] = idx[:, k % 11 == 5, 0]                   # two the same
    dist[:, k % 11 == 7, 0] = 0.0                                     # dist = 0: the 1e-10 clamp decides
    dist[:, k % 11 == 7, 1] = 3e-11
    dist[:, k % 11 == 9, :] = 0.0
    return fine, idx, dist


def walk_params(rng, Hd=256, act=D.ACT_RELU, ep=True, peak=3.0):
    W_att = (rng.standard_normal((DM, Hd)) / 16).astype(np.float32)
    att_ep = None
    if ep:
        s, h = bn(rng, Hd)
        att_ep = ((0.1 * rng.standard_normal(Hd)).astype(np.float32), s, h, act)
    w_fc = (rng.standard_normal(Hd) / np.sqrt(Hd)).astype(np.float32)
    Wc = (peak * 4 * rng.standard_normal((DM, CL))).astype(np.float32)
    sc, sh = bn(rng, CL)
    return W_att, att_ep, w_fc, 0.2, Wc, sc, sh


def coarse_rows(rng, B, m):
    """unit-scale rows; cloud b leans towards feature b."""
    c = rng.standard_normal((B, m, DM)) / 16
    c[np.arange(B), :, np.arange(B) % DM] += 0.5
    return c.astype(np.float32)


# the walk: (B, n, m, kind, Hd)
WALK_SHAPES = [(1, 1, 1, "nn", 256), (3, 127, 3, "nn", 256), (1, 128, 17, "nn", 256), (8, 129, 64, "nn", 256),
               (9, 300, 65, "mixed", 256), (3, 300, 200, "random", 256), (2, 129, 1024, "mixed", 256),
               (1, 300, 1024, "random", 1024), (9, 1, 200, "nn", 256)]


def walk_case(B, n, m, kind, Hd=256, act=D.ACT_RELU, ep=True):
    rng = seed("walk", B, n, m, kind, Hd, act, ep)
    fine, idx, dist = walk_geometry(rng, B, n, m, kind)
    return dict(fine=fine, idx=idx, dist=dist, coarse=coarse_rows(rng, B, m), B=B, n=n, m=m, Hd=Hd,
                par=walk_params(rng, Hd, act, ep))


def walk_ref(case, **kw):
    W_att, att_ep, w_fc, b_fc, Wc, sc, sh = case["par"]
    return walk(case["coarse"], Wc, case["idx"], case["dist"], W_att, att_ep, w_fc, b_fc, sc, sh, **kw)


# the head alone: vlad is arbitrary, not normalised
HEAD_KD = [8, 120, 128, 136, 256, 264, 1000, 16384]
HEAD_B = [1, 31, 32, 33]


def head_case(Kd, B, gating=True, clamp=False):
    """vlad rows of mixed scale.  clamp: a tiny bn1 shift and row 0 scaled down, so that |out|^2 of that row is under an
    l2_eps of 1e-3 and the clamp decides."""
    rng = seed("head", Kd, B, gating, clamp)
    vlad = (rng.standard_normal((B, Kd)) * np.exp(rng.uniform(-2, 2, (B, 1)))).astype(np.float32)
    par = list(head_params(rng, Kd, gating))
    if clamp:
        par[2] = (par[2] * 1e-3).astype(np.float32)
        vlad[0] *= np.float32(1e-4)
    return (vlad,) + tuple(par)


# the tail alone: synthetic apart / asum / coarse
TAIL_M = [1, 15, 16, 17, 625, 1024]
TAIL_B = [1, 7, 8, 9]


def tail_case(B, m, gating=True, zero_cloud=None, onehot=False):
    rng = seed("tail", B, m, gating, zero_cloud, onehot)
    coarse = coarse_rows(rng, B, m)
    apart = (rng.random((B, m, CL)) ** 4).astype(np.float32)
    if onehot:                                  # cluster k takes coarse row (k + 3 b) % m alone
        apart[:] = 0
        for b in range(B):
            apart[b, (np.arange(CL) + 3 * b) % m, np.arange(CL)] = 1.0 + np.arange(CL) / 64.0
    asum = (rng.random((B, CL)) * m / 8).astype(np.float32)
    if zero_cloud is not None:
        apart[zero_cloud], asum[zero_cloud] = 0, 0
    W2 = (rng.standard_normal((DM, CL)) / 16).astype(np.float32)
    return (apart, coarse, asum, W2) + head_params(rng, DM * CL, gating)
