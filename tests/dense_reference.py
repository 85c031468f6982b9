"""float64 numpy restatements of the dense matrix-pipe kernels (csrc/dense.hip, csrc/dense_x6.hip, csrc/dense_tail.hip),
the yardstick of tests/test_dense_kernels_gpu.py; tests/test_dense_reference.py pins it.  Written from the contracts in
include/dh3d_hip.h (section B) and the docstrings of dh3d_amd/pm.py, not from the kernels.

Every function returns (value, T) -- or (value, T, S) where the value went through a sigmoid.  T is the first-order
error scale of the value, as in tests/commuted_reference.py: the same sums taken over the absolute values of their terms,
T(a + b) = T(a) + T(b), T(a b) = T(a) |b| + |a| T(b), T(input) = |input|.  An f32 kernel that takes the same sums in any
order is within (Ktot + 16) 2^-24 T of the value, Ktot the length of the longest chain of additions behind an element
(`bound`).  S counts the sigmoids behind an element, each weighted by what multiplies it afterwards: the device's
sigmoid goes through a fast exponential whose error is an absolute allowance A_SIG, measured once, so the tests allow
bound(T) + A_SIG S.  A sigmoid passes T on divided by 4 (its slope is at most 1/4).

Branches.  ReLU is 1-Lipschitz, so a gate that an f32 rounding flips moves the output by no more than the rounding
itself: T of a ReLU output is T of its input where the gate is open or within the rounding of its threshold (|y| <
gate_tol * T(y), gate_tol = max(GATE_TOL, the relative bound of y)) and 0 where it is firmly shut -- either branch is
right there and the term the gate switches is in T at full size.  The l2 clamp max(sum x^2, eps) is continuous in the
same way: rows not firmly below the clamp carry the T of their squared norm into T of the reciprocal root.

The epilogue is common.h's dh3d_epilogue_apply: + pre_bias, x scale, + shift, act; a residual is added after act."""
import numpy as np

F64 = np.float64
EPS32 = 2.0 ** -24                        # unit roundoff of f32
SINGLE_PRODUCT_BOUND = 2.0 ** -20         # one bf16x6 product against the float64 product (test_dense_reference.py)
GATE_TOL = 1e-5
DIST_CLAMP = float(np.float32(1e-10))     # fmaxf(d, 1e-10f) of the inverse-distance weights
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2


def rel_bound(ktot):
    return (ktot + 16) * EPS32


def bound(T, ktot, S=None, a_sig=0.0):
    """|got - ref| allowed: (Ktot + 16) 2^-24 T (+ A_SIG S)."""
    b = rel_bound(ktot) * np.asarray(T, F64)
    return b if S is None else b + a_sig * np.asarray(S, F64)


def _f(x):
    return None if x is None else np.asarray(x, F64)


def sigmoid(z):
    z = np.asarray(z, F64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


# ------------------------------------------------------------------------------------------------- bf16x3 emulation
def _trunc_bf16(a):
    return (np.asarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def split3(a):
    """bf16x3.h split3: a (f32) -> c1, c2, c3 (f32 arrays holding bf16 values), truncation, exact remainders."""
    a = np.ascontiguousarray(a, np.float32)
    c1 = _trunc_bf16(a)
    r1 = a - c1
    c2 = _trunc_bf16(r1)
    r2 = r1 - c2
    return c1, c2, _trunc_bf16(r2)


SIX = ((1, 1), (1, 2), (2, 1), (1, 3), (3, 1), (2, 2))   # chunk products c_i d_j with i + j <= 4


def six_products(x, w, keep=SIX):
    """sum over (i, j) in `keep`, in that order, of c_i(x) d_j(w), every product and every partial sum rounded to f32
    (a product of two bf16 is exact in f32)."""
    c, d = split3(x), split3(w)
    acc = np.zeros(np.broadcast(c[0], d[0]).shape, np.float32)
    for i, j in keep:
        acc = (acc + c[i - 1] * d[j - 1]).astype(np.float32)
    return acc


# ------------------------------------------------------------------------------------------------- building blocks
def _relu(y, Ty, rtol):
    tol = max(GATE_TOL, rtol)
    live = (y > 0) | (np.abs(y) < tol * Ty)
    return np.maximum(y, 0.0), np.where(live, Ty, 0.0)


def epilogue(v, Tv, ep, ktot, Sv=None):
    """ep = (pre_bias, scale, shift, act), vectors over the last axis or None -> (value, T, S); S is None while no sigmoid
    is behind the value."""
    pb, sc, sh, act = ep if ep is not None else (None, None, None, ACT_NONE)
    pb, sc, sh = _f(pb), _f(sc), _f(sh)
    if pb is not None:
        v, Tv = v + pb, Tv + np.abs(pb)
    if sc is not None:
        v, Tv = v * sc, Tv * np.abs(sc)
        Sv = None if Sv is None else Sv * np.abs(sc)
    if sh is not None:
        v, Tv = v + sh, Tv + np.abs(sh)
    if act == ACT_RELU:
        v, Tv = _relu(v, Tv, rel_bound(ktot))          # (S passes a ReLU unchanged: it is 1-Lipschitz)
    elif act == ACT_SIGMOID:
        v, Tv = sigmoid(v), Tv / 4
        Sv = 1.0 + (0.0 if Sv is None else Sv / 4)
        Sv = np.broadcast_to(Sv, v.shape).copy()
    elif act != ACT_NONE:
        raise ValueError("act %r" % (act,))
    return v, Tv, Sv


def _ret(v, T, S):
    return (v, T) if S is None else (v, T, S)


def _cat(x1, x2):
    return _f(x1) if x2 is None else np.concatenate([_f(x1), _f(x2)], -1)


def matmul(x, Tx, W):
    W = _f(W)
    return x @ W, Tx @ np.abs(W)


def l2cat(v, Tv, prefix, eps, Sv=None):
    """[prefix | v / sqrt(max(sum v^2, eps))] over the last axis -> (value, T, S); the prefix columns are copies (T = 0:
    equal bit for bit).  S (None without a sigmoid behind v) goes through the same first-order rule as T."""
    ss, Tss = (v * v).sum(-1, keepdims=True), (2 * np.abs(v) * Tv).sum(-1, keepdims=True)
    den = np.maximum(ss, eps)
    rinv = 1.0 / np.sqrt(den)
    firmly_clamped = ss + GATE_TOL * Tss < eps
    Tr = rinv * (1.0 + np.where(firmly_clamped, 0.0, 0.5 * Tss / den))
    out, T = v * rinv, Tv * rinv + np.abs(v) * Tr
    S = None
    if Sv is not None:
        Sss = (2 * np.abs(v) * Sv).sum(-1, keepdims=True)
        S = Sv * rinv + np.abs(v) * rinv * np.where(firmly_clamped, 0.0, 0.5 * Sss / den)
    if prefix is not None:
        out = np.concatenate([_f(prefix), out], -1)
        T = np.concatenate([np.zeros_like(_f(prefix)), T], -1)
        S = None if S is None else np.concatenate([np.zeros_like(_f(prefix)), S], -1)
    return out, T, S


def l2norm_concat(x, eps, prefix=None):
    return l2cat(_f(x), np.abs(_f(x)), prefix, eps)[:2]


def idw_weights(dist):
    r = 1.0 / np.maximum(_f(dist), DIST_CLAMP)
    return r / r.sum(-1, keepdims=True)


def interp(rows, idx, dist, T_rows=None):
    """rows [B, m, C], idx / dist [B, n, 3] -> sum_t w_t rows[b, idx[b, i, t]] [B, n, C] and its T."""
    rows = _f(rows)
    T_rows = np.abs(rows) if T_rows is None else T_rows
    w = idw_weights(dist)[..., None]
    b = np.arange(rows.shape[0])[:, None, None]
    ix = np.asarray(idx, np.int64)
    return (rows[b, ix] * w).sum(2), (T_rows[b, ix] * w).sum(2)


def three_interpolate_idw(points, idx, dist):
    return interp(points, idx, dist)


def flex_pool(x, nbr):
    """max over the listed ids of the point's own cloud: x [B, N, C], nbr [B, N, K] -> [B, N, C] (exact: T = |value|)."""
    x = _f(x)
    p = x[np.arange(x.shape[0])[:, None, None], np.asarray(nbr, np.int64)].max(2)
    return p, np.abs(p)


# ------------------------------------------------------------------------------------------------- the operations
def linear(x1, W, x2=None, ep=None, residual=None):
    """epilogue([x1 | x2] @ W) + residual."""
    x = _cat(x1, x2)
    k = x.shape[-1]
    v, T = matmul(x, np.abs(x), W)
    v, T, S = epilogue(v, T, ep, k)
    if residual is not None:
        v, T = v + _f(residual), T + np.abs(_f(residual))
    return _ret(v, T, S)


def linear_slices(x1, W, slices):
    """x1 [R, C] @ W [C, 256 slices] in the layout [slices][R][256]."""
    v, T = linear(x1, W)
    R = v.shape[0]
    to = lambda a: np.ascontiguousarray(a.reshape(R, slices, 256).transpose(1, 0, 2))
    return to(v), to(T)


def upsample_linear(points, idx, dist, W, x2=None, ep=None, residual=None, l2=None, shortcut=None):
    """epilogue([interp(points) | x2] @ W) + residual; shortcut = (x3, W_sc, ep_sc): + epilogue_sc(x3 @ W_sc) instead;
    l2 = (prefix, eps): [prefix | l2_normalize(.)]."""
    u, Tu = interp(points, idx, dist)
    x = u if x2 is None else np.concatenate([u, _f(x2)], -1)
    Tx = Tu if x2 is None else np.concatenate([Tu, np.abs(_f(x2))], -1)
    k = x.shape[-1] + 3
    v, T = matmul(x, Tx, W)
    v, T, S = epilogue(v, T, ep, k)
    if shortcut is not None:
        x3, Wsc, ep_sc = shortcut
        k += np.shape(x3)[-1]
        r = linear(x3, Wsc, ep=ep_sc)
        v, T = v + r[0], T + r[1]
        if len(r) == 3:
            S = r[2] if S is None else S + r[2]
    elif residual is not None:
        v, T = v + _f(residual), T + np.abs(_f(residual))
    if l2 is not None:
        v, T, S = l2cat(v, T, l2[0], l2[1], S)
    return _ret(v, T, S)


def interp_combine(coarse_w, idx, dist, partial=None, ep=None, residual=None, l2=None):
    """act(BN(interp(coarse_w) + partial + pre_bias)) + residual, or [prefix | l2_normalize(.)]."""
    v, T = interp(coarse_w, idx, dist)
    if partial is not None:
        v, T = v + _f(partial), T + np.abs(_f(partial))
    v, T, S = epilogue(v, T, ep, 3)
    if residual is not None:
        v, T = v + _f(residual), T + np.abs(_f(residual))
    if l2 is not None:
        v, T, S = l2cat(v, T, l2[0], l2[1], S)
    return _ret(v, T, S)


def local_tail_fused(x1, x2, W_s, W_lower, ep_shortcut, ep_concat, coarse_w, idx, dist, prefix, l2_eps):
    """[prefix | l2_normalize(relu(BN_c(interp(coarse_w) + x2 W_lower + b_c)) + relu(BN_s(x1 W_s + b_s)))]; ep_* =
    (bias, scale, shift); prefix None: the sum itself."""
    u, Tu = interp(coarse_w, idx, dist)
    p, Tp = matmul(_f(x2), np.abs(_f(x2)), W_lower)
    k = np.shape(x2)[-1] + 3
    a, Ta, _ = epilogue(u + p, Tu + Tp, tuple(ep_concat) + (ACT_RELU,), k)
    s, Ts = linear(x1, W_s, ep=tuple(ep_shortcut) + (ACT_RELU,))
    v, T = a + s, Ta + Ts
    if prefix is not None:
        v, T, _ = l2cat(v, T, prefix, l2_eps)
    return v, T


def _head(hid_pre, T_pre, ep, w_fc, b_fc, ktot):
    hid, Th, Sh = epilogue(hid_pre, T_pre, ep, ktot)
    w = _f(w_fc)
    logit = hid @ w + float(b_fc)
    Tl = Th @ np.abs(w) + abs(float(b_fc))
    Sl = 0.0 if Sh is None else Sh @ np.abs(w)
    return sigmoid(logit)[..., None], (Tl / 4)[..., None], (1.0 + Sl / 4 + 0 * Tl)[..., None]


def mlp_head(h, W, w_fc, b_fc, ep=None):
    """sigmoid(act(BN(h @ W + b)) . w_fc + b_fc) [..., 1]."""
    h = _f(h)
    v, T = matmul(h, np.abs(h), W)
    return _head(v, T, ep, w_fc, b_fc, h.shape[-1])


def interp_head(coarse, idx, dist, W, w_fc, b_fc, ep=None):
    """mlp_head on interp(coarse), the wide conv taken on the coarse rows first: interp(coarse @ W)."""
    c = _f(coarse)
    H, TH = matmul(c, np.abs(c), W)
    v, T = interp(H, idx, dist, TH)
    return _head(v, T, ep, w_fc, b_fc, c.shape[-1] + 3)


def se_res(x, pool, W1, b1, W2, b2):
    """relu(x + x g), g = sigmoid(relu(pool @ W1 + b1) @ W2 + b2) -> (value, T, S).
    Ktot, the longest chain of sums feeding an element: C terms of pool @ W1 feed the hidden layer, C / 4 terms of the
    hidden layer feed the gate: C + C / 4 for the output (C alone for the hidden gate's own rounding tolerance).  S = |x|
    times the gate's: first order, the gate enters the output multiplied by x."""
    x, p = _f(x), _f(pool)
    C = x.shape[-1]
    h, Th, _ = epilogue(*matmul(p, np.abs(p), W1), (b1, None, None, ACT_RELU), C)
    z, Tz = matmul(h, Th, W2)
    g, Tg, Sg = epilogue(z, Tz, (b2, None, None, ACT_SIGMOID), C + C // 4)
    ax = np.abs(x)
    y, Ty, Sy = x + x * g, ax + ax * g + ax * Tg, ax * Sg
    on = x > 0                                   # 1 + g > 0: the gate is the sign of x, exact
    return np.where(on, y, 0.0), np.where(on, Ty, 0.0), np.where(on, Sy, 0.0)


def se_res_pool(x, nbr, W1, b1, W2, b2):
    return se_res(x, flex_pool(x, nbr)[0], W1, b1, W2, b2)


def se_res_pool_conv(x, nbr, W1, b1, W2, b2, Wc, ep):
    """-> (y, Ty, Sy), (z, Tz, Sz): y = se_res on flex_pool, z = epilogue(y @ Wc).  Ktot of z: the C + C / 4 of y, then the C
    terms of y @ Wc: 2 C + C / 4."""
    y, Ty, Sy = se_res_pool(x, nbr, W1, b1, W2, b2)
    C = y.shape[-1]
    v, T = matmul(y, Ty, Wc)
    S = Sy @ np.abs(_f(Wc))
    z, Tz, Sz = epilogue(v, T, ep, 2 * C + C // 4, S)
    return (y, Ty, Sy), (z, Tz, Sz)
