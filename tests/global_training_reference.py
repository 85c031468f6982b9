"""float64 torch restatements of the BatchNorm family and the global head's training kernels (csrc/train.hip: bn_colstats,
bn_finalize[_parts], scale_shift_act[_res], bn_bwd_sums, bn_bwd_finalize[_parts], bn_bwd_apply, bn_small_fwd / _bwd,
row_logit_sigmoid, sigmoid_bwd, netvlad_assign_rows[_bwd], context_gate, l2norm_rows_bwd, vlad_normalize, quadruplet_loss)
and of the two autograd nodes built from them (train_ops.attention_head / netvlad_assign), the yardstick of
tests/test_global_training_*.py.  Written from the contracts in include/dh3d_hip.h and the formulas of the reference
model (BN_train with biased variance, the moving variance Bessel-corrected or not; softmax(bn(s)) * att; intra-normalise
then L2 with the 1e-12 clamps; the lazy quadruplet loss), not from the kernels.

The convention is tests/commuted_reference.py's: every function returns, next to each output, an error scale T of the
same shape -- the same sum over the absolute values of its terms, propagated to first order.  Here the propagation is
done once, by the class E (a value with its T): T(input) = |input|, T(a + b) = T(a) + T(b), T(a b) = T(a) |b| + |a| T(b),
T(exp z) = exp(z) (1 + T(z)), T(sigmoid z) = s (1 - s) T(z) + s, T(rsqrt a) = rsqrt(a) (1 + T(a) / (2 a)).  Steps a kernel
takes in float64 (the finalize kernels' arithmetic on their f64 sums, bn_small's accumulation) add their terms weighed
by F64_STEP = 2^-29, the ratio of the two unit roundoffs.  The tests allow RTOL * T.

ReLU gates need no forgiveness: the gate of a BatchNorm site is a function of the f32 tensors x, scale, shift that the
test holds, and x.double() * scale.double() + shift.double() > 0 has exactly the sign of the f32 fmaf(x, scale, shift)
(the product is exact in float64, the sum correctly rounded).  `gate` is THE gate; every pass of a site must agree with
it bit for bit.  The only forgiven branches are the clamps max(ss, eps) of l2norm_rows_bwd and vlad_normalize: within
GATE_TOL of the threshold either branch is right, the term the branch switches enters T at full size (divided by RTOL).
"""
import numpy as np
import torch

from commuted_reference import EPS_L2, F64, GATE_TOL, RTOL, _f

F64_STEP = 2.0 ** -29


def f32(v):
    """A Python scalar as the kernels receive it (a float argument of the C ABI)."""
    return float(np.float32(v))


class E(object):
    """A float64 value v with its error scale t (same shape)."""

    def __init__(self, v, t=None):
        self.v = _f(v) if isinstance(v, torch.Tensor) else torch.tensor(float(v), dtype=F64)
        self.t = self.v.abs() if t is None else t

    @staticmethod
    def of(x, like=None):
        if isinstance(x, E):
            return x
        if not isinstance(x, torch.Tensor):
            x = torch.tensor(float(x), dtype=F64, device=like.v.device if like is not None else None)
        return E(x)

    def __add__(self, o):
        o = E.of(o, self)
        return E(self.v + o.v, self.t + o.t)

    __radd__ = __add__

    def __neg__(self):
        return E(-self.v, self.t)

    def __sub__(self, o):
        o = E.of(o, self)
        return E(self.v - o.v, self.t + o.t)

    def __rsub__(self, o):
        return E.of(o, self) - self

    def __mul__(self, o):
        o = E.of(o, self)
        return E(self.v * o.v, self.t * o.v.abs() + self.v.abs() * o.t)

    __rmul__ = __mul__

    def __matmul__(self, o):
        return E(self.v @ o.v, self.t @ o.v.abs() + self.v.abs() @ o.t)

    def __truediv__(self, o):
        o = E.of(o, self)
        return E(self.v / o.v, self.t / o.v.abs() + self.v.abs() * o.t / (o.v * o.v))

    def __getitem__(self, k):
        return E(self.v[k], self.t[k])

    def sum(self, *a, **k):
        return E(self.v.sum(*a, **k), self.t.sum(*a, **k))

    def reshape(self, *s):
        return E(self.v.reshape(*s), self.t.reshape(*s))

    def permute(self, *s):
        return E(self.v.permute(*s), self.t.permute(*s))

    def transpose(self, a, b):
        return E(self.v.transpose(a, b), self.t.transpose(a, b))

    def exact(self, scale=F64_STEP):
        """The same value as an input of a float64 step: its T weighed down."""
        return E(self.v, self.t * scale)

    def exp(self):
        e = self.v.exp()
        return E(e, e * (1 + self.t))

    def sigmoid(self):
        s = torch.sigmoid(self.v)
        return E(s, s * (1 - s) * self.t + s)

    def rsqrt(self):
        r = torch.rsqrt(self.v)
        return E(r, r * (1 + 0.5 * self.t / self.v))

    def softmax_last(self):
        """p = softmax(z): relative error of p_k = its own exponent's (rounding of z_k and of the exp) + the normaliser's
        (commuted_reference.nv_fwd_assign)."""
        p = torch.softmax(self.v, -1)
        return E(p, p * (1 + self.t + (p * self.t).sum(-1, keepdim=True)))

    def where(self, cond, other=None):
        """self where cond, else `other` (an E; default: exactly 0 with T = 0)."""
        if other is None:
            z = torch.zeros((), dtype=F64, device=self.v.device)
            return E(torch.where(cond, self.v, z), torch.where(cond, self.t, z))
        return E(torch.where(cond, self.v, other.v), torch.where(cond, self.t, other.t))

    def forgive(self, cond, size):
        """Where `cond`, a branch may go either way: the term it switches (|size|) enters T at full size."""
        return E(self.v, self.t + torch.where(cond, size.abs() / RTOL, torch.zeros_like(self.t)))

    def pair(self):
        return self.v, self.t


def Z(x):
    """Zero T: a constant that no rounding touches (masks, 0 / 1 factors)."""
    x = _f(x)
    return E(x, torch.zeros_like(x))


def C(v):
    """A Python scalar as an exact constant."""
    return Z(torch.tensor(float(v), dtype=F64))


def rows_live(R, mask, rows_per_cloud, device=None):
    """mask [clouds] (bool / bytes, None: all live), rows_per_cloud -> live [R] bool."""
    if mask is None:
        return torch.ones(R, dtype=torch.bool, device=device)
    return mask.to(torch.bool).repeat_interleave(int(rows_per_cloud))[:R]


def _rows(x, live):
    """x [R, ...] with the rows of padding clouds set to exactly 0 (NaN there must not leak)."""
    if live is None:
        return x
    return torch.where(live.reshape((-1,) + (1,) * (x.dim() - 1)), x, torch.zeros((), dtype=x.dtype, device=x.device))


def gate(x, scale, shift):
    """THE ReLU gate of a BatchNorm site: the sign of the f32 fmaf(x, scale, shift) (NaN: closed)."""
    assert x.dtype == scale.dtype == shift.dtype == torch.float32
    return x.double() * scale.double() + shift.double() > 0


def fold(mean, rstd, gamma, beta):
    """(scale, shift) as float32, as every kernel folds them: scale = fl(gamma rstd), shift = fl(beta - mean scale) in
    one rounding."""
    scale = (gamma.float() * rstd.float())
    shift = (beta.double() - mean.double() * scale.double()).float()
    return scale, shift


# -------------------------------------------------------------------------------------------------- BatchNorm, long form
def bn_colstats(x, live=None):
    """-> E (sum [C], sumsq [C]) of x [R, C] over the live rows."""
    x = E(_rows(x, live))
    return x.sum(0), (x * x).sum(0)


def bn_finalize(s1, s2, count, gamma, beta, eps, momentum, unbiased, run_mean, run_var):
    """s1, s2: E [C] (or [P, C] partial rows, summed here); count: float.  -> dict of E: mean, rstd, scale, shift,
    run_mean, run_var (running buffers bit-unchanged at count 0: their T is 0 then).  Exact f64 sums: pass s.exact()."""
    if s1.v.dim() == 2:
        s1, s2 = s1.sum(0), s2.sum(0)
    eps, momentum = f32(eps), f32(momentum)
    n = count if count > 1 else 1.0
    inv = C(1.0 / n)
    mean_d, ex2 = s1 * inv, s2 * inv                                     # float64 in the kernels
    var = ex2 - mean_d * mean_d
    var = E(var.v.clamp_min(0.0), var.t + (ex2.v + mean_d.v ** 2) * F64_STEP)
    mean = E(mean_d.v, mean_d.t + mean_d.v.abs())                        # stored as float32
    rstd = E(var.v + eps, var.t).rsqrt()
    scale = E(gamma) * rstd
    shift = E(beta) - mean * scale
    rm, rv = Z(run_mean), Z(run_var)                                     # count == 0: left alone, bit for bit
    if count > 0:
        uv = var * C(n / (n - 1.0)) if (unbiased and n > 1) else var
        uv = E(uv.v, uv.t + uv.v.abs())
        rm = C(momentum) * E(run_mean) + C(1 - momentum) * mean
        rv = C(momentum) * E(run_var) + C(1 - momentum) * uv
    return dict(mean=mean, rstd=rstd, scale=scale, shift=shift, run_mean=rm, run_var=rv)


def scale_shift_act(x, scale, shift, relu, residual=None):
    """-> E y [R, C] = act(x scale + shift) (+ residual, after the activation).  x, scale, shift: f32 tensors."""
    y = E(x) * E(scale) + E(shift)
    if relu:
        y = y.where(gate(x, scale, shift))
    if residual is not None:
        y = y + E(residual)
    return y


def _dy(dy, rowscale, colvec):
    if dy is not None:
        return E(dy)
    full = _f(rowscale)[:, None] * _f(colvec)[None, :]
    return E(full)            # one product of two inputs: T = |dy|


def bn_bwd_sums(x, mean, rstd, scale, shift, relu, dy=None, rowscale=None, colvec=None, live=None):
    """-> E (S1, S2, S3 or None) [C]: S1 = sum dz, S2 = sum dz xhat, S3 = sum rowscale act(y) (rank-one form only), over
    the live rows; xhat = (x - mean) rstd, y = x scale + shift, dz = dy [gate].  All arguments f32 tensors; (scale, shift)
    = fold(mean, rstd, gamma, beta)."""
    xs = _rows(x, live)
    on = gate(x, scale, shift) if relu else torch.ones_like(x, dtype=torch.bool)
    if live is not None:
        on = on & live[:, None]
    dz = _dy(None if dy is None else _rows(dy, live), None if rowscale is None else _rows(rowscale, live), colvec).where(on)
    xh = (E(xs) - E(mean)) * E(rstd)
    S3 = None
    if dy is None:
        y = E(xs) * E(scale) + E(shift)
        if relu:
            y = y.where(on)
        S3 = (E(_rows(rowscale, live))[:, None] * y).sum(0)
    return dz.sum(0), (dz * xh).sum(0), S3


def bn_bwd_finalize(S1, S2, count, mean, rstd, gamma):
    """S1, S2: E [C] or partial rows [P, C] -> dict of E: k2, k3 of bn_bwd_apply and grads = (sum S1, sum S2) as f32."""
    if S1.v.dim() == 2:
        S1, S2 = S1.sum(0), S2.sum(0)
    n = count if count > 1 else 1.0
    inv = C(1.0 / n)
    m1, m2 = S1 * inv, S2 * inv
    g, rs, mu = E(gamma), E(rstd), E(mean)
    m1 = E(m1.v, m1.t + m1.v.abs())          # rounded to f32 before the products
    m2 = E(m2.v, m2.t + m2.v.abs())
    k3 = E(g.v * rs.v * rs.v * m2.v, (g.v * rs.v * rs.v).abs() * m2.t)
    k2 = E(g.v * rs.v * m1.v - k3.v * mu.v, (g.v * rs.v).abs() * m1.t + k3.t * mu.v.abs())
    return dict(k2=k2, k3=k3, dbeta=E(S1.v, S1.t + S1.v.abs()), dgamma=E(S2.v, S2.t + S2.v.abs()))


def bn_bwd_apply(x, scale, shift, k2, k3, relu, dy=None, rowscale=None, colvec=None, live=None):
    """-> E dx [R, C] = scale dz - k2 - k3 x on the live rows, exactly 0 on the others; dz = dy [gate]."""
    xs = _rows(x, live)
    on = gate(x, scale, shift) if relu else torch.ones_like(x, dtype=torch.bool)
    dz = _dy(None if dy is None else _rows(dy, live), None if rowscale is None else _rows(rowscale, live), colvec).where(on)
    dx = E(scale) * dz - E(k2) - E(k3) * E(xs)
    if live is not None:
        dx = dx.where(live[:, None])
    return dx


def batch_norm_train(x, gamma, beta, eps, momentum, unbiased, relu, run_mean, run_var, dy, live=None, gate32=None):
    """The whole site as _BatchNormTrain / bn_small compose it (sums -> finalize -> apply, both directions) with the T of
    every step chained; gate32 = the f32 (scale, shift) the gate is taken from where the test holds the device's own
    (default: this function's statistics rounded to f32).  -> dict of E: y, dx, dgamma, dbeta, k2, k3, mean, rstd, scale,
    shift, run_mean, run_var, and the f32 tensors `scale32`, `shift32` the gate was taken from."""
    R = x.shape[0]
    cnt = float(R if live is None else int(live.sum()))
    s1, s2 = bn_colstats(x, live)
    st = bn_finalize(s1, s2, cnt, gamma, beta, eps, momentum, unbiased, run_mean, run_var)
    sc32, sh32 = gate32 if gate32 is not None else fold(st["mean"].v.float(), st["rstd"].v.float(), gamma, beta)
    on = gate(x, sc32, sh32) if relu else torch.ones_like(x, dtype=torch.bool)
    xs = E(_rows(x, live))
    y = xs * st["scale"] + st["shift"]
    y = y.where(on)
    onl = on if live is None else on & live[:, None]
    dz = E(_rows(dy, live)).where(onl)
    xh = (xs - st["mean"]) * st["rstd"]
    S1, S2 = dz.sum(0), (dz * xh).sum(0)
    n = cnt if cnt > 1 else 1.0
    m1, m2 = S1 * C(1.0 / n), S2 * C(1.0 / n)
    g = E(gamma)
    k3 = g * st["rstd"] * st["rstd"] * m2
    k2 = g * st["rstd"] * m1 - k3 * st["mean"]
    dx = st["scale"] * dz - k2 - k3 * xs
    if live is not None:
        dx = dx.where(live[:, None])
    out = dict(st)
    out.update(y=y, dx=dx, dgamma=S2, dbeta=S1, k2=k2, k3=k3, scale32=sc32, shift32=sh32)
    return out


# -------------------------------------------------------------------------------------------------- attention head rows
def row_logit_sigmoid(h, scale, shift, w, b):
    """-> E att [R] = sigmoid(sum_c relu(h scale + shift) w + b)."""
    y = scale_shift_act(h, scale, shift, True)
    return ((y * E(w)).sum(-1) + E(b).reshape(())).sigmoid()


def sigmoid_bwd(datt, att, live=None):
    """-> E (dlogit [n] = datt att (1 - att), 0 on padding rows; its sum)."""
    a = E(_rows(att, live))
    d = E(_rows(datt, live)) * a * (1.0 - a)
    if live is not None:
        d = d.where(live)
    return d, d.sum()


# -------------------------------------------------------------------------------------------------- NetVLAD assignment
def netvlad_assign_rows(s, scale, shift, att, rows_per_cloud=None):
    """-> E (a [R, 64] = softmax(s scale + shift) att, asum [R / rows_per_cloud, 64] or None, p)."""
    p = (E(s) * E(scale) + E(shift)).softmax_last()
    a = p * E(att)[:, None]
    asum = None if rows_per_cloud is None else a.reshape(-1, rows_per_cloud, a.v.shape[1]).sum(1)
    return a, asum, p


def netvlad_assign_rows_bwd(s, scale, shift, att, da):
    """-> E (dz [R, 64] = p (da att - sum_k da att p), datt [R] = sum_k da p)."""
    _, _, p = netvlad_assign_rows(s, scale, shift, att)
    da = E.of(da)
    datt = (da * p).sum(-1)
    dp = da * E(att)[:, None]
    inner = (dp * p).sum(-1)
    return p * (dp - inner[:, None]), datt


def context_gate(v, g, dy=None):
    """-> E y = v sigmoid(g); with dy: (y, dv = dy sig, dg = dy v sig (1 - sig))."""
    sig = E(g).sigmoid()
    y = E(v) * sig
    if dy is None:
        return y
    return y, E(dy) * sig, E(dy) * E(v) * sig * (1.0 - sig)


def l2norm_rows_bwd(x, dxn, eps=EPS_L2):
    """Backward of xn = x rsqrt(max(sum x^2, eps)): dx = inv dxn - x inv^3 (x . dxn) where the norm is live, inv dxn where
    the clamp holds it.  -> E dx [R, C]."""
    x, dxn = E(x), E.of(dxn)
    ss = (x * x).sum(-1, keepdim=True)
    dot = (x * dxn).sum(-1, keepdim=True)
    clamped = ss.v <= eps
    amb = (ss.v - eps).abs() <= GATE_TOL * ss.t
    inv = E(ss.v.clamp_min(eps), torch.where(clamped, torch.zeros_like(ss.t), ss.t)).rsqrt()
    k = (inv * inv * inv * dot)
    full = x * k
    dx = inv * dxn - full.where(~clamped)
    return dx.forgive(amb, full.v)


def vlad_normalize(V, asum, W2, g=None, eps=EPS_L2):
    """V [B, 64, 256], asum [B, 64], W2 [256, 64] -> dict of E: out [B, 16384] in (d, c) order, inv_c [B, 64], inv_t [B];
    with g [B, 16384]: dV, dasum, dW2 too (the projection terms only where the norm is not clamped)."""
    B = V.shape[0]
    W2t = E(W2).transpose(0, 1)                                   # [c, d]
    u = E(V) - E(asum)[:, :, None] * W2t[None]                    # [B, c, d]
    ssc = E((u.v * u.v).sum(-1), (2 * u.v.abs() * u.t).sum(-1))   # [B, c]
    cl_c = ssc.v <= eps
    amb_c = (ssc.v - eps).abs() <= GATE_TOL * ssc.t
    ic = E(ssc.v.clamp_min(eps), torch.where(cl_c, torch.zeros_like(ssc.t), ssc.t)).rsqrt()
    y1 = u * ic[:, :, None]
    tot = (ssc * ic * ic).sum(-1)                                 # [B]
    cl_t = tot.v <= eps
    amb_t = (tot.v - eps).abs() <= GATE_TOL * tot.t
    it = E(tot.v.clamp_min(eps), torch.where(cl_t, torch.zeros_like(tot.t), tot.t)).rsqrt()
    y = y1 * it[:, None, None]
    out = dict(out=y.permute(0, 2, 1).reshape(B, -1), inv_c=ic, inv_t=it, clamped_c=cl_c, clamped_t=cl_t)
    if g is None:
        return out
    gy = E(g).reshape(B, 256, 64).permute(0, 2, 1)                # [B, c, d]
    S = (gy * y).sum((1, 2))
    proj_t = y1 * (it * S)[:, None, None]
    dy1 = (gy - proj_t.where((~cl_t)[:, None, None])) * it[:, None, None]
    dy1 = dy1.forgive(amb_t[:, None, None], proj_t.v * it.v[:, None, None])
    Sc = (dy1 * y1).sum(-1)
    proj_c = y1 * Sc[:, :, None]
    du = (dy1 - proj_c.where((~cl_c)[:, :, None])) * ic[:, :, None]
    du = du.forgive(amb_c[:, :, None], proj_c.v * ic.v[:, :, None])
    out["dV"] = du
    out["dasum"] = -((du * W2t[None]).sum(-1))
    out["dW2"] = -((du * E(asum)[:, :, None]).sum(0).transpose(0, 1))      # [d, c]: summed over the clouds
    return out


# -------------------------------------------------------------------------------------------------- quadruplet loss
def _first_index(d, best):
    """The FIRST index along the last dimension where d == best."""
    n = d.shape[-1]
    ar = torch.arange(n, device=d.device).expand_as(d)
    return torch.where(d == best[..., None], ar, torch.full_like(ar, n)).min(-1).values


def quadruplet_loss(desc, B, P, Ng, m1, m2):
    """desc [B (2 + P + Ng), D] role-ordered (queries | positives | negatives | other negatives) -> E (loss [], grad
    [like desc]): loss = mean_b max_j relu(m1 + best_pos - |neg_j - q|^2) + mean_b max_j relu(m2 + best_pos - |neg_j -
    other|^2), best_pos = min_p |pos_p - q|^2; the gradient goes to the first index on ties and passes at a hinge of
    exactly 0."""
    m1, m2 = f32(m1), f32(m2)
    D = desc.shape[1]
    d = E(desc)
    q = d[:B][:, None]
    pos = d[B:B + B * P].reshape(B, P, D)
    neg = d[B + B * P:B + B * P + B * Ng].reshape(B, Ng, D)
    oth = d[B + B * P + B * Ng:][:, None]

    def sq(a, b):
        e = a - b
        return E((e.v * e.v).sum(-1), (2 * e.v.abs() * e.t).sum(-1)), e

    dpos, epos = sq(pos, q)
    dneg, eneg = sq(neg, q)
    doth, eoth = sq(neg, oth)
    bv = dpos.v.min(-1).values
    ps = _first_index(dpos.v, bv)
    bi = torch.arange(B, device=desc.device)
    best = dpos[bi, ps]
    h1 = (best[:, None] - dneg) + m1
    h2 = (best[:, None] - doth) + m2
    c1, c2 = h1.v.clamp_min(0), h2.v.clamp_min(0)
    j1 = _first_index(c1, c1.max(-1).values)
    j2 = _first_index(c2, c2.max(-1).values)
    w1, w2 = h1[bi, j1], h2[bi, j2]
    a1, a2 = w1.v >= 0, w2.v >= 0
    invB = 1.0 / B
    loss = ((w1.where(a1) + w2.where(a2)) * C(invB)).sum()
    g1 = Z(a1.to(F64) * invB)[:, None]
    g2 = Z(a2.to(F64) * invB)[:, None]
    ep = epos[bi, ps]                    # pos_ps - q
    e1 = eneg[bi, j1]                    # n1 - q
    e2 = eoth[bi, j2]                    # n2 - other
    two = C(2.0)
    gq = two * g1 * e1 - two * (g1 + g2) * ep
    zero = torch.zeros(B, P, D, dtype=F64, device=desc.device)
    gp_v, gp_t = zero.clone(), zero.clone()
    tp = two * (g1 + g2) * ep
    gp_v[bi, ps], gp_t[bi, ps] = tp.v, tp.t
    zero = torch.zeros(B, Ng, D, dtype=F64, device=desc.device)
    gn_v, gn_t = zero.clone(), zero.clone()
    t1, t2 = two * g1 * e1, two * g2 * e2
    gn_v[bi, j1] -= t1.v
    gn_t[bi, j1] += t1.t
    gn_v[bi, j2] -= t2.v
    gn_t[bi, j2] += t2.t
    go = t2
    grad = E(torch.cat([gq.v, gp_v.reshape(-1, D), gn_v.reshape(-1, D), go.v]),
             torch.cat([gq.t, gp_t.reshape(-1, D), gn_t.reshape(-1, D), go.t]))
    return loss, grad


# -------------------------------------------------------------------------------------------------- the composed nodes
def attention_head(X, W, b, gamma, beta, wfc, bfc, eps, momentum, run_mean, run_var, datt, live=None, h32=None,
                   scale32=None, shift32=None):
    """globalatt_block in training mode on rows X [R, Cin]: h = X W + b -> BN(batch statistics, Bessel-corrected moving
    variance) -> ReLU -> . w_fc + b_fc -> sigmoid, and every gradient for the upstream gradient datt.  The gate is taken
    from the f32 tensors (h32, scale32, shift32) when the test holds them (the device's own h and folded statistics),
    else from this function's float64 ones.  -> dict of E."""
    Xe, We = E(X), E(W)
    h = Xe @ We + E(b)
    hs = E(_rows(h.v, live), _rows(h.t, live))
    R = X.shape[0]
    cnt = float(R if live is None else int(live.sum()))
    st = bn_finalize(hs.sum(0), (hs * hs).sum(0), cnt, gamma, beta, eps, momentum, True, run_mean, run_var)
    if h32 is None:
        on = h.v * st["scale"].v + st["shift"].v > 0
    else:
        on = gate(h32, scale32, shift32)
    w = E(wfc.reshape(-1))
    y = (h * st["scale"] + st["shift"]).where(on)
    att = ((y * w).sum(-1) + E(bfc).reshape(())).sigmoid()
    da = E(_rows(datt, live))
    dl = da * att * (1.0 - att)
    if live is not None:
        dl = dl.where(live)
        on = on & live[:, None]
    dz = (dl[:, None] * w[None]).where(on)
    xh = (hs - st["mean"]) * st["rstd"]
    S1, S2 = dz.sum(0), (dz * xh).sum(0)
    dwfc = (dl[:, None] * E(_rows(y.v, live), _rows(y.t, live))).sum(0)
    n = cnt if cnt > 1 else 1.0
    inv = C(1.0 / n)
    k3 = E(gamma) * st["rstd"] * st["rstd"] * (S2 * inv)
    k2 = E(gamma) * st["rstd"] * (S1 * inv) - k3 * st["mean"]
    dh = st["scale"] * dz - k2 - k3 * hs
    if live is not None:
        dh = dh.where(live[:, None])
    out = dict(st)
    out.update(h=h, att=att, dlogit=dl, dgamma=S2, dbeta=S1, dwfc=dwfc, dbfc=dl.sum(), dh=dh,
               dW=Xe.transpose(0, 1) @ dh, dX=dh @ We.transpose(0, 1))
    return out


def l2norm_rows(x, eps=EPS_L2):
    x = E(x)
    ss = (x * x).sum(-1, keepdim=True)
    clamped = ss.v <= eps
    return x * E(ss.v.clamp_min(eps), torch.where(clamped, torch.zeros_like(ss.t), ss.t)).rsqrt()


def netvlad_assign(x, att, Wc, gamma, beta, eps, momentum, run_mean, run_var, dV, dasum, live_clouds=None):
    """NetVLAD's assignment in training mode on x [B, N, D], att [B N]: xn = l2norm(x), s = xn Wc, BN (batch statistics
    over the live clouds, biased moving variance), a = softmax(bn(s)) att, V[b] = a[b]^T xn[b], asum[b] = sum_n a[b];
    and every gradient for (dV, dasum).  -> dict of E."""
    B, N, D = x.shape
    live = None if live_clouds is None else live_clouds.repeat_interleave(N)
    x2 = x.reshape(B * N, D)
    xn = l2norm_rows(x2)
    We = E(Wc)
    s = xn @ We
    ss = E(_rows(s.v, live), _rows(s.t, live))
    cnt = float(B * N if live is None else int(live.sum()))
    st = bn_finalize(ss.sum(0), (ss * ss).sum(0), cnt, gamma, beta, eps, momentum, False, run_mean, run_var)
    p = (s * st["scale"] + st["shift"]).softmax_last()
    a = p * E(att)[:, None]
    a3, xn3 = a.reshape(B, N, 64), xn.reshape(B, N, D)
    V = a3.transpose(1, 2) @ xn3
    asum = a3.sum(1)
    dVe, dase = E(dV), E(dasum)
    da = (xn3 @ dVe.transpose(1, 2) + dase[:, None, :]).reshape(B * N, 64)
    dxn = (a3 @ dVe).reshape(B * N, D)
    datt = (da * p).sum(-1)
    dp = da * E(att)[:, None]
    dz = p * (dp - (dp * p).sum(-1)[:, None])
    dzl = E(_rows(dz.v, live), _rows(dz.t, live))
    xh = (ss - st["mean"]) * st["rstd"]
    S1, S2 = dzl.sum(0), (dzl * xh).sum(0)
    n = cnt if cnt > 1 else 1.0
    inv = C(1.0 / n)
    k3 = E(gamma) * st["rstd"] * st["rstd"] * (S2 * inv)
    k2 = E(gamma) * st["rstd"] * (S1 * inv) - k3 * st["mean"]
    ds = st["scale"] * dzl - k2 - k3 * ss
    if live is not None:
        ds = ds.where(live[:, None])
        datt = datt.where(live)
    dWc = xn.transpose(0, 1) @ ds
    dxn = dxn + ds @ We.transpose(0, 1)
    dx = l2norm_rows_bwd(x2, dxn).reshape(B, N, D)
    out = dict(st)
    out.update(V=V, asum=asum, dx=dx, datt=datt, dWc=dWc, dgamma=S2, dbeta=S1)
    return out
