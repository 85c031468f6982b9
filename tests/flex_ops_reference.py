"""float64 restatements of the drop-in flex operators (dh3d_amd/ops.py flex_convolution, flex_pooling, convolution_pointset
and their gradients), the yardstick of tests/test_flex_ops_paths_gpu.py; tests/test_flex_ops_reference.py pins it.  Written
from the operators' definitions (include/dh3d_hip.h section A; user_ops/kernels/flex_conv_kernel_gpu.cu.cc:46-385,
conv_pointset_kernel.cc:46-120, flex_pool_kernel_gpu.cu.cc as cited in csrc/flex_generic.hip), not from the kernels.  The
tensors are the operators' own channels-first ones: features [B,Din,N], positions [B,Dp,N], neighbourhoods [B,K,N] int32.

Every sum is evaluated twice, as in tests/local_training_reference.py: on the values, and on the absolute values of its
terms (the error scale T, so |fl(sum) - sum| <= n u T for any summation order of n terms).  A coordinate difference
p[nk] - p[c] counts as ONE term of size |p[nk] - p[c]| (a float32 subtraction is within u of its own result): a kernel
that multiplies first and subtracts afterwards is not covered by T, and the offset cloud shows it.

The two centre rules (flex_conv_kernel_gpu.cu.cc:77-79 against :196-202,314): the forward centres on the point itself,
both gradients on the list's rank-0 entry; conv_pointset centres on rank 0 everywhere.  centre_swapped=True evaluates
the OTHER rule and exists only for the power checks of tests/test_flex_ops_reference.py.
"""
import functools

import numpy as np
import torch

from local_training_reference import F64, U, f64, flex_pool_rule, flex_pool_scatter, gather, ulp_ratio  # noqa: F401

U64 = 2.0 ** -53                  # float64 unit roundoff (the _f64 twins are reported in these)


def _pm(x):
    """[B,C,N] -> float64 [B,N,C] on the CPU."""
    return f64(x).transpose(1, 2).contiguous()


def _cf(x):
    return x.transpose(1, 2).contiguous()


# ------------------------------------------------------------------------------------------------------- flex_conv
def _moments(fT, pT, nb, centre):
    """S0[m,i] = sum_k f[nk,i], Sd[m,d,i] = sum_k (p[nk,d] - centre[m,d]) f[nk,i] for the lists nb [B,M,K] (any M), and
    the same sums over |terms|.  Returns (S0, Sd, |S0|, |Sd|, dp [B,M,K,Dp])."""
    g, dp = gather(fT, nb), gather(pT, nb) - centre.unsqueeze(2)
    return (g.sum(2), torch.einsum("bmkd,bmki->bmdi", dp, g), g.abs().sum(2),
            torch.einsum("bmkd,bmki->bmdi", dp.abs(), g.abs()), dp)


def _centre(pT, nb, rank0):
    return gather(pT, nb[:, :, 0:1]).squeeze(2) if rank0 else pT


def _apply(S0, Sd, theta, bias):
    return S0 @ bias + torch.einsum("bmdi,dio->bmo", Sd, theta)


def flex_conv(f, p, nbr, theta, bias, centre_swapped=False):
    """out[b,o,n] = sum_k sum_i (bias[i,o] + sum_d theta[d,i,o] (p[nk,d] - p[n,d])) f[nk,i], nk = nbr[b,k,n]; any Dp.
    Returns (out, T) [B,Dout,N]."""
    fT, pT, nb = _pm(f), _pm(p), _cf(nbr)
    S0, Sd, A0, Ad, _ = _moments(fT, pT, nb, _centre(pT, nb, centre_swapped))
    th, bi = f64(theta), f64(bias)
    return _cf(_apply(S0, Sd, th, bi)), _cf(_apply(A0, Ad, th.abs(), bi.abs()))


def flex_conv_last_term(f, p, nbr, theta, bias, b, n):
    """What the LAST neighbour of point (b, n) adds to out[b, :, n] (a kernel that drops it is off by this)."""
    fT, pT, nb = _pm(f)[b:b + 1], _pm(p)[b:b + 1], _cf(nbr)[b:b + 1, n:n + 1, -1:]
    S0, Sd, _, _, _ = _moments(fT, pT, nb, pT[:, n:n + 1])
    return _apply(S0, Sd, f64(theta), f64(bias))[0, 0]


def flex_conv_grads(f, p, nbr, theta, bias, dout, centre_swapped=False):
    """Gradients of sum(out * dout) with the backward's centre, the list's rank-0 entry:
    dbias[i,o] = sum_{b,n} S0[n,i] dout[n,o], dtheta[d,i,o] = sum_{b,n} Sd[n,d,i] dout[n,o],
    df[nk,i] += sum_o dout[n,o] (bias[i,o] + sum_d (p[nk,d] - p[c(n),d]) theta[d,i,o]).
    Returns ((df, dtheta, dbias), (T_df, T_dtheta, T_dbias))."""
    fT, pT, nb, do = _pm(f), _pm(p), _cf(nbr), _pm(dout)
    th, bi = f64(theta), f64(bias)
    S0, Sd, A0, Ad, dp = _moments(fT, pT, nb, _centre(pT, nb, not centre_swapped))
    B, N, K = nb.shape
    tgt = (torch.arange(B).view(B, 1, 1) * N + nb.long()).reshape(-1)
    res = []
    for s0, sd, d, t, b_, q in ((S0, Sd, do, th, bi, dp), (A0, Ad, do.abs(), th.abs(), bi.abs(), dp.abs())):
        dbias = torch.einsum("bni,bno->io", s0, d)
        dtheta = torch.einsum("bndi,bno->dio", sd, d)
        dS0, dSd = d @ b_.t(), torch.einsum("bno,dio->bndi", d, t)
        per_k = dS0.unsqueeze(2) + torch.einsum("bnkd,bndi->bnki", q, dSd)
        df = torch.zeros(B * N, fT.shape[2], dtype=F64).index_add_(0, tgt, per_k.reshape(B * N * K, -1))
        res.append((_cf(df.view(B, N, -1)), dtheta, dbias))
    return res[0], res[1]


def flex_conv_centre_shift(p, nbr, theta, dout):
    """Per point, what a backward centred on the point itself instead of on rank 0 adds to EACH row its list names:
    delta[b,n,i] = sum_d (p[c(n),d] - p[n,d]) sum_o dout[n,o] theta[d,i,o]   [B,N,Din]."""
    pT, nb = _pm(p), _cf(nbr)
    return torch.einsum("bnd,bno,dio->bni", _centre(pT, nb, True) - pT, _pm(dout), f64(theta))


# --------------------------------------------------------------------------------------------------- conv_pointset
def _pointset_sums(fT, nb, self_centre):
    g = gather(fT, nb)
    d = g - (fT.unsqueeze(2) if self_centre else g[:, :, 0:1])
    return d.sum(2), d.abs().sum(2)


def conv_pointset(f, nbr, theta, bias, centre_swapped=False):
    """out[b,o,n] = bias[o] + sum_k sum_i theta[i,o] (f[nk,i] - f[n0,i]), n0 = nbr[b,0,n].  Returns (out, T)."""
    S, A = _pointset_sums(_pm(f), _cf(nbr), centre_swapped)
    th, bi = f64(theta), f64(bias)
    return _cf(S @ th + bi), _cf(A @ th.abs() + bi.abs())


def conv_pointset_grads(f, nbr, theta, bias, dout, centre_swapped=False):
    """dtheta[i,o] = sum_{b,n} S[n,i] dout[n,o], dbias[o] = sum_{b,n} dout[n,o], and with acc[n,i] = sum_o theta[i,o]
    dout[n,o]: df[nk,i] += acc[n,i] for every k and df[n0,i] -= K acc[n,i].  T_df counts both (the k = 0 pair cancels in
    the value and counts twice in T).  Returns ((df, dtheta, dbias), (T_df, T_dtheta, T_dbias))."""
    fT, nb, do, th = _pm(f), _cf(nbr), _pm(dout), f64(theta)
    S, A = _pointset_sums(fT, nb, centre_swapped)
    B, N, K = nb.shape
    own = torch.arange(N).view(1, N).expand(B, N) if centre_swapped else nb[:, :, 0].long()
    base = torch.arange(B).view(B, 1) * N
    tgt, tgt0 = (base.unsqueeze(2) + nb.long()).reshape(-1), (base + own).reshape(-1)
    res = []
    for s, d, t, sign in ((S, do, th, -1.0), (A, do.abs(), th.abs(), 1.0)):
        acc = (d @ t.t()).reshape(B * N, -1)
        df = torch.zeros_like(acc).index_add_(0, tgt, acc.repeat_interleave(K, 0)).index_add_(0, tgt0, sign * K * acc)
        res.append((_cf(df.view(B, N, -1)), torch.einsum("bni,bno->io", s, d), d.sum((0, 1))))
    return res[0], res[1]


# -------------------------------------------------------------------------------------------------------- flex_pool
def flex_pool(x, nbr):
    """The pool rule on the operator's layouts: x [B,D,N] float32 (or float64), nbr [B,K,N] -> (value [B,D,N], argmax
    [B,D,N] int32).  Exact: best starts at the type's lowest finite value with id 0 and `best < v` takes, so the first k
    of a tie wins and a list of nothing but -inf / NaN gives (lowest, 0)."""
    xn = np.ascontiguousarray(x.detach().cpu().numpy().transpose(0, 2, 1))
    nb = np.ascontiguousarray(nbr.cpu().numpy().transpose(0, 2, 1))
    best, arg = flex_pool_rule(xn, nb)
    if xn.dtype == np.float64:  # the rule's start value is float32's lowest; double's lists of nothing start lower
        none = ~(xn[np.arange(xn.shape[0])[:, None, None], nb] > -np.inf).any(2)
        best = np.where(none, -np.finfo(np.float64).max, best)
    return np.ascontiguousarray(best.transpose(0, 2, 1)), np.ascontiguousarray(arg.transpose(0, 2, 1))


def flex_pool_grad(dout, arg):
    """din[b,d,arg[b,d,n]] += dout[b,d,n].  Returns (din, T, contributions per entry) [B,D,N]."""
    din, mag, cnt = flex_pool_scatter(_pm(dout), torch.from_numpy(np.ascontiguousarray(arg.transpose(0, 2, 1))))
    return _cf(din), _cf(mag), _cf(cnt)


# ----------------------------------------------------------------------------------------------------- case builders
EXTENT = 12.0                     # the extent of the local-training tests' clouds
REMOVED = (7, 8)                  # ids no adversarial list names: their feature gradient is exactly 0


def cloud(B, N, Dp, kind, gen):
    """[B,Dp,N] float32: `rand` in [0, 12)^Dp; `offset` in [1000, 1060)^Dp (32 ulp of a coordinate is 1e-3 of a
    neighbour distance: only a kernel that subtracts coordinates FIRST keeps the result)."""
    r = torch.rand((B, N, Dp), generator=gen, dtype=torch.float32)
    return _cf(r * 60 + 1000 if kind == "offset" else r * EXTENT)


def knn_lists(p, K):
    """Exact kNN within each cloud, self first: p [B,Dp,N] -> [B,N,K] int32."""
    out = []
    for x in p.transpose(1, 2).double():
        out.append(torch.cdist(x, x).topk(K, dim=1, largest=False).indices)
    return torch.stack(out).to(torch.int32)


def adversarial_applies(N, K):
    """The adversarial recipe needs a list shorter than the cloud, a rank besides 0 for the hub, and a hub N-1 that is
    none of the removed ids."""
    return K >= 2 and N > K and N > max(REMOVED) + 1


def lists(kind, p, K, gen):
    """[B,K,N] int32 neighbourhoods of the cloud p [B,Dp,N]:
    knn          exact kNN, self first;
    adversarial  kNN with every 5th list rolled (rank 0 = the farthest neighbour), every (5j+1)-th given a random rank 0,
                 ranks 3..5 of every (5j+2)-th repeating rank 1 (K >= 6), the hub N-1 at rank K-1 of EVERY list, and
                 REMOVED replaced by id 0 everywhere; where the recipe does not apply (K = 1, N = 1, ...) -> random;
    hub0         kNN with point 0 at rank 0 of every list (conv_pointset: K N negative contributions onto one row);
    random       uniformly random ids (all 0 where N = 1)."""
    B, _, N = p.shape
    if kind == "adversarial" and not adversarial_applies(N, K):
        kind = "random"
    if kind == "random":
        return _cf(torch.randint(0, N, (B, N, K), generator=gen, dtype=torch.int32))
    nbr = knn_lists(p, K)
    if kind == "hub0":
        nbr[:, :, 0] = 0
    elif kind == "adversarial":
        nbr[:, ::5] = nbr[:, ::5].roll(1, dims=2)
        nbr[:, 1::5, 0] = torch.randint(0, N, nbr[:, 1::5, 0].shape, generator=gen, dtype=torch.int32)
        if K >= 6:
            nbr[:, 2::5, 3:6] = nbr[:, 2::5, 1:2]
        nbr[:, :, K - 1] = N - 1
        for r in REMOVED:
            nbr[nbr == r] = 0
    else:
        assert kind == "knn", kind
    return _cf(nbr)


def foreign(nbr):
    """[B,N] bool: the list's rank-0 entry is not the point itself."""
    return nbr[:, 0, :] != torch.arange(nbr.shape[2], dtype=nbr.dtype)


def _seed(*dims):
    return functools.reduce(lambda a, b: (a * 131 + int(b)) % (2 ** 31), dims, 7)


def conv_case(B, N, K, Din, Dout, Dp=3, lists_kind="adversarial", cloud_kind="rand", dtype=torch.float32):
    """One flex_convolution case on the CPU: dict(f, p, nbr, theta, bias, dout) in the operator's layouts."""
    gen = torch.Generator().manual_seed(_seed(B, N, K, Din, Dout, Dp, len(lists_kind), len(cloud_kind)))
    p = cloud(B, N, Dp, cloud_kind, gen)
    c = dict(p=p, nbr=lists(lists_kind, p, K, gen),
             f=torch.randn((B, Din, N), generator=gen),
             theta=torch.randn((Dp, Din, Dout), generator=gen) / Din ** 0.5,
             bias=torch.randn((Din, Dout), generator=gen) / (8 * Din) ** 0.5,
             dout=torch.randn((B, Dout, N), generator=gen))
    return {k: (v if v.dtype == torch.int32 else v.to(dtype)) for k, v in c.items()}


def pointset_case(B, N, K, Din, Dout, lists_kind="adversarial", dtype=torch.float32):
    """One convolution_pointset case: dict(f, nbr, theta, bias, dout); the lists are those of a 3-d cloud."""
    gen = torch.Generator().manual_seed(_seed(B, N, K, Din, Dout, len(lists_kind)))
    p = cloud(B, N, 3, "rand", gen)
    c = dict(nbr=lists(lists_kind, p, K, gen), f=torch.randn((B, Din, N), generator=gen),
             theta=torch.randn((Din, Dout), generator=gen) / Din ** 0.5, bias=torch.randn((Dout,), generator=gen),
             dout=torch.randn((B, Dout, N), generator=gen))
    return {k: (v if v.dtype == torch.int32 else v.to(dtype)) for k, v in c.items()}


POOL_GRID = (torch.arange(16, dtype=torch.float32) - 8.0) * 0.25      # the 16 values every finite feature takes
POOL_NEG_INF, POOL_NAN = (3, 4, 5), (6, 9)                            # points whose whole row is -inf / NaN
POOL_EMPTY = {20: POOL_NEG_INF + POOL_NAN, 21: POOL_NEG_INF[:1], 22: POOL_NAN[:1]}   # lists that hold nothing else


def pool_case(B, N, K, D, dtype=torch.float32):
    """One flex_pooling case: dict(f [B,D,N], nbr [B,K,N], dout).  Features on POOL_GRID's lower 15 values (ties
    everywhere); the hub N-1 -- rank K-1 of every adversarial list -- holds the 16th, the strict maximum, on the first
    quarter of the channels, so it is the argmax of ~N D/4 entries; three points are -inf and two NaN in every channel, and
    the lists of points 20, 21, 22 name nothing but those."""
    gen = torch.Generator().manual_seed(_seed(B, N, K, D))
    p = cloud(B, N, 3, "rand", gen)
    nbr = lists("adversarial", p, K, gen)
    f = POOL_GRID[torch.randint(0, 15, (3, B, D, N), generator=gen).amax(0)]    # skewed upwards: the maximum is often shared
    f[:, :(D + 3) // 4, N - 1] = POOL_GRID[15]
    f[:, :, list(POOL_NEG_INF)] = float("-inf")
    f[:, :, list(POOL_NAN)] = float("nan")
    for n, ids in POOL_EMPTY.items():
        nbr[:, :, n] = torch.tensor(ids, dtype=torch.int32).repeat(K)[:K].view(1, K)
    return dict(f=f.to(dtype), nbr=nbr, dout=torch.randn((B, D, N), generator=gen).to(dtype))


# ------------------------------------------------------------------------------------------- the cases and their bounds
# (plan, B, N, K, Din, Dout, Dp, lists, cloud): the smallest shapes at which each forward of csrc/flex_bwd.hip's
# fast_fwd_kind can go wrong; B * N is ragged everywhere.  Every shape runs `adversarial` (`random` where the recipe does
# not apply); the first of each plan also `knn` and `random`; one per plan (two on plan 1: a compile-time and a run-time
# K) also the offset cloud.
def _cases(plan, *shapes):
    out = []
    for s in shapes:
        extra, s = [x for x in s if isinstance(x, str)], tuple(x for x in s if not isinstance(x, str))
        s = s if len(s) == 6 else s + (3,)
        out.append((plan,) + s + ("adversarial", "rand"))
        out += [(plan,) + s + (("adversarial", "offset") if x == "offset" else (x, "rand")) for x in extra]
    return out


CONV_CASES = (
    # plan 3, the persistent bf16x6 kernel; 3 x 6001 = 18003 rows: more 64-point tiles than CUs, several per workgroup
    _cases(3, (1, 40, 8, 64, 64, "knn", "random"), (3, 999, 8, 32, 64, "offset"), (3, 6001, 8, 64, 64))
    # plan 1, compile-time K = 8: 64-point tiles; 32-point tiles (Din 64, Dout >= 128, <= 16384 rows); 64-point tiles
    # beyond (16500 rows); Din = 128 (32-point tiles); then compile-time K = 12; then the run-time-K loop
    + _cases(1, (2, 333, 8, 32, 128, "knn", "random", "offset"), (3, 45, 8, 64, 128), (3, 5500, 8, 64, 256),
             (1, 17, 8, 128, 128), (2, 300, 8, 128, 256),
             (2, 257, 12, 128, 128),
             (2, 300, 5, 64, 64, "offset"), (1, 129, 1, 128, 128), (2, 100, 16, 32, 64), (1, 333, 9, 64, 128))
    # plan 2, flex_S + GEMM; 36 -> 100: partial 32-wide transpose tiles on both channel counts
    + _cases(2, (1, 33, 3, 4, 4, "knn", "random"), (2, 100, 5, 16, 24), (1, 700, 12, 36, 100), (2, 257, 8, 48, 96, "offset"))
    # plan 0: channel counts off the %4 grid, Dp = 2 on x6's channels (not its position dimension), N = 1
    + _cases(0, (2, 100, 4, 3, 7, "knn", "random"), (1, 257, 8, 33, 64, "offset"), (2, 300, 8, 32, 64, 2), (4, 1, 1, 32, 64))
)
F64_CONV_CASES = [(0, 2, 100, 5, 16, 24, 3, "adversarial", "rand"), (0, 1, 257, 8, 33, 64, 3, "adversarial", "rand")]

POOL_CASES = [(2, 257, 8, 40), (3, 999, 8, 64), (2, 257, 8, 5), (1, 100, 12, 33)]          # D % 4 == 0: the pm kernel
F64_POOL_CASE = (2, 257, 8, 40)
POINTSET_CASES = [(B, N, K, Din, Dout, kind) for (B, N, K, Din, Dout) in ((2, 300, 8, 3, 32), (1, 257, 5, 32, 40),
                                                                          (2, 100, 12, 7, 9))
                  for kind in ("adversarial", "hub0")]
F64_POINTSET_CASE = (1, 257, 5, 32, 40, "adversarial")

# Bounds in u of the sum's own size T, one per group: 3 x the worst ratio of the group measured on the MI355X (the feature
# gradients' atomics change order from run to run), never below 1 (a result rounded once), the measured worst in the
# comment.  A float32 case counts under its own plan with ops.FAST_PATH on and under plan 0 with it off, whatever plan
# the shape is filed under; the backward of plans 1 - 3 is the factorised one (flex_S + two GEMMs + the atomics scatter),
# of plan 0 the reference formulation -- except N = 1 (4 x 1, K = 1), whose backward is factorised under plan 0.
# Plan 3's products are bf16x6 ones (each within dense_reference.SINGLE_PRODUCT_BOUND = 2^-20 = 16 u of the float64
# product, against 1 u for an f32 multiply): measured, they do not show -- its forward is the closest of the four.
BOUNDS = {
    # forward worst 2.22 (3 x 6001, 64 -> 64), df 2.15 (3 x 999, offset), dtheta 3.01 (1 x 40), dbias 1.35 (1 x 40, random)
    3: dict(out=6.7, df=6.5, dtheta=9.1, dbias=4.1),
    # forward 5.79 (3 x 5500, 64 -> 256), df 3.33 (1 x 129, K = 1), dtheta 2.06 (1 x 17, 128 -> 128), dbias 1.87 (1 x 129)
    1: dict(out=17.4, df=10.0, dtheta=6.2, dbias=5.6),
    # forward 3.00 (2 x 257, 48 -> 96), df 1.96 (1 x 33, random), dtheta 1.19 and dbias 0.86 (1 x 33, knn)
    2: dict(out=9.0, df=5.9, dtheta=3.6, dbias=2.6),
    # forward 7.04 (3 x 5500, 64 -> 256: 512 terms added one after the other), df 3.33 (1 x 129, K = 1), dtheta 1.87
    # (1 x 40), dbias 1.99 (4 x 1)
    0: dict(out=21.1, df=10.0, dtheta=5.6, dbias=6.0),
    # the _f64 twins, in float64 roundoffs U64 (the float64 reference's own rounding is in the measurement): forward 4.07,
    # df 1.91, dtheta 2.09, dbias 1.13
    "f64": dict(out=12.3, df=5.8, dtheta=6.3, dbias=3.4),
    # convolution_pointset: forward 4.86 (2 x 100, K = 12, hub0), df 4.38 (1 x 257, hub0: K N negative terms on one row),
    # dtheta 0.47, dbias 0.33
    "pointset": dict(out=14.6, df=13.2, dtheta=1.5, dbias=1.0),
    # its _f64 twin, in U64: forward 4.39, df 1.45, dtheta 2.19, dbias 0.00
    "pointset_f64": dict(out=13.2, df=4.4, dtheta=6.6, dbias=1.0),
    # flex_pooling's gradient: 2.38 (3 x 999, D = 64: 996 atomics onto one entry; 1.98 in another run); the _f64 twin 0.00
    "pool": dict(df=7.2),
}
