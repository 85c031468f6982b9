"""float64 restatements of the local training step's autograd nodes (dh3d_amd/train_ops.py, the flex_conv / group_point /
three_interpolate nodes the step calls), the yardstick of tests/test_local_training_nodes_gpu.py.  Written from the
operators' definitions (core/backbones.py, include/dh3d_hip.h) and the oracle's flex_pool rule, not from the kernels.

Every linear restatement is evaluated twice: on the values, and on their absolute values (the error scale T: the same
sums taken over |terms|, so |fl(sum) - sum| <= n u T for any summation order of n terms).  The tests report
max |got - ref| / (u T) -- the error in float32 unit roundoffs of the sum's own size -- and bound it.
"""
import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24                    # float32 unit roundoff
FLT_MIN = float(np.finfo(np.float32).tiny)


def f64(x):
    return x.detach().to(F64).cpu()


def gather(x, nbr):
    """x [B,N,C], nbr [B,M,K] (ids within the cloud) -> [B,M,K,C]."""
    B, M, K = nbr.shape
    return torch.gather(x.unsqueeze(1).expand(B, M, x.shape[1], x.shape[2]), 2,
                        nbr.long().unsqueeze(-1).expand(B, M, K, x.shape[2]))


def linear_grads(fn, inputs, dout):
    """fn multilinear in `inputs` (float64 CPU tensors): (out, grads, out_scale, grad_scales) -- the values and the same
    expression on |inputs|, |dout| (the error scale T of every output and gradient)."""
    res = []
    for absval in (False, True):
        xs = [(x.abs() if absval else x).clone().requires_grad_(True) for x in inputs]
        out = fn(*xs)
        gs = torch.autograd.grad(out, xs, dout.abs() if absval else dout, allow_unused=True)
        res.append((out.detach(), [None if g is None else g.detach() for g in gs]))
    return res[0][0], res[0][1], res[1][0], res[1][1]


def ulp_ratio(got, ref, scale):
    """max |got - ref| / (u * scale); an entry whose scale is 0 must be exactly 0."""
    err = (f64(got) - ref).abs()
    return float((err / (U * scale + 1e-300)).max())


def pointset_sums(xyz, nbr):
    """conv_pointset on coordinates (conv_pointset_kernel.cc:46-64, Din = 3): S[n] = sum_k (p[nbr[n,k]] - p[nbr[n,0]]),
    the centre the list's RANK-0 entry.  Returns (S, T(S)) [B,N,3]."""
    g = gather(xyz, nbr)
    dp = g - g[:, :, 0:1]
    return dp.sum(2), dp.abs().sum(2)


def flex_pool_rule(x, nbr):
    """FlexPool (oracle/dh3d_oracle.c dh3d_oracle_flex_pool_fwd): best = -FLT_MAX, index 0, `best < v` -- the FIRST k of
    a tie wins.  x [B,N,C] float32 numpy, nbr [B,N,K] -> (value [B,N,C] float32, argmax [B,N,C] int32 id in the cloud)."""
    B, N, C = x.shape
    K = nbr.shape[2]
    best = np.full((B, N, C), -np.finfo(np.float32).max, np.float32)
    arg = np.zeros((B, N, C), np.int32)
    bi = np.arange(B)[:, None]
    for k in range(K):
        ids = nbr[:, :, k]
        v = x[bi, ids]                                   # [B,N,C]
        take = best < v
        best = np.where(take, v, best)
        arg = np.where(take, ids[:, :, None], arg)
    return best, arg


def flex_pool_scatter(dout, arg):
    """FlexPoolGrad: din[b, arg[b,n,c], c] += dout[b,n,c] in float64.  Returns (din, T(din), contributions per entry)."""
    B, N, C = dout.shape
    d = dout.reshape(-1)
    tgt = ((torch.arange(B).view(B, 1, 1) * N + arg.long()) * C + torch.arange(C).view(1, 1, C)).reshape(-1)
    din = torch.zeros(B * N * C, dtype=F64).index_add_(0, tgt, d)
    mag = torch.zeros(B * N * C, dtype=F64).index_add_(0, tgt, d.abs())
    cnt = torch.zeros(B * N * C, dtype=F64).index_add_(0, tgt, torch.ones_like(d))
    return din.view(B, N, C), mag.view(B, N, C), cnt.view(B, N, C)


def se_gate(x, z, dy):
    """relu(x + x sigmoid(z)) (core/backbones.py:52-55) and its gradients, float64."""
    g = torch.sigmoid(z)
    pre = x + x * g
    on = (pre > 0).to(F64)
    return torch.relu(pre), on * dy * (1.0 + g), on * dy * x * g * (1.0 - g), g


def l2_normalize_rows(x, dy, eps):
    """tf.nn.l2_normalize: y = x / sqrt(max(|x|^2, eps)); dx = inv dy - x inv^3 (x . dy) where |x|^2 > eps, inv dy where the
    clamp holds (max() passes no gradient to |x|^2 there).  Returns (y, dx, T(y), T(dx))."""
    ss = (x * x).sum(1, keepdim=True)
    inv = 1.0 / torch.sqrt(torch.clamp(ss, min=eps))
    live = (ss > eps).to(F64)
    y = x * inv
    dx = inv * dy - live * x * inv ** 3 * (x * dy).sum(1, keepdim=True)
    tdx = inv * dy.abs() + live * x.abs() * inv ** 3 * (x.abs() * dy.abs()).sum(1, keepdim=True)
    return y, dx, x.abs() * inv, tdx


def flex_conv(feat, dp, theta, bias):
    """flex_conv (core/layers.py FlexConv; the factorised form of training.flex_conv_factorised):
    out[n] = sum_k (f[n_k] bias + sum_d dp_d(n,k) f[n_k] theta_d), dp = p[n_k] - p[n] (centre: the point itself).
    feat gathered [B,M,K,Din], dp [B,M,K,3]."""
    out = feat.sum(2) @ bias
    for d in range(3):
        out = out + (dp[..., d:d + 1] * feat).sum(2) @ theta[d]
    return out


def bn_train(x, gamma, beta, eps):
    """Training-mode BatchNorm over all rows (biased batch variance)."""
    mu = x.mean(0, keepdim=True)
    var = ((x - mu) ** 2).mean(0, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma + beta


def detection_block(feat, layers, wfc, bfc, masks):
    """detection_block (core/backbones.py:132-151) in training mode on rows feat [R, C]: Conv2D 1x1 + BNReLU per entry
    of `layers` (W [Cin,Cout], b, gamma, beta, eps), then the 1-channel logit and sigmoid.  `masks(i, pre)` gives the
    float64 0/1 ReLU pattern of layer i (from ActivationPatterns.take).  Returns att [R, 1]."""
    x = feat
    for i, (W, b, gamma, beta, eps) in enumerate(layers):
        pre = bn_train(x @ W + b, gamma, beta, eps)
        x = pre * masks(i, pre)
    return torch.sigmoid(x @ wfc + bfc)


# Entries where float64 and the float32 kernel take different sides of a kink must lie this close to it, relative to
# the largest |entry| of the tensor (the forward of the whole step agrees with float64 to ~1e-5 of that scale).
NEAR_KINK = 1e-3


class ActivationPatterns(object):
    """Which side of each kink the HIP forward took: every ReLU after a training BatchNorm (keyed by its module), the
    argmax of each flex_pool, the SE squeeze ReLU, the SE gate and the attention head's hidden ReLU (in call order).

    A float64 restatement that decides these itself differs from the kernels wherever a float32 pre-activation lies
    within rounding of 0 (or two pooled values within rounding of each other): there the gradients disagree by a whole
    dy, whichever side is right.  The restatement takes the kernels' patterns instead, and `take` checks that each
    entry where they differ from float64's own decision lies within NEAR_KINK of the kink -- a wrong pattern fails."""

    def __init__(self, monkeypatch):
        from dh3d_amd import pm
        from dh3d_amd import train_ops as T
        self.bn, self.pool, self.relu, self.gate, self.att = {}, [], [], [], []
        self.flips = 0
        bn0, relu0, gate0, att0 = T.batch_norm_train, T.relu, T.se_gate, T.attention_head

        def bn(x, bnmod, relu, *a, **k):
            y = bn0(x, bnmod, relu, *a, **k)
            if relu:
                self.bn[id(bnmod)] = y > 0
            return y

        def pool(x, nbr):
            self.pool.append(pm.flex_pool(x.detach().contiguous(), nbr, want_argmax=True)[1])
            return pool0(x, nbr)

        def relu(x):
            y = relu0(x)
            self.relu.append(y > 0)
            return y

        def gate(x, z):
            y = gate0(x, z)
            self.gate.append(y > 0)
            return y

        def att(X, conv, wfc, bfc, *a, **k):
            y = att0(X, conv, wfc, bfc, *a, **k)
            h = y.grad_fn.saved_tensors[2]          # the pre-activation [R, H] (overwritten by its backward)
            st = y.grad_fn.cfg[3]                   # its BatchNorm: relu(fmaf(h, scale, shift))
            pre = h.double() * st.stats[2].double() + st.stats[3].double()   # exact product: the sign of the fmaf
            self.att.append(pre > 0)
            return y

        pool0 = T.flex_pool
        for name, fn in (("batch_norm_train", bn), ("flex_pool", pool), ("relu", relu), ("se_gate", gate),
                         ("attention_head", att)):
            monkeypatch.setattr(T, name, fn)

    def take(self, pre, kmask):
        """pre (float64, any shape) and the kernel's boolean pattern of the same entries -> the mask as float64."""
        kmask = kmask.to(pre.device).reshape(pre.shape)
        flip = (pre.detach() > 0) != kmask
        if flip.any():
            near = float(pre.detach()[flip].abs().max()) / float(pre.detach().abs().max())
            assert near <= NEAR_KINK, ("an activation pattern differs from float64 away from the kink", near)
            self.flips += int(flip.sum())
        return kmask.to(F64)

    def bn_relu(self, pre, bnmod):
        return pre * self.take(pre, self.bn[id(bnmod)])

    def squeeze_relu(self, pre, i):
        return pre * self.take(pre, self.relu[i])

    def se_gate(self, pre, i):
        return pre * self.take(pre, self.gate[i])

    def head_relu(self, pre, i=0):
        return pre * self.take(pre, self.att[i])

    def flex_pool(self, x, nbr, i):
        """max over the neighbourhood at the kernel's argmax [B,N,C] (ids in the cloud); where it is not float64's
        first maximum, the two values must be within NEAR_KINK of each other."""
        arg = self.pool[i].to(x.device).long()
        got = torch.gather(x, 1, arg)
        best = gather(x.detach(), nbr.to(x.device)).max(2).values
        gap = float((best - got.detach()).max()) / float(x.detach().abs().max())
        assert gap <= NEAR_KINK, ("flex_pool's argmax is not a maximum", gap)
        self.flips += int((best > got.detach()).sum())
        return got
