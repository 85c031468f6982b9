"""Drop-in operator API: the reference's op names, argument orders and tensor layouts.

Mirrors user_ops/__init__.py (knn_bruteforce :50, flex_convolution :63-89, flex_convolution_transpose,
flex_pooling :115-135, convolution_pointset :205-225) and tf_ops/{sampling,grouping,interpolation}/tf_*.py
(prob_sample tf_sampling.py:15-26, farthest_point_sample tf_sampling.py:63-71, gather_point tf_sampling.py:38-61, query_ball_point / query_ball_point2
tf_grouping.py:9-36, select_top_k / knn_point tf_grouping.py:37-47,63-88, group_point tf_grouping.py:48-56,
three_nn / three_interpolate
tf_interpolate.py:8-34), with torch.autograd.Function standing in for the RegisterGradient hooks
(user_ops/__init__.py:95-111,141-151,231-246; tf_grouping.py:57-61; tf_interpolate.py:29-34).
Where TF raised InvalidArgument these raise ValueError.  Every op runs on the HIP library; there is no
CPU path.
"""
import torch

from . import _lib as L

__all__ = [
    "knn_bruteforce", "flex_convolution", "flex_convolution_transpose", "flex_pooling", "convolution_pointset",
    "farthest_point_sample", "group_point", "three_nn", "three_interpolate", "query_ball_point", "query_ball_point2",
    "knn_point", "select_top_k", "gather_point", "prob_sample",
]


# The reference-layout operators run on the fused MFMA kernels whenever the shape is one they serve (every DH3D
# layer); False forces the reference formulation (csrc/flex_generic.hip) -- the tests compare the two.
FAST_PATH = True


def _same(a, b, what):
    if a != b:
        raise ValueError("%s mismatch: %s vs %s" % (what, a, b))


# --------------------------------------------------------------------------- knn
def knn_bruteforce(positions, k, name=None):
    """positions [B, Dp, N] -> (neighborhood [B, N, K] int32, distances [B, N, K]).

    user_ops/ops/knn_bruteforce.cc:11-35; not differentiable."""
    p = L.require_cuda_f32(positions, "positions", 3)
    if int(k) <= 0:
        raise ValueError("k must be positive")
    B, Dp, N = p.shape
    nn = torch.empty((B, N, int(k)), dtype=torch.int32, device=p.device)
    dist = torch.empty((B, N, int(k)), dtype=torch.float32, device=p.device)
    with torch.cuda.device(p.device):
        L.check(L.lib().dh3d_knn_bruteforce(L.ptr(p), B, Dp, N, int(k), L.ptr(nn), L.ptr(dist),
                                            L.stream_ptr()), "knn_bruteforce")
    return nn, dist


# --------------------------------------------------------------------------- reference-layout dispatch
def _run(stem, like, args, what, ws_shape=None):
    """Enqueue dh3d_<stem>[_f64|_ws](*args, ...) on the device of `like` and the current stream:
      float64                                 -> dh3d_<stem>_f64 (flex_conv_op.cc:97-106 registers double too);
      float32, FAST_PATH, workspace_bytes > 0 -> dh3d_<stem>_ws, given a uint8 workspace of dh3d_<stem>_workspace_bytes(
                                                 *ws_shape) bytes (section A': csrc/flex_bwd.hip, csrc/flex_deconv.hip);
      otherwise                               -> dh3d_<stem> (section A, the reference formulation).
    ws_shape None: the operator has no section A' entry point."""
    lib, f64 = L.lib(), like.dtype == torch.float64
    fast = FAST_PATH and ws_shape is not None and not f64
    with torch.cuda.device(like.device):
        ws_bytes = getattr(lib, "dh3d_%s_workspace_bytes" % stem)(*ws_shape) if fast else 0
        if ws_bytes:
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=like.device)
            L.check(getattr(lib, "dh3d_%s_ws" % stem)(*args, L.ptr(ws), ws_bytes, L.stream_ptr()), what)
        else:
            L.check(getattr(lib, "dh3d_" + stem + ("_f64" if f64 else ""))(*args, L.stream_ptr()), what)


# --------------------------------------------------------------------------- flex_conv and its transpose
def _flex_conv_shapes(f, t, bi, nb, p):
    (B, Din, N), (Dp, Din_t, Dout) = f.shape, t.shape
    # shape function of user_ops/ops/flex_conv.cc:41-82
    _same(Din_t, Din, "Din(theta/features)")
    _same(tuple(bi.shape), (Din, Dout), "bias shape")
    _same((nb.shape[0], nb.shape[2]), (B, N), "neighborhood [B,_,N]")
    _same(tuple(p.shape), (B, Dp, N), "position shape")


def _flex_deconv_shapes(f, t, bi, nb, p):
    (B, Din, N), (Dp, Din_t, Dout) = f.shape, t.shape
    # shape function of user_ops/ops/flex_deconv.cc (FlexDeconv)
    _same((nb.shape[0], p.shape[0]), (B, B), "batch(features/neighborhood/position)")
    _same((nb.shape[2], p.shape[2]), (N, N), "N(features/neighborhood/position)")
    _same(p.shape[1], Dp, "Dp(theta/position)")
    _same(bi.shape[1], Dout, "Dout(theta/bias)")
    _same((Din_t, bi.shape[0]), (Din, Din), "Din(features/theta/bias)")


def _flex_function(name, stem, what, check_shapes):
    """The autograd.Function of flex_convolution (stem "flex_conv") or flex_convolution_transpose ("flex_deconv"): the
    same arguments, layouts and entry-point signatures; check_shapes(f, t, bi, nb, p) is the operator's own."""

    def forward(ctx, features, theta, bias, neighborhood, position):
        f = L.require_cuda_float(features, "features", 3)
        t = L.require_cuda_float(theta, "theta", 3, like=f)
        bi = L.require_cuda_float(bias, "bias", 2, like=f)
        nb = L.require_cuda_i32(neighborhood, "neighborhood", 3)
        p = L.require_cuda_float(position, "position", 3, like=f)
        check_shapes(f, t, bi, nb, p)
        (B, Din, N), (Dp, _, Dout) = f.shape, t.shape
        ctx.dims = d = (B, N, nb.shape[1], Dp, Din, Dout)  # the sizes every entry point and workspace query takes
        out = torch.empty((B, Dout, N), dtype=f.dtype, device=f.device)
        _run(stem + "_fwd", f, (L.ptr(f), L.ptr(t), L.ptr(bi), L.ptr(nb), L.ptr(p)) + d + (L.ptr(out),), what, d)
        ctx.save_for_backward(f, t, bi, nb, p)
        return out

    def backward(ctx, topdiff):
        f, t, bi, nb, p = ctx.saved_tensors
        td = topdiff.contiguous()
        gf, gt, gb = torch.empty_like(f), torch.empty_like(t), torch.empty_like(bi)
        _run(stem + "_bwd", f, (L.ptr(f), L.ptr(t), L.ptr(bi), L.ptr(nb), L.ptr(p), L.ptr(td)) + ctx.dims
             + (L.ptr(gf), L.ptr(gt), L.ptr(gb)), what + "_grad", ctx.dims)
        return gf, gt, gb, None, None

    # (a named class: autograd shows its nodes as _FlexConvBackward / _FlexDeconvBackward)
    return type(name, (torch.autograd.Function,), dict(forward=staticmethod(forward), backward=staticmethod(backward)))


_FlexConv = _flex_function("_FlexConv", "flex_conv", "flex_convolution", _flex_conv_shapes)
_FlexDeconv = _flex_function("_FlexDeconv", "flex_deconv", "flex_convolution_transpose", _flex_deconv_shapes)


def flex_convolution(features, position, neighborhood, theta, bias, name=None):
    """features [B,Din,N], position [B,Dp,N], neighborhood [B,K,N] int32, theta [Dp,Din,Dout],
    bias [Din,Dout] -> [B,Dout,N]   (user_ops/__init__.py:63-89; note its argument re-order)."""
    return _FlexConv.apply(features, theta, bias, neighborhood, position)


def flex_convolution_transpose(features, position, neighborhood, theta, bias, name=None):
    """features [B,Din,N], position [B,Dp,N], neighborhood [B,K,N] int32, theta [Dp,Din,Dout], bias [Din,Dout]
    -> [B,Dout,N]: every point spreads the features of its rank-0 neighbour to its whole list (FlexDeconv,
    user_ops.flex_convolution_transpose; the argument re-order of flex_convolution)."""
    return _FlexDeconv.apply(features, theta, bias, neighborhood, position)


# --------------------------------------------------------------------------- flex_pool
class _FlexPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, neighborhood):
        f = L.require_cuda_float(features, "features", 3)
        nb = L.require_cuda_i32(neighborhood, "neighborhood", 3)
        B, D, N = f.shape
        K = nb.shape[1]
        _same((nb.shape[0], nb.shape[2]), (B, N), "neighborhood [B,_,N]")  # ops/flex_pool.cc:35-56
        out = torch.empty_like(f)
        argmax = torch.empty((B, D, N), dtype=torch.int32, device=f.device)
        _run("flex_pool_fwd", f, (L.ptr(f), L.ptr(nb), B, N, K, D, L.ptr(out), L.ptr(argmax)), "flex_pooling",
             (B, N, K, D))
        ctx.save_for_backward(argmax)
        ctx.mark_non_differentiable(argmax)
        return out, argmax

    @staticmethod
    def backward(ctx, topdiff, _unused):
        (argmax,) = ctx.saved_tensors
        td = topdiff.contiguous()
        B, D, N = td.shape
        gf = torch.empty_like(td)
        _run("flex_pool_bwd", td, (L.ptr(td), L.ptr(argmax), B, N, D, L.ptr(gf)), "flex_pooling_grad")
        return gf, None


def flex_pooling(features, neighborhood, name=None):
    """features [B,D,N], neighborhood [B,K,N] -> (max values [B,D,N], argmax point ids [B,D,N] int32)
    (user_ops/__init__.py:115-135)."""
    return _FlexPool.apply(features, neighborhood)


# --------------------------------------------------------------------------- conv_pointset
class _ConvPointset(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, theta, bias, neighborhood):
        f = L.require_cuda_float(features, "features", 3)
        t = L.require_cuda_float(theta, "theta", 2, like=f)
        bi = L.require_cuda_float(bias, "bias", 1, like=f)
        nb = L.require_cuda_i32(neighborhood, "neighborhood", 3)
        (B, Din, N), (Din_t, Dout) = f.shape, t.shape
        _same(Din_t, Din, "Din(theta/features)")  # ops/conv_pointset.cc:38-73
        _same(bi.shape[0], Dout, "bias length")
        _same((nb.shape[0], nb.shape[2]), (B, N), "neighborhood [B,_,N]")
        ctx.dims = d = (B, N, nb.shape[1], Din, Dout)
        out = torch.empty((B, Dout, N), dtype=f.dtype, device=f.device)
        _run("conv_pointset_fwd", f, (L.ptr(f), L.ptr(t), L.ptr(bi), L.ptr(nb)) + d + (L.ptr(out),),
             "convolution_pointset")
        ctx.save_for_backward(f, t, nb)
        return out

    @staticmethod
    def backward(ctx, topdiff):
        f, t, nb = ctx.saved_tensors
        td = topdiff.contiguous()
        gf, gt = torch.empty_like(f), torch.empty_like(t)
        gb = torch.empty((t.shape[1],), dtype=f.dtype, device=f.device)
        _run("conv_pointset_bwd", f, (L.ptr(f), L.ptr(t), L.ptr(nb), L.ptr(td)) + ctx.dims
             + (L.ptr(gf), L.ptr(gt), L.ptr(gb)), "convolution_pointset_grad")
        return gf, gt, gb, None


def convolution_pointset(features, neighborhood, theta, bias, name=None):
    """features [B,Din,N], neighborhood [B,K,N], theta [Din,Dout], bias [Dout] -> [B,Dout,N]
    (user_ops/__init__.py:205-225)."""
    return _ConvPointset.apply(features, theta, bias, neighborhood)


# --------------------------------------------------------------------------- PointNet++ ops
def farthest_point_sample(npoint, inp, contract=None):
    """inp [B,N,3] -> idx [B,npoint] int32 (tf_sampling.py:63-71); not differentiable.

    contract (extension): None = the default kernels (distance rounded as fma(dz,dz,fma(dx,dx,dy*dy)), the LLVM/NVVM
    contraction of tf_sampling_g.cu:141); 1 / 0 = the any-N kernel with that contraction / the uncontracted
    (dx*dx+dy*dy)+dz*dz of an -fmad=false build (dh3d_farthest_point_sample_mode)."""
    x = L.require_cuda_f32(inp, "inp", 3)
    if x.shape[2] != 3:
        raise ValueError("FarthestPointSample expects (batch_size,num_points,3) inp shape")  # tf_sampling.cpp:105
    if int(npoint) <= 0:
        raise ValueError("FarthestPointSample expects positive npoint")  # tf_sampling.cpp:100
    B, N, _ = x.shape
    out = torch.empty((B, int(npoint)), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        if contract is None and N <= 16384:
            L.check(L.lib().dh3d_farthest_point_sample(B, N, int(npoint), L.ptr(x), None, L.ptr(out),
                                                       L.stream_ptr()), "farthest_point_sample")
        else:  # running min-distances in scratch, as the reference's allocate_temp (tf_sampling.cpp:115)
            temp = torch.empty((B, N), dtype=torch.float32, device=x.device)
            L.check(L.lib().dh3d_farthest_point_sample_mode(B, N, int(npoint), L.ptr(x), L.ptr(temp), L.ptr(out),
                                                            1 if contract is None else int(bool(contract)),
                                                            L.stream_ptr()), "farthest_point_sample")
    return out


def _query_ball(radius, nsample, xyz1, xyz2):
    from . import pm
    with torch.no_grad():  # ops.NoGradient('QueryBallPoint') (tf_grouping.py:22)
        n, m = (xyz1.shape[1], xyz2.shape[1]) if isinstance(xyz1, torch.Tensor) and xyz1.dim() == 3 and \
            isinstance(xyz2, torch.Tensor) and xyz2.dim() == 3 else (0, 0)
        # one rule on (n, m, nsample) alone -- never the batch or the data: a cloud gives the same rows in any batch
        if pm.ball_query_plan(n, m, int(nsample)) == 1:
            return pm.ball_query_grid(radius, nsample, xyz1, xyz2)
        return pm.ball_query_scan(radius, nsample, xyz1, xyz2)


def query_ball_point(radius, nsample, xyz1, xyz2):
    """radius float, nsample int, xyz1 [b,n,3] dataset, xyz2 [b,m,3] queries -> (idx [b,m,nsample] int32, pts_cnt [b,m]
    int32) (tf_grouping.py:9-22): per query the nsample lowest indices with d < radius in ascending order, then the first
    repeated; an empty ball's row is its nearest point, pts_cnt 0.  Not differentiable."""
    if isinstance(radius, torch.Tensor) or not float(radius) > 0.0:
        raise ValueError("QueryBallPoint expects positive radius")  # tf_grouping.cpp:90
    return _query_ball(float(radius), nsample, xyz1, xyz2)


def query_ball_point2(radii, nsample, xyz1, xyz2):
    """radii [b,m] float32, one per query (a radius <= 0 or NaN has no hits); otherwise query_ball_point
    (tf_grouping.py:23-36).  Not differentiable."""
    if not isinstance(radii, torch.Tensor):
        raise ValueError("QueryBallPoint2 expects radii as a (batch_size,npoint) tensor")
    return _query_ball(radii, nsample, xyz1, xyz2)


class _GroupPoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, idx):
        p = L.require_cuda_f32(points, "points", 3)
        ix = L.require_cuda_i32(idx, "idx", 3)
        b, n, c = p.shape
        _same(ix.shape[0], b, "batch(points/idx)")  # tf_grouping.cpp OP_REQUIRES
        m, ns = ix.shape[1], ix.shape[2]
        out = torch.empty((b, m, ns, c), dtype=torch.float32, device=p.device)
        with torch.cuda.device(p.device):
            L.check(L.lib().dh3d_group_point_fwd(b, n, c, m, ns, L.ptr(p), L.ptr(ix), L.ptr(out), L.stream_ptr()),
                    "group_point")
        ctx.save_for_backward(ix)
        ctx.pshape = (b, n, c)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (ix,) = ctx.saved_tensors
        b, n, c = ctx.pshape
        m, ns = ix.shape[1], ix.shape[2]
        go = grad_out.contiguous()
        gp = torch.empty((b, n, c), dtype=torch.float32, device=go.device)
        with torch.cuda.device(go.device):
            L.check(L.lib().dh3d_group_point_bwd(b, n, c, m, ns, L.ptr(go), L.ptr(ix), L.ptr(gp), L.stream_ptr()),
                    "group_point_grad")
        return gp, None


def group_point(points, idx):
    """points [b,n,c], idx [b,m,nsample] int32 -> [b,m,nsample,c] (tf_grouping.py:48-61)."""
    return _GroupPoint.apply(points, idx)


def select_top_k(k, dist):
    """k int, dist [b,m,n] float32 -> (idx [b,m,n] int32, dist_out [b,m,n]) (tf_grouping.py:37-47, the SelectionSort op):
    every row the partial selection sort of its first k entries -- strict <, first minimum, swap -- and the WHOLE row is
    returned; ties come out in the swap walk's order, not lowest id first.  1 <= k <= n.  Not differentiable."""
    from . import pm
    with torch.no_grad():  # ops.NoGradient('SelectionSort') (tf_grouping.py:47)
        return pm.select_top_k(k, dist)


def knn_point(k, xyz1, xyz2):
    """k int, xyz1 [b,n,c] dataset, xyz2 [b,m,c] queries -> (val [b,m,k] SQUARED distances, idx [b,m,k] int32)
    (tf_grouping.py:63-88): the first k columns of select_top_k on the matrix of squared distances, which the fused kernel
    never forms.  Not differentiable."""
    from . import pm
    with torch.no_grad():
        return pm.knn_point(k, xyz1, xyz2)


def gather_point(inp, idx):
    """inp [b,n,3], idx [b,m] int32 -> [b,m,3] (tf_sampling.py:38-61); the gradient is GatherPointGrad's scatter-add.
    group_point with nsample = 1 on the same entry points."""
    if isinstance(inp, torch.Tensor) and (inp.dim() != 3 or inp.shape[2] != 3):
        raise ValueError("GatherPoint expects (batch_size,num_points,3) inp shape")  # tf_sampling.cpp:131
    if isinstance(inp, torch.Tensor) and isinstance(idx, torch.Tensor) and (idx.dim() != 2 or idx.shape[0] != inp.shape[0]):
        raise ValueError("GatherPoint expects (batch_size,num_result) idx shape")  # tf_sampling.cpp:135
    ix = L.require_cuda_i32(idx, "idx", 2)
    return _GroupPoint.apply(inp, ix.unsqueeze(2)).squeeze(2)


def prob_sample(inp, inpr):
    """inp [b,n] float32 weights, inpr [b,m] float32 draws in [0, 1) -> [b,m] int32 (tf_sampling.py:15-26): id j of row b is
    drawn with probability proportional to inp[b], by the reference's own cumulative sums and halving walk, bit for bit
    (include/dh3d_hip.h "Weighted sampling").  Not differentiable.  utils.sample_by_weight draws inpr on the device."""
    from . import pm
    with torch.no_grad():  # ops.NoGradient('ProbSample') (tf_sampling.py:26)
        return pm.prob_sample(inp, inpr)[0]


def three_nn(xyz1, xyz2):
    """xyz1 [b,n,3], xyz2 [b,m,3] -> (dist [b,n,3] squared, idx [b,n,3] int32) (tf_interpolate.py:8-18)."""
    a = L.require_cuda_f32(xyz1, "xyz1", 3)
    q = L.require_cuda_f32(xyz2, "xyz2", 3)
    if a.shape[2] != 3 or q.shape[2] != 3:
        raise ValueError("ThreeNN expects (b,n,3) xyz1 and (b,m,3) xyz2")  # tf_interpolate.cpp:163,168
    _same(q.shape[0], a.shape[0], "batch(xyz1/xyz2)")
    b, n, _ = a.shape
    m = q.shape[1]
    dist = torch.empty((b, n, 3), dtype=torch.float32, device=a.device)
    idx = torch.empty((b, n, 3), dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        L.check(L.lib().dh3d_three_nn(b, n, m, L.ptr(a), L.ptr(q), L.ptr(dist), L.ptr(idx), L.stream_ptr()),
                "three_nn")
    return dist, idx


class _ThreeInterpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, idx, weight):
        p = L.require_cuda_f32(points, "points", 3)
        ix = L.require_cuda_i32(idx, "idx", 3)
        w = L.require_cuda_f32(weight, "weight", 3)
        b, m, c = p.shape
        n = ix.shape[1]
        _same(tuple(ix.shape), (b, n, 3), "idx shape")  # tf_interpolate.cpp:197-206
        _same(tuple(w.shape), (b, n, 3), "weight shape")
        out = torch.empty((b, n, c), dtype=torch.float32, device=p.device)
        with torch.cuda.device(p.device):
            L.check(L.lib().dh3d_three_interpolate_fwd(b, m, c, n, L.ptr(p), L.ptr(ix), L.ptr(w), L.ptr(out),
                                                       L.stream_ptr()), "three_interpolate")
        ctx.save_for_backward(ix, w)
        ctx.pshape = (b, m, c)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        ix, w = ctx.saved_tensors
        b, m, c = ctx.pshape
        n = ix.shape[1]
        go = grad_out.contiguous()
        gp = torch.empty((b, m, c), dtype=torch.float32, device=go.device)
        with torch.cuda.device(go.device):
            L.check(L.lib().dh3d_three_interpolate_bwd(b, n, c, m, L.ptr(go), L.ptr(ix), L.ptr(w), L.ptr(gp),
                                                       L.stream_ptr()), "three_interpolate_grad")
        return gp, None, None


def three_interpolate(points, idx, weight):
    """points [b,m,c], idx [b,n,3], weight [b,n,3] -> [b,n,c] (tf_interpolate.py:19-34)."""
    return _ThreeInterpolate.apply(points, idx, weight)
