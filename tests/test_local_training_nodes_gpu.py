"""GPU: the local training step's autograd nodes one by one (dh3d_amd/train_ops.py conv_pointset_xyz / flex_pool / se_gate /
relu / add_channel_bias / linear / l2_normalize_rows, training.flex_conv_factorised / detection_block_train, ops.group_point
/ three_interpolate), forward and every gradient, against the float64 restatements of tests/local_training_reference.py.

Shapes: the step's own (4 clouds x 4096 points, the model's channel counts, its geometry) and a ragged batch (5 x 777:
B*N = 3885 is odd, so every launch ends in a partial tile).  Errors are reported in float32 unit roundoffs u of each
sum's own size (the same sum over |terms|, local_training_reference.linear_grads) unless a comment says otherwise.
"""
import contextlib

import numpy as np
import pytest
import torch

import local_training_reference as LR

pytestmark = pytest.mark.gpu

STEP = (4, 4096)        # the local step: 2 x (anchor + positive) clouds of 4096 points
RAGGED = (5, 777)

# Bounds in u of the sum's own size T (the float64 sum over |terms|).  Measured worst cases on the MI355X in comments.
TOL_POINTSET = 16.0     # conv_pointset forward / dtheta / dbias: measured worst 5.8 (forward, 5 x 777)
TOL_GEMM = 16.0         # linear / add_channel_bias forward and gradients: measured worst 5.4 (dx, 16384 x 64 -> 128);
                        # in and out of the zero arena against each other: 0.63 (dW, 3885 x 192 -> 128)
TOL_FLEX = 8.0          # flex_conv_factorised forward and gradients: measured worst 2.6 (forward, stage 2)
TOL_GATHER = 12.0       # group_point / three_interpolate forward and backward: measured worst 4.3 (three_interpolate dy)
TOL_L2 = 8.0            # l2_normalize_rows: measured worst 3.3 (dx, 16384 rows)
# se_gate uses __expf: exp(z) is off by up to ~|z| u (z * log2(e) rounded before the hardware 2^x); bound in u of
# ((|z| + 1) |ref|), plus u |x dy| g for the cancellation in 1 - g.  Measured worst 1.65 (dx)
TOL_SE = 6.0
# detection_block_train: BatchNorm backward through four layers, f32 GEMMs over 16384 / 18000 rows; relative to each
# tensor's largest entry (biases in front of a BatchNorm compared against 1e-4 of the largest gradient), the float64
# side on the kernels' ReLU patterns.  Measured worst 7.1e-4 (detec_conv1.b at 6 x 3000: a bias in front of a
# BatchNorm, rounding noise against the floor); every other tensor within 3e-6
TOL_DET = 2e-3
# its attention output, absolute (values in (0, 1)): measured worst 3.95e-7 (6 x 3000)
TOL_DET_FWD = 2e-6


def _cloud(B, N, seed, extent=12.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((B, N, 3), generator=g, dtype=torch.float32) * extent


def _knn(xyz, k):
    """Exact kNN within each cloud (self first where the coordinates are unique) [B,N,k] int32."""
    d = torch.cdist(xyz.double(), xyz.double())
    return d.topk(k, dim=2, largest=False).indices.to(torch.int32)


def _model(dev, preset="detection_config", seed=3):
    from dh3d_amd import ConfigFactory
    from dh3d_amd.model import DH3D
    cfg = ConfigFactory(preset).getconfig()
    cfg.num_points, cfg.batch_size = STEP[1], STEP[0] // 2
    return DH3D(cfg).init_synthetic(seed).to(dev).eval().prepare()


@pytest.fixture(scope="module")
def step_geometry(dev):
    """The model's own geometry of a step batch: (model, xyz [4,4096,3], nbr [4,4096,8], level dict)."""
    m = _model(dev)
    pts = _cloud(*STEP, seed=11).to(dev)
    with torch.no_grad():
        geo = m._geometry(pts, None)
        m._join_side(geo)
        lv = geo.level(8, m.knn_num)
        nbr = geo.nbr if geo.nbr.shape[2] == 8 else geo.nbr[:, :, 0:8].contiguous()
    torch.cuda.synchronize()
    return m, geo.xyz, nbr.contiguous(), lv


def _param(t, dev):
    return t.detach().clone().to(dev).requires_grad_(True)


def _report(name, **ratios):
    print("%s: worst error ratios %s" % (name, {k: round(v, 3) for k, v in ratios.items()}))


# ------------------------------------------------------------------------------------------------ conv_pointset_xyz
@pytest.mark.parametrize("B,N", [STEP, RAGGED])
def test_conv_pointset_xyz_forward_and_gradients(dev, B, N):
    """S[n] = sum_k (p[nbr[n,k]] - p[nbr[n,0]]): the centre is the list's rank-0 entry, whatever it is.  A kernel that
    took the point itself as centre is off by (K - 1)(p[n] - p[nbr[n,0]]) on the rotated lists -- ~1e6 u."""
    from dh3d_amd import train_ops as T
    xyz = _cloud(B, N, seed=B * N)
    xyz[:, 5::9] = xyz[:, 4::9][:, : xyz[:, 5::9].shape[1]]     # coincident points (pairs of equal coordinates)
    nbr = _knn(xyz, 8)
    nbr[:, ::5] = nbr[:, ::5].roll(1, dims=2)                    # rank 0 is the FARTHEST neighbour, not the point
    nbr[:, 2::5, 3:6] = nbr[:, 2::5, 1:2]                        # repeated ids within a list
    assert (nbr[:, :, 0] != torch.arange(N, dtype=torch.int32)).sum() > B * N // 5
    Dout = 32                                                    # initconv 3 -> 32
    g = torch.Generator().manual_seed(7)
    theta, bias = torch.randn((3, Dout), generator=g), torch.randn((Dout,), generator=g)
    dout = torch.randn((B, N, Dout), generator=g)
    tt, tb = _param(theta, dev), _param(bias, dev)
    out = T.conv_pointset_xyz(xyz.to(dev), nbr.to(dev), tt, tb)
    dtheta, dbias = torch.autograd.grad(out, (tt, tb), dout.to(dev))
    S, TS = LR.pointset_sums(LR.f64(xyz), nbr)
    th, bi, do = LR.f64(theta), LR.f64(bias), LR.f64(dout)
    ref, Tref = S @ th + bi, TS @ th.abs() + bi.abs()
    rd = S.reshape(-1, 3).t() @ do.reshape(-1, Dout)
    Trd = TS.reshape(-1, 3).t() @ do.reshape(-1, Dout).abs()
    rb, Trb = do.reshape(-1, Dout).sum(0), do.reshape(-1, Dout).abs().sum(0)
    r = dict(out=LR.ulp_ratio(out, ref, Tref), dtheta=LR.ulp_ratio(dtheta, rd, Trd), dbias=LR.ulp_ratio(dbias, rb, Trb))
    _report("conv_pointset_xyz %dx%d" % (B, N), **r)
    assert max(r.values()) <= TOL_POINTSET, r


# -------------------------------------------------------------------------------------------------------- flex_pool
def _pool_case(B, N, C, seed):
    """Positive features on a coarse grid of values (exact ties between different points everywhere), kNN lists with a
    repeated id in some of them, and in every cloud one hub point that is in EVERY list and wins a quarter of the
    channels outright (up to 8 x N atomics onto one row)."""
    g = torch.Generator().manual_seed(seed)
    xyz = _cloud(B, N, seed)
    nbr = _knn(xyz, 8)
    nbr[:, 3::11, 2] = nbr[:, 3::11, 6]                          # an id repeated in one list
    hub = torch.randint(0, N, (B,), generator=g)
    nbr[torch.arange(B), :, 7] = hub.view(B, 1).to(torch.int32)  # the hub: last in every list of its cloud
    x = (torch.randint(1, 5, (B, N, C), generator=g).float() * 0.25)
    x[torch.arange(B), hub, : C // 4] = 4.0                      # ... and the strict maximum of C/4 channels
    return x, nbr


@pytest.mark.parametrize("B,N,C", [(4, 4096, 32), (4, 4096, 64), (5, 777, 64)])
def test_flex_pool_forward_argmax_and_scatter(dev, B, N, C):
    """Forward value and argmax by the reference rule (first k of a tie); backward puts dout on exactly that neighbour
    (din[cloud0 + argmax]).  No atomic collides on an entry: bit-equal; elsewhere within (n - 1) u of the sum over
    |terms| (n contributions: a bound for ANY summation order).  Rejected variants: the last tied k winning (half the
    tied entries go to another row: an O(1) error), cloud0 dropped (clouds 1.. scatter into cloud 0)."""
    from dh3d_amd import pm
    from dh3d_amd import train_ops as T
    x, nbr = _pool_case(B, N, C, seed=B * N + C)
    want, warg = LR.flex_pool_rule(x.numpy(), nbr.numpy())
    xd, nd = x.to(dev), nbr.to(dev)
    out, arg = pm.flex_pool(xd, nd, want_argmax=True)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(arg.cpu().numpy(), warg)
    ties = (x.numpy()[np.arange(B)[:, None, None], nbr.numpy()] == want[:, :, None, :]).sum(2) > 1
    assert ties.mean() > 0.3                                     # the rule is exercised on most entries
    # the autograd node, with a dout that is not contiguous
    xp = xd.clone().requires_grad_(True)
    out2 = T.flex_pool(xp, nd)
    assert torch.equal(out2, out)
    big = torch.randn((B, N, 2 * C), generator=torch.Generator().manual_seed(3)).to(dev)
    dout = big[:, :, ::2]
    assert not dout.is_contiguous()
    (din,) = torch.autograd.grad(out2, xp, dout)
    ref, mag, cnt = LR.flex_pool_scatter(LR.f64(dout), torch.from_numpy(warg))
    got = LR.f64(din)
    single = cnt <= 1
    assert torch.equal(got[single], ref[single]), float((got - ref)[single].abs().max())
    many = ~single
    err = ((got - ref).abs() / (LR.U * (cnt - 1).clamp(min=1) * mag))[many]
    assert int(cnt.max()) >= N // 2                              # the hub's rows take thousands of atomics
    _report("flex_pool %dx%dx%d" % (B, N, C), collided=float(err.max()), max_contributions=float(cnt.max()))
    assert float(err.max()) <= 1.0


# --------------------------------------------------------------------------------------------------- se_gate / relu
def _signed(R, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((R, C), generator=g) * 3
    x[::7, ::5] = 0.0
    x[3::7, ::5] = -0.0
    return x


def test_se_gate_forward_and_gradients(dev):
    """relu(x + x sigmoid(z)) on x of both signs, +0 and -0, and z up to +-90 where __expf saturates (exp(90) is beyond
    float32): dz stays finite and goes to 0 there."""
    from dh3d_amd import train_ops as T
    R, C = 3885, 64                                          # R * C / 4 = 62160 lanes: a partial last workgroup
    x = _signed(R, C, 5)
    g = torch.Generator().manual_seed(6)
    z = (torch.rand((R, C), generator=g) * 2 - 1) * 30
    z[::13] = (torch.rand((z[::13].shape), generator=g) * 2 - 1) * 90
    z[1::13, :8] = torch.tensor([90.0, -90.0, 88.0, -88.0, 89.5, -89.5, 0.0, -0.0])
    dy = torch.randn((R, C), generator=g)
    xd, zd = _param(x, dev), _param(z, dev)
    y = T.se_gate(xd, zd)
    dx, dz = torch.autograd.grad(y, (xd, zd), dy.to(dev))
    assert torch.isfinite(dz).all() and torch.isfinite(dx).all() and torch.isfinite(y).all()
    x6, z6, dy6 = LR.f64(x), LR.f64(z), LR.f64(dy)
    ry, rdx, rdz, gate = LR.se_gate(x6, z6, dy6)
    big = (z6.abs() + 1)
    ratios = dict(y=LR.ulp_ratio(y, ry, big * ry.abs()), dx=LR.ulp_ratio(dx, rdx, big * rdx.abs()),
                  dz=LR.ulp_ratio(dz, rdz, big * rdz.abs() + (x6 * dy6).abs() * gate + (x6 * dy6).abs() * LR.FLT_MIN / LR.U))
    sat = z6.abs() >= 80
    ratios["dz_saturated"] = float((LR.f64(dz)[sat].abs() / ((x6 * dy6)[sat].abs() + 1e-30)).max())
    _report("se_gate", **ratios)
    assert ratios["dz_saturated"] <= 1e-30                   # exp(-80) = 1.8e-35 x |x dy|
    assert max(ratios["y"], ratios["dx"], ratios["dz"]) <= TOL_SE, ratios
    off = x6 <= 0                                            # x = 0, -0 and negatives: no gradient at all
    assert (dx.cpu()[off] == 0).all() and (dz.cpu()[off] == 0).all()


def test_relu_forward_bit_exact_and_gradient(dev):
    from dh3d_amd import train_ops as T
    R, C = 3885, 64
    x = _signed(R, C, 8)
    dy = torch.randn((R, C), generator=torch.Generator().manual_seed(9))
    xd = _param(x, dev)
    y = T.relu(xd)
    (dx,) = torch.autograd.grad(y, xd, dy.to(dev))
    y, dx = y.cpu(), dx.cpu()
    nz = x != 0
    want = torch.where(x > 0, x, torch.zeros_like(x))
    assert torch.equal(y[nz].view(torch.int32), want[nz].view(torch.int32))   # bit for bit
    assert (y[~nz] == 0).all()                                               # +0 or -0 in, a zero out
    wdx = torch.where(x > 0, dy, torch.zeros_like(dy))
    assert torch.equal(dx.view(torch.int32), wdx.view(torch.int32))          # dy where y > 0, +0 elsewhere
    _report("relu", zeros_in=int((~nz).sum()))


# ---------------------------------------------------------------------------------------- add_channel_bias / linear
# (R, Cin, Cout): the step's 1x1 convs at B*N = 16384 rows (SE f1 / f2 of stage 1, concat conv, shortcut), stage 2's SE
# at the sampled level (2048 rows), the detector's first layers, and the ragged row count
LINEAR_SHAPES = [(16384, 64, 16), (16384, 16, 64), (16384, 192, 128), (16384, 64, 128), (16384, 128, 256),
                 (16384, 256, 1024), (2048, 128, 32), (3885, 64, 16), (3885, 192, 128), (18000, 128, 128),
                 (18000, 128, 256), (18000, 256, 1024)]


@pytest.mark.parametrize("R,Cin,Cout", LINEAR_SHAPES)
def test_linear_and_channel_bias_in_and_out_of_the_zero_arena(dev, R, Cin, Cout):
    """y = add_channel_bias(linear(x, W, b), c): forward, dx, dW, db, dc -- once inside pm.zero_arena with a begun arena
    (a split-reduction gemm_tn returns dW as an arena VIEW: checked before the next begin(), which clears it) and once
    outside.  Both against float64, and against each other."""
    from dh3d_amd import _lib as L
    from dh3d_amd import pm
    from dh3d_amd import train_ops as T
    g = torch.Generator().manual_seed(R + Cin * 7 + Cout)
    x, W = torch.randn((R, Cin), generator=g), torch.randn((Cin, Cout), generator=g) * 0.2
    b, c, dy = torch.randn((Cout,), generator=g), torch.randn((Cout,), generator=g), torch.randn((R, Cout), generator=g)
    ref, refg, Tref, Trefg = LR.linear_grads(lambda x_, W_, b_, c_: x_ @ W_ + b_ + c_,
                                             [LR.f64(t) for t in (x, W, b, c)], LR.f64(dy))
    split = bool(L.lib().dh3d_gemm_is_split(1, Cin, Cout, R, 1))
    got = {}
    for in_arena in (True, False):
        ts = [_param(t, dev) for t in (x, W, b, c)]
        arena = pm.ZeroArena(fixed_bytes=1 << 22, device=dev)
        arena.begin(dev)
        with pm.zero_arena(arena) if in_arena else contextlib.nullcontext():
            y = T.add_channel_bias(T.linear(ts[0], ts[1], ts[2]), ts[3])
            grads = torch.autograd.grad(y, ts, dy.to(dev))
        r = dict(y=LR.ulp_ratio(y, ref, Tref))
        for nm, gg, rg, tg in zip(("dx", "dW", "db", "dc"), grads, refg, Trefg):
            r[nm] = LR.ulp_ratio(gg, rg, tg)
        in_buf = grads[1].untyped_storage().data_ptr() == arena.buf.untyped_storage().data_ptr()
        assert in_buf == (in_arena and split), (in_arena, split)
        got[in_arena] = [t.detach().clone() for t in (y,) + tuple(grads)]
        if in_buf:
            arena.begin(dev)                                  # the view's lifetime ends here: it reads zeros now
            assert not grads[1].any()
        _report("linear+bias R=%d %d->%d %s" % (R, Cin, Cout, "arena" if in_arena else "no arena"), **r)
        assert max(r.values()) <= TOL_GEMM, r
    # split partials meet in atomics: the two runs agree up to their order, in u of the same scales
    r = {nm: LR.ulp_ratio(a, LR.f64(bb), tg) for a, bb, tg, nm in zip(got[True], got[False], [Tref] + list(Trefg),
                                                                      ("y", "dx", "dW", "db", "dc"))}
    _report("linear+bias R=%d %d->%d arena against no arena" % (R, Cin, Cout), **r)
    assert max(r.values()) <= TOL_GEMM, r


# ------------------------------------------------------------------------------------------ flex_conv_factorised
@pytest.mark.parametrize("stage", ["stage1", "stage2"])
def test_flex_conv_factorised_at_the_step_geometry(dev, stage, step_geometry):
    """Every flex_conv of a stage at full resolution on the model's own geometry (stage 1: 4 x 4096 points, kNN 8;
    stage 2: the dilate-8 level, 4 x 512): forward, dfeat (the atomics scatter over the neighbour lists), dtheta, dbias."""
    from dh3d_amd.training import flex_conv_factorised
    m, pts, nbr, lv = step_geometry
    if stage == "stage1":
        xyz, nb = pts, nbr
    else:
        xyz, nb = lv["xyz_s"].contiguous(), lv["nbr_s"].contiguous()
    mod = getattr(m, stage)
    B, M = xyz.shape[0], xyz.shape[1]
    x6, n6 = LR.f64(xyz), nb.cpu()
    dp = LR.gather(x6, n6) - x6.unsqueeze(2)
    for i in range(len(mod.outdims)):
        fc = getattr(mod, "flexconv_%d" % i)
        Din, Dout = fc.position_theta.shape[1], fc.position_theta.shape[2]
        gen = torch.Generator().manual_seed(31 + i)
        feat = torch.randn((B, M, Din), generator=gen)
        dout = torch.randn((B, M, Dout), generator=gen)
        f, th, bi = _param(feat, dev), _param(fc.position_theta, dev), _param(fc.position_bias, dev)
        out = flex_conv_factorised(f, xyz, nb, th, bi)
        grads = torch.autograd.grad(out, (f, th, bi), dout.to(dev))
        # (dp is an input too, so that the error scale takes |dp|: the coordinate differences enter the sums as data)
        ref, refg, Tref, Trefg = LR.linear_grads(lambda f_, t_, b_, d_: LR.flex_conv(LR.gather(f_, n6), d_, t_, b_),
                                                 [LR.f64(feat), LR.f64(fc.position_theta), LR.f64(fc.position_bias), dp],
                                                 LR.f64(dout))
        r = dict(out=LR.ulp_ratio(out, ref, Tref))
        for nm, gg, rg, tg in zip(("dfeat", "dtheta", "dbias"), grads, refg, Trefg):
            r[nm] = LR.ulp_ratio(gg, rg, tg)
        _report("flex_conv_factorised %s.%d %dx%d %d->%d" % (stage, i, B, M, Din, Dout), **r)
        assert max(r.values()) <= TOL_FLEX, r


# ----------------------------------------------------------------------------------- group_point / three_interpolate
def test_group_point_and_three_interpolate_at_the_step_level(dev, step_geometry):
    """The level's own indices: group_point(x2 [4,4096,64], idx [4,512]) (FPS ids: no two equal, the scatter is exact),
    the same with repeated indices (collisions in the scatter), three_interpolate(y [4,512,128], nn3_idx, IDW weights)."""
    from dh3d_amd import ops, pm
    m, pts, nbr, lv = step_geometry
    B, N = pts.shape[0], pts.shape[1]
    gen = torch.Generator().manual_seed(41)
    x2 = torch.randn((B, N, 64), generator=gen)
    idx = lv["idx"].to(torch.int32).contiguous()
    rep = idx.clone()
    rep[:, 1::3] = rep[:, 0::3][:, : rep[:, 1::3].shape[1]]        # every id of a third of the list twice or more
    rep[:, 2::7] = rep[:, 0:1]
    ratios = {}
    for nm, ix in (("group_point", idx), ("group_point_repeated", rep)):
        xp = _param(x2, dev)
        out = ops.group_point(xp, ix.unsqueeze(2)).squeeze(2)
        dout = torch.randn(out.shape, generator=gen)
        (dx,) = torch.autograd.grad(out, xp, dout.to(dev))
        i6 = ix.cpu().long()
        ref, refg, Tref, Trefg = LR.linear_grads(lambda a: torch.gather(a, 1, i6.unsqueeze(-1).expand(-1, -1, 64)),
                                                 [LR.f64(x2)], LR.f64(dout))
        assert torch.equal(LR.f64(out), ref)
        if nm == "group_point":
            assert torch.equal(LR.f64(dx), refg[0])                 # one contribution per entry: exact
        ratios[nm] = LR.ulp_ratio(dx, refg[0], Trefg[0])
    M, C = lv["xyz_s"].shape[1], 128
    y = torch.randn((B, M, C), generator=gen)
    w = pm.idw_weights(lv["nn3_dist"])
    i3 = lv["nn3_idx"]
    yp = _param(y, dev)
    up = ops.three_interpolate(yp, i3, w)
    dout = torch.randn(up.shape, generator=gen)
    (dy,) = torch.autograd.grad(up, yp, dout.to(dev))
    i6, w6 = i3.cpu().long(), LR.f64(w)
    ref, refg, Tref, Trefg = LR.linear_grads(lambda a: (LR.gather(a, i6) * w6.unsqueeze(-1)).sum(2), [LR.f64(y)],
                                             LR.f64(dout))
    ratios["three_interpolate"] = LR.ulp_ratio(up, ref, Tref)
    ratios["three_interpolate_bwd"] = LR.ulp_ratio(dy, refg[0], Trefg[0])
    _report("group_point / three_interpolate", **ratios)
    assert max(ratios.values()) <= TOL_GATHER, ratios


# --------------------------------------------------------------------------------------------- l2_normalize_rows
@pytest.mark.parametrize("R", [STEP[0] * STEP[1], RAGGED[0] * RAGGED[1]])
def test_l2_normalize_rows_with_the_local_eps(dev, R):
    """eps = 1e-8 (model.py:177): rows with |x|^2 <= eps take the clamp -- gradient inv dy, no projection -- and an
    all-zero row gives zeros forward and dy / 1e-4 backward."""
    from dh3d_amd import train_ops as T
    gen = torch.Generator().manual_seed(R)
    x = torch.randn((R, 128), generator=gen)
    x[::9] *= 1e-6                                 # |x|^2 ~ 1.3e-10: clamped
    x[4::9] *= 6e-6                                # |x|^2 ~ 4.6e-9: clamped, within 3x of the threshold
    x[7] = 0.0
    dy = torch.randn((R, 128), generator=gen)
    xp = _param(x, dev)
    y = T.l2_normalize_rows(xp, 1e-8)
    (dx,) = torch.autograd.grad(y, xp, dy.to(dev))
    ry, rdx, Ty, Tdx = LR.l2_normalize_rows(LR.f64(x), LR.f64(dy), 1e-8)
    clamped = (LR.f64(x) ** 2).sum(1) <= 1e-8
    assert clamped.sum() > R // 6
    r = dict(y=LR.ulp_ratio(y, ry, Ty), dx=LR.ulp_ratio(dx, rdx, Tdx),
             dx_clamped=LR.ulp_ratio(dx.cpu()[clamped], rdx[clamped], Tdx[clamped]))
    _report("l2_normalize_rows R=%d" % R, **r)
    assert not y.cpu()[7].any()
    assert max(r.values()) <= TOL_L2, r


# ------------------------------------------------------------------------------------------- detection_block_train
@pytest.mark.parametrize("B,N", [STEP, (6, 3000)])
def test_detection_block_train_against_float64(dev, B, N, monkeypatch):
    """detection_block_train on feat [B, N, 128] with the detector's own weights (the step's 4 x 4096 and a ragged
    18000 rows): the attention forward, and the gradients of feat and of every detector parameter (W, b, gamma, beta of
    each conv, the logit's W and b).  The float64 side takes the HIP forward's ReLU patterns (ActivationPatterns):
    deciding them itself, it put a whole dy on the other side of four entries within rounding of the 1024-wide layer's
    kink at 4 x 4096, which moved the feat gradient by 3e-2 -- a lottery over rounding, not a kernel error."""
    from dh3d_amd.training import detection_block_train
    m = _model(dev, seed=4)
    det = m.detection_block_reliable
    gen = torch.Generator().manual_seed(51)
    feat = torch.randn((B, N, 128), generator=gen)
    datt = torch.randn((B, N, 1), generator=gen)
    params = list(det.named_parameters())
    f = _param(feat, dev)
    pat = LR.ActivationPatterns(monkeypatch)
    att = detection_block_train(m, f, False, None)
    monkeypatch.undo()
    grads = torch.autograd.grad(att, [f] + [p for _, p in params], datt.to(dev))
    # float64
    f6 = LR.f64(feat).requires_grad_(True)
    p6 = {n: LR.f64(p).requires_grad_(True) for n, p in params}
    layers = []
    for i in range(len(det.conv_dims)):
        c = getattr(det, "detec_conv%d" % i)
        pre = "detec_conv%d." % i
        layers.append((p6[pre + "W"].reshape(c.cin, c.cout), p6[pre + "b"], p6[pre + "bn.gamma"], p6[pre + "bn.beta"],
                       c.bn.eps))
    last = len(layers) - 1
    masks = lambda i, pre: pat.take(pre, pat.att[0] if i == last else pat.bn[id(getattr(det, "detec_conv%d" % i).bn)])
    ref = LR.detection_block(f6.reshape(B * N, 128), layers, p6["detec_conv_fc.W"].reshape(-1, 1), p6["detec_conv_fc.b"],
                             masks)
    refg = torch.autograd.grad(ref, [f6] + [p6[n] for n, _ in params], LR.f64(datt).reshape(B * N, 1))
    fwd = float((LR.f64(att).reshape(-1) - ref.detach().reshape(-1)).abs().max())
    top = max(float(g.abs().max()) for g in refg)
    report = []
    for nm, a, b in zip(["feat"] + [n for n, _ in params], grads, refg):
        scale = max(float(b.abs().max()), 1e-4 * top)
        report.append((float((LR.f64(a).reshape(b.shape) - b).abs().max()) / scale, nm))
    report.sort(reverse=True)
    print("detection_block_train %dx%d: attention max abs error %.3g; gradient errors (relative to the tensor's largest "
          "entry): %s; kinks where float64 would have gone the other way: %d"
          % (B, N, fwd, [(round(e, 6), n) for e, n in report[:6]], pat.flips))
    assert len(report) == 1 + 4 * len(det.conv_dims) + 2
    assert fwd <= TOL_DET_FWD
    assert report[0][0] <= TOL_DET, report[0]
