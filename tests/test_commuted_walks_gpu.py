"""GPU: every entry point of the commuted training walks -- interp_bn_colstats / _bwd_sums / _bwd_apply,
interp_head_rows, three_interpolate_bwd_sorted, interp_scatter_scaled and netvlad_commuted_fwd_stats / _fwd_assign /
_bwd_sums / _bwd_apply -- kernel by kernel against the float64 restatements of tests/commuted_reference.py.

Each kernel gets f32 inputs (the NetVLAD chain: the previous kernel's outputs) and is compared with the float64
reference computed from exactly those inputs: |got - ref| <= RTOL * T + 1e-30 everywhere, T the reference's error
scale.  Power: dropping any one of a few chosen points (the last one of a partial block among them) from a sum or a
scatter must move some entry by more than that bound (by 10x for the median one), and per-point outputs must sit
well above it.  The cases span
the slot table's capacities (blocks touching exactly 56 / 57 / 64 / 65 / 200 distinct coarse rows), both layouts of G,
Hd 256 / 512 / 768 / 1024, m up to 1024, n below one block and with a partial last block, B beyond the eight XCDs,
Morton, identity (None) and random-permutation walk orders, real clouds (tests/golden/demo_clouds.npz), duplicate
neighbours, zero and widely spread distances, padding clouds whose inputs are NaN, and rows held by the l2 clamp."""
import os

import numpy as np
import pytest
import torch

import commuted_reference as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAN = float("nan")

# name: (B, n, m, Hd, row_major, order, idx kind, padding clouds, extras)
#   order: "sort" (spatial_sort of the cloud), "none" (index order), "perm" (records of a random permutation)
#   idx:   "real" (three_nn of demo clouds), ("blocks", D) (each 128-point block of the walk touches D rows), "random"
#   padding: None, "first", "last", "all_but_one"
CASES = {
    "real_b3_sort": (3, 4096, 512, 1024, 0, "sort", "real", None, "clamp"),
    "real_b3_perm_pad": (3, 4096, 512, 256, 1, "perm", "real", "first", "clamp"),
    "real_m1024": (1, 4096, 1024, 512, 1, "sort", "real", None, ""),   # (the first half of an 8192-point cloud)
    "blk56_n128": (1, 128, 512, 512, 1, "none", ("blocks", 56), None, "dup"),
    "blk57_n129": (3, 129, 512, 256, 0, "none", ("blocks", 57), "last", "dup"),
    "blk64_b9": (9, 1000, 1024, 768, 0, "none", ("blocks", 64), None, "dup spread"),
    "blk65_b22": (22, 4096, 512, 256, 1, "none", ("blocks", 65), "all_but_one", "dup zero"),
    "blk200": (3, 4096, 1024, 1024, 0, "none", ("blocks", 200), "first", "spread"),
    "blk56_m56": (9, 1000, 56, 256, 0, "none", ("blocks", 56), "last", "zero"),
    "m3_n100": (9, 100, 3, 512, 1, "perm", "random", "last", "dup zero spread"),
    "random_b22": (22, 129, 1024, 256, 0, "none", "random", "first", "clamp spread"),
    "n100_b1": (1, 100, 56, 1024, 1, "none", "random", None, "dup clamp"),
}

_WORST = {}


def _record(case, name, ratio):
    key = name.split("[")[0]
    _WORST.setdefault(key, (0.0, ""))
    if ratio > _WORST[key][0]:
        _WORST[key] = (ratio, case)


@pytest.fixture(scope="module")
def demo():
    return np.load(os.path.join(HERE, "golden", "demo_clouds.npz"))


def _lib():
    from dh3d_amd import _lib as L
    return L


def _call(name, *args):
    L = _lib()
    L.check(getattr(L.lib(), name)(*[L.ptr(a) if isinstance(a, torch.Tensor) or a is None else a for a in args]
                                   + [L.stream_ptr()]), name)


def _perm_records(B, n, g, dev):
    rec = torch.rand(B, n, 4, generator=g)
    perm = torch.stack([torch.randperm(n, generator=g) for _ in range(B)]).to(torch.int32)
    rec[..., 3] = perm.view(torch.float32)
    return rec.to(dev)


def _blocks_idx(B, n, m, D, g):
    """idx[p, t] = R_k[(3p + t) % D] over the points p of block k (index order): block k touches exactly min(D, the
    rows its points reach) distinct coarse rows R_k; R_0 of every cloud holds row m - 1."""
    idx = torch.empty(B, n, 3, dtype=torch.int64)
    for b in range(B):
        for k in range((n + 127) // 128):
            Rk = torch.randperm(m, generator=g)[:D]
            if k == 0 and not bool((Rk == m - 1).any()):
                Rk[0] = m - 1
            p = torch.arange(k * 128, min(n, k * 128 + 128))
            pl = p - k * 128
            for t in range(3):
                idx[b, p, t] = Rk[(3 * pl + t) % D]
    return idx


def _case(name, demo, dev):
    B, n, m, Hd, rm, order_kind, idx_kind, padding, extras = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if idx_kind == "real":
        keys = {512: ["global_a", "global_b"], 1024: ["global_c"]}[m]
        keys = [keys[b % len(keys)] for b in range(B)]
        pts = torch.from_numpy(np.stack([demo[k][:n] for k in keys]))
        idx = torch.from_numpy(np.stack([demo[k + "/nn3_idx"][:n] for k in keys])).long()
        dist = torch.from_numpy(np.stack([demo[k + "/nn3_dist"][:n] for k in keys])).double()
        assert pts.shape[1] == n and int(idx.max()) < m
    elif idx_kind == "random":
        idx = torch.randint(0, m, (B, n, 3), generator=g)
        dist = torch.rand(B, n, 3, generator=g, dtype=torch.float64) * 1e-2
    else:
        idx = _blocks_idx(B, n, m, idx_kind[1], g)
        dist = torch.rand(B, n, 3, generator=g, dtype=torch.float64) * 1e-2
    if not isinstance(idx_kind, tuple):
        idx[:, -1, 0] = m - 1                      # the last coarse row is used in every cloud (blocks: in R_0)
    if "dup" in extras:                            # i0 = i1 = i2 (two points per block keep their rows' other uses)
        for k in range(0, n, 128):
            for p in (k + 5, k + 77):
                if p < n - 1:
                    idx[:, p, 1:] = idx[:, p, :1]
    if "zero" in extras:                           # one zero distance, and all three zero
        dist[:, ::7, 0] = 0.0
        dist[:, 3::11, :] = 0.0
    if "spread" in extras:                         # distances over six decades
        dist = dist * 10.0 ** (6 * torch.rand(B, n, 3, generator=g, dtype=torch.float64) - 3)
    c = torch.randn(B, m, 256, generator=g)
    clamp_pts = None
    if "clamp" in extras:                          # coarse rows of norm 7e-7; points that use only them: |x|^2 < 1e-12
        rows = torch.unique(idx[:, ::97, 0].reshape(-1))[:8]
        c[:, rows] *= 7e-7 / c[:, rows].norm(dim=-1, keepdim=True)
        clamp_pts = torch.zeros(B, n, dtype=torch.bool)
        for b in range(B):
            sel = torch.isin(idx[b, :, 0], rows).nonzero().reshape(-1)[::2]
            idx[b, sel, 1:] = idx[b, sel, :1]
            clamp_pts[b, sel] = True
    if order_kind == "sort":
        from dh3d_amd import pm
        order = pm.spatial_sort(pts.to(dev).float().contiguous())[0]
    elif order_kind == "perm":
        order = _perm_records(B, n, g, dev)
    else:
        order = None
    live = torch.ones(B, dtype=torch.bool)
    if padding == "first":
        live[0] = False
    elif padding == "last":
        live[-1] = False
    elif padding == "all_but_one":
        live[:] = False
        live[B // 2] = True
    return dict(B=B, n=n, m=m, Hd=Hd, rm=rm, g=g, idx=idx.to(torch.int32).to(dev).contiguous(),
                dist=dist.float().to(dev).contiguous(), order=order, live=live.to(dev), c=c.to(dev),
                clamp_pts=None if clamp_pts is None else clamp_pts.to(dev), padding=padding)


def _walk_points(K):
    """A few (cloud, original point index) pairs of a live cloud: the last point of the walk (in a partial block if n %
    128), the first point of the last block, point 0 of the walk and one more."""
    b = int(K["live"].nonzero()[0 if K["padding"] != "first" else -1])
    n = K["n"]
    walk = torch.arange(n) if K["order"] is None else K["order"][b, :, 3].contiguous().view(torch.int32).cpu().long()
    pos = sorted({n - 1, (n - 1) // 128 * 128, 0, n // 3})
    return [(b, int(walk[q])) for q in pos]


def _nanpad(x, live, per_cloud_dims=1):
    """x [B, ...]: the padding clouds' entries set to NaN (their inputs must never be read)."""
    x = x.clone()
    x[~live] = NAN
    return x


class Checker:
    def __init__(self, case):
        self.case = case

    def close(self, name, got, ref, T, sel=None):
        got, ref, T = got.double(), ref.double(), T.double()
        if sel is not None:
            got, ref, T = got[sel], ref[sel], T[sel]
        assert bool(torch.isfinite(got).all()), (self.case, name, "non-finite output")
        dev = (got - ref).abs()
        bound = R.RTOL * T + 1e-30
        ratio = float((dev / (T + 1e-300)).max()) if dev.numel() else 0.0
        _record(self.case, name, ratio)
        bad = dev > bound
        if bool(bad.any()):
            i = int(bad.reshape(-1).nonzero()[0])
            raise AssertionError("%s %s: %d entries off, first |got-ref| %.3e, ref %.3e, T %.3e, max |got-ref|/T %.2e" % (
                self.case, name, int(bad.sum()), float(dev.reshape(-1)[i]), float(ref.reshape(-1)[i]),
                float(T.reshape(-1)[i]), ratio))

    def per_point_power(self, name, ref, T, sel):
        ref, T = ref[sel].double().abs(), T[sel].double()
        assert float((R.RTOL * T).median()) < 0.1 * float(ref.median()) + 1e-30, (self.case, name)

    def drop_power(self, name, ref, T, dropped):
        """Removing one point moves some entry by more than the bound for every chosen point, and by more than 10x
        the bound for the median one (a point of typical weight)."""
        ratios = []
        for (b, i), refd in dropped:
            move = (ref.double() - refd.double()).abs()
            ratios.append(float((move / (R.RTOL * T.double() + 1e-30)).max()))
            assert ratios[-1] > 1.0, (self.case, name, "dropping point", b, i, ratios[-1])
        if ratios:
            assert float(np.median(ratios)) > 10.0, (self.case, name, "dropping a point", ratios)


def _drops(K, w, extra, fn):
    """fn(w, extra) evaluated with each chosen point removed (weights and per-point scalars zero)."""
    out = []
    for b, i in _walk_points(K):
        w2 = w.clone()
        w2[b, i] = 0.0
        ex2 = []
        for e in extra:
            e2 = e.clone()
            e2[b, i] = 0.0
            ex2.append(e2)
        out.append(((b, i), fn(w2, ex2)))
    return out


def _slices(Gf, rm):
    B, m, Hd = Gf.shape
    if rm:
        return Gf.reshape(B * m, Hd).contiguous()
    return Gf.reshape(B * m, Hd // 256, 256).permute(1, 0, 2).contiguous()


def _unslice(X, B, m, rm):
    if rm:
        return X.reshape(B, m, -1)
    return X.permute(1, 0, 2).reshape(B, m, -1)


@pytest.mark.parametrize("name", sorted(CASES))
def test_attention_walks_match_float64(dev, demo, name):
    K = _case(name, demo, dev)
    B, n, m, Hd, rm, g = K["B"], K["n"], K["m"], K["Hd"], K["rm"], K["g"]
    idx, dist, order, live = K["idx"], K["dist"], K["order"], K["live"]
    mask = live.to(torch.uint8) if K["padding"] else None
    chk = Checker(name)
    w = R.idw_weights(dist)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    Gf = rnd(B, m, Hd)
    Gin = _nanpad(Gf, live) if mask is not None else Gf
    G = _slices(Gin, rm)

    # colstats
    part = torch.zeros(2, B, Hd, dtype=torch.float64, device=dev)
    _call("dh3d_interp_bn_colstats", G, Hd, rm, idx, dist, order, B, n, m, mask, part)
    ref, T = R.interp_bn_colstats(Gf, idx, w, live)
    chk.close("interp_bn_colstats", part, ref, T)
    assert float(part[:, ~live].abs().max() if (~live).any() else 0.0) == 0.0
    chk.drop_power("interp_bn_colstats", ref, T, _drops(K, w, [], lambda w2, e: R.interp_bn_colstats(Gf, idx, w2, live)[0]))

    # the training forward of the head (no mask: every cloud's rows; compared on the live ones)
    scale, shift = (0.5 + torch.rand(Hd, generator=g)).to(dev), (0.5 * torch.randn(Hd, generator=g)).to(dev)
    wfc, bfc = rnd(Hd) / Hd ** 0.5, rnd(1)
    from dh3d_amd import pm
    att = torch.full((B * n,), NAN, device=dev)
    ep = _lib().make_epilogue(None, scale, shift, pm.ACT_RELU)
    L = _lib()
    L.check(L.lib().dh3d_interp_head_sorted_fwd_dev(L.ptr(G), Hd, rm, L.ptr(idx), L.ptr(dist), L.ptr(order), B, n, m,
                                                    ep, L.ptr(wfc), L.ptr(bfc), L.ptr(att), L.stream_ptr()), "head")
    ref, T = R.interp_head_rows(Gf, idx, w, scale, shift, wfc, float(bfc))
    chk.close("interp_head_rows", att.reshape(B, n), ref, T, sel=live)
    chk.per_point_power("interp_head_rows", ref, T, live)

    # backward sums
    dlogit = rnd(B, n)
    dl_in = _nanpad(dlogit, live) if mask is not None else dlogit
    mean, rstd = 0.1 * rnd(Hd), (0.5 + torch.rand(Hd, generator=g)).to(dev)
    gamma, beta = (0.5 + torch.rand(Hd, generator=g)).to(dev), 0.3 * rnd(Hd)
    part3 = torch.zeros(3, B, Hd, dtype=torch.float64, device=dev)
    _call("dh3d_interp_bn_bwd_sums", G, Hd, rm, idx, dist, order, B, n, m, mask, dl_in, wfc, mean, rstd, gamma, beta,
          part3)
    ref, T = R.interp_bn_bwd_sums(Gf, idx, w, dlogit, wfc, mean, rstd, gamma, beta, live)
    chk.close("interp_bn_bwd_sums", part3, ref, T)
    assert float(part3[:, ~live].abs().max() if (~live).any() else 0.0) == 0.0
    chk.drop_power("interp_bn_bwd_sums", ref, T, _drops(K, w, [dlogit], lambda w2, e: R.interp_bn_bwd_sums(
        Gf, idx, w2, e[0], wfc, mean, rstd, gamma, beta, live)[0]))

    # backward apply (dG zeroed by the caller)
    k2, k3 = 0.1 * rnd(Hd), 0.1 * rnd(Hd)
    dG = torch.zeros_like(G)
    _call("dh3d_interp_bn_bwd_apply", G, Hd, rm, idx, dist, order, B, n, m, mask, dl_in, wfc, scale, shift, k2, k3, dG)
    ref, T = R.interp_bn_bwd_apply(Gf, idx, w, dlogit, wfc, scale, shift, k2, k3, live)
    got = _unslice(dG, B, m, rm)
    chk.close("interp_bn_bwd_apply", got, ref, T)
    assert float(got[~live].abs().max() if (~live).any() else 0.0) == 0.0
    chk.drop_power("interp_bn_bwd_apply", ref, T, _drops(K, w, [dlogit], lambda w2, e: R.interp_bn_bwd_apply(
        Gf, idx, w2, e[0], wfc, scale, shift, k2, k3, live)[0]))

    # three_interpolate's backward on the walk (explicit weights; overwrites its NaN-filled output; no mask)
    dY = rnd(B, n, 256)
    wt = torch.rand(B, n, 3, generator=g).to(dev)
    wt = (wt / wt.sum(-1, keepdim=True)).contiguous()
    gp = torch.full((B, m, 256), NAN, device=dev)
    _call("dh3d_three_interpolate_bwd_sorted", B, n, 256, m, dY, idx, wt, order, gp)
    ref, T = R.three_interpolate_bwd(dY, idx, wt, m)
    chk.close("three_interpolate_bwd_sorted", gp, ref, T)
    chk.drop_power("three_interpolate_bwd_sorted", ref, T,
                   _drops(K, wt.double(), [], lambda w2, e: R.three_interpolate_bwd(dY, idx, w2, m)[0]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_netvlad_walks_match_float64(dev, demo, name):
    K = _case(name, demo, dev)
    B, n, m, g = K["B"], K["n"], K["m"], K["g"]
    idx, dist, order, live = K["idx"], K["dist"], K["order"], K["live"]
    mask = live.to(torch.uint8) if K["padding"] else None
    pad = (lambda x: _nanpad(x, live)) if mask is not None else (lambda x: x)
    chk = Checker(name)
    w = R.idw_weights(dist)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    lv = live[:, None].expand(B, n)
    c = K["c"]
    Wc = rnd(256, 64) / 16.0
    cw = (c.reshape(B * m, 256) @ Wc).reshape(B, m, 64)
    c_in, cw_in = pad(c).reshape(B * m, 256).contiguous(), pad(cw).reshape(B * m, 64).contiguous()

    # fwd_stats: s, rinv on the fine points, per-cloud statistics of s
    s = torch.full((B * n, 64), NAN, device=dev)
    rinv = torch.full((B * n,), NAN, device=dev)
    part = torch.zeros(2, B, 64, dtype=torch.float64, device=dev)
    _call("dh3d_netvlad_commuted_fwd_stats", c_in, cw_in, idx, dist, order, B, n, m, mask, s, rinv, part)
    f = R.nv_fwd_stats(c, cw, idx, w, live)
    s3, r2 = s.reshape(B, n, 64), rinv.reshape(B, n)
    chk.close("nv_fwd_stats.s", s3, f["s"], f["T_s"], sel=lv)
    chk.close("nv_fwd_stats.rinv", r2, f["rinv"], f["T_rinv"], sel=lv)
    chk.close("nv_fwd_stats.part", part, f["part"], f["T_part"])
    assert float(part[:, ~live].abs().max() if (~live).any() else 0.0) == 0.0
    chk.per_point_power("nv_fwd_stats.s", f["s"], f["T_s"], lv)
    chk.drop_power("nv_fwd_stats.part", f["part"], f["T_part"],
                   _drops(K, w, [], lambda w2, e: R.nv_fwd_stats(c, cw, idx, w2, live)["part"]))
    if K["clamp_pts"] is not None:
        assert bool(f["clamped"][K["clamp_pts"] & lv].all()) and bool((K["clamp_pts"] & lv).any())
    # what the later kernels read of a padding cloud is NaN
    s_in, rinv_in = pad(s3).reshape(B * n, 64).contiguous(), pad(r2).reshape(B * n).contiguous()

    # fwd_assign
    scale, shift = (1.0 + 2 * torch.rand(64, generator=g)).to(dev), 0.5 * rnd(64)
    att = (0.25 + 0.75 * torch.rand(B, n, generator=g)).to(dev)
    att_in = pad(att).reshape(B * n).contiguous()
    p = torch.full((B * n, 64), NAN, device=dev)
    asum = torch.zeros(B, 64, device=dev)
    Ap = torch.zeros(B * m, 64, device=dev)
    _call("dh3d_netvlad_commuted_fwd_assign", s_in, rinv_in, att_in, scale, shift, idx, dist, order, B, n, m, mask, p,
          asum, Ap)
    fa = R.nv_fwd_assign(s3, r2, att, scale, shift, idx, w, m, live)
    p3 = p.reshape(B, n, 64)
    chk.close("nv_fwd_assign.p", p3, fa["p"], fa["T_p"], sel=lv)
    chk.close("nv_fwd_assign.asum", asum, fa["asum"], fa["T_asum"])
    chk.close("nv_fwd_assign.Ap", Ap.reshape(B, m, 64), fa["Ap"], fa["T_Ap"])
    if (~live).any():
        assert float(asum[~live].abs().max()) == 0.0 and float(Ap.reshape(B, m, 64)[~live].abs().max()) == 0.0
    chk.per_point_power("nv_fwd_assign.p", fa["p"], fa["T_p"], lv)
    drops = _drops(K, w, [att], lambda w2, e: R.nv_fwd_assign(s3, r2, e[0], scale, shift, idx, w2, m, live))
    chk.drop_power("nv_fwd_assign.asum", fa["asum"], fa["T_asum"], [(k, d["asum"]) for k, d in drops])
    chk.drop_power("nv_fwd_assign.Ap", fa["Ap"], fa["T_Ap"], [(k, d["Ap"]) for k, d in drops])

    # bwd_sums
    E = (c.reshape(B * m, 256) @ (rnd(256, 64) / 16.0)).reshape(B, m, 64)   # c dV^T: small on the tiny rows too
    dasum = rnd(B, 64)
    mean, rstd = 0.05 * rnd(64), (5.0 + 5 * torch.rand(64, generator=g)).to(dev)
    dz = torch.full((B * n, 64), NAN, device=dev)
    datt = torch.full((B * n,), NAN, device=dev)
    t2 = torch.full((B * n,), NAN, device=dev)
    part = torch.zeros(2, B, 64, dtype=torch.float64, device=dev)
    _call("dh3d_netvlad_commuted_bwd_sums", pad(E).reshape(B * m, 64).contiguous(), pad(p3).reshape(B * n, 64).contiguous(),
          s_in, att_in, rinv_in, dasum, mean, rstd, idx, dist, order, B, n, m, mask, dz, datt, t2, part)
    bs = R.nv_bwd_sums(E, p3, s3, att, r2, dasum, mean, rstd, idx, w, live)
    dz3, datt2, t22 = dz.reshape(B, n, 64), datt.reshape(B, n), t2.reshape(B, n)
    chk.close("nv_bwd_sums.dz", dz3, bs["dz"], bs["T_dz"], sel=lv)
    chk.close("nv_bwd_sums.datt", datt2, bs["datt"], bs["T_datt"])     # padding clouds: exactly 0
    chk.close("nv_bwd_sums.t2", t22, bs["t2"], bs["T_t2"], sel=lv)
    chk.close("nv_bwd_sums.part", part, bs["part"], bs["T_part"])
    if (~live).any():
        assert float(datt2[~live].abs().max()) == 0.0 and float(part[:, ~live].abs().max()) == 0.0
    chk.per_point_power("nv_bwd_sums.dz", bs["dz"], bs["T_dz"], lv)
    chk.per_point_power("nv_bwd_sums.datt", bs["datt"], bs["T_datt"], lv)
    chk.drop_power("nv_bwd_sums.part", bs["part"], bs["T_part"], _drops(K, w, [att], lambda w2, e: R.nv_bwd_sums(
        E, p3, s3, e[0], r2, dasum, mean, rstd, idx, w2, live)["part"]))

    # bwd_apply: q (0 where the l2 clamp held the row) and dcw
    k1, k2, k3 = scale, 0.1 * rnd(64), 0.5 * rnd(64)
    q = torch.full((B * n,), NAN, device=dev)
    dcw = torch.zeros(B * m, 64, device=dev)
    _call("dh3d_netvlad_commuted_bwd_apply", pad(dz3).reshape(B * n, 64).contiguous(), s_in, rinv_in,
          pad(t22).reshape(B * n).contiguous(), k1, k2, k3, idx, dist, order, B, n, m, mask, q, dcw)
    ba = R.nv_bwd_apply(dz3, s3, r2, t22, k1, k2, k3, idx, w, m, f["clamped"], f["clamp_amb"], live)
    q2 = q.reshape(B, n)
    if K["clamp_pts"] is not None:   # (reported: how far the kernel's q is off on the clamped rows)
        naive = R.nv_bwd_apply(dz3, s3, r2, t22, k1, k2, k3, idx, w, m, torch.zeros_like(f["clamped"]), None, live)
        cl = f["clamped"] & lv
        _record(name, "nv_bwd_apply.q on clamped rows, |got| / (RTOL T of the unclamped formula)",
                float((q2[cl].double().abs() / (R.RTOL * naive["T_q"][cl])).max()))
    chk.close("nv_bwd_apply.q", q2, ba["q"], ba["T_q"], sel=lv)
    chk.close("nv_bwd_apply.dcw", dcw.reshape(B, m, 64), ba["dcw"], ba["T_dcw"])
    if (~live).any():
        assert float(dcw.reshape(B, m, 64)[~live].abs().max()) == 0.0
    chk.drop_power("nv_bwd_apply.dcw", ba["dcw"], ba["T_dcw"], _drops(K, w, [], lambda w2, e: R.nv_bwd_apply(
        dz3, s3, r2, t22, k1, k2, k3, idx, w2, m, f["clamped"], f["clamp_amb"], live)["dcw"]))

    # interp_scatter_scaled ADDS to a pre-filled dc
    dc0 = rnd(B, m, 256)
    dc = dc0.clone().reshape(B * m, 256)
    _call("dh3d_interp_scatter_scaled", c_in, pad(q2).reshape(B * n).contiguous(), idx, dist, order, B, n, m, mask, dc)
    ref, T = R.interp_scatter_scaled(c, q2, idx, w, dc0, live)
    chk.close("interp_scatter_scaled", dc.reshape(B, m, 256), ref, T)
    if (~live).any():
        assert torch.equal(dc.reshape(B, m, 256)[~live], dc0[~live])
    qd = q2.double()
    drops = []
    for (b, i) in _walk_points(K):
        if float(qd[b, i].abs()) > 0:
            w2 = w.clone()
            w2[b, i] = 0.0
            drops.append(((b, i), R.interp_scatter_scaled(c, q2, idx, w2, dc0, live)[0]))
    chk.drop_power("interp_scatter_scaled", ref, T, drops)


def test_zz_report_worst_ratios():
    """Prints the worst |got - ref| / T per output over the cases run (informational; run with -s or -rA)."""
    for k in sorted(_WORST):
        print("worst %-70s %.3e  (%s)" % (k, _WORST[k][0], _WORST[k][1]))
