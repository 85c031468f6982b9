"""local_tail_fused (csrc/dense_tail.hip) with the up-sampled coarse rows as the INITIAL value of the lower block's
accumulators: the interpolated value is the first addend of the accumulation chain, the gathers run ahead of both GEMMs.

Every case compares with the float64 restatement tests/dense_reference.local_tail_fused within 2e-6 * max|y| (y: the
restatement's feature columns), checks that the xyz prefix is bit-equal and that no row behind R is written (the output
buffer is NaN-filled and longer than R).  Shapes: the smallest at which the kernel's structure differs --
  (1, 32, 3)    one tile: seven waves of the workgroup own no rows, move their share of the weights and take the barriers;
                every row mixes the same three coarse rows;
  (2, 96, 9)    tiles of two clouds in one workgroup: the per-cloud base of the coarse rows differs between waves;
  (3, 288, 40)  27 tiles = four workgroups, the last one partial; the XCD remap of the block index is live.
Variants: 'clamped' (a dist row of exact zeros, one of three equal distances: the clamp of idw3), 'cw1e3' (coarse rows
x 1e3 against a unit-scale GEMM term: a seeding error is not hidden under the products; the accumulation then rounds at
ulp(1e3) 24 times at worst, 1.4e-6 relative to the ELEMENT, under the bound), 'cw0' (coarse rows all zero: the
GEMM-only restatement), 'dead_relu' (a shift of -1e4 on the concat branch: the output is the shortcut alone)."""
import numpy as np
import pytest
import torch

import dense_reference as D

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 3), (2, 96, 9), (3, 288, 40)]
VARIANTS = ["base", "clamped", "cw1e3", "cw0", "dead_relu"]
PAD = 8
_REF = {}


def _case(shape, variant):
    """Inputs and the float64 restatements (with and without prefix), computed once per (shape, variant)."""
    key = (shape, variant)
    if key in _REF:
        return _REF[key]
    B, n, m = shape
    rng = np.random.default_rng(1000 * n + VARIANTS.index(variant))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    x1, x2 = f(B, n, 64), f(B, n, 64)
    Ws, Wl = (f(64, 128) / 8).astype(np.float32), (f(64, 128) / 8).astype(np.float32)
    cw = (0.25 * f(B, m, 128) + (np.arange(B)[:, None, None] + 1.0)).astype(np.float32)   # cloud b around b + 1
    idx = rng.integers(0, m, (B, n, 3)).astype(np.int32)
    dist = (rng.random((B, n, 3)) * 1e-2 + 1e-4).astype(np.float32)
    xyz = f(B, n, 3)
    e_s = [0.1 * f(128), (0.5 + rng.random(128)).astype(np.float32), 0.1 * f(128)]
    e_c = [0.1 * f(128), (0.5 + rng.random(128)).astype(np.float32), 0.1 * f(128)]
    if variant == "clamped":
        dist[:, 0::5, :] = 0.0
        dist[:, 1::5, :] = np.float32(0.0625)
        dist[:, 2::5, 0] = 0.0
    elif variant == "cw1e3":
        cw = (cw * np.float32(1e3)).astype(np.float32)
    elif variant == "cw0":
        cw[:] = 0.0
    elif variant == "dead_relu":
        e_c[2] = np.full(128, -1e4, np.float32)
    ins = dict(x1=x1, x2=x2, Ws=Ws, Wl=Wl, cw=cw, idx=idx, dist=dist, xyz=xyz, e_s=e_s, e_c=e_c)
    refs = {pre: D.local_tail_fused(x1, x2, Ws, Wl, e_s, e_c, cw, idx, dist, xyz if pre else None, 1e-12)[0]
            for pre in (True, False)}
    if variant == "dead_relu":   # the restatement itself is the shortcut alone
        short = np.maximum((x1.astype(np.float64) @ Ws + e_s[0]) * e_s[1] + e_s[2], 0)
        assert np.allclose(refs[False], short, rtol=1e-12, atol=0)
    _REF[key] = (ins, refs)
    return _REF[key]


@pytest.mark.parametrize("prefix", [True, False], ids=["prefix", "plain"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_seeded_tail_vs_float64(dev, shape, variant, prefix):
    from dh3d_amd import _lib as L
    from dh3d_amd import pm
    B, n, m = shape
    ins, refs = _case(shape, variant)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    R, width = B * n, 131 if prefix else 128
    buf = torch.full((R + PAD, width), float("nan"), dtype=torch.float32, device=dev)
    keep = [T(v) for v in ins["e_s"] + ins["e_c"]]
    args = [T(ins["x1"]), T(ins["x2"]), pm.pack_weight_x3(T(ins["Ws"])), pm.pack_weight_x3(T(ins["Wl"]))]
    geo = [T(ins["cw"]), T(ins["idx"]), T(ins["dist"]), T(ins["xyz"]) if prefix else None]
    L.check(L.lib().dh3d_local_tail_fused_fwd(*[L.ptr(a) for a in args], L.make_epilogue(*keep[:3], D.ACT_RELU),
                                              L.make_epilogue(*keep[3:], D.ACT_RELU), *[L.ptr(a) for a in geo], 1e-12,
                                              B, n, m, L.ptr(buf), L.stream_ptr()), "local_tail_fused")
    torch.cuda.synchronize()
    fill = torch.full((1,), float("nan"), dtype=torch.float32).view(torch.int32).item()
    assert bool((buf[R:].view(torch.int32) == fill).all()), "rows past R were written"
    got = buf[:R].cpu().numpy().reshape(B, n, width)
    ref = np.asarray(refs[prefix]).reshape(B, n, width)
    if prefix:
        assert np.array_equal(got[..., :3], ins["xyz"]), "the xyz prefix is not bit-equal"
        got, ref = got[..., 3:], ref[..., 3:]
    assert np.isfinite(got).all()
    err, bound = np.abs(got - ref).max(), 2e-6 * np.abs(ref).max()
    print("local_tail_fused %s %s %s: max|got - ref| %.3e, bound %.3e" % (shape, variant, "prefix" if prefix else "plain", err, bound))
    assert err <= bound, (err, bound)
