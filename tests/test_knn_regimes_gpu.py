"""GPU parity of the brute-force kNN (ops.knn_bruteforce / pm.knn_xyz: csrc/knn.hip knn_launch, the any-Dp kernel) and of
the pruned scan (pm.knn_sorted: knn_sorted_launch) in every launch regime -- the tables of tests/knn_regime_cases.py, whose
coverage tests/test_knn_plan.py pins without a GPU.

Every case asserts the launch plan it was written for (pm.knn_sorted_plan / pm.knn_plan, the launchers' own functions)
before it compares anything, and runs into outputs pre-filled with the grid regime test's sentinels, none of which may
survive.  Then, bit for bit: the pruned scan == pm.knn_xyz on the whole batch; the [B, 3, N] and the [B, N, 3] layout of
the brute force == each other; and on the sampled clouds (knn_regime_cases.sampled_clouds, N <= 4096) ids and distance
bits == oracle.knn_bruteforce.

Against plain float64 (`_check_float64`), which shares nothing with the oracle's rounding model: with d* the sorted K
smallest float64 distances of a query and d the float64 distances of the ids returned for it,
    ids distinct and in [0, N) (rank >= N: id -1, distance FLT_MAX), returned f32 distances non-decreasing,
    |d_i - d*_i| <= 8 * 2^-24 * d*_i   and   |returned_i - d_i| <= 8 * 2^-24 * d*_i   at every rank i.
The bound is derived, not measured.  With u = 2^-24: the f32 inputs are exact in float64; each coordinate difference
carries one f32 rounding (1 + u), its square (1 + u)^2; the product and the two fma of sqrt(fma(dz, dz, fma(dy, dy,
dx * dx))) add at most three more roundings to a term, and all terms are positive, so the sum is within 5 u relative;
the square root halves that and, correctly rounded, adds one u: 3.5 u on a returned distance.  The kernel ranks by those
distances, so its i-th smallest is within 3.5 u of d*_i (order statistics move no more than the values), and the true
distance of the id at rank i within another 3.5 u of that: 7 u (1 + 3.5 u) < 8 u.  Purely relative -- a distance of 0 is
computed exactly -- which needs that no squared difference underflows: every cloud is checked for it (`_no_underflow`)."""
import numpy as np
import pytest
import torch

import knn_regime_cases as C
from test_knn_grid_regimes_gpu import DIST_SENTINEL, NN_SENTINEL

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)
REL = 8.0 * 2.0 ** -24


def _prefilled(B, N, K, dev):
    nn = torch.full((B, N, K), NN_SENTINEL, dtype=torch.int32, device=dev)
    dist = torch.full((B, N, K), DIST_SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    return nn, dist


def _assert_written(got, out, what):
    nn, dist = out
    assert got[0] is nn and got[1] is dist
    assert not bool((nn == NN_SENTINEL).any()), what + " left ids unwritten"
    assert not bool((dist.view(torch.int32) == DIST_SENTINEL).any()), what + " left distances unwritten"
    return nn, dist


def _assert_same(a, b, what, kinds):
    """(ids, distances) a == b bit for bit, naming the clouds that differ"""
    bad = ((a[0] != b[0]) | (a[1].view(torch.int32) != b[1].view(torch.int32))).flatten(1).any(1).nonzero().flatten().tolist()
    assert not bad, (what, "clouds that differ", bad[:8], [kinds[b_] for b_ in bad[:8]])


def _no_underflow(p64):
    """no nonzero coordinate difference of the cloud is so small that its f32 square is subnormal (< 2^-126)"""
    for a in range(p64.shape[1]):
        gaps = torch.diff(torch.sort(p64[:, a]).values)
        gaps = gaps[gaps > 0]
        assert gaps.numel() == 0 or float(gaps.min()) >= 2.0 ** -60


def _check_float64(p, nn, dist, where):
    """p [N, Dp] float32 on the device, nn / dist [N, K] the kernel's rows for it: the module docstring's properties"""
    N, K = p.shape[0], nn.shape[1]
    k = min(K, N)
    p64 = p.double()
    _no_underflow(p64)
    dstar = []
    for i in range(0, N, 1024):
        d_all = (p64[i:i + 1024, None, :] - p64[None, :, :]).pow(2).sum(-1).sqrt()
        dstar.append(torch.topk(d_all, k, dim=1, largest=False, sorted=True).values)
    dstar = torch.cat(dstar)
    ids = nn[:, :k].long()
    assert bool(((ids >= 0) & (ids < N)).all()), where
    srt = ids.sort(1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), (where, "an id twice in a row")
    if K > N:
        assert bool((nn[:, N:] == -1).all()) and bool((dist[:, N:] == FLT_MAX).all()), (where, "padding")
    assert bool((dist[:, 1:] >= dist[:, :-1]).all()), (where, "distances decrease")
    d = (p64[:, None, :] - p64[ids]).pow(2).sum(-1).sqrt()
    bound = REL * dstar
    worst = float(((d - dstar).abs() - bound).max())
    assert worst <= 0, (where, "true distance of a returned id beyond the bound by", worst)
    worst = float(((dist[:, :k].double() - d).abs() - bound).max())
    assert worst <= 0, (where, "returned distance beyond the bound by", worst)


def _check_references(oracle, c, pos, nn, dist, case):
    """pos [B, N, Dp] on the device; the sampled clouds against the CPU oracle (bits) and against float64 (bounds)"""
    if c.N > 4096:
        return
    for b in C.sampled_clouds(c):
        where = (case, b, c.kinds[b])
        nn_o, d_o = oracle.knn_bruteforce(np.ascontiguousarray(pos[b:b + 1].cpu().numpy().transpose(0, 2, 1)), c.K)
        assert np.array_equal(nn[b].cpu().numpy(), nn_o[0]), where
        assert np.array_equal(dist[b].cpu().numpy().view(np.uint32), d_o[0].view(np.uint32)), where
        _check_float64(pos[b], nn[b], dist[b], where)


@pytest.mark.parametrize("case", list(C.SORTED_CASES))
def test_knn_sorted_regime(dev, oracle, case):
    """pm.knn_sorted in the regime the case names: no sentinel left, ids and distance bits == pm.knn_xyz on every cloud,
    == the oracle on the sampled ones, and within the float64 bounds there."""
    from dh3d_amd import pm
    c = C.SORTED_CASES[case]
    B = len(c.kinds)
    assert pm.knn_sorted_plan(B, c.N, c.K) == c.plan
    t = torch.from_numpy(np.array(C.batch(c))).to(dev)    # (a copy: the shared array is read-only)
    srt, gbox = pm.spatial_sort(t)
    out = _prefilled(B, c.N, c.K, dev)
    got = _assert_written(pm.knn_sorted(srt, gbox, c.K, out=out), out, "knn_sorted")
    out_b = _prefilled(B, c.N, c.K, dev)
    ref = _assert_written(pm.knn_xyz(t, c.K, out=out_b), out_b, "knn_xyz")
    _assert_same(got, ref, (case, "knn_sorted != knn_xyz"), c.kinds)
    _check_references(oracle, c, t, got[0], got[1], case)


@pytest.mark.parametrize("case", list(C.BRUTE_CASES))
def test_knn_bruteforce_regime(dev, oracle, case):
    """dh3d_knn_bruteforce ([B, Dp, N]) and pm.knn_xyz ([B, N, 3]) in the regime the case names: no sentinel left, the two
    layouts equal bit for bit (Dp = 3), == the oracle on the sampled clouds and within the float64 bounds there."""
    from dh3d_amd import _lib as L
    from dh3d_amd import ops, pm
    c = C.BRUTE_CASES[case]
    B = len(c.kinds)
    assert pm.knn_plan(B, c.N, c.K, c.Dp) == c.plan
    t = torch.from_numpy(np.array(C.batch(c)[:, :, :c.Dp])).to(dev)                  # [B, N, Dp] (a copy)
    pos = t.transpose(1, 2).contiguous()                                             # [B, Dp, N]
    out = _prefilled(B, c.N, c.K, dev)
    with torch.cuda.device(dev):
        L.check(L.lib().dh3d_knn_bruteforce(L.ptr(pos), B, c.Dp, c.N, c.K, L.ptr(out[0]), L.ptr(out[1]), L.stream_ptr()),
                "knn_bruteforce")
    got = _assert_written(out, out, "knn_bruteforce")
    _assert_same(ops.knn_bruteforce(pos, c.K), got, (case, "ops.knn_bruteforce != the entry it wraps"), c.kinds)
    if c.Dp == 3:
        out_x = _prefilled(B, c.N, c.K, dev)
        got_x = _assert_written(pm.knn_xyz(t, c.K, out=out_x), out_x, "knn_xyz")
        _assert_same(got_x, got, (case, "[B, N, 3] != [B, 3, N]"), c.kinds)
    _check_references(oracle, c, t, got[0], got[1], case)


def test_knn_out_is_validated(dev):
    """pm.knn_sorted / pm.knn_xyz refuse an `out` of the wrong shape, type, layout or device, as pm.knn_grid does"""
    from dh3d_amd import pm
    t = torch.from_numpy(np.array(C.batch(C.SORTED_CASES["pad_4x5_k8"]))).to(dev)
    srt, gbox = pm.spatial_sort(t)
    nn, dist = _prefilled(4, 5, 8, dev)
    bad = [(nn[:, :, :4], dist), (nn, dist.double()), (nn.long(), dist), (nn, dist.cpu()),
           (nn, _prefilled(4, 8, 5, dev)[1].transpose(1, 2)), (_prefilled(3, 5, 8, dev)[0], dist)]
    for out in bad:
        with pytest.raises(ValueError):
            pm.knn_sorted(srt, gbox, 8, out=out)
        with pytest.raises(ValueError):
            pm.knn_xyz(t, 8, out=out)
    assert bool((nn == NN_SENTINEL).all())   # nothing ran
