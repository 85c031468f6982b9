"""GPU: select_top_k, knn_point and gather_point against the float32 restatement (tests/knn_point_reference.py) -- torch.equal
on ids AND values, no tolerance and no row left out, because the restatement defines the ties too: whole rows of
select_top_k over the row lengths, k and value patterns its kernels branch on; knn_point over sizes, cloud kinds and both
kernels (the plan's every answer is hit); the op against select_top_k on the matrix of the same rounding; as the producer of
group_point's idx; gather_point forward and backward with repeated indices; across batchings and runs; under graph capture;
and on sentinel-filled outputs."""
import os
import zlib

import numpy as np
import pytest
import torch

import knn_point_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _equal(name, got, exp):
    got, exp = got.cpu(), torch.from_numpy(np.ascontiguousarray(exp))
    assert got.dtype == exp.dtype and got.shape == exp.shape, (name, got.dtype, got.shape, exp.dtype, exp.shape)
    if not torch.equal(got, exp):
        bad = (got != exp).reshape(-1, got.shape[-1]).any(-1).nonzero()
        r = int(bad[0])
        raise AssertionError("%s: %d rows differ, first %d:\n%s\nvs\n%s" % (
            name, len(bad), r, got.reshape(-1, got.shape[-1])[r].tolist()[:80], exp.reshape(-1, exp.shape[-1])[r].tolist()[:80]))


# ------------------------------------------------------------------------------------------------ select_top_k
SEL_NS = (1, 2, 63, 64, 65, 1000, 4096)
PATTERNS = ("random", "few_values", "all_equal", "descending", "ascending")


def _rows(pattern, b, m, n, rng):
    if pattern == "random":
        return rng.standard_normal((b, m, n)).astype(np.float32)
    if pattern == "few_values":          # 1-7 distinct numbers a row, signs and both zeros among them
        pool = np.array([-1.5, -0.0, 0.0, 0.25, 3.0, 7.5, 1e-30], np.float32)
        out = np.empty((b, m, n), np.float32)
        for r in range(b * m):
            out.reshape(-1, n)[r] = rng.choice(pool[rng.permutation(7)[:1 + r % 7]], n)
        return out
    if pattern == "all_equal":
        return np.full((b, m, n), 2.5, np.float32)
    ramp = np.broadcast_to(np.arange(n, dtype=np.float32), (b, m, n))
    return np.ascontiguousarray(-ramp if pattern == "descending" else ramp)


def _sel_cases():
    cases = []
    for n in SEL_NS:
        for k in sorted({k for k in (1, 2, 8, 64, n) if k <= n}):
            cases.append((n, k))
    return cases


@pytest.mark.parametrize("n,k", _sel_cases(), ids=lambda v: str(v))
def test_select_top_k_whole_rows(dev, n, k):
    from dh3d_amd import ops
    b, m = 2, 3
    for pattern in PATTERNS:
        dist = _rows(pattern, b, m, n, _rng("sel", n, k, pattern))
        exp_idx, exp_out = R.select_top_k(k, dist)
        d = _t(dist, dev)
        idx, out = ops.select_top_k(k, d)
        assert idx.data_ptr() != d.data_ptr() and out.data_ptr() != d.data_ptr()     # freshly allocated
        _equal("select_top_k %s n=%d k=%d idx" % (pattern, n, k), idx, exp_idx)
        # values bit for bit (-0 stays -0): compare the patterns
        _equal("select_top_k %s n=%d k=%d out" % (pattern, n, k), out.view(torch.int32), exp_out.view(np.int32))
        _equal("input untouched", d, dist)


def test_select_top_k_many_rows_tie_heavy(dev):
    from dh3d_amd import ops
    rng = _rng("sel-many")
    dist = rng.integers(0, 5, (4, 500, 300)).astype(np.float32)
    for k in (5, 64, 200, 300):
        exp_idx, exp_out = R.select_top_k(k, dist)
        idx, out = ops.select_top_k(k, _t(dist, dev))
        _equal("many rows k=%d idx" % k, idx, exp_idx)
        _equal("many rows k=%d out" % k, out, exp_out)


def test_select_top_k_refuses_bad_k(dev):
    from dh3d_amd import ops
    d = torch.zeros(2, 3, 10, device=dev)
    for k in (0, -1, 11):
        with pytest.raises(ValueError, match="SelectionSort expects 1 <= k <= n"):
            ops.select_top_k(k, d)


# ------------------------------------------------------------------------------------------------ knn_point
NS = (1, 63, 64, 65, 1000, 4096, 8192, 16384)
KS = (1, 3, 8, 32, 64, 128)
KINDS = ("uniform", "lattice", "duplicates", "slab", "outside")


def _cloud(kind, b, n, m, rng, c=3):
    if kind == "lattice":       # integers scaled by 2^-3: exact arithmetic, ties everywhere
        x1 = (rng.integers(0, 12, (b, n, c)).astype(np.float32) * np.float32(0.125))
    elif kind == "slab":
        x1 = rng.random((b, n, c), dtype=np.float32)
        x1[..., -1] *= np.float32(1e-3)
    else:
        x1 = rng.random((b, n, c), dtype=np.float32)
    if kind == "duplicates" and n > 1:
        x1[:, n // 2:] = x1[:, : n - n // 2]
    if m == n:
        x2 = x1.copy()
    else:
        x2 = np.take_along_axis(x1, rng.integers(0, n, (b, m))[..., None], 1).copy()
        if kind != "lattice":
            x2[:, m // 2:] += rng.normal(0, 0.05, (b, m - m // 2, c)).astype(np.float32)
    if kind == "outside":       # queries beyond the dataset's bounding box
        x2 = (x2 + np.float32(3.0)).astype(np.float32)
    return np.ascontiguousarray(x1, np.float32), np.ascontiguousarray(x2, np.float32)


def _knn_cases():
    cases, i = [], 0
    for n in NS:
        for m in sorted({1, 64, 1000, n}):
            ks = [k for k in KS if k <= n]
            cases.append((KINDS[i % len(KINDS)], 1 if n * m > 1 << 24 else 2, n, m, 3, ks[i % len(ks)]))
            i += 1
    for j, k in enumerate(KS):                       # every k and every kind on the sizes the benchmark runs
        cases.append((KINDS[j % len(KINDS)], 2, (8192, 4096)[j % 2], (1000, 64)[j % 2], 3, k))
    for j, kind in enumerate(KINDS):
        cases.append((kind, 2, 1000, 1000, 3, KS[(j + 2) % len(KS)]))
    for j, c in enumerate((1, 2, 4, 16, 64)):        # the generic kernel
        cases.append((KINDS[j % len(KINDS)], 2, 1000, 64, c, (8, 64, 3, 128, 32)[j]))
        cases.append(("uniform", 1, 65, 65, c, 65))
    return cases


KNN_CASES = _knn_cases()


def test_knn_cases_cover_what_they_claim():
    from dh3d_amd import pm
    assert {c[2] for c in KNN_CASES} == set(NS) and {c[5] for c in KNN_CASES} >= set(KS)
    for n in NS:
        assert {c[3] for c in KNN_CASES if c[2] == n} >= {1, 64, 1000, n}
    assert {c[0] for c in KNN_CASES} == set(KINDS)
    assert {c[4] for c in KNN_CASES} == {1, 2, 3, 4, 16, 64}
    plans = {pm.knn_point_plan(c[2], c[3], c[4], c[5]) for c in KNN_CASES}
    assert plans == {0, 1}, plans                      # every kernel the plan can name is run
    assert pm.knn_point_plan(100, 10, 3, 0) == -1 and pm.knn_point_plan(5000, 10, 3, 2000) == -1


@pytest.mark.parametrize("case", KNN_CASES, ids=lambda c: "%s-b%d-n%d-m%d-c%d-k%d" % c)
def test_knn_point_equals_restatement(dev, case):
    from dh3d_amd import ops
    kind, b, n, m, c, k = case
    x1, x2 = _cloud(kind, b, n, m, _rng(case), c)
    exp_val, exp_idx = R.knn_point(k, x1, x2)
    val, idx = ops.knn_point(k, _t(x1, dev), _t(x2, dev))
    _equal("%s idx" % (case,), idx, exp_idx)
    _equal("%s val" % (case,), val, exp_val)


@pytest.mark.parametrize("name,k", [("global_c", 32), ("local_268", 64), ("dso_9000", 8), ("global_a", 128)])
def test_knn_point_on_demo_clouds_in_metres(dev, name, k):
    from dh3d_amd import ops
    x1 = np.ascontiguousarray(np.load(os.path.join(GOLDEN, "demo_clouds.npz"))[name][None], np.float32)
    x2 = np.ascontiguousarray(x1[:, ::8])
    exp_val, exp_idx = R.knn_point(k, x1, x2)
    val, idx = ops.knn_point(k, _t(x1, dev), _t(x2, dev))
    _equal("%s idx" % name, idx, exp_idx)
    _equal("%s val" % name, val, exp_val)
    assert float(val[:, :, 0].max()) == 0.0           # every query is a cloud point


@pytest.mark.parametrize("n,m,c,k", [(1000, 200, 3, 8), (1000, 200, 3, 64), (300, 50, 3, 128), (500, 100, 5, 16),
                                     (64, 64, 3, 64), (100, 30, 3, 100)])
def test_op_is_the_first_k_columns_of_select_top_k(dev, n, m, c, k):
    """The same rows by two kernels: knn_point (fused for c = 3, k <= 64, else the generic one) and select_top_k on the
    matrix of the same rounding."""
    from dh3d_amd import ops
    x1, x2 = _cloud("lattice" if k % 16 else "uniform", 2, n, m, _rng("cols", n, m, c, k), c)
    d = _t(R.sqdist(x1, x2), dev)
    val, idx = ops.knn_point(k, _t(x1, dev), _t(x2, dev))
    sidx, sout = ops.select_top_k(k, d)
    assert torch.equal(idx, sidx[..., :k]) and torch.equal(val, sout[..., :k])


def test_group_point_consumes_the_rows(dev):
    from dh3d_amd import ops
    rng = _rng("group")
    x1, x2 = _cloud("uniform", 2, 2048, 256, rng)
    points = np.ascontiguousarray(np.concatenate([x1, rng.standard_normal((2, 2048, 5)).astype(np.float32)], -1))
    _, idx = ops.knn_point(16, _t(x1, dev), _t(x2, dev))
    out = ops.group_point(_t(points, dev), idx)
    _, ref_idx = R.knn_point(16, x1, x2)
    expect = np.stack([points[bi][ref_idx[bi]] for bi in range(2)])      # out[b, j, l] = points[b, idx[b, j, l]]
    assert torch.equal(out.cpu(), torch.from_numpy(expect))


def test_gather_point_forward_and_backward(dev):
    from dh3d_amd import ops
    from test_ops_gpu import close
    rng = _rng("gather")
    b, n, m = 3, 500, 1200
    inp = rng.standard_normal((b, n, 3)).astype(np.float32)
    idx = rng.integers(0, n, (b, m)).astype(np.int32)
    idx[:, :400] = idx[:, 400:800]                   # repeated indices
    idx[0, :100] = 7
    go = rng.standard_normal((b, m, 3)).astype(np.float32)
    p = _t(inp, dev).requires_grad_()
    out = ops.gather_point(p, _t(idx, dev))
    assert out.shape == (b, m, 3)
    assert torch.equal(out.detach().cpu(), torch.from_numpy(R.gather_point(inp, idx)))
    out.backward(_t(go, dev))
    exp = R.gather_point_grad(inp.shape, idx, go)
    # the tolerance of group_point's gradient in tests/test_ops_gpu.py
    assert close(p.grad.cpu().numpy(), exp.astype(np.float32), 1e-5, 1e-5)
    picks = ops.farthest_point_sample(64, _t(inp, dev))      # the reference's pairing: gather_point(xyz, fps(...))
    assert torch.equal(ops.gather_point(_t(inp, dev), picks).cpu(),
                       torch.from_numpy(R.gather_point(inp, picks.cpu().numpy())))


def test_same_rows_alone_in_a_batch_and_again(dev):
    from dh3d_amd import ops
    for c, k in ((3, 32), (3, 128), (4, 16)):
        x1, x2 = _cloud("duplicates", 8, 3000, 500, _rng("batch", c, k), c)
        t1, t2 = _t(x1, dev), _t(x2, dev)
        whole = ops.knn_point(k, t1, t2)
        again = ops.knn_point(k, t1, t2)
        assert torch.equal(whole[0], again[0]) and torch.equal(whole[1], again[1])
        for i in (0, 3, 7):
            one = ops.knn_point(k, t1[i:i + 1].contiguous(), t2[i:i + 1].contiguous())
            assert torch.equal(one[0][0], whole[0][i]) and torch.equal(one[1][0], whole[1][i]), (c, k, i)
        exp_val, exp_idx = R.knn_point(k, x1[:1], x2[:1])
        _equal("batch idx", whole[1][:1], exp_idx)
        _equal("batch val", whole[0][:1], exp_val)


@pytest.mark.parametrize("c,k", [(3, 16), (3, 100), (6, 8)])
def test_graph_capture_and_replay_equal_eager(dev, c, k):
    from dh3d_amd import ops
    b, n, m = 2, 4096, 512
    xa1, xa2 = _cloud("uniform", b, n, m, _rng("graph-a", c, k), c)
    xb1, xb2 = _cloud("lattice", b, n, m, _rng("graph-b", c, k), c)
    s1, s2 = _t(xa1, dev), _t(xa2, dev)

    def run():
        val, idx = ops.knn_point(k, s1, s2)
        sidx, sout = ops.select_top_k(k, val)          # (any [b,m,k] matrix: the second entry point in the same graph)
        return val, idx, sidx, sout

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run()
    for x1, x2 in ((xb1, xb2), (xa1, xa2), (xb1, xb2)):  # three replays
        s1.copy_(_t(x1, dev)); s2.copy_(_t(x2, dev))
        for o in outs:
            o.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        eager = run()
        for o, e in zip(outs, eager):
            assert torch.equal(o, e)
        exp_val, exp_idx = R.knn_point(k, x1, x2)
        _equal("graph idx", outs[1], exp_idx)
        _equal("graph val", outs[0], exp_val)


def test_sentinel_filled_outputs_are_fully_overwritten(dev):
    """The C entry points on outputs pre-filled with a sentinel: every element is written (both knn kernels, both
    select_top_k kernels)."""
    from dh3d_amd import _lib as L
    lib = L.lib()
    for n, m, c, k in ((1000, 37, 3, 8), (1000, 37, 3, 64), (1000, 37, 3, 100), (200, 5, 7, 200), (65, 70, 3, 1)):
        x1, x2 = _cloud("uniform", 2, n, m, _rng("sentinel", n, m, c, k), c)
        t1, t2 = _t(x1, dev), _t(x2, dev)
        val = torch.full((2, m, k), -7.0, device=dev)
        idx = torch.full((2, m, k), -7, dtype=torch.int32, device=dev)
        L.check(lib.dh3d_knn_point(2, n, m, c, k, L.ptr(t1), L.ptr(t2), L.ptr(val), L.ptr(idx), L.stream_ptr()), "knn_point")
        exp_val, exp_idx = R.knn_point(k, x1, x2)
        _equal("sentinel idx", idx, exp_idx)
        _equal("sentinel val", val, exp_val)
    for n, k in ((300, 7), (300, 300), (2000, 1500)):
        dist = _rng("sentinel-sel", n, k).integers(0, 9, (2, 3, n)).astype(np.float32)
        d = _t(dist, dev)
        out = torch.full((2, 3, n), -7.0, device=dev)
        outi = torch.full((2, 3, n), -7, dtype=torch.int32, device=dev)
        L.check(lib.dh3d_select_top_k(2, n, 3, k, L.ptr(d), L.ptr(outi), L.ptr(out), L.stream_ptr()), "select_top_k")
        exp_idx, exp_out = R.select_top_k(k, dist)
        _equal("sentinel select idx", outi, exp_idx)
        _equal("sentinel select out", out, exp_out)
