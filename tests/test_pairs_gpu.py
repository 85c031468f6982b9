"""GPU: the training-batch builders of dh3d_amd.pairs (csrc/pairs.hip) against the numpy restatement of their contract
(tests/pairs_reference.py).  Integer outputs and copied rows are compared exactly -- kernel and restatement get the same
float32 inputs and the rules are exact in float64 --; augmented coordinates within one float32 ulp (the two float64 chains
differ by a few double ulps of log / cos, far below half a float32 ulp, so the final roundings differ by one step at most)."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairs_reference as P  # noqa: E402

SEED = 0x5EEDC0FFEE123457  # (above 2^62: the whole 64 bits travel)
AUG_CASES = [("Rotate1D",), ("Jitter",), ("Scale",), ("RotateSmall",), ("Shift",), P.AUG_ORDER]
# (N, sample_nodes, B): N odd / a power of two / the limit; M = 1, N // 2 and 256; one pair and four
NODE_CASES = [(64, 1, 1), (64, 32, 4), (1001, 1, 4), (1001, 500, 1), (1001, 256, 4), (4096, 1, 1), (4096, 2048, 1),
              (4096, 256, 4), (16384, 256, 1)]
TIE_CASES = ["duplicates", "lattice"]


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cloud(rng, n, extent=20.0):
    return (rng.standard_normal((n, 3)) * extent).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ resample
def _resample_case(B, Nsrc, T, ns, seed):
    rng = np.random.default_rng(B * 1000 + Nsrc + T)
    pts = np.full((B, Nsrc, 3), np.nan, dtype=np.float32)
    for b, n in enumerate(ns):
        pts[b, :n] = _cloud(rng, n)
    exp = [P.resample_cloud(pts[b], ns[b], T, seed, b) for b in range(B)]
    return pts, np.stack([e[0] for e in exp]), np.array([e[1] for e in exp], dtype=np.int32)


def _run_resample(dev, pts, ns, T, seed, dirty=0x5A):
    """The C entry point on sentinel-filled outputs and a dirty workspace."""
    from dh3d_amd import _lib as L
    from dh3d_amd import pairs
    B, Nsrc, _ = pts.shape
    x, n, sd = _T(pts, dev), _T(np.asarray(ns, dtype=np.int32), dev), pairs.seed_tensor(seed, dev)
    out = torch.full((B, T, 3), -7.5, dtype=torch.float32, device=dev)
    orig = torch.full((B,), -9, dtype=torch.int32, device=dev)
    nbytes = L.lib().dh3d_resample_clouds_ws_bytes(B, Nsrc, T)
    ws = torch.full((nbytes,), dirty, dtype=torch.uint8, device=dev)
    L.check(L.lib().dh3d_resample_clouds(B, Nsrc, T, L.ptr(x), L.ptr(n), L.ptr(sd), L.ptr(out), L.ptr(orig), L.ptr(ws), nbytes,
                                         L.stream_ptr()), "resample_clouds")
    torch.cuda.synchronize()
    return out.cpu().numpy(), orig.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("B,Nsrc,T,ns", [
    (1, 300, 64, [65]), (5, 300, 64, [0, 1, 63, 64, 65]), (1, 1000, 64, [1000]), (5, 4200, 4096, [4099, 0, 4096, 4095, 4200]),
    (1, 1, 1, [1]), (2, 1500, 3000, [1500, 7]), (1, 300, 1, [300]), (1, 1100, 1025, [1026])])
def test_resample_equals_restatement(dev, B, Nsrc, T, ns):
    from dh3d_amd import pairs
    pts, exp, exp_orig = _resample_case(B, Nsrc, T, ns, SEED)
    got, orig = _run_resample(dev, pts, ns, T, SEED)
    assert np.array_equal(orig, exp_orig)
    assert np.array_equal(got, exp), [int((got[b] != exp[b]).any()) for b in range(B)]
    again, _ = _run_resample(dev, pts, ns, T, SEED, dirty=0xFF)       # run to run, another workspace content
    assert np.array_equal(again, got)
    via_py, orig_py = pairs.resample_clouds(_T(pts, dev), _T(np.asarray(ns, dtype=np.int32), dev), T, seed=SEED)
    assert np.array_equal(via_py.cpu().numpy(), exp) and np.array_equal(orig_py.cpu().numpy(), exp_orig)
    other, _ = _run_resample(dev, pts, ns, T, SEED + 1)
    if any(n > T or 1 < n < T for n in ns):
        assert not np.array_equal(other, got)                            # another seed, another choice
    assert np.array_equal(other, _resample_case(B, Nsrc, T, ns, SEED + 1)[1])


@pytest.mark.gpu
def test_resample_largest_source(dev):
    pts, exp, exp_orig = _resample_case(1, 131072, 8192, [131072], SEED)
    got, orig = _run_resample(dev, pts, [131072], 8192, SEED)
    assert np.array_equal(orig, exp_orig) and np.array_equal(got, exp)


@pytest.mark.gpu
def test_resample_does_not_depend_on_the_batch(dev):
    """Cloud b's rows depend on (seed, b) and its own rows: the same cloud at the same index of another batch."""
    pts, exp, _ = _resample_case(3, 500, 128, [500, 100, 300], SEED)
    other = pts.copy()
    other[0, :400] = other[0, 100:500]
    got, _ = _run_resample(dev, other, [77, 100, 300], 128, SEED)
    assert np.array_equal(got[1:], exp[1:])


# ------------------------------------------------------------------------------------------------------------- augment
def _ulp_ok(got, exp64):
    exp = exp64.astype(np.float32)
    step = np.spacing(np.maximum(np.abs(got), np.abs(exp)))
    return np.abs(got.astype(np.float64) - exp.astype(np.float64)) <= step.astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 1000), (2, 8192)])
@pytest.mark.parametrize("aug", AUG_CASES, ids=lambda a: "+".join(a))
def test_augment_within_one_ulp(dev, aug, shape):
    from dh3d_amd import pairs
    B, N = shape
    pts = _cloud(np.random.default_rng(N), B * N).reshape(B, N, 3)
    out, par = pairs.augment_clouds(_T(pts, dev), aug, seed=SEED)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for b in range(B):
        exp64, epar = P.augment_cloud64(pts[b], aug, SEED, b)
        ok = _ulp_ok(out[b], exp64)
        assert ok.all(), (b, int((~ok).sum()), np.abs(out[b] - exp64).max())
        for key in ("rot1d", "scale", "rot_small", "shift"):
            err = np.abs(par[key][b].cpu().numpy() - epar[key]).max()
            assert err <= 1e-12, (key, b, err)
    if tuple(aug) == ("Jitter",):
        # |jitter| <= clip exactly; the output is the float64 sum rounded once: half a float32 ulp of the result, and the
        # result is within 0.1 of the input, so one float32 ulp of the (larger of the two) coordinates covers it
        diff = np.abs(out.astype(np.float64) - pts.astype(np.float64))
        assert (diff <= 0.1 + np.spacing(np.maximum(np.abs(pts), np.abs(out))).astype(np.float64)).all(), diff.max()
        assert diff.max() > 0.09                                         # and the clip is reached
    again, _ = pairs.augment_clouds(_T(pts, dev), aug, seed=SEED)
    assert torch.equal(again.cpu(), torch.from_numpy(out))
    if tuple(aug) != ():
        assert not torch.equal(pairs.augment_clouds(_T(pts, dev), aug, seed=SEED + 1)[0].cpu(), torch.from_numpy(out))


@pytest.mark.gpu
def test_augment_order_and_parameters(dev):
    from dh3d_amd import pairs
    pts = _cloud(np.random.default_rng(4), 600).reshape(2, 300, 3)
    a, pa = pairs.augment_clouds(_T(pts, dev), ("Shift", "Jitter", "Rotate1D"), seed=SEED, sigma=0.01, clip=0.02, shift_range=0.5)
    b, _ = pairs.augment_clouds(_T(pts, dev), ("Rotate1D", "Jitter", "Shift"), seed=SEED, sigma=0.01, clip=0.02, shift_range=0.5)
    assert torch.equal(a, b)                                             # the order of the names does not matter
    assert torch.equal(pa["rot_small"].cpu(), torch.eye(3, dtype=torch.float64).expand(2, 3, 3)) and torch.equal(pa["scale"].cpu(), torch.ones(2, dtype=torch.float64))
    for c in range(2):
        exp64, _ = P.augment_cloud64(pts[c], ("Rotate1D", "Jitter", "Shift"), SEED, c, sigma=0.01, clip=0.02, shift_range=0.5)
        assert _ulp_ok(a[c].cpu().numpy(), exp64).all()
    none, pn = pairs.augment_clouds(_T(pts, dev), (), seed=SEED)
    assert torch.equal(none.cpu(), torch.from_numpy(pts)) and float(pn["shift"].abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------------------- nodes
@functools.lru_cache(maxsize=None)
def _node_case(N, M, B):
    rng = np.random.default_rng(N * 7 + M + B)
    pc1 = np.stack([_cloud(rng, N) for _ in range(B)])
    pc2 = np.stack([(pc1[b] + rng.standard_normal((N, 3)).astype(np.float32) * np.float32(0.05))[rng.permutation(N)] for b in range(B)])
    return (pc1, pc2) + _node_expect(pc1, pc2, M)


def _node_expect(pc1, pc2, M):
    anc, pos, gap = [], [], np.inf
    for b in range(pc1.shape[0]):
        rep = {}
        a, p = P.sample_pair_nodes(pc1[b], pc2[b], M, SEED, b, report=rep)
        anc.append(a), pos.append(p)
        gap = min(gap, rep["min_gap"])
    return np.stack(anc), np.stack(pos), gap


@functools.lru_cache(maxsize=None)
def _tie_case(kind):
    rng = np.random.default_rng(9)
    if kind == "duplicates":   # a padded resample_clouds output without jitter: 700 points padded to 1024, twice
        src = _cloud(rng, 700)
        pc1 = np.stack([P.resample_cloud(src, 700, 1024, SEED, b)[0] for b in range(2)])
        pc2 = np.stack([P.resample_cloud(src, 700, 1024, SEED, 2 + b)[0] for b in range(2)])
    else:                      # an integer lattice, shuffled: equal distances everywhere
        g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
        pc1 = np.stack([g[rng.permutation(512)] for _ in range(2)])
        pc2 = np.stack([(g + np.float32(0.5 * b))[rng.permutation(512)] for b in range(2)])
    return (pc1, pc2) + _node_expect(pc1, pc2, 64)


def _check_nodes(dev, pc1, pc2, M, anc, pos):
    from dh3d_amd import pairs
    a, p = pairs.sample_pair_nodes(_T(pc1, dev), _T(pc2, dev), M, seed=SEED)
    torch.cuda.synchronize()
    assert a.dtype == torch.int32 and tuple(a.shape) == anc.shape
    assert torch.equal(a.cpu(), torch.from_numpy(anc)), int((a.cpu().numpy() != anc).sum())
    assert torch.equal(p.cpu(), torch.from_numpy(pos)), int((p.cpu().numpy() != pos).sum())
    a2, p2 = pairs.sample_pair_nodes(_T(pc1, dev), _T(pc2, dev), M, seed=SEED)
    assert torch.equal(a2, a) and torch.equal(p2, p)


def test_node_fixtures_have_true_ties_or_clear_gaps():
    """CPU: in every fixture below the best and the second-best d2 among non-identical rows are either equal (a true tie,
    decided by the first-maximum / lowest-j rules) or further apart than any double rounding could move them."""
    for N, M, B in NODE_CASES:
        assert _node_case(N, M, B)[4] > 1e-9, (N, M, B)
    for kind in TIE_CASES:
        assert _tie_case(kind)[4] == 0.0 or _tie_case(kind)[4] > 1e-9, kind
    assert _tie_case("lattice")[4] == 0.0
    dup = _tie_case("duplicates")
    assert len(np.unique(dup[0][0], axis=0)) < 1024 and len(np.unique(dup[1][0], axis=0)) < 1024


@pytest.mark.gpu
@pytest.mark.parametrize("N,M,B", NODE_CASES)
def test_pair_nodes_equal_restatement(dev, N, M, B):
    pc1, pc2, anc, pos, _ = _node_case(N, M, B)
    _check_nodes(dev, pc1, pc2, M, anc, pos)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", TIE_CASES)
def test_pair_nodes_ties(dev, kind):
    pc1, pc2, anc, pos, _ = _tie_case(kind)
    _check_nodes(dev, pc1, pc2, 64, anc, pos)


# ------------------------------------------------------------------------------------------------------------ builders
def _sources(dev, B=3, Nsrc=2600, ns=(2048, 1500, 2000)):
    """Sources of at most numpts = 2048 points: both draws keep every point, so an anchor's source point is in pc2."""
    rng = np.random.default_rng(12)
    src = np.full((B, Nsrc, 3), np.nan, dtype=np.float32)
    for b, n in enumerate(ns):
        src[b, :n] = (rng.random((n, 3), dtype=np.float32) * np.float32(30.0))
    return src, np.asarray(ns, dtype=np.int32)


@pytest.mark.gpu
def test_make_local_pairs_is_its_stages(dev):
    from dh3d_amd import pairs
    src, ns = _sources(dev)
    B, numpts, M = 3, 2048, 64
    x, n = _T(src, dev), _T(ns, dev)
    out = pairs.make_local_pairs(x, n, numpts=numpts, sample_nodes=M, seed=SEED)
    torch.cuda.synchronize()
    assert tuple(out["points"].shape) == (2 * B, numpts, 3) and tuple(out["R"].shape) == (B, 3, 3)
    assert tuple(out["sample_idx"].shape) == (2 * B, M) and out["sample_idx"].dtype == torch.int32
    # the stage functions by hand, each on the device's own intermediates
    drawn, orig = pairs.resample_clouds(torch.cat([x, x]), torch.cat([n, n]), numpts, seed=SEED)
    assert torch.equal(orig.cpu(), torch.from_numpy(np.concatenate([ns, ns])))
    both, _ = pairs.augment_clouds(drawn, ("Jitter",), seed=SEED)
    assert torch.equal(out["points"][:B], both[:B]) and torch.equal(out["pc2"], both[B:])
    trans, R = pairs.rotate_pairs(both[B:].contiguous(), math.pi, seed=SEED)
    assert torch.equal(out["points"][B:], trans) and torch.equal(out["R"], R)
    anc, pos = pairs.sample_pair_nodes(both[:B].contiguous(), both[B:].contiguous(), M, seed=SEED)
    assert torch.equal(out["sample_idx"], torch.cat([anc, pos]))
    # and the restatement of each stage on those intermediates
    drawn_np, both_np = drawn.cpu().numpy(), both.cpu().numpy()
    for b in range(2 * B):
        assert np.array_equal(drawn_np[b], P.resample_cloud(src[b % B], ns[b % B], numpts, SEED, b)[0])
        assert _ulp_ok(both_np[b], P.augment_cloud64(drawn_np[b], ("Jitter",), SEED, b)[0]).all()
    for b in range(B):
        Rot = P.pair_rotation(SEED, b)
        assert np.abs(R[b].cpu().numpy().astype(np.float64) - Rot).max() <= 2.0 ** -24
        assert _ulp_ok(trans[b].cpu().numpy(), P.rows_mat3(both_np[B + b].astype(np.float64), Rot)).all()
        a_np, p_np = P.sample_pair_nodes(both_np[b], both_np[B + b], M, SEED, b)
        assert np.array_equal(anc[b].cpu().numpy(), a_np) and np.array_equal(pos[b].cpu().numpy(), p_np)
    # pc1 and pc2 are two jittered draws of one cloud: an anchor's own source point, jittered again, is in pc2, at most
    # 2 * clip per axis away, and the nearest point of pc2 is no further; the rotation keeps distances up to float32
    # rounding of coordinates <= ~45 (a few 1e-6) -- 1e-4 covers it
    pts64 = out["points"].cpu().numpy().astype(np.float64)
    idx = out["sample_idx"].cpu().numpy()
    for b in range(B):
        a = pts64[b][idx[b]] @ out["R"][b].cpu().numpy().astype(np.float64)
        d = np.linalg.norm(a - pts64[B + b][idx[B + b]], axis=1)
        assert d.max() <= 2 * 0.1 * math.sqrt(3) + 1e-4, (b, d.max())


@pytest.mark.gpu
def test_make_local_pairs_replays_fresh_batches(dev):
    """A seed tensor bumped between two replays of a captured graph gives two different batches, each the eager call's."""
    from dh3d_amd import pairs
    src, ns = _sources(dev)
    x, n = _T(src, dev), _T(ns, dev)
    sd = torch.tensor([11], dtype=torch.int64, device=dev)
    kw = dict(numpts=2048, sample_nodes=64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pairs.make_local_pairs(x, n, seed=sd, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pairs.make_local_pairs(x, n, seed=sd, **kw)
    seen = []
    for s in (101, 102):
        sd.fill_(s)
        graph.replay()
        torch.cuda.synchronize()
        seen.append({k: v.clone() for k, v in out.items()})
        eager = pairs.make_local_pairs(x, n, seed=s, **kw)
        for k in eager:
            assert torch.equal(seen[-1][k], eager[k]), (s, k)
    assert not torch.equal(seen[0]["points"], seen[1]["points"]) and not torch.equal(seen[0]["sample_idx"], seen[1]["sample_idx"])
    assert not torch.equal(seen[0]["R"], seen[1]["R"])


@pytest.mark.gpu
def test_make_local_pairs_feeds_the_local_trainer(dev):
    from dh3d_amd import ConfigFactory, pairs
    from dh3d_amd.model import DH3D
    from dh3d_amd.training import LocalTrainer
    cfg = ConfigFactory("detection_config").getconfig()
    cfg.num_points, cfg.batch_size, cfg.sampled_kpnum = 2048, 3, 64
    model = DH3D(cfg).init_synthetic(5).to(dev).eval().prepare()
    src, ns = _sources(dev)
    batch = pairs.make_local_pairs(_T(src, dev), _T(ns, dev), numpts=2048, sample_nodes=64, seed=SEED)
    loss = LocalTrainer(model, graph_step=False).step(batch["points"], batch["R"], batch["sample_idx"])
    assert math.isfinite(loss), loss


@pytest.mark.gpu
def test_make_global_batch_is_its_stages(dev):
    from dh3d_amd import pairs
    rng = np.random.default_rng(21)
    ns = np.array([3000, 2500, 2048, 1000, 2049], dtype=np.int32)
    src = np.full((5, 3000, 3), np.nan, dtype=np.float32)
    for b, k in enumerate(ns):
        src[b, :k] = _cloud(rng, k)
    x, n = _T(src, dev), _T(ns, dev)
    out = pairs.make_global_batch(x, n, 2048, seed=SEED)
    aug = ("Jitter", "RotateSmall", "Shift", "Rotate1D")
    drawn, orig = pairs.resample_clouds(x, n, 2048, seed=SEED)
    assert torch.equal(out, pairs.augment_clouds(drawn, aug, seed=SEED)[0])
    assert torch.equal(orig.cpu(), torch.from_numpy(np.minimum(ns, 2048)))
    drawn_np, out_np = drawn.cpu().numpy(), out.cpu().numpy()
    for b in range(5):
        assert np.array_equal(drawn_np[b], P.resample_cloud(src[b], ns[b], 2048, SEED, b)[0])
        assert _ulp_ok(out_np[b], P.augment_cloud64(drawn_np[b], aug, SEED, b)[0]).all()
