"""CPU: the numpy restatement of the training-batch builders (tests/pairs_reference.py) against the reference's own
formulas (core/augment.py, imported from the reference tree where it is present), against direct transcriptions of the
selection and node rules, and the distribution of its random streams."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairs_reference as P  # noqa: E402

REF_AUGMENT = os.path.join(os.environ.get("DH3D_REFERENCE", "/root/reference"), "core", "augment.py")
SEED = 20240607


def _augment_module():
    if not os.path.isfile(REF_AUGMENT):
        pytest.skip("the reference tree is not here")
    spec = importlib.util.spec_from_file_location("ref_augment", REF_AUGMENT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Streams:
    """np.random.randn / uniform that hand out the restatement's values for cloud b: the class being applied decides the
    stream (set by the test through `current`)."""

    def __init__(self, seed, b):
        self.seed, self.b, self.current = seed, b, None

    def randn(self, *shape):
        stream = {"Jitter": P.JITTER, "RotateSmall": P.ROTATESMALL}[self.current]
        n = int(np.prod(shape))
        return P.normal(self.seed, stream, self.b, np.arange(n)).reshape(shape)

    def uniform(self, low=0.0, high=1.0, size=None):
        stream = {"RotateZ": P.ROTATE1D, "Scale": P.SCALE, "Shift": P.SHIFT}[self.current]
        U = P.unit_co(P.u(self.seed, stream, self.b, np.arange(size or 1)))
        v = low + (high - low) * U   # numpy's own formula for uniform(low, high)
        return v if size else float(v[0])


def _apply_reference(mod, names, data64, streams, monkeypatch):
    monkeypatch.setattr(mod.np.random, "randn", streams.randn)
    monkeypatch.setattr(mod.np.random, "uniform", streams.uniform)
    v = data64.copy()
    for a in mod.get_augmentations_from_list(list(names), upright_axis=2):
        streams.current = type(a).__name__
        v = a.apply(v)
    return v


@pytest.mark.parametrize("names", [("Rotate1D",), ("Jitter",), ("Scale",), ("RotateSmall",), ("Shift",),
                                   ("Shift", "Rotate1D", "RotateSmall", "Jitter", "Scale")])
def test_restatement_equals_the_reference_classes(names, monkeypatch):
    mod = _augment_module()
    rng = np.random.default_rng(5)
    pts = (rng.standard_normal((500, 3)) * 20).astype(np.float32)
    for b in (0, 3):
        exp = _apply_reference(mod, names, pts.astype(np.float64), _Streams(SEED, b), monkeypatch)
        got, _ = P.augment_cloud64(pts, names, SEED, b)
        # float64 rounding: np.dot may sum a row's three products in another order or fused (a few ulps of the largest
        # term, |coordinate| <= ~100 -> 100 * 2^-52 * a few); everything else is the same operation on the same values
        assert np.abs(got - exp).max() <= 8 * 100 * 2.0 ** -52, (names, b, np.abs(got - exp).max())


def test_choice_is_the_m_smallest_keys_in_index_order():
    for n, m, b in ((1, 1, 0), (10, 3, 1), (1000, 64, 2), (4099, 4096, 3), (777, 777, 4)):
        keys = P.u(SEED, P.RESAMPLE, b, np.arange(n))
        order = np.lexsort((np.arange(n), keys))          # by key, then index
        assert len(np.unique(keys)) == n                   # splitmix64 is a bijection
        assert np.array_equal(P.choice(SEED, P.RESAMPLE, b, n, m), np.sort(order[:m]))


def test_resample_rules():
    rng = np.random.default_rng(1)
    pts = rng.standard_normal((50, 3)).astype(np.float32)
    pts[30:] = np.nan
    out, k = P.resample_cloud(pts, 30, 8, SEED, 2)
    assert k == 8 and np.array_equal(out, pts[P.choice(SEED, P.RESAMPLE, 2, 30, 8)])
    out, k = P.resample_cloud(pts, 30, 64, SEED, 2)
    draws = [int(P.u(SEED, P.PAD, 2, j)) % 30 for j in range(34)]
    assert k == 30 and np.array_equal(out[:30], pts[:30]) and np.array_equal(out[30:], pts[draws])
    out, k = P.resample_cloud(pts, 0, 5, SEED, 0)
    assert k == 0 and np.all(out == np.float32(100000.0))
    out, k = P.resample_cloud(pts, 30, 30, SEED, 1)
    assert k == 30 and np.array_equal(out, pts[:30])


def _farthest_sampler_sample(pts, k, first):
    """core/utils.py FarthestSampler.sample, transcribed, with the first pick injected; float64 on the float32 points."""
    def calc_distances(p0, points):
        return ((p0 - points) ** 2).sum(axis=1)
    pts = pts.astype(np.float64)
    farthest_pts_ind = [first]
    distances = calc_distances(pts[first], pts)
    for i in range(1, k):
        farthest_pts_ind.append(np.argmax(distances))
        distances = np.minimum(distances, calc_distances(pts[farthest_pts_ind[i]], pts))
    return np.asarray(farthest_pts_ind)


@pytest.mark.parametrize("N,M", [(64, 32), (1001, 100), (600, 1)])
def test_node_rules_against_direct_code(N, M):
    rng = np.random.default_rng(N)
    pc1 = (rng.standard_normal((N, 3)) * 10).astype(np.float32)
    pc2 = (pc1 + rng.standard_normal((N, 3)).astype(np.float32) * np.float32(0.05))[rng.permutation(N)]
    rep = {}
    anc, pos = P.sample_pair_nodes(pc1, pc2, M, SEED, 1, report=rep)
    keys = P.u(SEED, P.SUBSET, 1, np.arange(N))
    subset = np.sort(np.lexsort((np.arange(N), keys))[:N // 2])
    first = int(P.u(SEED, P.FIRST, 1, 0)) % (N // 2)
    assert np.array_equal(anc, subset[_farthest_sampler_sample(pc1[subset], M, first)])
    diff = pc1[anc].astype(np.float64)[:, None, :] - pc2.astype(np.float64)[None, :, :]
    assert np.array_equal(pos, np.argmin((diff ** 2).sum(axis=2), axis=1))
    assert len(set(anc.tolist())) == M and rep["min_gap"] > 1e-9   # random clouds: no tie, far above double rounding


def test_ties_go_to_the_first_maximum_and_the_lowest_index():
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    rep = {}
    anc, pos = P.sample_pair_nodes(g, np.concatenate([g[:32], g[:32]]), 8, SEED, 0, report=rep)
    assert rep["min_gap"] == 0.0                       # a lattice: true ties
    assert np.all(pos < 32)                            # every row of pc2 is there twice: the lower copy is taken
    d = ((g[anc].astype(np.float64)[:, None] - np.concatenate([g[:32], g[:32]]).astype(np.float64)[None]) ** 2).sum(-1)
    assert np.array_equal(pos, d.argmin(axis=1))


def test_stream_distributions():
    # jitter normals before clipping: n values, mean 0 and variance 1.  The sample mean has standard error 1 / sqrt(n), the
    # sample standard deviation about 1 / sqrt(2 n); five standard errors each (a false alarm once in ~2e6).
    n = 3 * 40000
    clipped, z = P.jitter_values(40000, SEED, 7)
    assert abs(z.mean()) <= 5.0 / np.sqrt(n) and abs(z.std() - 1.0) <= 5.0 / np.sqrt(2 * n)
    assert np.abs(clipped).max() <= 0.1 and np.array_equal(clipped, np.clip(0.05 * z, -0.1, 0.1))
    assert (np.abs(clipped) == 0.1).mean() == pytest.approx(0.0455, abs=5 * np.sqrt(0.0455 * 0.9545 / n))  # P(|z| > 2)
    # a choice of m = 16 from n = 64 over T seeds: each index is chosen with probability 1/4, a count is binomial(T, 1/4)
    # with standard deviation sqrt(T * 3/16); five of them, over 64 indices
    T, counts = 2000, np.zeros(64)
    for s in range(T):
        counts[P.choice(s, P.SUBSET, 0, 64, 16)] += 1
    assert np.abs(counts - T / 4).max() <= 5 * np.sqrt(T * 3 / 16), counts
    # pad draws and the first pick are u mod n: uniform over [0, n)
    draws = (P.u(SEED, P.PAD, 3, np.arange(64000)) % np.uint64(64)).astype(np.int64)
    assert np.abs(np.bincount(draws, minlength=64) - 1000).max() <= 5 * np.sqrt(1000 * 63 / 64)


def test_uniform_ranges_and_parameters():
    big = np.uint64(0xFFFFFFFFFFFFFFFF)
    assert P.unit_co(big) < 1.0 and P.unit_co(np.uint64(0)) == 0.0
    assert P.unit_oc(big) == 1.0 and P.unit_oc(np.uint64(0)) == 2.0 ** -53
    assert int(P.splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF   # the published first output of splitmix64 from state 0
    for b in range(20):
        par = P.augment_params(P.AUG_ORDER, SEED, b)
        assert 0.8 <= par["scale"] < 1.25 and np.all(np.abs(par["shift"]) <= 0.1)
        for R in (par["rot1d"], par["rot_small"], P.pair_rotation(SEED, b)):
            assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1) < 1e-15
        assert np.arccos(min(1.0, (np.trace(par["rot_small"]) - 1) / 2)) <= 0.18 * np.sqrt(3) + 1e-12


def test_composed_builders_are_the_stages():
    rng = np.random.default_rng(3)
    src = (rng.standard_normal((2, 300, 3)) * 5).astype(np.float32)
    out = P.make_local_pairs(src, [300, 120], 128, 16, SEED)
    assert out["points"].shape == (4, 128, 3) and out["sample_idx"].shape == (4, 16) and out["R"].shape == (2, 3, 3)
    for b in range(2):
        anc, pos = out["sample_idx"][b], out["sample_idx"][2 + b]
        a, p = out["points"][b][anc].astype(np.float64) @ out["R"][b].astype(np.float64), out["points"][2 + b][pos]
        # pc1 and pc2 are two jittered draws of one cloud: the anchor's own source point, jittered again, is in pc2 unless
        # the draw dropped it (cloud 0 keeps 128 of 300), so only the padded cloud 1 (every point kept) is bounded
        if b == 1:
            assert np.linalg.norm(a - p, axis=1).max() <= 2 * 0.1 * np.sqrt(3) + 1e-4
    g = P.make_global_batch(src, [300, 120], 128, SEED)
    assert g.shape == (2, 128, 3) and g.dtype == np.float32
