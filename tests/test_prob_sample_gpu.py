"""GPU: dh3d_prob_sample / dh3d_prob_sample_seeded against the numpy restatement (tests/prob_sample_reference.py): the
cumulative sums bit for bit and the ids, at the row lengths where the kernel changes path (quad tails, the 32-quad step
of the reference's LDS padding, the 64-quad segment a wave holds, odd tree sizes, one / two / three chunks joined by the
compensated sum), on uniform, wide-range, tied integer
and non-monotone rows; counts, void rows, slot independence, graph replay and the Python surface."""
import functools

import numpy as np
import pytest
import torch

import prob_sample_reference as R

pytestmark = pytest.mark.gpu
F32 = np.float32


def make_rows(kind, b, n, rng):
    if kind == "uniform":
        return rng.random((b, n)).astype(F32)
    if kind == "wide":
        return np.stack([R.wide_range_row(rng, n) for _ in range(b)])
    if kind == "integer":                      # zero runs, exact sums: ties everywhere
        w = rng.integers(0, 9, (b, n)).astype(F32)
        w[rng.random((b, n)) < 0.5] = 0
        w[:, 0] = np.where(w.sum(axis=1) == 0, 1, w[:, 0])
        return w
    assert kind == "dip"                       # the non-monotone fixture in row 0, wide-range rows of its length behind it
    first = R.non_monotone_row()[0]
    return np.stack([first] + [R.wide_range_row(rng, len(first)) for _ in range(b - 1)])


def make_draws(cum, m, rng, extra=()):
    """Draws of one row: 0, 1, the tie values cum[r] / total and one float above them, then uniform ones."""
    n = len(cum)
    at = (cum[rng.choice(n, min(n, 24), replace=False)] / cum[-1]).astype(F32)
    special = np.concatenate([np.asarray(extra, dtype=F32), [F32(0), F32(1)], at, np.nextafter(at, F32(2))]).astype(F32)
    special = special[special <= 1]
    if m > len(special):
        return np.concatenate([special, rng.random(m - len(special)).astype(F32)])
    return rng.choice(special, m, replace=False)


CASES = [("uniform", 3, 1, 1), ("uniform", 1, 2, 5), ("wide", 3, 3, 5), ("integer", 1, 4, 300), ("uniform", 3, 5, 5),
         ("wide", 1, 7, 1), ("integer", 3, 8, 5), ("uniform", 33, 37, 300), ("wide", 3, 127, 1025), ("uniform", 1, 128, 5),
         ("integer", 3, 129, 300), ("wide", 33, 132, 5), ("uniform", 3, 8191, 300), ("wide", 1, 8192, 1025),
         ("integer", 3, 8193, 5), ("uniform", 3, 8195, 1025), ("wide", 3, 16389, 300), ("uniform", 1, 20000, 1025),
         ("integer", 1, 20000, 300), ("dip", 1, 0, 300), ("dip", 3, 0, 1025),
         # the 64-quad segment of a wave: its edge, a partial second one, odd numbers of segments
         ("uniform", 3, 255, 5), ("wide", 1, 256, 300), ("uniform", 3, 257, 5), ("integer", 1, 261, 5), ("uniform", 3, 769, 5),
         ("wide", 1, 1300, 300), ("wide", 3, 4100, 300)]


@pytest.mark.parametrize("kind,b,n,m", CASES)
def test_sums_and_ids_are_the_restatements(dev, kind, b, n, m):
    from dh3d_amd import pm
    rng = np.random.default_rng(b * 100003 + n * 7 + m)
    w = make_rows(kind, b, n, rng)
    cum = np.stack([R.cumsum(row) for row in w])
    extra = (R.non_monotone_row()[2],) if kind == "dip" else ()
    draws = np.stack([make_draws(c, m, rng, extra) for c in cum])
    exp = np.stack([R.walk(c, d) for c, d in zip(cum, draws)])
    ids, temp = pm.prob_sample(torch.from_numpy(w).to(dev), torch.from_numpy(draws).to(dev))
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (b, m) and tuple(temp.shape) == w.shape
    assert np.array_equal(temp.cpu().numpy().view(np.int32), cum.view(np.int32)), "cumulative sums differ in some bit"
    assert np.array_equal(ids.cpu().numpy(), exp)
    if kind == "dip":   # the fixture does what it is there for: the sums step down, a sorted search would answer otherwise
        assert (np.diff(cum[0]) < 0).any()
        other = np.minimum(np.searchsorted(cum[0], draws[0] * cum[0, -1], side="left"), w.shape[1] - 1)
        assert (other != exp[0]).any()


def abi_seeded(w, m, count, seed, dev, temp_fill=None):
    """dh3d_prob_sample_seeded on caller-made buffers: (ids, temp) as numpy; out starts at -7, temp at temp_fill."""
    from dh3d_amd import _lib as L
    b, n = w.shape
    wt = torch.from_numpy(w).to(dev)
    ct = None if count is None else torch.tensor(count, dtype=torch.int32, device=dev)
    sd = torch.tensor([seed], dtype=torch.int64, device=dev)
    temp = torch.full((b, n), float("nan") if temp_fill is None else temp_fill, dtype=torch.float32, device=dev)
    out = torch.full((b, m), -7, dtype=torch.int32, device=dev)
    L.check(L.lib().dh3d_prob_sample_seeded(b, n, m, L.ptr(wt), L.ptr(ct), L.ptr(sd), L.ptr(temp), L.ptr(out), L.stream_ptr()),
            "prob_sample_seeded")
    torch.cuda.synchronize()
    return out.cpu().numpy(), temp.cpu().numpy()


@functools.lru_cache(maxsize=None)
def seeded_case(n):
    """Seven rows: counts 0, 1, mid, n, n + 7, -3, and a row of zeros; the entries behind a row's count are NaN."""
    rng = np.random.default_rng(n)
    w = R.wide_range_row(rng, 7 * n).reshape(7, n)
    count = [0, 1, n // 2 + 1, n, n + 7, -3, n]
    w[6] = 0
    for b, c in enumerate(count):
        w[b, min(max(c, 0), n):] = np.nan
    return w, count


@pytest.mark.parametrize("n", [300, 8195])
@pytest.mark.parametrize("seed", [7, (1 << 63) + 12345])
def test_seeded_form_counts_and_void_rows(dev, n, seed):
    w, count = seeded_case(n)
    m = 300
    exp = R.sample_by_weight(w, m, count=count, seed=seed)
    ids, temp = abi_seeded(w, m, count, seed - (1 << 64) if seed >= 1 << 63 else seed, dev)
    assert np.array_equal(ids, exp)
    assert (exp[[0, 5, 6]] == -1).all() and (exp[1] == 0).all() and exp[2].max() <= n // 2 and exp[[1, 2, 3, 4]].min() >= 0
    for b in (2, 3):
        nb = min(count[b], n)
        assert np.array_equal(temp[b, :nb].view(np.int32), R.cumsum(w[b, :nb]).view(np.int32))
    # temp's prior content changes nothing
    ids2, _ = abi_seeded(w, m, count, seed - (1 << 64) if seed >= 1 << 63 else seed, dev, temp_fill=1e30)
    assert np.array_equal(ids2, exp)


def test_seeded_row_depends_on_its_slot_and_entries_only(dev):
    rng = np.random.default_rng(9)
    w = rng.random((5, 1000)).astype(F32)
    full, _ = abi_seeded(w, 64, None, 21, dev)
    assert np.array_equal(full, R.sample_by_weight(w, 64, seed=21))
    for b in (0, 2, 4):
        alone = np.ones((b + 1, 1000), dtype=F32)     # the same row at its slot, other rows (and another batch size) round it
        alone[b] = w[b]
        got, _ = abi_seeded(alone, 64, None, 21, dev)
        assert np.array_equal(got[b], full[b])
    assert not np.array_equal(full[0], abi_seeded(w[[1, 0]], 64, None, 21, dev)[0][1])   # another slot: other draws


def test_graph_replay_draws_afresh(dev):
    from dh3d_amd import utils
    rng = np.random.default_rng(4)
    w = R.wide_range_row(rng, 3 * 500).reshape(3, 500)
    count = [500, 123, 0]
    wt = torch.from_numpy(w).to(dev)
    ct = torch.tensor(count, dtype=torch.int32, device=dev)
    sd = torch.tensor([1], dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        utils.sample_by_weight(wt, 40, count=ct, seed=sd)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ids = utils.sample_by_weight(wt, 40, count=ct, seed=sd)
    seen = []
    for seed in (5, 6):
        sd.fill_(seed)
        graph.replay()
        torch.cuda.synchronize()
        seen.append(ids.cpu().numpy().copy())
        assert np.array_equal(seen[-1], R.sample_by_weight(w, 40, count=count, seed=seed))
    assert not np.array_equal(seen[0], seen[1])
    assert np.array_equal(utils.sample_by_weight(wt, 40, count=ct, seed=6).cpu().numpy(), seen[1])   # an int seed, eager


def test_python_surface(dev):
    from dh3d_amd import ops
    rng = np.random.default_rng(3)
    w = torch.from_numpy(rng.random((2, 50)).astype(F32)).to(dev).requires_grad_(True)
    r = torch.from_numpy(rng.random((2, 7)).astype(F32)).to(dev)
    with pytest.raises(ValueError, match=r"ProbSample expects \(batch_size,num_choices\) inp shape"):
        ops.prob_sample(w[0], r)
    with pytest.raises(ValueError, match=r"ProbSample expects \(batch_size,num_points\) inpr shape"):
        ops.prob_sample(w, r[0])
    with pytest.raises(ValueError, match=r"ProbSample expects \(batch_size,num_points\) inpr shape"):
        ops.prob_sample(w, r[:1])
    with pytest.raises(ValueError, match="GPU"):
        ops.prob_sample(w.detach().cpu(), r.cpu())
    with pytest.raises(ValueError):
        ops.prob_sample(w.double(), r)
    ids = ops.prob_sample(w, r)
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (2, 7) and not ids.requires_grad
    assert np.array_equal(ids.cpu().numpy(), R.prob_sample(w.detach().cpu().numpy(), r.cpu().numpy())[0])
    pts = torch.from_numpy(rng.random((2, 50, 3)).astype(F32)).to(dev)
    got = ops.gather_point(pts, ids).cpu().numpy()
    host = np.stack([pts[b].cpu().numpy()[ids[b].cpu().numpy()] for b in range(2)])
    assert np.array_equal(got, host)
