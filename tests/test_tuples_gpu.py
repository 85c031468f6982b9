"""GPU: the training-tuple kernels of dh3d_amd.tuples (csrc/tuples.hip) against the numpy restatement of their contract
(tests/tuples_reference.py).  Every output is an integer id or a flag, kernel and restatement get the same float64 positions
and float32 descriptors and the rules are exact in float64: everything is compared bit for bit."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tuples_reference as T  # noqa: E402
from pairs_reference import u, unit_co  # noqa: E402

SEED = 0x5EEDC0FFEE123457  # (above 2^62: the whole 64 bits travel)


def _T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _scatter(M, side, seed):
    """M places uniform in a square of `side` metres at UTM-sized offsets; places 3 and 5 share their coordinates."""
    pos = T.OFFSET + np.random.default_rng(seed).random((M, 2)) * side
    if M > 5:
        pos[5] = pos[3]
    return pos


def _desc(M, D, seed, distinct=None):
    """float32 descriptors; distinct = k: only k different rows, so most distances tie and the id decides."""
    rng = np.random.default_rng(seed)
    if distinct:
        return rng.standard_normal((distinct, D)).astype(np.float32)[rng.integers(0, distinct, M)]
    return rng.standard_normal((M, D)).astype(np.float32)


def _queries(n, Q, seed, first=None):
    """Q query slots: random live places; with Q >= 5, slot 1 holds -1 and slot 3 the first place behind the live map."""
    q = np.random.default_rng(seed).integers(0, n, Q).astype(np.int32)
    if first is not None:
        q[0] = first
    if Q >= 5:
        q[1], q[3] = -1, n
        if n > 5:
            q[2], q[4] = 3, 5  # the two places at identical coordinates
    return q


def _run(dev, pos, queries, num_pos, num_neg, count=None, other_neg=True, desc=None, num_hard=0, pool_fraction=1.0,
         pos_radius=10.0, neg_radius=50.0, seed=SEED):
    """The C entry point on sentinel-filled outputs: every element must be written."""
    from dh3d_amd import _lib as L
    from dh3d_amd import pairs
    M, Q = pos.shape[0], len(queries)
    p, qs, sd = _T(pos, dev), _T(np.asarray(queries, dtype=np.int32), dev), pairs.seed_tensor(seed, dev)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    d = None if desc is None else _T(desc, dev)
    i32 = dict(dtype=torch.int32, device=dev)
    out = {"pos": torch.full((Q, num_pos), -7, **i32), "neg": torch.full((Q, num_neg), -7, **i32),
           "other": torch.full((Q,), -7, **i32) if other_neg else None, "valid": torch.full((Q,), -7, **i32)}
    L.check(L.lib().dh3d_sample_tuples(L.ptr(p), L.ptr(cnt), M, L.ptr(qs), Q, num_pos, num_neg, pos_radius, neg_radius, L.ptr(d),
                                       d.stride(0) if d is not None else 0, d.shape[1] if d is not None else 0, num_hard,
                                       pool_fraction, L.ptr(sd), L.ptr(out["pos"]), L.ptr(out["neg"]), L.ptr(out["other"]),
                                       L.ptr(out["valid"]), L.stream_ptr()), "sample_tuples")
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _same(got, exp):
    for k in ("pos", "neg", "other", "valid"):
        if exp[k] is None:
            assert got[k] is None, k
        else:
            assert np.array_equal(got[k], exp[k]), (k, got[k], exp[k])


def _behind(a, n):
    """The array with NaN behind its first n rows: rows at or beyond the live map are never read."""
    a = a.copy()
    a[n:] = np.nan
    return a


# name: (positions, live count or None, Q, num_pos, num_neg, other_neg, num_hard, pool_fraction, D, distinct descriptor rows)
CASES = {
    "one_place": (lambda: _scatter(1, 10.0, 1), None, 1, 1, 1, True, 0, 1.0, 0, None),
    "m63": (lambda: _scatter(63, 110.0, 2), None, 5, 1, 1, True, 1, 1.0, 8, None),
    "m64": (lambda: _scatter(64, 110.0, 3), None, 5, 2, 8, True, 3, 0.25, 8, None),
    "m65_count64": (lambda: _scatter(65, 100.0, 4), 64, 17, 2, 8, False, 8, 1.0, 256, 9),
    "m65_small_pool": (lambda: _scatter(65, 72.0, 5), None, 5, 1, 8, True, 8, 0.25, 8, None),
    "grid": (T.grid_positions, None, 17, 2, 18, True, 0, 1.0, 0, None),
    "grid_hard": (T.grid_positions, None, 5, 2, 18, True, 3, 0.25, 256, None),
    "grid_count500": (T.grid_positions, 500, 17, 2, 18, True, 18, 1.0, 8, 40),
    "route": (T.route_positions, None, 17, 2, 18, True, 0, 1.0, 0, None),
    "route_no_other": (T.route_positions, None, 17, 2, 18, False, 3, 0.0, 8, None),
    "route_all_hard": (T.route_positions, None, 5, 2, 18, True, 18, 1.0, 256, None),
    "route_single": (T.route_positions, None, 1, 2, 8, True, 3, 1.0, 8, None),
    "m4099": (lambda: _scatter(4099, 300.0, 6), None, 5, 8, 64, True, 0, 1.0, 0, None),
    "m4099_hard": (lambda: _scatter(4099, 250.0, 7), None, 5, 8, 64, True, 64, 0.25, 256, 300),
    "m4099_count3000": (lambda: _scatter(4099, 600.0, 8), 3000, 17, 2, 18, True, 3, 0.25, 8, None),
    "m4099_no_other": (lambda: _scatter(4099, 600.0, 9), None, 17, 1, 1, False, 1, 1.0, 256, None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_sample_tuples_is_the_restatement(dev, name):
    make, count, Q, num_pos, num_neg, other_neg, num_hard, fraction, D, distinct = CASES[name]
    pos = make()
    M = pos.shape[0]
    n = M if count is None else count
    desc = _desc(M, D, 11, distinct) if D else None
    queries = _queries(n, Q, 12)
    if name == "grid":
        queries[6] = 300  # a central place: fewer than 18 places lie beyond 50 m
    kw = dict(count=count, other_neg=other_neg, desc=desc, num_hard=num_hard, pool_fraction=fraction)
    exp = T.sample_tuples(pos, queries, num_pos, num_neg, seed=SEED, **kw)
    if count is not None:  # NaN behind the live map, in positions and descriptors alike
        pos = _behind(pos, n)
        kw["desc"] = None if desc is None else _behind(desc, n)
    got = _run(dev, pos, queries, num_pos, num_neg, seed=SEED, **kw)
    _same(got, exp)
    if Q >= 5:  # the slots that hold no live place
        assert (got["pos"][[1, 3]] == -1).all() and (got["neg"][[1, 3]] == -1).all() and not got["valid"][[1, 3]].any()
    if name == "grid":  # both outcomes of `valid` occur among the live slots
        assert got["valid"][2] == 1 and got["valid"][6] == 0 and (got["pos"][6] >= 0).all() and (got["neg"][6] == -1).all()
    if name == "m65_small_pool":  # a pool smaller than num_hard: the row is filled up with random negatives
        sizes = []
        for b, q in enumerate(queries):
            if 0 <= q < n:
                neg = T.sets(pos, int(q), n)[1]
                sizes.append(((unit_co(u(SEED, T.POOL, b, neg)) < fraction).sum(), len(neg)))
        assert any(0 < pool < num_hard <= total for pool, total in sizes), sizes


@pytest.mark.gpu
def test_a_query_with_no_possible_other_negative(dev):
    """Four places round the query, eight far away: all eight are the negative row, and every place is then within the
    positive radius of the query or IS a chosen negative -- the rows are filled, the other negative is -1, valid is 0."""
    rng = np.random.default_rng(3)
    pos = T.OFFSET + np.concatenate([rng.random((4, 2)) * 5.0, np.array([200.0, 0.0]) + rng.random((8, 2)) * 80.0])
    exp = T.sample_tuples(pos, [0, 2], 2, 8, seed=SEED)
    got = _run(dev, pos, [0, 2], 2, 8, seed=SEED)
    _same(got, exp)
    assert (got["pos"] >= 0).all() and (np.sort(got["neg"], axis=1) == np.arange(4, 12)).all()
    assert (got["other"] == -1).all() and not got["valid"].any()
    assert _run(dev, pos, [0, 2], 2, 8, other_neg=False, seed=SEED)["valid"].all()


@pytest.mark.gpu
@pytest.mark.parametrize("D", [8, 256])
def test_hard_negatives_are_the_retrieval_order(dev, D):
    """An independent check of the hard stage: with every negative in the pool and the whole row hard, the row is the
    front of dh3d_retrieve's exact order of the map round the query's descriptor, restricted to NEG(q)."""
    from dh3d_amd import tuples
    from dh3d_amd.retrieval import search_descriptors_sq
    pos = _scatter(64, 200.0, 21)
    desc = _desc(64, D, 22, distinct=20 if D == 8 else None)
    p, d = _T(pos, dev), _T(desc, dev)
    queries = np.array([0, 3, 17, 40, 63], dtype=np.int32)
    out = tuples.sample_tuples(p, _T(queries, dev), 1, 8, desc=d, num_hard=8, pool_fraction=1.0, seed=SEED)
    neg = out["neg"].cpu().numpy()
    for b, q in enumerate(queries):
        order = search_descriptors_sq(d, d[q:q + 1], 64)[0][0].cpu().numpy()
        allowed = set(T.sets(pos, int(q), 64)[1].tolist())
        assert len(allowed) >= 8
        assert neg[b].tolist() == [j for j in order.tolist() if j in allowed][:8], (b, q)


@pytest.mark.gpu
def test_a_slot_does_not_depend_on_the_other_slots(dev):
    from dh3d_amd import tuples
    pos = T.route_positions()
    desc = _desc(602, 8, 31)
    p, d = _T(pos, dev), _T(desc, dev)
    many = _queries(602, 17, 32, first=150)
    kw = dict(desc=d, num_hard=3, pool_fraction=0.25, seed=SEED)
    a = tuples.sample_tuples(p, _T(many, dev), 2, 18, **kw)
    b = tuples.sample_tuples(p, _T(many[:1], dev), 2, 18, **kw)
    for k in ("pos", "neg", "other", "valid"):
        assert torch.equal(a[k][:1], b[k]), k
    exp = T.sample_tuples(pos, many, 2, 18, desc=desc, num_hard=3, pool_fraction=0.25, seed=SEED)
    _same({k: v.cpu().numpy() for k, v in a.items()}, exp)


@pytest.mark.gpu
@pytest.mark.parametrize("name,count,Q", [("grid", None, 450), ("grid", 500, 40), ("route", None, 620), ("route", 77, 5),
                                          ("grid", None, 1), ("grid", None, "eligible")])
def test_counts_and_queries_are_the_restatement(dev, name, count, Q):
    """tuple_counts and draw_queries on the two maps; Q above the number of places that can be queries (412 on the grid,
    600 on the route) takes the -1 / ok = 0 path.  Q = 1 and Q = that number itself are the select's k = 1 and k = n."""
    from dh3d_amd import tuples
    pos = T.grid_positions() if name == "grid" else T.route_positions()
    M = pos.shape[0]
    n = M if count is None else count
    exp_pos, exp_neg = T.tuple_counts(pos, count)
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    n_pos, n_neg = tuples.tuple_counts(_T(_behind(pos, n), dev), cnt)
    assert np.array_equal(n_pos.cpu().numpy(), exp_pos) and np.array_equal(n_neg.cpu().numpy(), exp_neg)
    eligible = int(((exp_pos[:n] >= 2) & (exp_neg[:n] >= 18)).sum())
    if Q == "eligible":
        Q = eligible
    for seed in (SEED, 1):
        exp_q, exp_ok = T.draw_queries(exp_pos, exp_neg, Q, 2, 18, count, seed)
        queries, ok = tuples.draw_queries(n_pos, n_neg, Q, 2, 18, count=cnt, seed=seed)
        assert np.array_equal(queries.cpu().numpy(), exp_q) and int(ok) == exp_ok
    if count is None and Q > eligible:
        assert exp_ok == 0 and exp_q[-1] == -1 and exp_q[0] >= 0
    elif count is None:
        assert exp_ok == 1 and (exp_q >= 0).all() and len(set(exp_q.tolist())) == Q


def _bank(dev, points, seed):
    """The route as a PlaceIndex that holds a cloud of `points` points (some shorter) and an 8-float descriptor per place."""
    from dh3d_amd.retrieval import PlaceIndex
    pos = T.route_positions()
    rng = np.random.default_rng(seed)
    clouds = (rng.standard_normal((602, points, 3)) * 20.0).astype(np.float32)
    counts = rng.integers(points // 2, points + 1, 602).astype(np.int32)
    bank = PlaceIndex(dim=8, capacity=640, device=dev, points=points)
    bank.add(_desc(602, 8, seed + 1), pos, cloud=clouds, cloud_count=counts)
    return bank, pos


@pytest.mark.gpu
def test_make_quadruplet_batch_replays_fresh_batches(dev):
    """bank -> counts -> queries -> tuples -> clouds -> batch captured as one graph with a device seed: every replay is the
    eager call with that seed, and two seeds give two batches."""
    from dh3d_amd import tuples
    bank, _ = _bank(dev, 96, 41)
    sd = torch.tensor([11], dtype=torch.int64, device=dev)
    kw = dict(numpts=64, num_hard=2, pool_fraction=0.25)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tuples.make_quadruplet_batch(bank, 2, 2, 18, seed=sd, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tuples.make_quadruplet_batch(bank, 2, 2, 18, seed=sd, **kw)
    seen = []
    for s in (101, 102, SEED):
        sd.fill_(s - (1 << 64) if s >= 1 << 63 else s)
        graph.replay()
        torch.cuda.synchronize()
        seen.append({k: v.clone() for k, v in out.items()})
        eager = tuples.make_quadruplet_batch(bank, 2, 2, 18, seed=s, **kw)
        for k in eager:
            assert torch.equal(seen[-1][k], eager[k]), (s, k)
        assert bool(eager["valid"].all()) and int(eager["ok"]) == 1 and tuple(eager["points"].shape) == (2 * 22, 64, 3)
    assert not torch.equal(seen[0]["ids"], seen[1]["ids"]) and not torch.equal(seen[0]["points"], seen[1]["points"])


@pytest.mark.gpu
def test_make_quadruplet_batch_feeds_the_quadruplet_trainer(dev):
    from dh3d_amd import ConfigFactory, pairs, tuples
    from dh3d_amd.model import DH3D
    from dh3d_amd.training import QuadrupletTrainer
    bank, pos = _bank(dev, 600, 51)
    B, P, Ng = 1, 2, 3
    batch = tuples.make_quadruplet_batch(bank, B, P, Ng, numpts=512, seed=SEED)
    # the restatement's ids, in the role order losses._split expects
    n_pos, n_neg = T.tuple_counts(pos)
    queries, ok = T.draw_queries(n_pos, n_neg, B, P, Ng, seed=SEED)
    t = T.sample_tuples(pos, queries, P, Ng, seed=SEED)
    ids = np.concatenate([queries, t["pos"].ravel(), t["neg"].ravel(), t["other"]])
    assert ok == 1 and t["valid"].all() and (ids >= 0).all()
    assert np.array_equal(batch["ids"].cpu().numpy(), ids)
    assert np.array_equal(batch["valid"].cpu().numpy(), t["valid"]) and int(batch["ok"]) == 1
    rows = _T(ids.astype(np.int64), dev)
    points = pairs.make_global_batch(bank.cloud.index_select(0, rows), bank.cloud_count.index_select(0, rows), 512, seed=SEED)
    assert torch.equal(batch["points"], points) and tuple(points.shape) == (B * (1 + P + Ng + 1), 512, 3)
    cfg = ConfigFactory("global_config").getconfig()
    cfg.batch_size, cfg.num_pos, cfg.num_neg = B, P, Ng
    model = DH3D(cfg).init_synthetic(7).to(dev).eval().prepare()
    loss = QuadrupletTrainer(model, graph_step=False, graph_backbone=False).step(batch["points"])
    assert math.isfinite(loss), loss
