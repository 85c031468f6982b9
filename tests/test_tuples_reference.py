"""CPU: the numpy restatement of "Training tuples" (tests/tuples_reference.py) against the reference loader's own logic
(core/datasets.py Global_train_dataset_triplet.__iter__): with the positives / nonnegtives dict of its tuple pickles built
from the positions by brute force, every pick of the restatement is one the reference's set arithmetic could have made --
and the other negative is, beyond that, never the query nor a chosen negative (the header's stated deviation)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tuples_reference as T  # noqa: E402


def _sets_dict(pos, pos_radius=10.0, neg_radius=50.0):
    """{i: {"positives": [...], "nonnegtives": [...]}} as the reference's pickles hold them: plain Python floats, one pair
    at a time.  The query is its own non-negative and not its own positive."""
    out = {}
    xs, ys = pos[:, 0].tolist(), pos[:, 1].tolist()
    for i in range(len(xs)):
        p, nn = [], []
        for j in range(len(xs)):
            dx, dy = xs[j] - xs[i], ys[j] - ys[i]
            d2 = dx * dx + dy * dy
            if d2 <= pos_radius * pos_radius and j != i:
                p.append(j)
            if d2 <= neg_radius * neg_radius:
                nn.append(j)
        out[i] = {"positives": p, "nonnegtives": nn}
    return out


@pytest.fixture(scope="module")
def maps():
    out = {}
    for name, pos in (("grid", T.grid_positions()), ("route", T.route_positions())):
        out[name] = (pos, _sets_dict(pos), T.tuple_counts(pos))
    return out


def test_the_inputs_are_the_ones_the_cases_were_chosen_on(maps):
    pos, d, (n_pos, n_neg) = maps["grid"]
    d2 = (pos[:, None, 0] - pos[None, :, 0]) ** 2 + (pos[:, None, 1] - pos[None, :, 1]) ** 2
    assert pos.shape == (576, 2) and (d2 == 100.0).sum() == 1920 and (d2 == 2500.0).sum() == 1152
    assert ((n_pos >= 2) & (n_neg >= 18)).sum() == 412
    pos, d, (n_pos, n_neg) = maps["route"]
    assert pos.shape == (602, 2) and ((n_pos >= 2) & (n_neg >= 18)).sum() == 600
    assert n_pos.min() == 1 and n_pos.max() == 10 and list(n_pos[600:]) == [1, 1] and n_pos[150] == 8


def test_the_restatement_and_the_header_state_one_contract():
    """The restatement was written from include/dh3d_hip.h "Training tuples": its stream numbers, radii and limits are the
    ones that section and the Python module give."""
    from dh3d_amd import tuples
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "dh3d_hip.h")).read()
    section = header[header.index("Training tuples"):header.index("int dh3d_sample_tuples")]
    for number, name in ((T.POS_KEYS, "positive keys"), (T.NEG_KEYS, "negative keys"), (T.POOL, "pool membership"),
                         (T.OTHER_KEYS, "other-negative keys"), (T.QUERY_KEYS, "query keys")):
        assert "%d %s" % (number, name) in section, name
    import inspect
    for fn in (T.sets, T.tuple_counts, T.sample_slot):
        p = inspect.signature(fn).parameters
        assert (p["pos_radius"].default, p["neg_radius"].default) == (tuples.POS_RADIUS, tuples.NEG_RADIUS) == (10.0, 50.0)
    assert "pos_radius = 10.0, neg_radius = 50.0" in section
    assert (tuples.MAX_PLACES, tuples.MAX_QUERIES, tuples.MAX_PICK, tuples.DESC_MAX) == (1 << 20, 65535, 64, 256)
    for limit in ("M <= 2^20", "Q <= 65535", "1 <= num_pos <= 64", "1 <= num_neg <= 64", "0 <= num_hard <= num_neg", "D <= 256"):
        assert limit in section, limit


@pytest.mark.parametrize("name", ["grid", "route"])
def test_counts_are_the_dict_sizes(maps, name):
    pos, d, (n_pos, n_neg) = maps[name]
    M = len(pos)
    assert [len(d[i]["positives"]) for i in range(M)] == list(n_pos)
    assert [M - len(d[i]["nonnegtives"]) for i in range(M)] == list(n_neg)
    # a shorter live map: the counts of the first places among themselves, zeros behind
    a, b = T.tuple_counts(pos, count=100)
    sub = _sets_dict(pos[:100])
    assert [len(sub[i]["positives"]) for i in range(100)] == list(a[:100]) and not a[100:].any() and not b[100:].any()


@pytest.mark.parametrize("name", ["grid", "route"])
def test_queries_are_the_shuffle_with_its_continue(maps, name):
    pos, d, (n_pos, n_neg) = maps[name]
    M = len(pos)
    can = {i for i in range(M) if len(d[i]["positives"]) >= 2 and M - len(d[i]["nonnegtives"]) >= 18}
    orders = []
    for seed in range(5):
        q, ok = T.draw_queries(n_pos, n_neg, len(can), 2, 18, seed=seed)
        assert ok == 1 and set(q.tolist()) == can            # every place the loader would not skip, each once
        orders.append(q.tolist())
        q2, ok2 = T.draw_queries(n_pos, n_neg, 7, 2, 18, seed=seed)
        assert ok2 == 1 and q2.tolist() == orders[-1][:7]    # fewer queries: the front of the same shuffle
        q3, ok3 = T.draw_queries(n_pos, n_neg, len(can) + 3, 2, 18, seed=seed)
        assert ok3 == 0 and q3.tolist() == orders[-1] + [-1, -1, -1]
    assert len({tuple(o) for o in orders}) == 5


@pytest.mark.parametrize("name,other_neg", [("grid", True), ("route", True), ("route", False)])
def test_picks_are_picks_the_reference_could_make(maps, name, other_neg):
    pos, d, (n_pos, n_neg) = maps[name]
    M = len(pos)
    everyone = set(range(M))
    filled = unfilled = 0
    for seed in range(12):
        queries = list(np.random.default_rng(seed).integers(0, M, 6)) + ([600, 601] if name == "route" else [300])
        for b, q in enumerate(queries):
            q = int(q)
            p, g, other, valid = T.sample_slot(pos, q, b, 2, 18, other_neg=other_neg, seed=seed)
            positives, nonneg = d[q]["positives"], d[q]["nonnegtives"]
            if len(positives) < 2:                         # the reference's `continue`
                assert (p == -1).all() and valid == 0
            else:
                assert len(set(p.tolist())) == 2 and set(p.tolist()) <= set(positives)
            if len(everyone - set(nonneg)) < 18:           # (np.random.choice raises there)
                assert (g == -1).all() and valid == 0 and (other is None or other == -1)
                unfilled += 1
                continue
            assert len(set(g.tolist())) == 18 and not set(g.tolist()) & set(nonneg)
            if other_neg:
                neighbours = set(positives)
                for neg in g.tolist():
                    neighbours |= set(d[neg]["positives"])
                assert other >= 0 and other not in neighbours and other != q and other not in g.tolist()
            else:
                assert other is None
            assert valid == int(len(positives) >= 2)
            filled += 1
    assert filled and (unfilled or name == "route")        # the grid's centre has too few negatives


def test_out_of_map_queries_and_radii(maps):
    pos, d, _ = maps["route"]
    for q in (-1, 602, 100):                                 # (100 with a live map of 100 places)
        p, g, other, valid = T.sample_slot(pos, q, 0, 2, 18, count=100 if q == 100 else None)
        assert (p == -1).all() and (g == -1).all() and other == -1 and valid == 0
    # other radii: the sets follow them
    wide = _sets_dict(pos, 25.0, 30.0)
    p, g, other, valid = T.sample_slot(pos, 40, 1, 5, 30, pos_radius=25.0, neg_radius=30.0, seed=3)
    assert valid == 1 and set(p.tolist()) <= set(wide[40]["positives"]) and not set(g.tolist()) & set(wide[40]["nonnegtives"])


def test_hard_negatives_lead_the_row(maps):
    pos, d, _ = maps["route"]
    M = len(pos)
    rng = np.random.default_rng(5)
    desc = rng.standard_normal((M, 8)).astype(np.float32)
    q, b = 150, 2
    negatives = sorted(set(range(M)) - set(d[q]["nonnegtives"]))
    dist = ((desc[negatives].astype(np.float64) - desc[q].astype(np.float64)) ** 2).sum(axis=1)
    nearest = [negatives[i] for i in np.argsort(dist, kind="stable")[:3]]
    p, g, other, valid = T.sample_slot(pos, q, b, 2, 18, desc=desc, num_hard=3, pool_fraction=1.0, seed=9)
    assert g[:3].tolist() == nearest and len(set(g.tolist())) == 18 and valid == 1
    assert not set(g.tolist()) & set(d[q]["nonnegtives"])
    # an empty pool: the row is the random one
    g0 = T.sample_slot(pos, q, b, 2, 18, desc=desc, num_hard=3, pool_fraction=0.0, seed=9)[1]
    assert g0.tolist() == T.sample_slot(pos, q, b, 2, 18, seed=9)[1].tolist()


def test_positive_picks_are_uniform(maps):
    """Route query 150 has 8 positives; over seeds 0..3999 in slot 3 with num_pos = 2 every positive is picked about 1000
    times: Pearson's statistic against the uniform expectation stays below 24.3, the 99.9 % point of chi-square with 7
    degrees of freedom (deterministic: 7.9 with stream 11 as the header specifies it)."""
    pos, d, _ = maps["route"]
    positives = d[150]["positives"]
    assert len(positives) == 8
    hits = dict.fromkeys(positives, 0)
    for seed in range(4000):
        for j in T.sample_slot(pos, 150, 3, 2, 18, other_neg=False, seed=seed)[0]:
            hits[int(j)] += 1
    expect = 4000 * 2 / 8
    stat = sum((c - expect) ** 2 / expect for c in hits.values())
    print("chi-square %.2f" % stat)
    assert stat < 24.3, stat
