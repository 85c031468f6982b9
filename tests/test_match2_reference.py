"""CPU: the numpy restatement behind the dh3d_match_descriptors2 tests (tests/match2_reference.py) -- it agrees with the
float64 reference where that one is decisive, the screen's bound E of csrc/match.hip holds on every builder, ties,
duplicates and single candidates come out as the contract says, and on the planted fixture the filters do not lose
precision."""
import numpy as np
import pytest

import match2_reference as m2
import registration_reference as ref

F = np.float32


def _builders():
    rng = np.random.default_rng(3)
    yield "unit D=4", m2.unit(rng, 192, 4), m2.unit(rng, 200, 4)
    a = m2.unit(rng, 192, 128)
    b = m2.unit(rng, 200, 128)
    b[:96] = a[:96] + (0.05 * rng.standard_normal((96, 128))).astype(F)
    yield "unit D=128 with true matches", a, b
    yield "unit D=256", m2.unit(rng, 128, 256), m2.unit(rng, 130, 256)
    yield "fpfh-like", m2.fpfh_like(rng, 192), m2.fpfh_like(rng, 200)
    yield ("shared offset",) + m2.shared_offset(rng, 160, 128)
    yield ("all equal",) + m2.all_equal(40, 36)
    yield ("ulp neighbours",) + m2.ulp_neighbours(rng, 64, 36)
    yield ("duplicates",) + m2.with_duplicates(rng, 64, 128)


def test_rule_agrees_with_float64_reference():
    rng = np.random.default_rng(0)
    for D in (4, 36, 128):
        a, b = m2.unit(rng, 300, D), m2.unit(rng, 257, D)
        got = m2.match2(a, b, 300, 257)
        ids, best, rel = ref.match(a, b)
        clear = rel > 1e-5
        assert clear.sum() > 250
        assert (got["nn1"][clear] == ids[clear]).all()
        assert np.abs(got["dist1"] - best).max() < 1e-5
        # the reverse direction is the same search with the roles swapped
        ids_r, best_r, rel_r = ref.match(b, a)
        clear = rel_r > 1e-5
        assert (got["rev"][clear] == ids_r[clear]).all() and np.abs(got["rev_dist"] - best_r).max() < 1e-5
        swapped = m2.match2(b, a, 257, 300)
        assert (swapped["nn1"] == got["rev"]).all() and (swapped["s1"] == got["rev_s"]).all()


def test_screen_error_is_within_the_bound():
    worst = {}
    for name, a, b in _builders():
        S = m2.rule_sums(a, b).astype(np.float64)
        s, E = m2.screen(a, b)
        ratio = float((np.abs(s.astype(np.float64) - S) / E.astype(np.float64)).max())
        worst[name] = ratio
        print("%-32s max |s - rule| / E = %.4f" % (name, ratio))
        assert ratio <= 1.0, (name, ratio)
        # what the kernel relies on, after the roundings of the tests themselves
        assert ((s - E).astype(F) <= S).all() and ((s + E).astype(F) >= S).all(), name
    print("largest ratio: %.4f (%s)" % (max(worst.values()), max(worst, key=worst.get)))


def test_survivors_per_row_are_few_except_under_cancellation():
    """How many pairs the screen cannot exclude against the row's final second-best rule value."""
    for name, a, b in _builders():
        S = m2.rule_sums(a, b)
        s, E = m2.screen(a, b)
        second = np.sort(S, axis=1)[:, 1]
        n = ((s - E).astype(F) <= second[:, None]).sum(1)
        print("%-32s survivors per row: mean %.1f max %d of %d" % (name, n.mean(), n.max(), S.shape[1]))
        assert (n >= 2).all(), name
        if name.startswith("unit") or name == "fpfh-like":
            assert n.mean() < 4.0, (name, n.mean())


def test_ties_duplicates_and_single_candidates():
    rng = np.random.default_rng(1)
    a, b = m2.with_duplicates(rng, 64, 128)
    r = m2.match2(a, b, 64, 64, ratio=1.0)
    assert (r["nn1"][:4] == [5, 20, 20, 7]).all() and (r["nn2"][:3] == [9, 21, 21]).all()
    assert (r["s1"][:3] == r["s2"][:3]).all() and r["s1"][2] == 0.0 and r["s1"][3] == 0.0
    assert (r["match"][:3] == -1).all() and r["match"][3] == 7          # ratio 1: exact ties are rejected, a clear best is kept
    assert (m2.match2(a, b, 64, 64)["match"][:4] == [5, 20, 20, 7]).all()
    assert r["rev"][30] == 2 and r["rev"][20] == 2 and r["rev"][21] == 2 and r["rev"][7] == 3
    mu = m2.match2(a, b, 64, 64, mutual=True)
    assert mu["match"][2] == 20 and mu["match"][3] == 7 and mu["match"][1] == -1   # positive 20 prefers anchor 2 (S = 0)
    # one candidate: kept whatever the ratio; no second neighbour
    r = m2.match2(a, b, 64, 1, ratio=0.5, mutual=False)
    assert (r["nn1"] == 0).all() and (r["nn2"] == -1).all() and np.isinf(r["dist2"]).all() and (r["match"] == 0).all()
    assert r["rev"][0] == r["s1"].argmin() and (r["rev"][1:] == -1).all() and r["num_kept"] == 64
    # no candidate, no anchor, counts beyond the rows
    r = m2.match2(a, b, 40, 0, ratio=0.9, mutual=True)
    assert (r["nn1"] == -1).all() and (r["match"] == -1).all() and np.isinf(r["dist1"]).all() and (r["rev"] == -1).all()
    r = m2.match2(a, b, 0, 50, mutual=True)
    assert (r["nn1"] == -1).all() and (r["rev"] == -1).all() and np.isinf(r["rev_dist"]).all() and r["num_kept"] == 0
    assert (m2.match2(a, b, 99, -3)["nn1"] == -1).all()
    # all rows equal: every S is 0, ids 0 and 1, the reverse id 0
    a, b = m2.all_equal(40, 36)
    r = m2.match2(a, b, 40, 40, ratio=1.0, mutual=True)
    assert (r["nn1"] == 0).all() and (r["nn2"] == 1).all() and (r["s2"] == 0).all() and (r["rev"] == 0).all()
    assert (r["match"] == -1).all()
    r = m2.match2(a, b, 40, 40, mutual=True)
    assert r["match"][0] == 0 and (r["match"][1:] == -1).all() and r["num_kept"] == 1
    # one ulp apart: the nearer id wins although a lower id is one ulp behind
    a, b = m2.ulp_neighbours(rng, 64, 36)
    r = m2.match2(a, b, 64, 64)
    k = np.round(b[:, 1] * 4096).astype(int)
    first = int(np.flatnonzero(k == k.min())[0])
    assert k[:3].tolist() == [3, 3, 3] and first >= 3 and (r["nn1"] == first).all()
    assert (r["s1"] == F(0.5625) + F(k.min() ** 2 * 2.0 ** -24)).all()


def test_planted_fixture_filters_do_not_lose_precision():
    rows_a, rows_b, truth, _ = m2.planted()
    a, b, truth = rows_a[0, :, 3:131], rows_b[0, :, 3:131], truth[0]
    orphans = int((truth < 0).sum())
    assert 150 < orphans < 260                       # the stated share: 0.4 of 512
    S = m2.rule_sums(a, b)
    plain = m2.match2(a, b, 512, 512, S=S)
    prec = lambda m: float((m[m >= 0] == truth[m >= 0]).mean())
    p0 = prec(plain["match"])
    assert plain["num_kept"] == 512 and 0.5 < p0 < 0.7
    for kw in (dict(ratio=0.9), dict(mutual=True), dict(ratio=0.9, mutual=True)):
        r = m2.match2(a, b, 512, 512, S=S, **kw)
        print(kw, "kept", r["num_kept"], "precision %.3f (unfiltered %.3f)" % (prec(r["match"]), p0))
        assert r["num_kept"] >= 200 and prec(r["match"]) >= p0, kw
    assert prec(m2.match2(a, b, 512, 512, S=S, ratio=0.9, mutual=True)["match"]) > 0.95
