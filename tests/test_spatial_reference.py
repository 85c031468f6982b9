"""CPU: the numpy restatement of the spatial sort (tests/spatial_reference.py) against answers worked out by hand, and the
cases of the GPU test (tests/test_spatial_sort_gpu.py) against their own premises."""
import math
import time

import numpy as np
import pytest

import spatial_reference as R

F = np.float32


def _corners(size, n=200, seed=0):
    """A uniform cloud whose extents are exactly `size` (lo = 0)."""
    return R._box(n, np.random.default_rng(seed), size)


def _morton6(q):
    """The plain Morton code of three 6-bit values, z above y above x, written out bit by bit."""
    code = np.zeros(len(q), np.int64)
    for i in range(6):
        for a in range(3):
            code |= ((q[:, a] >> i) & 1) << (3 * i + a)
    return code


# ------------------------------------------------------------------------------------------------ known answers
def test_cube_is_the_plain_morton_code():
    # Equal widths: z is visited first and neither y nor x is > 1.25 x it -> z; then z is half as wide, y is > 1.25 x it and
    # x is not > 1.25 x y -> y; then x is the only axis twice as wide as the best -> x.  All three are halved: the same
    # again, four times.  Axes 2 1 0 2 1 0 ... in 2-bit fields, step 0 lowest: 0b000110 repeated = 0x186186.
    r = R.restate(_corners((40, 40, 40)))
    assert r["sched"] == 0x186186 == R.SCHED_CUBE and r["nb"] == [4, 4, 4]
    assert R.step_axes(r["sched"]) == [2, 1, 0] * 6
    assert np.array_equal(r["scale"], np.full(3, 64 / 40, F))
    assert np.array_equal(r["code"], _morton6(r["q"])) and r["q"].max() == 63 and r["code"].max() < 1 << 18


def test_36_36_8_by_hand():
    # widths (x, y, z), every step visits z, y, x; "y" = y beats z, "x" = x beats the best so far, both by > 1.25 x:
    #  0: (36, 36, 8)        z 8; y 36 > 10; x 36 > 45 no             -> y
    #  1: (36, 18, 8)        z 8; y 18 > 10; x 36 > 22.5              -> x
    #  2: (18, 18, 8)        z 8; y 18 > 10; x 18 > 22.5 no           -> y
    #  3: (18, 9, 8)         z 8; y 9 > 10 no; x 18 > 10              -> x
    #  4: (9, 9, 8)          z 8; y 9 > 10 no; x 9 > 10 no            -> z
    #  5: (9, 9, 4)          z 4; y 9 > 5; x 9 > 11.25 no             -> y
    #  6: (9, 4.5, 4)        z 4; y 4.5 > 5 no; x 9 > 5               -> x
    #  7: (4.5, 4.5, 4)      z 4; y 4.5 > 5 no; x 4.5 > 5 no          -> z
    #  8: (4.5, 4.5, 2)      z 2; y 4.5 > 2.5; x 4.5 > 5.625 no       -> y
    #  9: (4.5, 2.25, 2)     z 2; y 2.25 > 2.5 no; x 4.5 > 2.5        -> x
    # 10: (2.25, 2.25, 2)    z 2; y 2.25 > 2.5 no; x 2.25 > 2.5 no    -> z
    # 11: (2.25, 2.25, 1)    z 1; y 2.25 > 1.25; x 2.25 > 2.8125 no   -> y
    # x 4, y 5, z 3 bits: 16 x 32 x 8 cells of 2.25 x 1.125 x 1.  (Not 5 + 5 + 2: inside the tie band the axis visited
    # first keeps the bit, so y runs one bit ahead of x and z joins as soon as x and y are within 25 % of it.)
    steps = [1, 0, 1, 0, 2, 1, 0, 2, 1, 0, 2, 1]
    sched, nb, width = R.deal_grid_bits(np.array([36, 36, 8], F))
    assert [(sched >> (2 * s)) & 3 for s in range(12)] == steps and sched == sum(a << (2 * s) for s, a in enumerate(steps))
    assert nb == [4, 5, 3] and np.array_equal(width, np.array([2.25, 1.125, 1], F))
    r = R.restate(_corners((36, 36, 8)))
    assert r["sched"] == sched and np.array_equal(r["scale"], np.array([64, 128, 32], F) / np.array([36, 36, 8], F))
    # the code: 18 steps from the top bit, every step the next most significant bit of its axis' nb + 2
    q = r["q"][:1]
    bits = {0: format(int(q[0, 0]), "06b"), 1: format(int(q[0, 1]), "07b"), 2: format(int(q[0, 2]), "05b")}
    took, word = {0: 0, 1: 0, 2: 0}, ""
    for a in steps + [2, 1, 0, 2, 1, 0]:
        word += bits[a][took[a]]
        took[a] += 1
    assert int(word, 2) == int(r["code"][0])


def test_slab_and_tall_by_hand():
    # 60 x 60 x 6, widths (x, y, z) before every step and who beats whom by > 1.25 x:
    #  0: (60, 60, 6) y beats z, x 60 > 75 no -> y     1: (60, 30, 6) x 60 > 37.5 -> x       2: (30, 30, 6) -> y
    #  3: (30, 15, 6) x 30 > 18.75 -> x                4: (15, 15, 6) -> y                   5: (15, 7.5, 6) y 7.5 > 7.5 no -> x
    #  6: (7.5, 7.5, 6) nobody beats z -> z            7: (7.5, 7.5, 3) y; x 7.5 > 9.375 no -> y
    #  8: (7.5, 3.75, 3) y 3.75 > 3.75 no; x -> x      9: (3.75, 3.75, 3) -> z              10: (3.75, 3.75, 1.5) -> y
    # 11: (3.75, 1.875, 1.5) y 1.875 > 1.875 no; x -> x.         5 + 5 + 2: 32 x 32 x 4 cells of 1.875 x 1.875 x 1.5
    steps = lambda sched: "".join("xyz"[(sched >> (2 * s)) & 3] for s in range(12))
    sched, nb, width = R.deal_grid_bits(np.array([60, 60, 6], F))
    assert steps(sched) == "yxyxyxzyxzyx" and nb == [5, 5, 2] and np.array_equal(width, np.array([1.875, 1.875, 1.5], F))
    sched8, nb8, _ = R.deal_grid_bits(np.array([60, 60, 8], F))      # the 60 x 60 x 8 slab of DESIGN.md: the same deal
    assert sched8 == sched and nb8 == [5, 5, 2]
    # 1 x 1 x 100: z stays the widest (100 ... 3.125 against 1) until it holds 6 bits; then y (visited first), x 1 > 0.625,
    # y 0.5 against x 0.5 ... alternating
    sched, nb, width = R.deal_grid_bits(np.array([1, 1, 100], F))
    assert steps(sched) == "zzzzzzyxyxyx" and nb == [3, 3, 6] and np.array_equal(width, np.array([.125, .125, 1.5625], F))


def test_the_tie_band_is_not_strict():
    # (1, 1.25, 1): z 1; y 1.25 > 1.25 no; x no -> z.  (1, 1.25, .5): y 1.25 > .625; x 1 > 1.5625 no -> y.
    # (1, .625, .5): y .625 > .625 no; x 1 > .625 -> x.  Everything is half of the start, exactly: the cube's schedule.
    sched, nb, _ = R.deal_grid_bits(np.array([1, 1.25, 1], F))
    assert sched == R.SCHED_CUBE and nb == [4, 4, 4]
    # one ulp over: y 1.25+ > 1.25 -> y first; then (1, .625+, 1) -> z; then (1, .625+, .5): y > .625, x 1 > .78 -> x;
    # again halves of the start: y z x four times
    sched, nb, _ = R.deal_grid_bits(np.array([1, R.TIE_OVER, 1], F))
    assert [(sched >> (2 * s)) & 3 for s in range(12)] == [1, 2, 0] * 4 and nb == [4, 4, 4] and sched != R.SCHED_CUBE
    rng = np.random.default_rng(1)
    assert R.restate(R.cloud("tie125", 500, rng))["sched"] == R.SCHED_CUBE
    assert R.restate(R.cloud("tie125_over", 500, rng))["sched"] != R.SCHED_CUBE


def test_line_takes_six_bits_then_the_cap():
    # y and z have width 0: x wins (anything > 0) until it holds 6 bits; then z is visited first and y's 0 is not > 0
    r = R.restate(R.cloud("line", 300, np.random.default_rng(2)))
    assert R.step_axes(r["sched"])[:12] == [0] * 6 + [2] * 6 and r["nb"] == [6, 0, 6]
    assert np.all(r["q"][:, 1:] == 0) and r["q"][:, 0].max() == 255
    assert np.all(np.diff(r["q"][r["order"], 0]) >= 0)    # x's 8 bits are the code's top 6 and bits 3 and 0: order = x's cell
    assert r["scale"][1] == F(4) / F(1e-30) and r["scale"][2] == F(256) / F(1e-30)


def test_single_repeated_point():
    n = 300
    r = R.restate(R.cloud("one_point", n, np.random.default_rng(3)))
    assert r["nb"] == [0, 6, 6] and R.step_axes(r["sched"])[:12] == [2] * 6 + [1] * 6      # z to its cap, then y
    assert r["occupied"] == 1 and np.all(r["code"] == 0) and np.array_equal(r["order"], np.arange(n))
    assert r["cells"][0] == 0 and np.all(r["cells"][1:4097] == n)
    assert r["cells"][4106] == 1 and r["cells"][4107] == r["sched"]
    assert np.array_equal(r["gbox"][:, 0:3], r["gbox"][:, 4:7]) and np.all(r["gbox"][:, [3, 7]] == 0)


def test_below_the_clamp_everything_is_cell_zero():
    r = R.restate(R.cloud("tiny", 300, np.random.default_rng(4)))
    assert np.array_equal(r["ext"], np.full(3, np.ldexp(F(255), -124))) and np.all(r["ext"] < F(1e-30)) and np.all(r["ext"] > 0)
    assert r["sched"] == R.SCHED_CUBE and np.array_equal(r["scale"], np.full(3, F(64) / F(1e-30)))
    assert np.all(r["code"] == 0) and np.array_equal(r["order"], np.arange(300)) and not R.has_denormal(r)


# ------------------------------------------------------------------------------------------------ quantisation edges
@pytest.mark.parametrize("kind,top,step", [("lattice", (64, 64, 64), (1, 1, 1)), ("lattice_slab", (128, 64, 16), (1, 1, .5))])
def test_boundary_points_land_in_the_upper_cell_and_the_maximum_is_clipped(kind, top, step):
    p = R.cloud(kind, 2000, np.random.default_rng(5))
    r = R.restate(p)
    assert np.array_equal(r["ext"], np.array(top, F)) and np.array_equal(r["scale"], F(1) / np.array(step, F))
    steps = p / np.array(step, F)                           # exact: every coordinate is a whole number of steps
    assert np.array_equal(steps, np.trunc(steps))
    qmax = np.array([(4 << b) - 1 for b in r["nb"]])
    assert np.array_equal(qmax + 1, np.array(top) / np.array(step))
    assert np.array_equal(r["q"], np.minimum(steps.astype(np.int64), qmax[None, :]))   # k steps -> cell k, the upper one
    for a in range(3):                                       # the maximum quantises to 2^(nb + 2): only the clip holds it
        assert (steps[:, a] == qmax[a] + 1).any() and r["q"][steps[:, a] == qmax[a] + 1, a].min() == qmax[a]
    if kind == "lattice":
        assert r["sched"] == R.SCHED_CUBE
    else:
        assert r["nb"] == [5, 4, 3]


@pytest.mark.parametrize("kind", ["cube", "slab", "negative", "far_slab"])
def test_the_maximum_lands_in_the_last_cell(kind):
    r = R.restate(R.cloud(kind, 777, np.random.default_rng(6)))
    for a in range(3):
        assert r["q"][:, a].min() == 0 and r["q"][:, a].max() == (4 << r["nb"][a]) - 1
    top = np.array([r["records"][:, a].max() for a in range(3)], F)
    assert np.array_equal(R.quantise(top[None, :], r["lo"], r["scale"], r["nb"])[0], [(4 << b) - 1 for b in r["nb"]])


# ------------------------------------------------------------------------------------------------ order, boxes, table
@pytest.mark.parametrize("kind,n", [("twice", 1000), ("two_points", 333), ("lattice", 3000), ("slab", 130)])
def test_order_is_stable_and_outputs_follow_their_definitions(kind, n):
    p = R.cloud(kind, n, np.random.default_rng(7))
    r = R.restate(p)
    code, order = r["code"], r["order"]
    assert order.tolist() == [i for _, i in sorted(zip(code.tolist(), range(n)))]          # (code, index), plainly
    same = np.diff(code[order]) == 0
    assert (same.any() or kind == "slab") and np.all(np.diff(order)[same] > 0)              # ties stay in index order
    if kind == "twice":     # the two copies of a point: equal codes, the earlier index first
        _, inv = np.unique(p, axis=0, return_inverse=True)
        pos = np.empty(n, np.int64)
        pos[order] = np.arange(n)
        for u in range(inv.max() + 1):
            i = np.flatnonzero(inv.ravel() == u)
            assert len(set(code[i].tolist())) == 1 and np.all(np.diff(pos[i]) > 0)
    assert np.array_equal(r["records"], p[order])
    for g in range((n + 63) // 64):
        blk = p[order[64 * g:64 * g + 64]]
        assert np.array_equal(r["gbox"][g], np.concatenate([blk.min(0), [0], blk.max(0), [0]]).astype(F))
    cell = (code[order] >> 6).tolist()
    table = [next((i for i, c in enumerate(cell) if c >= want), n) for want in range(4097)]
    assert r["cells"][:4097].tolist() == table and table[0] == 0 and table[4096] == n
    assert r["occupied"] == len(set(cell))
    assert r["cells"][4100:4103].view(F).tolist() == r["lo"].tolist()
    assert r["cells"][4103:4106].view(F).tolist() == r["scale"].tolist()


def test_restating_16384_points_is_quick():
    p = R.cloud("slab", 16384, np.random.default_rng(8))
    R.restate(p)
    t0 = time.perf_counter()
    R.restate(p)
    assert time.perf_counter() - t0 < 1.0


# ------------------------------------------------------------------------------------------------ the GPU test's cases
def test_flag_thresholds_are_clear_of_an_integer():
    """A last-bit difference between two exp() cannot move int(0.6 * 4096 * (1 - exp(-N / 4096))): for every N the GPU
    tests put through the rule the real value is farther than 1e-9 from an integer (its last bit is worth ~5e-13)."""
    sizes = set(R.SIZES) | {n for n, _ in R.FAR_CASES} | {R.FPS_M, 625, 1024}     # 512 / 625 / 1024: the sampled sets
    assert 8192 in sizes                                                          # 2125.0000079: the closest call, kept
    for n in sorted(sizes):
        t = 0.6 * 4096.0 * (1.0 - math.exp(-n / 4096.0))
        assert abs(t - round(t)) > 1e-9, (n, t)
        assert R.occupancy_threshold(n) == math.floor(t)
    assert abs(0.6 * 4096.0 * (1.0 - math.exp(-2.0)) - 2125.0000079) < 1e-6 and R.occupancy_threshold(8192) == 2125


def test_cases_cover_what_they_claim():
    cases = R.SORT_CASES
    assert {n for n, _ in cases} == set(R.SIZES) and all(1 <= len(ks) <= 4 for _, ks in cases)
    assert all(len(set(ks)) == len(ks) for _, ks in cases)                   # a batch mixes kinds
    for n in R.SIZES:
        kinds = {k for m, ks in cases if m == n for k in ks}
        assert "cube" in kinds and len(kinds - {"cube"}) >= 1, n
    for k in R.KINDS:
        ns = [n for n, ks in cases if k in ks]
        assert any(n <= 1024 for n in ns), k
        if k == "one_point":
            assert max(ns) <= 4096
        else:
            assert any(n > 4096 for n in ns), k
    # each of the five instantiations (N <= 1024, 2048, 4096, 8192, 16384) from both sides of its limit
    assert {1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384} <= set(R.SIZES)


@pytest.mark.parametrize("case", R.SORT_CASES + list(R.FAR_CASES), ids=R.case_id)
def test_case_premises(case):
    """No cloud of the GPU test touches a float32 denormal (the denormal mode stays out of the contract), every flag is
    decided by whole cells, and the kinds are what their names say at every size that can show it."""
    n, kinds = case
    batch = R.make_batch(case)
    assert np.array_equal(batch, R.make_batch(case))                         # the case alone decides the clouds
    for kind, p in zip(kinds, batch):
        r = R.restate(p)
        assert not R.has_denormal(r), kind
        # occupied and the threshold are integers: crowded means at least one whole cell short (trivially; held anyway)
        assert (r["threshold"] - r["occupied"] >= 1) if r["cells"][4106] else (r["occupied"] - r["threshold"] >= 0), kind
        assert np.array_equal(np.sort(r["order"]), np.arange(n)) and r["cells"][4096] == n
        if n >= 2 and kind in R.BOXES:
            want = np.array(R.BOXES[kind], F)
            if not kind.startswith("far_"):
                assert np.array_equal(r["ext"], want), kind
            cube = kind in ("cube", "tie125", "far_cube")
            assert (r["sched"] == R.SCHED_CUBE) == cube, kind                # both code paths of the kernel
        if kind.startswith("far_"):
            assert np.abs(p).max() > 50 * r["ext"].max() and r["cells"][4106] == 0   # far from the origin; cell lists
        if kind == "one_point":
            assert r["occupied"] == 1
        if kind == "two_points" and n >= 2:
            assert r["occupied"] == 2
        if kind == "plane":
            assert r["ext"][2] == 0 and r["nb"][2] == 0
        if kind == "negative":
            assert p.max() < 0
