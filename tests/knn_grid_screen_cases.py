"""Pass 0 of knn_grid_kernel (dh3d_amd/csrc/knn.hip) restated in numpy -- which candidates a query pools from its 27 inner
cells, whether it takes the screened drain, and the screen's threshold -- and the clouds of tests/test_knn_grid_screen_gpu.py,
so that tests/test_knn_grid_screen_host.py can hold those clouds to their premises without a GPU.

The rule (knn.hip, `drain_screened`), per query, L = 4 lanes:
  pool      every record of the 27 cells around the query's cell of the grid with D bits dropped (the first pass's box test
            passes every cell while the bound is infinite), T records in an order that changes from run to run;
  choice    a wave serves 16 consecutive queries of the sorted order and decides for all of them: it screens when every one
            of its pools fits the row next to its squared distances (T <= 80, kGridScreenCap; nothing overflowed kGridCap
            then) and some pool is longer than two trips of the old drain (T > 32).  Any other wave drains as before the
            screen;
  deal      lane l takes the slots l, l + L, ... of the pool;
  U         the largest over the lanes of a lane's second smallest squared distance (+inf for a lane with fewer than two,
            NaN never counted: a pool below 2 L is ranked whole);  thr = fl(U * 1.000001f);  the candidates with s <= thr
            are ranked, the others dropped.
The grid itself (origin, scale, schedule, crowded flag) comes from spatial_reference.restate, which is bit exact."""
import zlib

import numpy as np

import spatial_reference as R
from test_ops_gpu import _knn_clouds

F = np.float32
LANES = 4
SCREEN_CAP = 80
SCREEN_MIN = 32   # some pool of the wave must be longer
WAVE_QUERIES = 16
GRID_STEPS = 12


def grid_drop(n):
    """knn_grid_plan's D: one bit of the cell code less for every halving below 3072 points"""
    d = 0
    while d < 6 and (n << d) <= 3072:
        d += 1
    return d


def rank_code(ids, n):
    """the reference's CUB rank of a candidate id (knn_ladder + knn_offer)"""
    for top, t, v in ((32, 32, 1), (64, 64, 1), (128, 128, 1), (256, 128, 2), (512, 128, 4), (1024, 256, 4), (2048, 256, 8),
                      (4096, 512, 8), (8192, 1024, 8)):
        if n <= top:
            break
    else:
        t, v = 1024, (n + 1023) // 1024
    ids = np.asarray(ids, np.int64)
    return (ids & (t - 1)) * v + (ids >> (t.bit_length() - 1))


def sqdist(q, c):
    """query [3], candidates [M, 3] -> float32 [M]: the kernel's chain fma(dz, dz, fma(dy, dy, dx * dx)) (evaluated in float64
    and rounded once more per step: exact wherever the terms are, e.g. on lattices)"""
    d = (c.astype(F) - q.astype(F)[None, :]).astype(np.float64)
    s = (d[:, 0] * d[:, 0]).astype(F).astype(np.float64)
    s = (d[:, 1] * d[:, 1] + s).astype(F).astype(np.float64)
    return (d[:, 2] * d[:, 2] + s).astype(F)


def keys(s, ids, n):
    """the 64-bit (bits of the rounded distance, rank code) keys the kernel orders candidates by"""
    return (np.sqrt(s.astype(F)).view(np.uint32).astype(np.uint64) << np.uint64(32)) | rank_code(ids, n).astype(np.uint64)


def coarse_cells(xyz, drop):
    """one cloud -> (cell [N, 3] of the grid with `drop` bits left out, cells per axis [3], the sort's crowded flag, the sorted
    order [N])"""
    r = R.restate(xyz)
    axes = R.step_axes(r["sched"])[:GRID_STEPS - drop]
    nc = [axes.count(a) for a in range(3)]
    cell = np.stack([r["q"][:, a] >> (2 + r["nb"][a] - nc[a]) for a in range(3)], 1)
    return cell, [1 << b for b in nc], int(r["cells"][4106]), r["order"]


def pool_sizes(cell, dims):
    """T per query: the records in the 3 x 3 x 3 cells around its own (cells outside the grid hold nothing)"""
    h = np.zeros([d + 2 for d in dims], np.int64)
    np.add.at(h, (cell[:, 0] + 1, cell[:, 1] + 1, cell[:, 2] + 1), 1)
    box = np.zeros(dims, np.int64)
    for ox in range(3):
        for oy in range(3):
            for oz in range(3):
                box += h[ox:ox + dims[0], oy:oy + dims[1], oz:oz + dims[2]]
    return box[cell[:, 0], cell[:, 1], cell[:, 2]]


def screened(t, order):
    """pool sizes [N] and the sorted order -> bool [N]: does the query's wave take the screened drain?"""
    n = len(t)
    ts = np.zeros(-(-n // WAVE_QUERIES) * WAVE_QUERIES, np.int64)   # (the slots past N pool nothing)
    ts[:n] = t[order]
    ts = ts.reshape(-1, WAVE_QUERIES)
    wave = (ts <= SCREEN_CAP).all(1) & (ts > SCREEN_MIN).any(1)
    out = np.empty(n, bool)
    out[order] = np.repeat(wave, WAVE_QUERIES)[:n]
    return out


def pool_of(cell, qi):
    """ids of query qi's pool, ascending"""
    return np.flatnonzero((np.abs(cell - cell[qi][None, :]) <= 1).all(1))


def threshold(s_dealt):
    """s in pool order (slot i goes to lane i % L) -> (U, thr), float32"""
    u = F(-np.inf)
    for lane in range(LANES):
        mine = s_dealt[lane::LANES]
        mine = np.sort(mine[~np.isnan(mine)])
        u = max(u, mine[1] if len(mine) >= 2 else F(np.inf))
    u = F(u)
    with np.errstate(over="ignore"):
        return u, F(u * F(1.000001))


# ------------------------------------------------------------------------------------------------ the clouds
# Two candidates whose squared distances differ by one unit of 2^-32 and whose square roots round to the same float32
# (tests/test_knn_small_screen_gpu.py's pair, scaled by 1/16 so that both lie inside the query's 27 cells; every term of the
# chain stays exact on the 2^-16 lattice).  The reference orders them by (distance, rank code): the lower rank code wins.
COLLAPSE_A = np.array([1200, 1264, 1173], np.int64)   # s * 2^32 = 4413625
COLLAPSE_B = np.array([2045, 465, 124], np.int64)     # s * 2^32 = 4413626
COLLAPSE_NEAR = np.array([[-200, 150, 80], [300, -100, 50], [-350, -50, -120], [100, 200, -300], [-150, 330, -260],
                          [60, -400, 210]], np.int64)   # nearest first
COLLAPSE_SITES = 6   # site j: records 9 j .. 9 j + 8 = the query, six nearer points, the pair (B first at even j)


def collapse_site(j):
    return np.array([13000 + 7000 * j, 52000 - 6500 * j, 20000 + 4100 * ((3 * j) % 7)], np.int64)   # units of 2^-16


def _collapse(n, rng):
    pts = rng.random((n, 3), dtype=F)
    sites = np.stack([collapse_site(j) for j in range(COLLAPSE_SITES)]).astype(np.float64) / 65536
    while True:   # nothing else within 0.045 of a site: the pair (at 0.032) is the 8th and 9th neighbour
        near = (np.linalg.norm(pts[:, None, :].astype(np.float64) - sites[None], axis=2) < 0.045).any(1)
        if not near.any():
            break
        pts[near] = rng.random((int(near.sum()), 3), dtype=F)
    for j in range(COLLAPSE_SITES):
        q = collapse_site(j)
        pair = [COLLAPSE_B, COLLAPSE_A] if j % 2 == 0 else [COLLAPSE_A, COLLAPSE_B]
        block = np.concatenate([[q], q + COLLAPSE_NEAR, [q + pair[0]], [q + pair[1]]])
        pts[9 * j:9 * j + 9] = (block.astype(np.float64) / 65536).astype(F)
    return pts


def _many_copies(n, rng):
    """groups of 9..12 identical points in a uniform cloud; the groups come in threes a hundredth apart, so the pools around
    them are past the screened drain's 80 as well: copies on both drains"""
    pts = rng.random((n, 3), dtype=F)
    at = 0
    for trio in range(12):
        c = (rng.random(3, dtype=F) * F(0.8) + F(0.1)).astype(F)
        for g in range(3 if trio < 4 else 1):
            size = 9 + (trio + g) % 4
            pts[at:at + size] = c + F(0.01) * F(g)
            at += size
    return pts[rng.permutation(n)]


def _dense_cell(n, rng):
    """about 400 points in one cell of the 16^3 grid (a twentieth wide, around the centre of cell 8, 8, 8): pools around it
    overflow kGridCap, the cloud as a whole is nowhere near crowded"""
    pts = rng.random((n, 3), dtype=F)
    pts[:400] = F(0.53125) + (rng.random((400, 3), dtype=F) - F(0.5)) * F(0.05)
    return pts[rng.permutation(n)]


def _margin(n, rng):
    """a uniform cube and 40 points scattered up to 0.06 outside it: the grid stretches to them, the cube's cells hold a third more
    (pools past 80 beside screened ones) -- `outliers` itself is flagged crowded and never gets here"""
    pts = rng.random((n, 3), dtype=F)
    pts[:40] = rng.random((40, 3), dtype=F) * F(1.12) - F(0.06)
    return pts[rng.permutation(n)]


MAKERS = {"collapse": _collapse, "many_copies": _many_copies, "dense_cell": _dense_cell, "margin": _margin}


def cloud(kind, n, rng):
    if kind in MAKERS:
        return MAKERS[kind](n, rng)
    return _knn_clouds(kind, 1, n, rng)[0]


# id: (N, Ks, per-cloud kinds, per-cloud crowded flags, plan code: the knn_grid_kernel<4, code> that serves the batch)
CASES = {
    "uniform_d0": (8192, (8, 5), ("uniform",) * 2, (0, 0), 4),
    "uniform_d1": (3000, (1, 3), ("uniform",) * 3, (0, 0, 0), 4),
    "uniform_d3": (700, (8,), ("uniform",) * 2, (0, 0), 4),
    "lattice_8192": (8192, (8, 4), ("lattice",), (0,), 4),
    "lattice_4096": (4096, (8, 4), ("lattice",), (0,), 4),
    "duplicates": (8192, (8,), ("duplicates",), (0,), 4),
    "many_copies": (8192, (8,), ("many_copies",), (0,), 4),
    "collapse": (8192, (8,), ("collapse",), (0,), 4),
    "dense_cell": (8192, (8,), ("dense_cell",), (0,), 4),
    "margin": (8192, (8,), ("margin",), (0,), 4),
    "plane": (8192, (8,), ("plane",), (0,), 4),
    "oxford_extent": (8192, (8,), ("oxford_extent",) * 2, (0, 0), 4),
    "tiny_5": (5, (8,), ("uniform",), (0,), 4),
    "tiny_7": (7, (8,), ("uniform",), (0,), 4),
    "tiny_9": (9, (8,), ("uniform",), (0,), 4),
    "mixed_6x8192": (8192, (8,), ("scene", "uniform") * 3, (1, 0) * 3, 4),
    "uniform_code2": (4096, (8,), ("uniform",) * 21, (0,) * 21, 2),
    "uniform_code0": (4096, (5,), ("uniform",) * 66, (0,) * 66, 0),
}


def batch(case):
    """float32 [B, N, 3]; the seed depends on the case alone"""
    n, _, kinds, _, _ = CASES[case]
    rng = np.random.default_rng(zlib.crc32(repr(("knn_grid_screen", case)).encode()))
    return np.ascontiguousarray(np.stack([cloud(k, n, rng) for k in kinds]))
