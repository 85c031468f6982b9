"""Pass 1 of knn_grid_kernel (dh3d_amd/csrc/knn.hip) restated in numpy -- which cells a query looks at after its 27 inner cells
-- and the clouds of tests/test_knn_grid_box_gpu.py, so that tests/test_knn_grid_box_host.py can hold the premise of the cell-set
rule, and the GPU cases the regimes they are there for, without a GPU.

The rule, per query, on the grid with D bits dropped (knn_grid_screen_cases.coarse_cells):
  bound     the K-th smallest distance among the records of the 27 cells around the query's own (the query included); none
            when they hold fewer than K;
  box       the cells the ball of r = bound * 1.0001 meets, per axis, clipped to the grid, as offsets [lo, hi] from the query's
            cell (lo <= 0 <= hi); without a bound: the +-2 block, clipped;
  wide      a box of more than BOX_CELLS = 640 cells: nothing is enumerated, the query restarts over the 64-point groups;
  set       the cells of the box outside its inner block [max(lo, -1), min(hi, 1)]^3: the only cells whose ranges pass 1 looks
            up.  Empty: the query does nothing in pass 1;
  waves     16 consecutive queries of the sorted order share a wave: one whose sets are all empty skips pass 1 whole.
The rule it replaced walked every (dy, dz) column of the box -- all 25 of the +-2 block without a bound, with a ball wider than
+-2 in x or a box of more than 128 columns -- and asked for the ranges of 2 cells (dx = -2, 2) per column with |dy|, |dz| <= 1 and
of 5 per other column, columns outside the grid skipped.  `columns` and `ranges_old` count that.
The distances here are float64: a query within a rounding of a cell face may fall the other way on the device.  The tests only
count regimes."""
import zlib

import numpy as np

import knn_grid_screen_cases as S
from test_ops_gpu import _knn_clouds

F = np.float32
BOX_CELLS = 640
POOL_CAP = 256   # kGridCap
WAVE_QUERIES = 16


def pass0_bound(xyz, cell, dims, K):
    """float64 [N]: the K-th distance within the 27 cells (inf: fewer than K there).  Cell by cell: its queries share a pool."""
    n = len(xyz)
    p = xyz.astype(np.float64)
    lin = (cell[:, 0] * dims[1] + cell[:, 1]) * dims[2] + cell[:, 2]
    order = np.argsort(lin, kind="stable")
    first = np.searchsorted(lin[order], np.arange(dims[0] * dims[1] * dims[2] + 1))
    out = np.full(n, np.inf)
    for c in np.unique(lin):
        cz, cy, cx = c % dims[2], c // dims[2] % dims[1], c // (dims[1] * dims[2])
        pool = []
        for ax in range(max(cx - 1, 0), min(cx + 2, dims[0])):
            for ay in range(max(cy - 1, 0), min(cy + 2, dims[1])):
                z0, z1 = max(cz - 1, 0), min(cz + 1, dims[2] - 1)   # (consecutive z: one contiguous run of the order)
                a = (ax * dims[1] + ay) * dims[2]
                pool.append(order[first[a + z0]:first[a + z1 + 1]])
        pool = np.concatenate(pool)
        if len(pool) < K:
            continue
        qs = order[first[c]:first[c + 1]]
        d = np.linalg.norm(p[qs][:, None, :] - p[pool][None, :, :], axis=2)
        out[qs] = np.partition(d, K - 1, axis=1)[:, K - 1]
    return out


def restate(xyz, K, drop):
    """one cloud -> dict of per-query arrays (original point order) and the grid"""
    cell, dims, flag, order = S.coarse_cells(xyz, drop)
    r = S.R.restate(xyz)
    dims = np.array(dims)
    width = r["ext"].astype(np.float64) / dims   # (ext: the grid's extent per axis)
    lo0 = r["lo"].astype(np.float64)
    bound = pass0_bound(xyz, cell, dims, K)
    have = np.isfinite(bound)
    rad = np.where(have, bound, 0.0) * 1.0001
    p = xyz.astype(np.float64)
    lo = np.clip(np.floor((p - rad[:, None] - lo0) / width).astype(np.int64), 0, dims - 1) - cell
    hi = np.clip(np.floor((p + rad[:, None] - lo0) / width).astype(np.int64), 0, dims - 1) - cell
    lo, hi = np.minimum(lo, 0), np.maximum(hi, 0)
    lo[~have] = np.maximum(-2, -cell[~have])
    hi[~have] = np.minimum(2, dims - 1 - cell[~have])
    b = hi - lo + 1
    inner = np.minimum(hi, 1) - np.maximum(lo, -1) + 1
    wide = have & (b.prod(1) > BOX_CELLS)
    ncell = np.where(wide, 0, b.prod(1) - inner.prod(1))
    # the column rule this one replaced
    by_box = have & (lo[:, 0] >= -2) & (hi[:, 0] <= 2) & (b[:, 1] * b[:, 2] <= 128)
    ylo = np.where(by_box, lo[:, 1], np.maximum(-2, -cell[:, 1]))
    yhi = np.where(by_box, hi[:, 1], np.minimum(2, dims[1] - 1 - cell[:, 1]))
    zlo = np.where(by_box, lo[:, 2], np.maximum(-2, -cell[:, 2]))
    zhi = np.where(by_box, hi[:, 2], np.minimum(2, dims[2] - 1 - cell[:, 2]))
    columns = (yhi - ylo + 1) * (zhi - zlo + 1)
    inner_cols = (np.minimum(yhi, 1) - np.maximum(ylo, -1) + 1) * (np.minimum(zhi, 1) - np.maximum(zlo, -1) + 1)
    ranges_old = 2 * inner_cols + 5 * (columns - inner_cols)
    return dict(cell=cell, dims=dims, flag=flag, order=order, bound=bound, lo=lo, hi=hi, wide=wide, ncell=ncell,
                columns=columns, ranges_old=ranges_old, lo0=lo0, width=width)


def wave_cells(st):
    """cells of the set per wave of 16 queries of the sorted order"""
    n = len(st["ncell"])
    c = np.zeros(-(-n // WAVE_QUERIES) * WAVE_QUERIES, np.int64)
    c[:n] = st["ncell"][st["order"]]
    return c.reshape(-1, WAVE_QUERIES).sum(1)


def pass1_pool(xyz, st, qi):
    """records query qi pools in pass 1: those of the cells of its set whose box lies within its bound (all, without one)"""
    cell, dims = st["cell"], st["dims"]
    if st["wide"][qi] or st["ncell"][qi] == 0:
        return 0
    d = cell - cell[qi]
    in_box = ((d >= st["lo"][qi]) & (d <= st["hi"][qi])).all(1) & (np.abs(d) > 1).any(1)
    c0 = st["lo0"] + cell * st["width"]
    q = xyz[qi].astype(np.float64)
    gap = np.maximum(np.maximum(c0 - q, q - (c0 + st["width"])), 0.0)
    return int((in_box & (np.linalg.norm(gap, axis=1) <= st["bound"][qi])).sum())


def regimes(st):
    """counts of the queries of one cloud by what pass 1 does with them"""
    have = np.isfinite(st["bound"])
    return dict(empty=int((have & ~st["wide"] & (st["ncell"] == 0)).sum()),
                nonempty=int((st["ncell"] > 0).sum()),
                no_kth=int((~have).sum()),
                wide=int(st["wide"].sum()))


# ------------------------------------------------------------------------------------------------ the clouds
def _outside(lo, hi, n, rng):
    """n uniform points of the unit cube outside the box [lo, hi)"""
    out = np.empty((0, 3), F)
    while len(out) < n:
        p = rng.random((2 * n + 16, 3), dtype=F)
        out = np.concatenate([out, p[~((p >= lo) & (p < hi)).all(1)]])
    return out[:n]


HOLE_CELLS = ([(x, y, z) for x in (0, 15) for y in (0, 15) for z in (0, 15)]                      # the grid's corners
              + [(0, 0, 7), (0, 15, 8), (15, 0, 6), (15, 15, 9), (0, 7, 0), (0, 8, 15), (15, 6, 0), (15, 9, 15),
                 (7, 0, 0), (8, 0, 15), (6, 15, 0), (9, 15, 15)]                                   # its edges
              + [(0, 5, 10), (15, 10, 5), (5, 0, 11), (11, 15, 4), (4, 11, 0), (10, 4, 15)]        # its faces
              + [(4, 4, 4), (4, 8, 12), (8, 12, 4), (12, 4, 8), (12, 12, 12), (8, 4, 11), (3, 12, 8), (11, 8, 2),
                 (7, 7, 7), (2, 3, 13), (13, 2, 3), (6, 13, 13), (9, 9, 3), (13, 7, 12)])          # inside
assert len(HOLE_CELLS) == 40


CORNERS = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], F)


def _holes(n, rng):
    """a uniform cube; around each of 40 cells of its 16^3 grid the points of the 27-cell neighbourhood are taken out and
    scattered again over the cube, all but m = 0 / 3 / 8 of them.  m = 3: they go into the middle cell -- queries with fewer
    than K records in their 27 cells (the +-2 block, then the restart); m = 8: one in the middle of the middle cell and seven
    1.2 cells off along the diagonals -- its K-th distance after pass 0 is 2.08 cells, two or more cells away in every
    direction; and everywhere queries beside a hole, boxes clipped at the border"""
    pts = rng.random((n, 3), dtype=F)
    for i, c in enumerate(HOLE_CELLS):
        m = (0, 3, 8)[i % 3]
        lo, hi = (np.array(c, F) - 1) / 16, (np.array(c, F) + 2) / 16
        move = np.flatnonzero(((pts >= lo) & (pts < hi)).all(1))
        pts[move] = _outside(lo, hi, len(move), rng)
        if m == 3:
            pts[move[:m]] = (np.array(c, F) + F(0.1) + F(0.8) * rng.random((m, 3), dtype=F)) / 16
        if m == 8:
            pts[move[:8]] = np.clip((np.array(c, F) + F(0.5) + F(1.2) * np.concatenate([np.zeros((1, 3), F), CORNERS[:7]])) / 16,
                                    0, F(0.999))
    return pts


def _slab(n, rng):
    return (rng.random((n, 3), dtype=F) * np.array([1, 1, 0.13], F)).astype(F)


OVERFLOW_QUERY = 0     # the record of _overflow's query
OVERFLOW_COPIES = 300


def _overflow(n, rng):
    """a uniform cube with the 27 cells around cell (8, 8, 8) emptied but for a query at its centre and seven points 1.2 cells
    off along the diagonals (its K-th distance after pass 0: 2.08 cells), and 300 copies of one point 2 cells from the query in
    x: their cell belongs to its pass-1 set, lies within its bound and passes kGridCap -- the query goes to the restart"""
    w = F(1 / 16)
    lo, hi = np.full(3, 7 * w, F), np.full(3, 10 * w, F)
    pts = _outside(lo, hi, n, rng)
    q = np.full(3, 8.5 * w, F)
    pts[OVERFLOW_QUERY] = q
    pts[1:8] = q + CORNERS[:7] * F(1.2) * w
    pts[8:8 + OVERFLOW_COPIES] = q + np.array([2 * w, 0, 0], F)
    return pts


MAKERS = {"holes": _holes, "slab": _slab, "overflow": _overflow}


def cloud(kind, n, rng):
    if kind in MAKERS:
        return MAKERS[kind](n, rng)
    return _knn_clouds(kind, 1, n, rng)[0]


# id: (N, Ks, per-cloud kinds, grid drop D, the regimes that must occur in cloud 0 at the first K: regimes()' keys)
CASES = {
    "uniform_2x4096": (4096, (8, 3), ("uniform",) * 2, 0, ("nonempty", "empty")),
    "uniform_3x8192": (8192, (8, 1), ("uniform",) * 3, 0, ("empty", "nonempty")),
    "holes_2x8192": (8192, (8,), ("holes",) * 2, 0, ("empty", "nonempty", "no_kth")),
    "slab_2x8192": (8192, (8,), ("slab",) * 2, 0, ("empty", "nonempty")),
    "lattice_2x4096": (4096, (8,), ("lattice",) * 2, 0, ("nonempty",)),
    "duplicates_2x4096": (4096, (8,), ("duplicates",) * 2, 0, ("nonempty",)),
    "coarse_4x700": (700, (8,), ("uniform",) * 4, 3, ("nonempty",)),
    "coarse_6x300": (300, (8,), ("uniform",) * 6, 4, ("nonempty",)),
    "coarse_2x5": (5, (8,), ("uniform",) * 2, 6, ("no_kth",)),
    "overflow_1x8192": (8192, (8,), ("overflow",), 0, ("empty", "nonempty")),
}


def batch(case):
    """float32 [B, N, 3]; the seed depends on the case alone"""
    n, _, kinds, _, _ = CASES[case]
    rng = np.random.default_rng(zlib.crc32(repr(("knn_grid_box", case)).encode()))
    return np.ascontiguousarray(np.stack([cloud(k, n, rng) for k in kinds]))


def bench_cube(n):
    """the bench's cube (bench.synthetic_clouds' first cloud: rng.random, seed 2002)"""
    return np.random.default_rng(2002).random((n, 3), dtype=F)
