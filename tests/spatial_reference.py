"""The spatial sort (dh3d_amd/csrc/spatial.hip) restated in numpy from the rule in its comments: no torch, no GPU, and no
Python loop over points.  Everything that decides an output is float32 min / max, one subtraction, one multiply, one
correctly rounded division, a truncation and comparisons against `* 1.25f` and `* 0.5f` -- all exact IEEE operations, all
done here in np.float32 -- so the restatement predicts every output BIT FOR BIT and nothing that uses it needs a tolerance.

The rule, per cloud of N <= 16384 points:
  1. lo = min, ext = max - min per axis.
  2. The 12 grid bits are dealt one at a time to the axis whose cells are currently the widest: the axes are visited z, y, x;
     a later axis wins only if its width is > 1.25f x the best so far; an axis takes at most 6 bits; the winner's width is
     halved.  sched holds the 12 winners, 2 bits each, step 0 in the low bits; nb[a] = grid bits of axis a.
  3. scale[a] = float32(4 << nb[a]) / max(ext[a], 1e-30f): every axis is quantised to nb + 2 bits.
  4. q[a] = clip(trunc((x[a] - lo[a]) * scale[a]), 0, (4 << nb[a]) - 1).
  5. The 18-bit code: the schedule is walked from the code's top bit down -- steps 0..11 from sched, steps 12..17 are
     z y x z y x -- and every step deposits the next most significant of its axis' nb + 2 bits.
  6. The order is stable by code: (code, original index).
  7. Records (x, y, z, bits(index)) in that order.
  8. gbox[g] = (min xyz, 0, max xyz, 0) of records 64 g .. 64 g + 63 (the last group may be partial).
  9. cells[c], c = 0..4096: the first sorted position whose 12-bit cell (code >> 6) is >= c; so an empty cell opens where the
     next one does and entry 4096 is N.
 10. Header: slots 4100..4105 = lo and scale (float bits), 4107 = sched, 4106 = 1 when the cloud occupies fewer than
     int(0.6 * 4096 * (1 - exp(-N / 4096))) of the 4096 cells (crowded), else 0.  Slots 4097..4099 and 4108..4111 are
     unspecified.

The module also holds the clouds (`cloud`) and the batches (`SORT_CASES`) the GPU test runs, so that the CPU tests can hold
the cases themselves to their premises: no denormal extent or cell width, flag thresholds clear of an integer."""
import math

import numpy as np

F = np.float32
CELL_INTS = 4112
SCHED_CUBE = 0x186186          # z y x z y x ...: axis 2 1 0 repeated
TAIL_AXES = (2, 1, 0, 2, 1, 0)  # steps 12..17
MIN_NORMAL = float(np.finfo(np.float32).tiny)


# ------------------------------------------------------------------------------------------------ the rule
def deal_grid_bits(ext):
    """ext float32[3] -> (sched, nb[3], width[3]): rule 2.  width = the cell widths after the deal, ext * 2^-nb."""
    w = [F(e) for e in ext]
    nb = [0, 0, 0]
    sched = 0
    for s in range(12):
        a, best = -1, None
        for ax in (2, 1, 0):
            if nb[ax] >= 6:
                continue
            if a < 0 or w[ax] > best * F(1.25):
                a, best = ax, w[ax]
        nb[a] += 1
        w[a] = w[a] * F(0.5)
        sched |= a << (2 * s)
    return sched, nb, np.array(w, F)


def step_axes(sched):
    """The axis of every one of the 18 steps (step 0 = the code's top bit)."""
    return [(sched >> (2 * s)) & 3 for s in range(12)] + list(TAIL_AXES)


def occupancy_threshold(n):
    """Fewer occupied cells than this: crowded (slot 4106).  Double arithmetic, as the launcher's."""
    return int(0.6 * 4096.0 * (1.0 - math.exp(-float(n) / 4096.0)))


def quantise(xyz, lo, scale, nb):
    """Rule 4 -> int64 [N, 3].  The clip is done in float: the device's float -> int conversion saturates, numpy's does not."""
    t = np.trunc((xyz - lo[None, :]) * scale[None, :])                  # float32 throughout
    qmax = np.array([(4 << b) - 1 for b in nb], F)
    return np.clip(t, F(0), qmax[None, :]).astype(np.int64)


def cell_code(q, sched, nb):
    """Rule 5 -> int64 [N] 18-bit codes."""
    rem = [b + 2 for b in nb]
    code = np.zeros(len(q), np.int64)
    for st, a in enumerate(step_axes(sched)):
        rem[a] -= 1
        code |= ((q[:, a] >> rem[a]) & 1) << (17 - st)
    assert rem == [0, 0, 0]
    return code


def restate(xyz):
    """One cloud float32 [N, 3] -> dict of everything the kernel writes (and the intermediate quantities)."""
    xyz = np.ascontiguousarray(xyz, F)
    n = len(xyz)
    assert xyz.ndim == 2 and xyz.shape[1] == 3 and 1 <= n <= 16384
    lo, hi = xyz.min(0), xyz.max(0)
    ext = hi - lo
    sched, nb, width = deal_grid_bits(ext)
    scale = np.array([4 << b for b in nb], F) / np.maximum(ext, F(1e-30))
    q = quantise(xyz, lo, scale, nb)
    code = cell_code(q, sched, nb)
    order = np.lexsort((np.arange(n), code))
    rec = xyz[order]
    ng = (n + 63) // 64
    starts = np.arange(ng) * 64
    gbox = np.zeros((ng, 8), F)
    gbox[:, 0:3] = np.minimum.reduceat(rec, starts, axis=0)
    gbox[:, 4:7] = np.maximum.reduceat(rec, starts, axis=0)
    cell = code[order] >> 6
    table = np.searchsorted(cell, np.arange(4097), side="left").astype(np.int32)
    occupied = len(np.unique(cell))
    cells = np.zeros(CELL_INTS, np.int32)
    cells[:4097] = table
    cells[4100:4103] = lo.view(np.int32)
    cells[4103:4106] = scale.view(np.int32)
    cells[4106] = int(occupied < occupancy_threshold(n))
    cells[4107] = sched
    return dict(lo=lo, ext=ext, sched=sched, nb=nb, width=width, scale=scale, q=q, code=code, order=order.astype(np.int32),
                records=rec, gbox=gbox, cells=cells, occupied=occupied, threshold=occupancy_threshold(n))


COMPARED_SLOTS = np.r_[0:4097, 4100:4108]   # the table, origin + scale, crowded flag, schedule


def has_denormal(r):
    """Does a restated cloud touch float32 denormals where the result could depend on the denormal mode?  The extents, the
    cell widths of the deal, the offsets x - lo and their scaled values are the only places a tiny cloud could."""
    def bad(v):
        v = np.abs(np.asarray(v, np.float64))
        return bool(np.any((v > 0) & (v < MIN_NORMAL)))
    off = r["records"] - r["lo"][None, :]
    return bad(r["records"]) or bad(r["ext"]) or bad(r["width"]) or bad(off) or bad(off * r["scale"][None, :])


# ------------------------------------------------------------------------------------------------ the clouds
FAR = np.array([5000, -3000, 200], F)
TIE_OVER = np.nextafter(F(1.25), F(2))
KINDS = ("cube", "slab", "scene36", "tall", "line", "plane", "tiny", "one_point", "two_points", "twice", "lattice",
         "lattice_slab", "tie125", "tie125_over", "negative", "far_cube", "far_slab")
BOXES = {"cube": (40, 40, 40), "slab": (60, 60, 6), "scene36": (36, 36, 8), "tall": (1, 1, 100), "tie125": (1, 1.25, 1),
         "tie125_over": (1, TIE_OVER, 1), "far_cube": (40, 40, 40), "far_slab": (60, 60, 6)}


def _box(n, rng, size):
    """Uniform in [0, size], with two points on opposite corners (n >= 2): the extents are exactly `size`."""
    p = rng.random((n, 3), dtype=F) * np.array(size, F)
    if n >= 2:
        a, b = rng.choice(n, 2, replace=False)
        p[a], p[b] = 0, np.array(size, F)
    return p


def cloud(kind, n, rng):
    """One cloud float32 [n, 3] of a kind.  No -0.0 anywhere: min / max would not say which zero they return."""
    if kind in BOXES:
        p = _box(n, rng, BOXES[kind])
        if kind.startswith("far_"):
            p = p + FAR
    elif kind == "line":        # along x; y and z constant
        p = np.stack([rng.random(n, dtype=F) * F(50) - F(10), np.full(n, 3.5, F), np.full(n, -1.25, F)], 1)
    elif kind == "plane":       # one extent exactly 0
        p = _box(n, rng, (30, 20, 0)) + np.array([0, 0, 1.5], F)
    elif kind == "tiny":        # extent 255 * 2^-124 ~ 1.2e-35, below the 1e-30f clamp; multiples of 2^-124: nothing denormal
        j = rng.integers(0, 256, (n, 3))
        if n >= 2:
            a, b = rng.choice(n, 2, replace=False)
            j[a], j[b] = 0, 255
        p = np.ldexp(j.astype(F), -124).astype(F)
    elif kind == "one_point":
        p = np.tile(np.array([[1.5, -2.25, 3.0]], F), (n, 1))
    elif kind == "two_points":
        p = np.array([[1.5, -2.25, 3.0], [2.5, -2.0, 3.0]], F)[rng.integers(0, 2, n)]
        if n >= 2:
            p[0], p[n - 1] = (1.5, -2.25, 3.0), (2.5, -2.0, 3.0)
    elif kind == "twice":       # every point twice, shuffled
        half = _box((n + 1) // 2, rng, (40, 40, 40)) - F(20)
        p = np.concatenate([half, half])[:n][rng.permutation(n)]
    elif kind == "lattice":     # 4 + 4 + 4 grid bits, 64 steps of exactly 1 per axis: every coordinate on a boundary
        p = rng.integers(0, 65, (n, 3)).astype(F)
        if n >= 2:
            a, b = rng.choice(n, 2, replace=False)
            p[a], p[b] = 0, 64
    elif kind == "lattice_slab":  # 128 x 64 x 16 deals 5 + 4 + 3: steps of 1, 1 and 1/2 -- the deposit-table path
        p = rng.integers(0, (129, 65, 33), (n, 3)).astype(F) * np.array([1, 1, 0.5], F)
        if n >= 2:
            a, b = rng.choice(n, 2, replace=False)
            p[a], p[b] = 0, (128, 64, 16)
    elif kind == "negative":
        p = _box(n, rng, (40, 30, 35)) - np.array([50, 45, 40], F)
    else:
        raise KeyError(kind)
    p = np.ascontiguousarray(p, F) + F(0)          # -0.0 + 0.0 = +0.0
    assert p.shape == (n, 3) and p.dtype == F and not np.any(np.signbit(p) & (p == 0))
    return p


SIZES = (1, 5, 63, 64, 65, 100, 1000, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 9000, 16383, 16384)


def _sort_cases():
    """(N, kinds of the batch): every size with the cube and three other kinds in turn, then every kind at 1000, 4097 and
    16384.  The all-identical cloud stays at N <= 4096."""
    others = [k for k in KINDS if k != "cube"]
    cases = []
    for i, n in enumerate(SIZES):
        ks = [others[(3 * i + j) % len(others)] for j in range(3)]
        cases.append((n, ("cube",) + tuple("two_points" if k == "one_point" and n > 4096 else k for k in ks)))
    for n in (1000, 4097, 16384):
        ks = [k for k in KINDS if not (k == "one_point" and n > 4096)]
        cases += [(n, tuple(ks[j:j + 4])) for j in range(0, len(ks), 4)]
    return cases


SORT_CASES = _sort_cases()
FAR_CASES = ((4097, ("far_cube", "far_slab")), (1000, ("far_cube", "far_slab")))   # the consumers' clouds
FPS_M = 512


def case_id(case):
    return "%d-%s" % (case[0], "+".join(case[1]))


def make_batch(case):
    """(N, kinds) -> float32 [B, N, 3]; the seed depends on the case alone."""
    import zlib
    n, kinds = case
    rng = np.random.default_rng(zlib.crc32(repr(case).encode()))
    return np.stack([cloud(k, n, rng) for k in kinds])
