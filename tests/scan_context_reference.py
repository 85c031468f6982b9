"""A numpy restatement of the two Scan Context rules of include/dh3d_hip.h (dh3d_scan_context, dh3d_scan_context_distance),
step by step in the number formats the header names, and the seeded scenes the tests share.  Nothing here runs on a GPU and
nothing of the package is imported: the tables are built by the header's formulas, and tests/test_scan_context_reference.py
checks that the package builds the same bits."""
import numpy as np

F32, F64 = np.float32, np.float64


def tables(num_rings, num_sectors, max_radius):
    """sector_dir [Ns/2 - 1, 2] = (cos, sin)(2 pi k / Ns), k = 1 .. Ns/2 - 1; ring_edge2 [Nr + 1] = (i max_radius / Nr)^2."""
    ang = 2.0 * np.pi * np.arange(1, num_sectors // 2, dtype=F64) / num_sectors
    edge = np.arange(num_rings + 1, dtype=F64) * float(max_radius) / num_rings
    return np.stack([np.cos(ang), np.sin(ang)], axis=1), edge * edge


def bins_of(xyz, center, sector_dir, ring_edge2, z_offset):
    """Per point of xyz [n, >=3] float32: (counts [n] bool, ring [n], sector [n], h [n] float32) by the header's rules --
    every count is made literally, over all i and all k."""
    Nr, half = ring_edge2.shape[0] - 1, sector_dir.shape[0] + 1
    xyz = np.asarray(xyz, F32)
    cx, cy = (F32(0), F32(0)) if center is None else (F32(center[0]), F32(center[1]))
    with np.errstate(all="ignore"):
        dx, dy, h = xyz[:, 0] - cx, xyz[:, 1] - cy, xyz[:, 2] + F32(z_offset)
        assert dx.dtype == F32 and dy.dtype == F32 and h.dtype == F32
        X, Y = dx.astype(F64), dy.astype(F64)
        r2 = X * X + Y * Y
        counts = np.isfinite(dx) & np.isfinite(dy) & np.isfinite(h) & (r2 < ring_edge2[Nr]) & (h > 0)
        ring = (r2[:, None] >= ring_edge2[None, 1:Nr]).sum(1)
        upper = (Y > 0) | ((Y == 0) & (X > 0))
        X, Y = np.where(upper, X, -X), np.where(upper, Y, -Y)
        a, b = sector_dir[None, :, 0] * Y[:, None], sector_dir[None, :, 1] * X[:, None]
        sector = np.where(upper, 0, half) + ((a - b) >= 0).sum(1)
    return counts, ring, sector, h


def scan_context(points, num_valid=None, center=None, num_rings=20, num_sectors=60, max_radius=80.0, z_offset=2.0):
    """(desc [P, Nr, Ns] float32, ring_key [P, Nr] float32) of points [P, N, >=3]."""
    points = np.asarray(points, F32)
    P, N = points.shape[:2]
    sector_dir, ring_edge2 = tables(num_rings, num_sectors, max_radius)
    desc = np.zeros((P, num_rings, num_sectors), F32)
    for p in range(P):
        n = N if num_valid is None else min(max(int(num_valid[p]), 0), N)
        counts, ring, sector, h = bins_of(points[p, :n], None if center is None else center[p], sector_dir, ring_edge2, z_offset)
        np.maximum.at(desc[p], (ring[counts], sector[counts]), h[counts])
    return desc, ring_keys(desc)


def ring_keys(desc):
    """s = 0.0; for j ascending: s += (double)desc[.., r, j]; key = (float)(s / Ns)."""
    s = np.zeros(desc.shape[:-1], F64)
    for j in range(desc.shape[-1]):
        s = s + desc[..., j].astype(F64)
    return (s / F64(desc.shape[-1])).astype(F32)


def shifted_distances(q, c):
    """d_n for n = 0 .. Ns-1 of two images [Nr, Ns], float64."""
    q, c = np.asarray(q, F32).astype(F64), np.asarray(c, F32).astype(F64)
    Ns = q.shape[1]
    wq, wc = (q * q).sum(0), (c * c).sum(0)
    d = np.ones(Ns, F64)
    for n in range(Ns):
        cs, wcs = np.roll(c, -n, axis=1), np.roll(wc, -n)        # column j of cs = column (j + n) % Ns of c
        both = (wq != 0) & (wcs != 0)
        m = int(both.sum())
        if m:
            cos = (q[:, both] * cs[:, both]).sum(0) / np.sqrt(wq[both] * wcs[both])
            d[n] = 1.0 - (1.0 / m) * cos.sum()
    return d


def distance(qry, mp, cand, map_count=None):
    """(dist [Q, C] float64, shift [Q, C] int32, gap [Q, C] float64: second-best d_n minus best, inf for an invalid id)."""
    Q, C = cand.shape
    r = mp.shape[0] if map_count is None else min(max(int(map_count), 0), mp.shape[0])
    dist, shift, gap = np.full((Q, C), np.inf), np.full((Q, C), -1, np.int32), np.full((Q, C), np.inf)
    memo = {}
    for qi in range(Q):
        for ci in range(C):
            i = int(cand[qi, ci])
            if 0 <= i < r:
                if (qi, i) not in memo:
                    memo[(qi, i)] = shifted_distances(qry[qi], mp[i])
                d = memo[(qi, i)]
                n = int(np.argmin(d))                               # the first minimum: the smallest shift
                dist[qi, ci], shift[qi, ci] = d[n], n
                gap[qi, ci] = np.partition(d, 1)[1] - d[n]
    return dist, shift, gap


def order_of(dist, cand):
    """The slots of every row sorted ascending by (dist, id, slot)."""
    return np.stack([np.lexsort((np.arange(dist.shape[1]), cand[q], dist[q])) for q in range(dist.shape[0])]).astype(np.int32)


def search(map_desc, map_keys, count, qry_desc, qry_keys, k, candidates):
    """The chain of ScanContextIndex.search over the first `count` places: ring-key top-`candidates` by (float64 squared
    distance summed over the columns in order, id), the shifted distance, the first k by (dist, id, slot).  Returns
    (place, dist, shift, yaw, gap), each [Q, k]."""
    Q, Ns = qry_desc.shape[0], qry_desc.shape[2]
    cand = np.full((Q, candidates), -1, np.int32)
    d2 = np.zeros((Q, count), F64)
    for c in range(map_keys.shape[1]):
        diff = qry_keys[:, None, c].astype(F64) - map_keys[None, :count, c].astype(F64)
        d2 = d2 + diff * diff
    for q in range(Q):
        top = np.lexsort((np.arange(count), d2[q]))[:candidates]
        cand[q, :top.shape[0]] = top
    dist, shift, gap = distance(qry_desc, map_desc, cand, count)
    top = order_of(dist, cand)[:, :k]
    shift = np.take_along_axis(shift, top, 1)
    with np.errstate(invalid="ignore"):
        yaw = np.where(shift >= 0, shift.astype(F64) * (2.0 * np.pi) / Ns, np.nan)
    return np.take_along_axis(cand, top, 1), np.take_along_axis(dist, top, 1), shift, yaw, np.take_along_axis(gap, top, 1)


def scene(seed, n_walls=12, per_wall=200, n_ground=1600, extent=20.0):
    """A seeded street scene, [n_walls * per_wall + n_ground, 3] float32 within +-extent: random wall segments whose points
    reach from the ground (z = -2, the sensor 2 m above it) up to a random top, and a noisy ground plane."""
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(n_walls):
        a, b = rng.uniform(-extent, extent, 2), rng.uniform(-extent, extent, 2)
        t = rng.random((per_wall, 1))
        xy = a + t * (b - a) + rng.normal(0.0, 0.02, (per_wall, 2))
        z = -2.0 + rng.random(per_wall) * rng.uniform(1.0, 8.0)
        parts.append(np.concatenate([xy, z[:, None]], 1))
    g = rng.uniform(-extent, extent, (n_ground, 2))
    parts.append(np.concatenate([g, -2.0 + np.abs(rng.normal(0.0, 0.03, (n_ground, 1))) + 0.01], 1))
    pts = np.clip(np.concatenate(parts, 0), -extent, extent)
    return rng.permutation(pts).astype(F32)


def rotate_quarter(points, quarters):
    """Exact rotation about z by quarters * 90 deg: (x, y) -> (-y, x) per quarter turn (no rounding)."""
    p = np.array(points, F32, copy=True)
    for _ in range(quarters % 4):
        p[..., 0], p[..., 1] = -p[..., 1].copy(), p[..., 0].copy()
    return p


def boundary_cloud(max_radius=20.0):
    """Points on every edge the bin rules have, for max_radius = 20, Nr = 20 (ring edges at whole metres), and the
    (counts, ring, sector) the rules give them at Ns = 60, worked out by hand:
      (3, 4)   r2 = 25 = edge 5 exactly -> ring 5 (>=);  angle 53.13 deg -> sector 8
      axes     (+x: H 0, no k passes: sector 0), (+y: sector 15), (-x: H 1, negated to +x: sector 30), (-y: sector 45)
      origin   H 1, negated to (-0, -0): every k passes (-0 - -0 = 0 >= 0): sector 30 + 29 = 59, ring 0
      h        -0.0 and below: not counted;  NaN / inf anywhere: not counted;  r2 >= 400: not counted"""
    z = 1.0
    rows = [
        (3, 4, z, True, 5, 8), (1, 0, z, True, 1, 0), (0, 1, z, True, 1, 15), (-1, 0, z, True, 1, 30), (0, -1, z, True, 1, 45),
        (0, 0, z, True, 0, 59), (-0.0, 0.0, z, True, 0, 59), (-3, -4, z, True, 5, 38), (0.5, 0, z, True, 0, 0),
        (19.5, 0, z, True, 19, 0), (20, 0, z, False, 0, 0), (12, 16, z, False, 0, 0), (0, -20, z, False, 0, 0), (25, 3, z, False, 0, 0),
        (2, 2, -2.0, False, 0, 0), (2, 2, -2.5, False, 0, 0), (2, 2, np.nan, False, 0, 0), (np.nan, 2, z, False, 0, 0),
        (2, np.inf, z, False, 0, 0), (-np.inf, 2, z, False, 0, 0), (2, 2, np.inf, False, 0, 0), (2, 2, -np.inf, False, 0, 0),
        (2, 2, -1.9999999, True, 2, 7),
    ]
    a = np.array(rows, F64)
    return a[:, :3].astype(F32), a[:, 3].astype(bool), a[:, 4].astype(int), a[:, 5].astype(int)


def distance_fixture(num_rings=20, num_sectors=60, Q=48, C=8, n_scenes=24, radius=20.0, seed=7):
    """The distance test's inputs: a map of n_scenes scene images, their rolls by a seeded shift, and one image of zeros
    (R = 2 n_scenes + 1 rows, the last 4 of them beyond map_count); Q queries drawn from the scene images, rolled again; C
    candidate ids per query with -1, ids at and above the count and a repeated id mixed in.  The last query is the image of
    zeros and its first candidate the map's image of zeros.  Returns (qry, map, cand int32, map_count)."""
    rng = np.random.default_rng(seed)
    base, _ = scan_context(np.stack([scene(100 + s) for s in range(n_scenes)]), None, None, num_rings, num_sectors, radius, 2.0)
    rolled = np.stack([np.roll(base[s], int(rng.integers(num_sectors)), axis=1) for s in range(n_scenes)])
    mp = np.concatenate([base, np.zeros((1, num_rings, num_sectors), F32), rolled], 0)
    zero_id, R = n_scenes, 2 * n_scenes + 1
    count = R - 4
    qry = np.stack([np.roll(base[int(rng.integers(n_scenes))], int(rng.integers(num_sectors)), axis=1) for _ in range(Q)])
    qry[Q - 1] = 0
    cand = rng.integers(0, count - 1, (Q, C)).astype(np.int32)
    cand += cand >= zero_id                          # (the image of zeros only where it is put below)
    cand[:, C - 1] = cand[:, 0]                      # a repeated id in every row
    cand[::3, 1] = -1
    cand[1::3, 2] = count                            # at the count
    cand[2::3, 3] = R - 1                            # above it, inside the buffer
    cand[Q // 2, 4] = R + 1000                       # outside the buffer: nothing may be read
    cand[Q - 1, 1:C - 1] = -1                        # the image of zeros has no best shift: keep its pairs few
    cand[Q - 1, 0] = cand[Q - 1, C - 1] = zero_id
    cand[Q - 1, 4] = 1
    return qry.astype(F32), mp.astype(F32), cand, count
