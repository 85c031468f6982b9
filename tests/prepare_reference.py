"""Plain numpy restatement of the three stages of prepare_clouds (include/dh3d_hip.h dh3d_prepare_clouds,
csrc/prepare.hip), written from the stated semantics -- the yardstick of the prepare tests.  One cloud at a time, float64
where the semantics say double, every expression in the stated order (numpy contracts nothing).

voxel_grid(pts, voxel)        stage 1: (float32 voxel points in the order of their lowest member, or None beyond 2^21 cells)
radius_counts(pts, radius)    stage 2: for every point the number of points at d2 < r2, itself included
fixed_size(pts, targetnum..)  stage 3: (points [targetnum,3], num_valid, centroid)
prepare_cloud(...)            the three in a row: dict(points, num_valid, counts, centroid), a void cloud as the device's
"""
import numpy as np

PAD = np.float32(100000.0)
CELL_LIMIT = 1 << 21


def _sq3(d):
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def voxel_cells(pts, voxel):
    """cell = floor((double(p) - (double(lo) - voxel/2)) / voxel) per axis, float64 [n,3] (a true division)."""
    p = np.asarray(pts, np.float32).astype(np.float64)
    origin = p.min(axis=0) - float(voxel) / 2.0
    return np.floor((p - origin) / float(voxel))


def voxel_grid(pts, voxel):
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    n = pts.shape[0]
    if n == 0:
        return np.zeros((0, 3), np.float32)
    cell = voxel_cells(pts, voxel)
    if not ((cell >= 0).all() and (cell < CELL_LIMIT).all()):
        return None
    c = cell.astype(np.int64)
    key = c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)
    order = np.argsort(key, kind="stable")            # members of a voxel in ascending index
    ks = key[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    count = np.diff(np.r_[starts, n])
    p64 = pts.astype(np.float64)
    sums = np.zeros((starts.size, 3), np.float64)
    for r in range(int(count.max())):                 # the r-th member of every voxel that has one: one rounding per add
        sel = np.flatnonzero(count > r)
        sums[sel] = sums[sel] + p64[order[starts[sel] + r]]
    mean = (sums / count[:, None].astype(np.float64)).astype(np.float32)
    return mean[np.argsort(order[starts], kind="stable")]


def radius_counts(pts, radius, chunk=1 << 21):
    """#{j : d2(i, j) < r2} for every i (j = i included), by a cell list of its own: candidates from the 27 cells of edge a
    little over the radius around a point's cell, each tested with the stated expression."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    n = pts.shape[0]
    out = np.zeros(n, np.int64)
    if n == 0:
        return out
    p = pts.astype(np.float64)
    r2 = float(radius) * float(radius)
    cell = np.floor((p - p.min(axis=0)) / (float(radius) * 1.001)).astype(np.int64)
    dims = cell.max(axis=0) + 3                        # a free layer either side: a neighbour's key never wraps
    assert float(dims[0]) * float(dims[1]) * float(dims[2]) < 2.0 ** 62

    def lin(c):
        return ((c[:, 0] + 1) * dims[1] + (c[:, 1] + 1)) * dims[2] + (c[:, 2] + 1)

    order = np.argsort(lin(cell), kind="stable")
    cs, ps = cell[order], p[order]
    uniq, starts, cnts = np.unique(lin(cs), return_index=True, return_counts=True)
    acc = np.zeros(n, np.int64)
    for off in np.ndindex(3, 3, 3):
        nk = lin(cs + (np.array(off, np.int64) - 1))
        pos = np.minimum(np.searchsorted(uniq, nk), uniq.size - 1)
        q_all = np.flatnonzero(uniq[pos] == nk)
        c_all = cnts[pos[q_all]]
        edges = np.r_[0, np.cumsum(c_all)]
        lo = 0
        while lo < q_all.size:                         # pieces of at most ~chunk candidate pairs
            hi = max(lo + 1, int(np.searchsorted(edges, edges[lo] + chunk, side="right")) - 1)
            q, c = q_all[lo:hi], c_all[lo:hi]
            tot = int(c.sum())
            qi = np.repeat(q, c)
            pj = np.repeat(starts[pos[q]], c) + (np.arange(tot) - np.repeat(np.cumsum(c) - c, c))
            acc += np.bincount(qi, weights=_sq3(ps[qi] - ps[pj]) < r2, minlength=n).astype(np.int64)
            lo = hi
    out[order] = acc
    return out


def centroid_of(pts):
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    return pts.astype(np.float64).mean(axis=0) if pts.shape[0] else np.zeros(3, np.float64)


def select_nearest(pts, targetnum, centroid):
    """Indices (ascending) of the targetnum points with the smallest (d2 to the centroid, index)."""
    d2 = _sq3(np.asarray(pts, np.float32).astype(np.float64) - np.asarray(centroid, np.float64))
    return np.sort(np.lexsort((np.arange(d2.size), d2))[:targetnum])


def fixed_size(pts, targetnum, sortby_dis=True, centroid=None):
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    m = pts.shape[0]
    centroid = centroid_of(pts) if centroid is None else np.asarray(centroid, np.float64)
    if m <= targetnum:
        return np.concatenate([pts, np.full((targetnum - m, 3), PAD, np.float32)], axis=0), m, centroid
    keep = select_nearest(pts, targetnum, centroid) if sortby_dis else np.arange(targetnum)
    return pts[keep], targetnum, centroid


def prepare_cloud(pts, targetnum, voxel_size=0.2, radius=1.0, nb_points=4, sortby_dis=True, centroid=None):
    """centroid: None for numpy's own float64 mean, or the mean to select with (the device's: its summation tree differs from
    numpy's in the last bits, and the selection is defined on the centroid the op returns)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    n = pts.shape[0]
    void = dict(points=np.full((targetnum, 3), PAD, np.float32), num_valid=0, counts=np.array([n, -1, -1], np.int32),
                centroid=np.zeros(3, np.float64), stage1=None, stage2=None)
    s1 = pts if voxel_size is None else voxel_grid(pts, voxel_size)
    if s1 is None:
        return void
    if radius is None:
        s2 = s1
    else:
        if s1.shape[0] and not (np.floor((s1.astype(np.float64) - s1.astype(np.float64).min(axis=0))
                                         / (float(radius) * (1.0 + 2.0 ** -20))) < CELL_LIMIT).all():
            return void
        s2 = s1[radius_counts(s1, radius) > nb_points]
    own = centroid_of(s2)
    out, nv, c = fixed_size(s2, targetnum, sortby_dis, centroid)
    return dict(points=out, num_valid=nv, counts=np.array([n, s1.shape[0], s2.shape[0]], np.int32), centroid=own, stage1=s1,
                stage2=s2)


# ------------------------------------------------------------------------------------------------ shared inputs
def street_scene(seed=7):
    """A synthetic street of 60 300 points in metres: a ground plane (40 000), two facing walls (10 000 each) and 300 stray
    points in the air above them; scanner-like noise of a centimetre."""
    rng = np.random.default_rng(seed)
    g = np.stack([rng.uniform(-30, 30, 40000), rng.uniform(-8, 8, 40000), rng.normal(0, 0.01, 40000)], axis=1)
    w1 = np.stack([rng.uniform(-30, 30, 10000), rng.normal(-8, 0.01, 10000), rng.uniform(0, 6, 10000)], axis=1)
    w2 = np.stack([rng.uniform(-30, 30, 10000), rng.normal(8, 0.01, 10000), rng.uniform(0, 6, 10000)], axis=1)
    stray = np.stack([rng.uniform(-30, 30, 300), rng.uniform(-6, 6, 300), rng.uniform(8, 30, 300)], axis=1)
    pts = np.concatenate([g, w1, w2, stray], axis=0)
    return np.ascontiguousarray(pts[rng.permutation(pts.shape[0])], np.float32)


def lattice(n, step):
    a = np.arange(n, dtype=np.float32) * np.float32(step)
    return np.ascontiguousarray(np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3))


def tie_cases():
    """name -> (points, keyword arguments of prepare_cloud): the places where another reading of the semantics would show."""
    rng = np.random.default_rng(11)
    f32 = np.float32
    below = np.nextafter(f32(0.125), f32(0))
    faces = np.array([[0, 0, 0], [0.125, 0, 0], [below, 0, 0], [0.375, 0.125, 0], [0.25, below, 0.125], [0.125, 0.125, 0.125],
                      [below, below, below], [0.625, 0, 0], [0.5, 0.375, 0.375]], f32)
    dup = np.concatenate([np.tile(np.array([[1.5, 2.5, -0.5]], f32), (40, 1)), np.tile(np.array([[4.0, 4.0, 4.0]], f32), (5, 1)),
                          rng.random((60, 3), dtype=np.float32)], axis=0)
    dup = dup[rng.permutation(dup.shape[0])]
    crowd = np.concatenate([rng.random((5000, 3), dtype=np.float32) * f32(0.09), rng.random((300, 3), dtype=np.float32) * f32(0.09)
                            + f32(1.0), rng.random((20, 3), dtype=np.float32) * f32(0.09) + f32(2.0),
                            rng.random((2000, 3), dtype=np.float32) * f32(3.0)], axis=0)
    crowd = crowd[rng.permutation(crowd.shape[0])]
    return {
        # points on voxel faces (origin -0.125, faces at 0.125 + 0.25 k): a face belongs to the cell above it
        "voxel_faces": (faces, dict(targetnum=16, voxel_size=0.25, radius=None)),
        # neighbours at exactly d2 = 1 = r2: the strict test leaves every point alone with itself -> m = 0
        "shell_unit_lattice": (lattice(5, 1.0), dict(targetnum=64, voxel_size=None, radius=1.0, nb_points=1)),
        # step 0.5: 6 + 12 + 8 neighbours inside, 6 exactly on the shell; a corner counts 8 (11 with <=): nb_points = 8 drops it
        "shell_half_lattice": (lattice(6, 0.5), dict(targetnum=256, voxel_size=None, radius=1.0, nb_points=8)),
        # exact ties in d2 to the centroid: the lowest indices win
        "select_ties": (lattice(9, 0.5), dict(targetnum=100, voxel_size=None, radius=1.0, nb_points=4)),
        "select_ties_first": (lattice(9, 0.5), dict(targetnum=100, voxel_size=None, radius=None, sortby_dis=False)),
        "duplicates": (dup, dict(targetnum=128, voxel_size=0.2, radius=1.0, nb_points=4)),
        "duplicates_no_voxel": (dup, dict(targetnum=64, voxel_size=None, radius=1.0, nb_points=4)),
        # voxels of 5000, 300 and 20 members (clusters 0.09 wide, each inside one cell): the three ways the members are ordered
        "crowded_voxels": (crowd, dict(targetnum=1024, voxel_size=0.2, radius=1.0, nb_points=4)),
        "m_equals_targetnum": (lattice(6, 0.5), dict(targetnum=216, voxel_size=0.2, radius=None)),
        # 216 points in 9 exact tie groups of d2, the first and the last of 8: the select at k = 1, at k = a whole first
        # group, and with the threshold inside the last group, taking 1 and 7 of its 8
        **{"select_ties_k%d" % t: (lattice(6, 0.5), dict(targetnum=t, voxel_size=None, radius=None)) for t in (1, 8, 209, 215)},
    }
