"""numpy float32 restatement of query_ball_point / query_ball_point2 (tf_ops/grouping: CPU twin
test/query_ball_point.cpp:19-47, kernels tf_grouping_g.cu:3-92), with this project's empty-ball rule.

Per query, over the dataset points in index order:  d = max(sqrtf((dx*dx + dy*dy) + dz*dz), 1e-20f) -- every operation a
separate float32 rounding, as the twin's g++ -O2 x86-64 build computes it (no fma contraction, IEEE sqrtf) -- a hit is
d < radius (strict).  The row: the min(hits, nsample) smallest hit indices in ascending order, then the first of them
repeated; pts_cnt = min(hits, nsample).  Empty ball: nsample copies of the index of the nearest point (same d, lowest
index on ties), pts_cnt = 0 (the twin leaves that row unwritten)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = np.float32(1e-20)


def distances(xyz1, xyz2):
    """d [m, n] float32 of one cloud: xyz1 [n,3] dataset, xyz2 [m,3] queries, in the twin's rounding order."""
    p, q = np.asarray(xyz1, np.float32), np.asarray(xyz2, np.float32)
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    s = (dx * dx + dy * dy) + dz * dz
    assert s.dtype == np.float32
    return np.maximum(np.sqrt(s), TINY)


def query_ball_point(radius, nsample, xyz1, xyz2, chunk=512):
    """radius: a float, or per-query radii [b,m] (query_ball_point2); xyz1 [b,n,3]; xyz2 [b,m,3]
    -> (idx [b,m,nsample] int32, pts_cnt [b,m] int32)."""
    xyz1, xyz2 = np.asarray(xyz1, np.float32), np.asarray(xyz2, np.float32)
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    radii = np.broadcast_to(np.asarray(radius, np.float32), (b, m))
    idx = np.empty((b, m, nsample), np.int32)
    cnt = np.empty((b, m), np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(b):
            for j0 in range(0, m, chunk):
                d = distances(xyz1[i], xyz2[i, j0:j0 + chunk])
                hit = d < radii[i, j0:j0 + chunk, None]
                rank = np.cumsum(hit, axis=1)
                keep = hit & (rank <= nsample)
                c = np.minimum(rank[:, -1], nsample).astype(np.int32)
                rows = np.empty((d.shape[0], nsample), np.int32)
                rr, kk = np.nonzero(keep)
                rows[rr, rank[rr, kk] - 1] = kk
                fill = np.where(c > 0, rows[:, 0], np.argmin(d, axis=1)).astype(np.int32)  # argmin: the lowest index of a tie
                pad = np.arange(nsample)[None, :] >= c[:, None]
                rows[pad] = np.broadcast_to(fill[:, None], rows.shape)[pad]
                idx[i, j0:j0 + chunk], cnt[i, j0:j0 + chunk] = rows, c
    return idx, cnt


def golden_cases():
    """The cases of golden/twins_ball.npz: name -> dict(xyz1 [1,n,3], xyz2 [1,m,3], radius, nsample, idx [1,m,nsample] int32
    -- the twin's rows, -1 where it wrote nothing).  Clouds that several cases share are stored once ("<case>/xyz1_from")."""
    z = np.load(os.path.join(GOLDEN, "twins_ball.npz"))
    demo = None
    out = {}
    for name in [str(s) for s in z["cases"]]:
        src = str(z[name + "/xyz1_from"]) if name + "/xyz1_from" in z.files else name + "/xyz1"
        if src.startswith("demo:"):
            demo = demo if demo is not None else np.load(os.path.join(GOLDEN, "demo_clouds.npz"))
            xyz1 = demo[src[5:]]
        else:
            xyz1 = z[src]
        out[name] = dict(xyz1=np.ascontiguousarray(xyz1, np.float32)[None], xyz2=z[name + "/xyz2"].astype(np.float32)[None],
                         radius=float(z[name + "/radius"]), nsample=int(z[name + "/nsample"]),
                         idx=z[name + "/idx"].astype(np.int32)[None])
    return out
