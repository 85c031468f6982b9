"""Regenerates tests/golden/twins_ball.npz: inputs and the rows of the REFERENCE's own query_ball_point_cpu
(tf_ops/grouping/test/query_ball_point.cpp:19-47), called through ctypes in oracle/_ref/libref_grouping.so (built by
build() when the reference tree is present; the twin is in it under its C++ name).  Only data goes into the fixture: the
clouds, the queries, radius / nsample and the twin's rows.  idx is pre-filled with -1: the twin leaves the row of an empty
ball unwritten, and those are the only rows it cannot judge.

    python tests/golden/make_ball_golden.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TWIN = "_Z20query_ball_point_cpuiiifiPKfS0_Pi"  # void query_ball_point_cpu(int b, int n, int m, float radius, int nsample, const float*, const float*, int*)


def twin_rows(radius, nsample, xyz1, xyz2):
    lib = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_grouping.so"))
    fn = getattr(lib, TWIN)
    fn.restype = None
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p]
    x1, x2 = np.ascontiguousarray(xyz1, np.float32), np.ascontiguousarray(xyz2, np.float32)
    idx = np.full((x2.shape[0], nsample), -1, np.int32)
    fn(1, x1.shape[0], x2.shape[0], float(radius), nsample, x1.ctypes.data, x2.ctypes.data, idx.ctypes.data)
    return idx


def cases():
    rng = np.random.default_rng(20240)
    f32 = np.float32
    cube = rng.uniform(-1.0, 1.0, (8192, 3)).astype(f32)
    demo = np.load(os.path.join(HERE, "demo_clouds.npz"))["global_c"]
    c = []  # (name, xyz1 or "name of the case / demo cloud that holds it", xyz2, radius, nsample)
    c.append(("cube_r02_k16", cube, cube[:1024], 0.2, 16))
    c.append(("cube_r01_k32", "cube_r02_k16/xyz1", cube[:1024], 0.1, 32))
    # queries that are not dataset points, a third of them outside the cloud's bounding box
    q = rng.uniform(-1.15, 1.15, (768, 3)).astype(f32)
    c.append(("cube_offcloud_r025_k24", "cube_r02_k16/xyz1", q, 0.25, 24))
    # a demo cloud in metres, queries = every 8th point
    c.append(("demo_global_c_r15_k32", "demo:global_c", demo[::8], 1.5, 32))
    # a slab: z extent a tenth of x / y
    slab = (rng.uniform(-1.0, 1.0, (4096, 3)) * np.array([1.0, 1.0, 0.1])).astype(f32)
    c.append(("slab_r015_k16", slab, slab[::4], 0.15, 16))
    # integer lattice 16^3 scaled by 2^-3, shuffled; radius = exactly the lattice distance sqrt(1 + 4 + 4) / 8 = 0.375: all
    # arithmetic exact, the points AT the radius are not hits (strict <)
    g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3)
    lat = (rng.permutation(g) * 0.125).astype(f32)
    c.append(("lattice_r0375_k64", lat, lat[:512], 0.375, 64))
    c.append(("lattice_r0125_k8", "lattice_r0375_k64/xyz1", lat[:512], 0.125, 8))   # only the point itself is inside
    # duplicated points: every point four times, in shuffled order
    base = rng.uniform(-1.0, 1.0, (512, 3)).astype(f32)
    dup = base[rng.permutation(np.repeat(np.arange(512), 4))]
    c.append(("duplicates_r02_k12", dup, dup[:512], 0.2, 12))
    c.append(("cube_r01_k1", "cube_r02_k16/xyz1", cube[1024:1536], 0.1, 1))
    small = rng.uniform(-1.0, 1.0, (20, 3)).astype(f32)
    c.append(("nsample_gt_n_r08_k32", small, rng.uniform(-1.0, 1.0, (64, 3)).astype(f32), 0.8, 32))
    return c


def main():
    out = {"cases": np.array([n for n, *_ in cases()])}
    clouds = {}
    full = part = rows = 0
    for name, xyz1, xyz2, radius, nsample in cases():
        if isinstance(xyz1, str):
            out[name + "/xyz1_from"] = np.array(xyz1)
            x1 = np.load(os.path.join(HERE, "demo_clouds.npz"))[xyz1[5:]] if xyz1.startswith("demo:") else clouds[xyz1]
        else:
            out[name + "/xyz1"] = clouds[name + "/xyz1"] = x1 = xyz1
        radius = np.float32(radius)
        idx = twin_rows(radius, nsample, x1, xyz2)
        out[name + "/xyz2"], out[name + "/radius"], out[name + "/nsample"] = xyz2, radius, np.int32(nsample)
        out[name + "/idx"] = idx.astype(np.int16 if x1.shape[0] < 32768 else np.int32)
        written = idx[:, 0] >= 0
        distinct = np.array([len(set(r)) for r in idx[written]])
        is_full = distinct == nsample   # (a full row holds nsample distinct ids; nsample = 1: every written row)
        full += int(is_full.sum()); part += int((~is_full).sum()); rows += idx.shape[0]
        print("%-26s n %5d m %5d r %.4g k %3d: empty %5.1f %%, full %5.1f %%, part %5.1f %%, median ids %g"
              % (name, x1.shape[0], xyz2.shape[0], radius, nsample, 100 * (1 - written.mean()),
                 100 * is_full.sum() / len(idx), 100 * (~is_full).sum() / len(idx), np.median(distinct)))
        assert (1 - written.mean()) <= 0.10, name
    print("fixture: full %.1f %%, partly filled %.1f %% of %d rows" % (100 * full / rows, 100 * part / rows, rows))
    assert full >= 0.2 * rows and part >= 0.2 * rows
    path = os.path.join(HERE, "twins_ball.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.exit(main())
