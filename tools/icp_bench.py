"""Time dense ICP refinement (csrc/icp.hip, registration.refine_icp) on P pairs of N x N points, T iterations: the cell-list
and the scan association, on subsets of the demo clouds and on a uniform cube, with device events around `iters`
back-to-back calls after a warm-up; next to register_clouds without refinement (the forward passes, matching and RANSAC
that produce the start pose) on `--reg-pairs` pairs.  Per iteration = (T iterations - 0 iterations) / T; the fit alone is
timed on one-anchor clouds, where the association costs nothing and every positive point is a pair; an association is the
difference.  "padded": the demo pairs with 6144 valid rows of 8192 and rows of 100000.0 behind them in both clouds, as
prepare_clouds pads.  Pose errors are registration.transform_errors' (compareTransform: |dt| in metres, the sum of the
three |Euler angles| in degrees -- a start 2 degrees off about one axis reads as about 3).  "plane": on the demo pairs, the
anchor normals at k = 16 (the kNN and the normals kernel timed apart), then point-to-plane ICP (registration.refine_icp_plane
on given normals, cell lists) at 5, 10 and 20 iterations next to point-to-point at the same counts, each with its pose error
against the truth; and both fits alone on eight-anchor clouds (the plane fit needs normals that span space).  Generalized ICP
(registration.refine_icp_gicp on given normals of both clouds, epsilon 1e-3) runs in the same pass at the same counts: its
rows carry besides the positive normals' cost (kNN + normals kernel, positive_normals_us) and the time per iteration
(iteration_us, against the same call at 0 iterations), and gicp_step8_us stands next to the other two fits'.  Prints one
JSON line.

    python tools/icp_bench.py [--pairs 64] [--points 8192] [--iterations 20] [--iters 5] [--reg-pairs 8]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dh3d_amd import registration as reg  # noqa: E402


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def pairs(rng, clouds, P, N):
    """Anchor and positive: random N-point subsets of a cloud, the positive moved by a known pose with 2 cm noise; the start
    pose is 0.5 m off and turned by 2 degrees about a random axis (about 3 degrees as transform_errors' sum of |Euler
    angles|, which is what the result reports as start_ddeg)."""
    A, Y, T, T0 = (np.zeros((P, N, 3), np.float32), np.zeros((P, N, 3), np.float32), np.zeros((P, 3, 4)), np.zeros((P, 3, 4)))
    for p in range(P):
        c = clouds[p % len(clouds)].astype(np.float64)
        A[p] = c[rng.permutation(len(c))[:N]]
        R, t = rot(rng.standard_normal(3), rng.uniform(0.2, 1.0)), rng.standard_normal(3) * 2.0
        Y[p] = (c[rng.permutation(len(c))[:N]] - t) @ R + rng.normal(0.0, 0.02, (N, 3))
        d = rng.standard_normal(3)
        T[p] = np.concatenate([R, t[:, None]], axis=1)
        T0[p] = np.concatenate([rot(rng.standard_normal(3), math.radians(2.0)) @ R, (t + d / np.linalg.norm(d) * 0.5)[:, None]], axis=1)
    return A, Y, T, T0


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1000.0 / iters  # us per call


def plane_rows(a, rng, demo_pairs, ypos, eye):
    from dh3d_amd.utils import batched_knn
    tA, tY, tT0, Tgt = demo_pairs
    P, N, T = a.pairs, a.points, a.iterations
    out = dict(k=16)
    out["knn_us"] = timed(lambda: batched_knn(tA, 16), a.iters)
    nbr = batched_knn(tA, 16)[0]
    out["normals_us"] = timed(lambda: reg.estimate_normals(tA, nbr=nbr), a.iters)
    nrm = reg.estimate_normals(tA, nbr=nbr)["normals"]
    out["positive_knn_us"] = timed(lambda: batched_knn(tY, 16), a.iters)
    nbr_y = batched_knn(tY, 16)[0]
    out["positive_normals_us"] = timed(lambda: reg.estimate_normals(tY, nbr=nbr_y), a.iters)
    nrm_y = reg.estimate_normals(tY, nbr=nbr_y)["normals"]
    path = 2 if N <= reg.ICP_GRID_MAX else 1
    gicp_kw = dict(anchor_normals=nrm, positive_normals=nrm_y, epsilon=1e-3)
    gicp0 = timed(lambda: reg.refine_icp_gicp(tA, tY, tT0, iterations=0, path=path, **gicp_kw), a.iters)
    for method, fn, kw in (("plane", reg.refine_icp_plane, dict(anchor_normals=nrm)), ("point", reg.refine_icp, {}),
                           ("gicp", reg.refine_icp_gicp, gicp_kw)):
        for it in sorted({5, 10, T}):
            us = timed(lambda: fn(tA, tY, tT0, iterations=it, path=path, **kw), a.iters)
            r = fn(tA, tY, tT0, iterations=it, path=path, **kw)
            dt, dd = reg.transform_errors(Tgt, r["Rt"], r["valid"])
            row = dict(refine_us=us, end_dt=float(dt.mean()), end_dt_max=float(dt.max()), end_ddeg=float(dd.mean()),
                       fitness=float(r["fitness"].mean()), rmse=float(r["rmse"].mean()))
            if method == "plane":
                row["rmse_plane"] = float(r["rmse_plane"].mean())
            if method == "gicp":
                row.update(rmse_gicp=float(r["rmse_gicp"].mean()), iteration_us=(us - gicp0) / it,
                           positive_normals_us=out["positive_knn_us"] + out["positive_normals_us"])
            out["%s_%d" % (method, it)] = row
    # both fits alone: eight anchors at the corners of a small cube with normals that span space; every positive pairs up
    t = lambda v: torch.from_numpy(v).cuda()
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
    eight = t(np.tile(0.25 * corners, (P, 1, 1)))
    n8 = t(np.tile(corners / np.float32(math.sqrt(3.0)), (P, 1, 1)))
    ny = reg.estimate_normals(ypos, k=16)["normals"]
    for method, fn, kw in (("plane", reg.refine_icp_plane, dict(anchor_normals=n8)), ("point", reg.refine_icp, {}),
                           ("gicp", reg.refine_icp_gicp, dict(anchor_normals=n8, positive_normals=ny))):
        f0 = timed(lambda: fn(eight, ypos, eye, max_dist=10.0, iterations=0, path=1, **kw), a.iters)
        fT = timed(lambda: fn(eight, ypos, eye, max_dist=10.0, iterations=T, path=1, **kw), a.iters)
        out["%s_step8_us" % method] = (fT - f0) / T     # one 8-anchor scan + one fit
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reg-pairs", type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    P, N, T = a.pairs, a.points, a.iterations
    rng = np.random.default_rng(0)
    demo = np.load(os.path.join(ROOT, "tests", "golden", "demo_clouds.npz"))
    cube = [rng.random((2 * N, 3)) * 40.0 - 20.0]
    res = dict(pairs=P, points=N, iterations=T, plan=reg.icp_plan(N, N))
    t = lambda v: torch.from_numpy(v).cuda()

    # the fit alone: one anchor, every positive within reach of it
    one = t(np.zeros((P, 1, 3), np.float32))
    ypos = t((rng.random((P, N, 3)) - 0.5).astype(np.float32))
    eye = t(np.tile(np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1), (P, 1, 1)))
    f0 = timed(lambda: reg.refine_icp(one, ypos, eye, max_dist=10.0, iterations=0, path=1), a.iters)
    fT = timed(lambda: reg.refine_icp(one, ypos, eye, max_dist=10.0, iterations=T, path=1), a.iters)
    res["fit_us"] = fit_us = (fT - f0) / T

    for name, clouds in (("demo", [demo["local_268"], demo["local_642"]]), ("cube", cube),
                         ("padded", [demo["local_268"], demo["local_642"]])):
        A, Y, Tgt, T0 = pairs(rng, clouds, P, N)
        cnt = None
        if name == "padded":
            live = (3 * N) // 4
            A[:, live:], Y[:, live:] = 100000.0, 100000.0
            cnt = torch.full((P,), live, dtype=torch.int32, device="cuda")
        tA, tY, tT0 = t(A), t(Y), t(T0)
        entry = {}
        for path, label in ((2, "grid"), (1, "scan")):
            if path == 2 and N > reg.ICP_GRID_MAX:
                continue
            n = max(1, a.iters // (4 if path == 1 else 1))
            u0 = timed(lambda: reg.refine_icp(tA, tY, tT0, None, cnt, cnt, iterations=0, path=path), n)
            uT = timed(lambda: reg.refine_icp(tA, tY, tT0, None, cnt, cnt, iterations=T, path=path), n)
            per = (uT - u0) / T
            entry[label] = dict(refine_us=uT, evaluate_us=u0, iteration_us=per, associate_us=per - fit_us)
        out = reg.refine_icp(tA, tY, tT0, None, cnt, cnt, iterations=T)
        dt, dd = reg.transform_errors(Tgt, out["Rt"], out["valid"])
        dt0, dd0 = reg.transform_errors(Tgt, T0)
        entry.update(start_dt=float(dt0.mean()), start_ddeg=float(dd0.mean()), end_dt=float(dt.mean()), end_ddeg=float(dd.mean()),
                     fitness=float(out["fitness"].mean()), rmse=float(out["rmse"].mean()))
        res[name] = entry
        if name == "demo":
            demo_pairs = (tA, tY, tT0, Tgt)
        if name == "demo" and a.reg_pairs > 0:
            from dh3d_amd import ConfigFactory
            from dh3d_amd.model import DH3D
            model = DH3D(ConfigFactory("detection_config").getconfig()).init_synthetic(0).cuda().eval().prepare()
            q = min(a.reg_pairs, P)
            with torch.no_grad():
                res["register_clouds"] = dict(pairs=q, us=timed(lambda: reg.register_clouds(model, tA[:q], tY[:q]), a.iters))
                res["register_clouds_refined"] = dict(pairs=q, us=timed(lambda: reg.register_clouds(model, tA[:q], tY[:q], refine=True),
                                                                        a.iters))
    res["plane"] = plane_rows(a, rng, demo_pairs, ypos, eye)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
