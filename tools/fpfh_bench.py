"""Time the FPFH chain (csrc/fpfh.hip, registration.compute_fpfh) on P clouds of N points -- random subsets of the demo
clouds, rows in random order -- at K = 16 and 32: the kNN, the normals (k = 16, given ids), stage 1 (dh3d_spfh_counts) and
stage 2 (dh3d_fpfh) each on its own, and the chain compute_fpfh(points, k=K) that runs all of them; with device events
around back-to-back calls after a warm-up: `--kernel-iters` (200) for the single kernels, so that a window is 20-60 ms,
`--iters` (20) for the calls of a millisecond and more.  These are WARM numbers: every iteration reads the same inputs (80 MB
in all, a cloud's rows 480 KiB), which stay in the caches between iterations.  Next to each stage its floor: the bytes its gathers fetch (stage 1: 24
per pair, the neighbour's point and normal; stage 2: 49 per pair, the neighbour's point, its pair count and its 36-byte
count row) over the copy bandwidth measured here (a 256 MiB device-to-device copy, read + write); "stream_bytes" are the ids,
the point's own rows and the output, read or written once in order.  "local": the same two kernels on lists that name the
K rows after the point (the same arithmetic, gathers that fall on neighbouring rows): the difference to the real lists is
what the scattered gathers cost.  "zero_normals": stage 1 on the real lists with every normal zero -- the same ids, the same
gathers (the kernel requests the four rows of a pair before it tests any of them) and stores, but no pair is usable, so the
float64 frame, its two square roots, divisions and atan2 are not run: the difference is what that arithmetic costs.
register_fpfh is timed on `--reg-pairs` pairs (a cloud against its moved, permuted, noisy
copy) with its pose errors.  Prints one JSON line and writes it to profiles/fpfh_bench.json.

    python tools/fpfh_bench.py [--clouds 64] [--points 8192] [--iters 20] [--kernel-iters 200] [--reg-pairs 8]
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
from dh3d_amd import _lib as L  # noqa: E402
from dh3d_amd import registration as reg  # noqa: E402
from dh3d_amd.utils import batched_knn  # noqa: E402


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


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


def stages(x, nrm, nbr, iters):
    """Stage 1 and stage 2 alone, on given normals and ids: (us, us)."""
    P, N, K = nbr.shape
    lib = L.lib()
    counts = torch.empty((P, N, 36), dtype=torch.uint8, device=x.device)
    out = torch.empty((P, N, 36), dtype=torch.float32, device=x.device)

    def one():
        L.check(lib.dh3d_spfh_counts(L.ptr(x), 3, L.ptr(nrm), 3, None, L.ptr(nbr), P, N, K, 0.0, L.ptr(counts), L.stream_ptr()), "s1")

    def two():
        L.check(lib.dh3d_fpfh(L.ptr(x), 3, None, L.ptr(nbr), L.ptr(counts), None, P, N, K, N, 0.0, L.ptr(out), L.stream_ptr()), "s2")
    return timed(one, iters), timed(two, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=64)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--reg-pairs", type=int, default=8)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    P, N = a.clouds, a.points
    rng = np.random.default_rng(0)
    demo = np.load(os.path.join(ROOT, "tests", "golden", "demo_clouds.npz"))
    clouds = [demo["local_268"], demo["local_642"]]
    X = np.stack([clouds[p % 2][rng.permutation(len(clouds[p % 2]))[:N]] for p in range(P)]).astype(np.float32)
    x = torch.from_numpy(X).cuda()
    res = dict(clouds=P, points=N, iters=a.iters, kernel_iters=a.kernel_iters, warm=True)
    ki = a.kernel_iters

    big = torch.empty((256 << 20,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(big)
    copy_us = timed(lambda: dst.copy_(big), ki)
    bw = 2.0 * big.numel() / (copy_us * 1e-6)            # bytes per second, read + write
    res["copy_gbps"] = bw / 1e9
    del big, dst

    nbr16 = batched_knn(x, 16)[0]
    res["normals_us"] = timed(lambda: reg.estimate_normals(x, nbr=nbr16), ki)
    nrm = reg.estimate_normals(x, nbr=nbr16)["normals"]
    for K in (16, 32):
        row = dict(knn_us=timed(lambda: batched_knn(x, K), a.iters))
        nbr = batched_knn(x, K)[0]
        row["stage1_us"], row["stage2_us"] = stages(x, nrm, nbr, ki)
        local = ((torch.arange(N, device="cuda")[:, None] + torch.arange(1, K + 1, device="cuda")[None, :]) % N).to(torch.int32)
        row["stage1_local_us"], row["stage2_local_us"] = stages(x, nrm, local[None].expand(P, N, K).contiguous(), ki)
        row["stage1_zero_normals_us"] = stages(x, torch.zeros_like(nrm), nbr, ki)[0]
        pairs = P * N * K
        g1, g2 = 24 * pairs, 49 * pairs
        row["stage1_gather_bytes"], row["stage2_gather_bytes"] = g1, g2
        row["stage1_stream_bytes"] = 4 * pairs + P * N * (24 + 36)
        row["stage2_stream_bytes"] = 4 * pairs + P * N * (12 + 36 + 144)
        row["stage1_floor_us"], row["stage2_floor_us"] = g1 / bw * 1e6, g2 / bw * 1e6
        row["chain_us"] = timed(lambda: reg.compute_fpfh(x, k=K), a.iters)
        row["chain_given_us"] = timed(lambda: reg.compute_fpfh(x, nrm, nbr=nbr), ki)   # stage 1 + stage 2 + the allocations
        res["k%d" % K] = row

    q = min(a.reg_pairs, P)
    if q > 0:
        Y, T = np.zeros((q, N, 3), np.float32), np.zeros((q, 3, 4))
        for p in range(q):
            R, t = rot(rng.standard_normal(3), rng.uniform(0.2, 1.0)), rng.standard_normal(3) * 2.0
            Y[p] = ((X[p].astype(np.float64) - t) @ R + rng.normal(0.0, 0.02, (N, 3)))[rng.permutation(N)]
            T[p] = np.concatenate([R, t[:, None]], axis=1)
        y = torch.from_numpy(Y).cuda()
        for label, kw in (("register_fpfh", {}), ("register_fpfh_refined", dict(refine=True)),
                          ("register_fpfh_ratio_mutual", dict(match={"ratio": 0.9, "mutual": True}))):
            us = timed(lambda: reg.register_fpfh(x[:q], y, **kw), a.iters)
            out = reg.register_fpfh(x[:q], y, **kw)
            dt, dd = reg.transform_errors(T, out["Rt"], out["valid"])
            res[label] = dict(pairs=q, keypoints=int(out["match"].shape[1]), us=us, valid=int(out["valid"].sum()),
                              dt_mean=float(dt.mean()), dt_max=float(dt.max()), ddeg_mean=float(dd.mean()), ddeg_max=float(dd.max()),
                              inlier_ratio=float(out["inlier_ratio"].mean()), trials=float(out["trials"].float().mean()))
            if "num_kept" in out:  # the correspondences the ratio test and the mutual check leave to RANSAC
                res[label]["kept"] = float(out["num_kept"].float().mean())
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "fpfh_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
