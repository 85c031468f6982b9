"""Time the registration kernels (csrc/registration.hip) on P cloud pairs x M keypoints, D = 128: dh3d_match_descriptors
and dh3d_ransac_rigid separately, with device events around `iters` back-to-back calls after a warm-up.  The RANSAC time
depends on the trial count, so three inlier shares are timed: 0.5 (10-40 trials: one round of 256), 0.2 (~570 trials:
three rounds) and 0 (max_trials + 1 = 10001 trials: 40 rounds, the worst case).  Prints one JSON line.

    python tools/registration_bench.py [--pairs 64] [--keypoints 512] [--iters 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dh3d_amd import registration as reg  # noqa: E402


def rows(rng, P, M, D, inlier_share):
    x = (rng.random((P, M, 3)) * 40 - 20).astype(np.float32)
    y = x + np.float32(3.0)  # a translation; outliers below get random positives
    da = rng.standard_normal((P, M, D)).astype(np.float32)
    da /= np.linalg.norm(da, axis=-1, keepdims=True)
    db = da.copy()
    out = rng.random((P, M)) >= inlier_share
    y[out] = (rng.random((int(out.sum()), 3)) * 40 - 20).astype(np.float32)
    ra = np.concatenate([x, da, np.zeros((P, M, 1), np.float32)], -1)
    rb = np.concatenate([y, db, np.zeros((P, M, 1), np.float32)], -1)
    return torch.from_numpy(ra).cuda(), torch.from_numpy(rb).cuda()


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--keypoints", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    P, M, D = a.pairs, a.keypoints, 128
    rng = np.random.default_rng(0)
    cnt = torch.full((P,), M, dtype=torch.int32, device="cuda")
    res = dict(pairs=P, keypoints=M, desc_dim=D)
    ra, rb = rows(rng, P, M, D, 0.5)
    res["match_us"] = timed(lambda: reg.match_descriptors(ra[:, :, 3:131], cnt, rb[:, :, 3:131], cnt), a.iters)
    for share in (0.5, 0.2, 0.0):
        ra, rb = rows(rng, P, M, D, share)
        match, _ = reg.match_descriptors(ra[:, :, 3:131], cnt, rb[:, :, 3:131], cnt)
        out = reg.ransac_rigid(ra, rb, match, cnt)
        trials = out["trials"].cpu().numpy()
        us = timed(lambda: reg.ransac_rigid(ra, rb, match, cnt), max(1, a.iters // (10 if share == 0 else 1)))
        res["ransac_inliers%g" % share] = dict(us=us, trials_min=int(trials.min()), trials_max=int(trials.max()))
    res["register_us"] = timed(lambda: reg.register(ra, cnt, rb, cnt), max(1, a.iters // 10))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
