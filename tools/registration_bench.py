"""Time the registration kernels (csrc/registration.hip) on P cloud pairs x M keypoints, D = 128: dh3d_match_descriptors
and dh3d_ransac_rigid separately, with device events around `iters` back-to-back calls after a warm-up.  The RANSAC time
depends on the trial count, so three inlier shares are timed: 0.5 (10-40 trials: one round of 256), 0.2 (~570 trials:
three rounds) and 0 (max_trials + 1 = 10001 trials: 40 rounds, the worst case).  Prints one JSON line.

dh3d_gnc_rigid runs on the same three fixtures (`gnc_inliers*`: median time and spread over `--reps` windows alternating
with ransac_rigid, the fit count, validity, and both estimators' mean pose errors against the fixtures' truth) and on
8 x 4096 correspondences, in windows of the same `--iters` calls on every fixture.  Its fit count depends on the extent and
the threshold only: `gnc_iterations_equal` says whether the three fixtures ran the same fits, `gnc_times_agree` whether the
three medians lie within the largest spread of their windows.

dh3d_match_descriptors2 (csrc/match.hip) is timed beside the plain matcher at 64 x 512 x 512 x 128 and 8 x 4096 x 4096 x 36,
`--reps` windows of `iters` calls each, the variants alternating inside a repetition: one plain call, two (the second with
the roles swapped: what a mutual check costs without the new entry), the new entry forward only (match={}) and with both
filters.  Each figure is the median over the repetitions with its spread (max - min); `ok` says whether the new call stays
within the plain matcher's time plus that matcher's spread.  ransac_rigid is then timed on the unfiltered and on the
filtered ids of fixtures whose outliers carry unrelated descriptors.  That part is also written to --out.

    python tools/registration_bench.py [--pairs 64] [--keypoints 512] [--iters 20] [--reps 5] [--out profiles/match2_bench.json]
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


def desc_rows(rng, P, M, D, inlier_share, noise=0.03):
    """As rows, but an outlier's positive also carries an unrelated descriptor, and the true partners differ by `noise` per
    component: what the ratio test and the mutual check are there to tell apart."""
    ra, rb = rows(rng, P, M, D, 1.0)
    out = torch.from_numpy(rng.random((P, M)) >= inlier_share).cuda()
    unrelated = torch.from_numpy(rng.standard_normal((P, M, D)).astype(np.float32)).cuda()
    unrelated /= unrelated.norm(dim=-1, keepdim=True)
    rb[:, :, 3:3 + D] += noise * torch.from_numpy(rng.standard_normal((P, M, D)).astype(np.float32)).cuda()
    rb[:, :, 3:3 + D] = torch.where(out[:, :, None], unrelated, rb[:, :, 3:3 + D])
    rb[:, :, :3] = torch.where(out[:, :, None], torch.from_numpy((rng.random((P, M, 3)) * 40 - 20).astype(np.float32)).cuda(),
                               rb[:, :, :3])
    return ra, rb


def match2_times(rng, P, M, D, iters, reps):
    """The four matcher variants on one shape, alternating inside every repetition: median and spread in us."""
    ra, rb = desc_rows(rng, P, M, D, 0.5)
    a, b = ra[:, :, 3:3 + D], rb[:, :, 3:3 + D]
    cnt = torch.full((P,), M, dtype=torch.int32, device="cuda")
    variants = dict(
        plain_one=lambda: reg.match_descriptors(a, cnt, b, cnt),
        plain_two=lambda: (reg.match_descriptors(a, cnt, b, cnt), reg.match_descriptors(b, cnt, a, cnt)),
        match2_forward=lambda: reg.match_descriptors2(a, cnt, b, cnt),
        match2_ratio_mutual=lambda: reg.match_descriptors2(a, cnt, b, cnt, ratio=0.9, mutual=True))
    runs = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            runs[k].append(timed(fn, iters))
    row = dict(pairs=P, keypoints=M, desc_dim=D, iters=iters, reps=reps)
    for k, v in runs.items():
        row[k + "_us"] = dict(median=float(np.median(v)), spread=float(max(v) - min(v)))
    med = lambda k: row[k + "_us"]["median"]
    row["forward_ok"] = med("match2_forward") <= med("plain_one") + row["plain_one_us"]["spread"]
    row["both_ok"] = med("match2_ratio_mutual") <= med("plain_two") + row["plain_two_us"]["spread"]
    row["kept"] = float(reg.match_descriptors2(a, cnt, b, cnt, ratio=0.9, mutual=True)["num_kept"].float().mean())
    return row


TRUTH = np.concatenate([np.eye(3), np.full((3, 1), -3.0)], axis=1)  # rows' pose: anchor = positive - 3


def pose_errors(out):
    """Mean translation / rotation error of a fit's poses against the fixtures' truth (transform_errors: a pair without a
    pose counts 3 m / 6 deg, eval_align.m's catch), and how many pairs are valid."""
    dt, dd = reg.transform_errors(np.broadcast_to(TRUTH, (out["Rt"].shape[0], 3, 4)), out["Rt"], out["valid"])
    return dict(valid=int(out["valid"].sum()), rte_mean=float(dt.mean()), rre_mean=float(dd.mean()))


def estimators(xa, xb, ids, cnt, iters, reps, ransac_iters=None):
    """ransac_rigid and gnc_rigid on the same correspondences, alternating inside every repetition: each one's median time
    and spread (max - min) in us over `reps` windows of `iters` calls (recorded in the entry), its validity and pose errors,
    RANSAC's trials and GNC's fits.  ransac_iters: a shorter window for RANSAC alone, where it runs to its trial cap; GNC's
    window is the same on every fixture, so that its times compare."""
    fits = dict(ransac=lambda: reg.ransac_rigid(xa, xb, ids, cnt), gnc=lambda: reg.gnc_rigid(xa, xb, ids, cnt))
    calls = dict(ransac=iters if ransac_iters is None else ransac_iters, gnc=iters)
    runs = {k: [] for k in fits}
    for _ in range(reps):
        for k, fn in fits.items():
            runs[k].append(timed(fn, calls[k]))
    res = {}
    for k, fn in fits.items():
        out = fn()
        res[k] = dict(us=float(np.median(runs[k])), us_spread=float(max(runs[k]) - min(runs[k])), iters=calls[k], reps=reps,
                      **pose_errors(out))
        fits_run = out["trials"].cpu().numpy()
        res[k].update({"iterations_min" if k == "gnc" else "trials_min": int(fits_run.min()),
                       "iterations_max" if k == "gnc" else "trials_max": int(fits_run.max())})
    return res


def ransac_on_filtered(rng, P, M, D, iters):
    """ransac_rigid on the plain ids and on the ratio + mutual ids of the outlier fixtures; gnc_rigid beside it."""
    cnt = torch.full((P,), M, dtype=torch.int32, device="cuda")
    res = {}
    for share in (0.5, 0.2):
        ra, rb = desc_rows(rng, P, M, D, share)
        a, b = ra[:, :, 3:3 + D], rb[:, :, 3:3 + D]
        plain, _ = reg.match_descriptors(a, cnt, b, cnt)
        kept = reg.match_descriptors2(a, cnt, b, cnt, ratio=0.9, mutual=True)
        row = dict(kept=float(kept["num_kept"].float().mean()))
        for label, ids in (("unfiltered", plain), ("filtered", kept["match"])):
            out = reg.ransac_rigid(ra, rb, ids, cnt)
            row[label] = dict(us=timed(lambda: reg.ransac_rigid(ra, rb, ids, cnt), iters), valid=int(out["valid"].sum()),
                              trials=float(out["trials"].float().mean()), inlier_ratio=float(out["inlier_ratio"].mean()))
            both = estimators(ra, rb, ids, cnt, iters, 3)
            row[label].update(ransac_rte_mean=both["ransac"]["rte_mean"], ransac_rre_mean=both["ransac"]["rre_mean"],
                              gnc=both["gnc"])
        res["inliers%g" % share] = row
    return res


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "match2_bench.json"))
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
        both = estimators(ra, rb, match, cnt, a.iters, a.reps, ransac_iters=max(1, a.iters // (10 if share == 0 else 1)))
        res["gnc_inliers%g" % share] = dict(both["gnc"], ransac=both["ransac"])
    # the two conditions on the GNC entries: one fit count for every inlier share, and therefore one time (within the
    # spread of the repeated windows)
    g = [res["gnc_inliers%g" % s] for s in (0.5, 0.2, 0.0)]
    res["gnc_iterations_equal"] = len({(e["iterations_min"], e["iterations_max"]) for e in g}) == 1
    res["gnc_times_agree"] = max(e["us"] for e in g) - min(e["us"] for e in g) <= max(e["us_spread"] for e in g)
    # the pair that fills the staging: 8 x 4096 correspondences at 50 % inliers
    ra4, rb4 = rows(np.random.default_rng(1), 8, 4096, 4, 0.5)  # (its own stream: the fixtures below stay what they were)
    cnt4 = torch.full((8,), 4096, dtype=torch.int32, device="cuda")
    ids4 = torch.arange(4096, dtype=torch.int32, device="cuda").repeat(8, 1)
    res["gnc_8x4096_inliers0.5"] = estimators(ra4, rb4, ids4, cnt4, a.iters, a.reps)
    res["register_us"] = timed(lambda: reg.register(ra, cnt, rb, cnt), max(1, a.iters // 10))
    m2 = dict(shape_512x128=match2_times(rng, 64, 512, 128, a.iters, a.reps),
              shape_4096x36=match2_times(rng, 8, 4096, 36, a.iters, a.reps),
              ransac=ransac_on_filtered(rng, P, M, D, a.iters))
    res["match2"] = m2
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(m2) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
