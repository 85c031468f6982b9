"""Time the ISS detector (csrc/iss.hip, registration.iss_keypoints) on P street scenes of N points (bench.py's
scene_like_clouds scaled to +-20 m) at 2.0 / 1.5 m, with device events around back-to-back calls after a warm-up:
  iss_us            the whole call (pack, sort, moments, suppression, select);
  sort_us           dh3d_spatial_sort_cells alone (pm.spatial_sort_cells on the same clouds);
  kernels           the call split by kernel -- sort, moments, nms, select -- from a `rocprofv3 --kernel-trace --stats` run of
                    a child process of this tool (`--no-trace` skips it; "not measured" where the trace could not be read);
  tensor_ops_us     a chunked tensor-op statement of the same rule (float32 memberships by broadcasting, float64 moments by
                    einsum, torch.linalg.eigvalsh, the suppression as a masked comparison) on `--torch-clouds` of the clouds,
                    per cloud, next to the kernel's time per cloud; its keypoints are compared with the kernel's;
  register_fpfh     on tools/fpfh_bench.py's pairs (a demo cloud against its moved, permuted, noisy copy), with the spread
                    keypoints (4096 of 8192 by index) and with ISS keypoints: time and error from the truth.
What bounds the kernels is told from the counts next to the times: records walked per point (the box's) against members
(the ball's), and the float64 operations the moments need.  Prints one JSON line and writes it to profiles/iss_bench.json.

    python tools/iss_bench.py [--clouds 64] [--points 8192] [--iters 20] [--torch-clouds 2] [--reg-pairs 8] [--no-trace]
"""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from dh3d_amd import pm  # noqa: E402
from dh3d_amd import registration as reg  # noqa: E402

R_S, R_N, GAMMA, MIN_NB = 2.0, 1.5, 0.975, 5
NOT_MEASURED = "not measured"


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


def scenes(P, N):
    return (bench.scene_like_clouds(P, N, 2009, "cpu") * 20.0).cuda()


def tensor_ops_iss(x, chunk=512):
    """The rule on ONE cloud [N, 3] by tensor ops -> (ids of the keypoints, most salient first; saliency [N])."""
    N = x.shape[0]
    x64 = x.double()
    rs2, rn2 = torch.tensor(R_S, device=x.device) ** 2, torch.tensor(R_N, device=x.device) ** 2
    sal = torch.zeros(N, device=x.device)
    nt = torch.zeros(N, dtype=torch.int64, device=x.device)
    for s in range(0, N, chunk):
        d = x[None, :, :] - x[s:s + chunk, None, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        S = d2 < rs2
        nt[s:s + chunk] = (d2 < rn2).sum(1)
        e = (x64[None, :, :] - x64[s:s + chunk, None, :]) * S[:, :, None]
        m = S.sum(1).double()
        u = e.sum(1) / m[:, None]
        C = torch.einsum("ija,ijb->iab", e, e) / m[:, None, None] - u[:, :, None] * u[:, None, :]
        lam = torch.linalg.eigvalsh(C).flip(1)
        ok = (m >= MIN_NB) & (lam[:, 1] < GAMMA * lam[:, 0]) & (lam[:, 2] < GAMMA * lam[:, 1]) & (lam[:, 2] > 0)
        sal[s:s + chunk] = torch.where(ok, lam[:, 2], torch.zeros_like(lam[:, 2])).float()
    keep = torch.zeros(N, dtype=torch.bool, device=x.device)
    idx = torch.arange(N, device=x.device)
    for s in range(0, N, chunk):
        d = x[None, :, :] - x[s:s + chunk, None, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        T = (d2 < rn2) & (idx[None, :] != idx[s:s + chunk, None])
        si = sal[s:s + chunk, None]
        beaten = (T & ((sal[None, :] > si) | ((sal[None, :] == si) & (idx[None, :] < idx[s:s + chunk, None])))).any(1)
        keep[s:s + chunk] = (sal[s:s + chunk] > 0) & (nt[s:s + chunk] >= MIN_NB) & ~beaten
    k = idx[keep]
    order = torch.argsort(sal[k], descending=True, stable=True)   # (k ascends: a stable sort keeps the lowest index first)
    return k[order], sal


def kernel_split(P, N, iters):
    """The per-kernel averages (us) of the detector's launches, from a rocprofv3 kernel trace of a child process."""
    out = tempfile.mkdtemp(prefix="iss_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "iss", "--", sys.executable, os.path.abspath(__file__),
           "--child", "--clouds", str(P), "--points", str(N), "--iters", str(iters)]
    try:
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        db = sorted(glob.glob(os.path.join(out, "**", "*.db"), recursive=True))[0]
        c = sqlite3.connect(db)
        cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
        namecol = "name" if "name" in cols else "kernel_name"
        rows = c.execute("select %s, count(*), avg(end-start) from kernels group by %s" % (namecol, namecol)).fetchall()
    except Exception as exc:  # the profiler is not there, or its output has another form
        return dict(status=NOT_MEASURED, why=repr(exc)[:200])
    split = dict(sort=0.0, moments=0.0, nms=0.0, select=0.0)
    for name, calls, avg in rows:
        per_call = avg / 1e3 * calls / (iters + 1)     # (the child makes iters + 1 calls; the sort is several launches a call)
        if "iss_moments" in name:
            split["moments"] += per_call
        elif "iss_nms" in name:
            split["nms"] += per_call
        elif "iss_select" in name:
            split["select"] += per_call
        elif "cloud_pack" in name or "spatial_sort" in name:
            split["sort"] += per_call
    split["kernels_seen"] = sorted(set(n[:60] for n, _, _ in rows))
    return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=64)
    ap.add_argument("--points", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-clouds", type=int, default=2)
    ap.add_argument("--reg-pairs", type=int, default=8)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true", help="the traced child: the detector's calls and nothing else")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    P, N = a.clouds, a.points
    x = scenes(P, N)
    if a.child:
        for _ in range(a.iters + 1):
            reg.iss_keypoints(x, None, R_S, R_N)
        torch.cuda.synchronize()
        return
    res = dict(clouds=P, points=N, iters=a.iters, salient_radius=R_S, non_max_radius=R_N, warm=True)
    rs = torch.full((P,), R_S, device="cuda")
    rn = torch.full((P,), R_N, device="cuda")
    res["iss_us"] = timed(lambda: reg.iss_keypoints(x, None, rs, rn), 5 * a.iters)      # (a window of ~0.2 s)
    res["sort_us"] = timed(lambda: pm.spatial_sort_cells(x), 5 * a.iters)
    out = reg.iss_keypoints(x, None, rs, rn)
    nb = out["num_neighbors"].double()
    res["keypoints_mean"] = float(out["count"].double().mean())
    res["members_salient_mean"], res["members_nonmax_mean"] = float(nb[:, :, 0].mean()), float(nb[:, :, 1].mean())
    res["salient_share"] = float((out["saliency"] > 0).double().mean())
    # what the moments need: per member 3 conversions and subtractions and 9 multiply-adds in float64; per record of the box
    # (about (2r)^3 / (4/3 pi r^3) = 1.9 times the members of the wider ball) the float32 test
    res["moments_f64_flop"] = float(nb[:, :, 0].sum()) * 21.0
    res["kernels"] = dict(status=NOT_MEASURED) if a.no_trace else kernel_split(P, N, a.iters)

    q = min(a.torch_clouds, P)
    if q > 0:
        res["tensor_ops_us_per_cloud"] = timed(lambda: [tensor_ops_iss(x[p]) for p in range(q)], 2) / q
        res["iss_us_per_cloud"] = res["iss_us"] / P
        same = 0
        for p in range(q):
            ids, sal = tensor_ops_iss(x[p])
            mine = out["ids"][p, :int(out["count"][p])].long()
            same += int(len(ids) == len(mine) and bool((ids == mine).all()))
        res["tensor_ops_same_keypoints"] = "%d of %d clouds" % (same, q)

    q = min(a.reg_pairs, P)
    if q > 0:   # tools/fpfh_bench.py's pairs
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from fpfh_bench import rot
        rng = np.random.default_rng(0)
        demo = np.load(os.path.join(ROOT, "tests", "golden", "demo_clouds.npz"))
        clouds = [demo["local_268"], demo["local_642"]]
        X = np.stack([clouds[p % 2][rng.permutation(len(clouds[p % 2]))[:N]] for p in range(P)]).astype(np.float32)[:q]
        Y, T = np.zeros((q, N, 3), np.float32), np.zeros((q, 3, 4))
        for p in range(q):
            R, t = rot(rng.standard_normal(3), rng.uniform(0.2, 1.0)), rng.standard_normal(3) * 2.0
            Y[p] = ((X[p].astype(np.float64) - t) @ R + rng.normal(0.0, 0.02, (N, 3)))[rng.permutation(N)]
            T[p] = np.concatenate([R, t[:, None]], axis=1)
        xa, y = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
        iss = {"method": "iss", "salient_radius": R_S, "non_max_radius": R_N}
        for label, kw in (("register_fpfh_spread", {}), ("register_fpfh_iss", dict(keypoints=iss))):
            us = timed(lambda: reg.register_fpfh(xa, y, **kw), a.iters)
            o = reg.register_fpfh(xa, y, **kw)
            dt, dd = reg.transform_errors(T, o["Rt"], o["valid"])
            res[label] = dict(pairs=q, keypoints=float(o["num_corr"].double().mean()), us=us, valid=int(o["valid"].sum()),
                              failed=int(((dt > 2) | (dd > 5)).sum()), dt_mean=float(dt.mean()), dt_max=float(dt.max()),
                              ddeg_mean=float(dd.mean()), ddeg_max=float(dd.max()),
                              inlier_ratio=float(o["inlier_ratio"].mean()), trials=float(o["trials"].float().mean()))
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "iss_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
