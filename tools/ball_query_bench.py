"""Times query_ball_point four ways and prints ONE JSON line:
  scan        the scan kernel (dh3d_query_ball_point)
  sort+grid   dh3d_spatial_sort_cells + the cell-list kernel (what the op runs where the plan says 1)
  grid        the cell-list kernel alone (a caller that already holds the sort, as the model does)
  torch       what a user has without this library: torch.cdist + mask + sort
on b = 8, n = 8192 uniform clouds in [-1, 1]^3 with m = 1024 FPS picks as queries, (radius, nsample) in (0.1, 32),
(0.2, 32), (0.4, 64); m = n = 8192 at (0.1, 32); and the demo clouds (tests/golden/demo_clouds.npz) in metres.  Per entry:
median / min / max in microseconds of --launches launches after --warmup, each between a pair of device events on the
current stream (the C entry points on preallocated outputs; the torch formulation through torch), plus the median hit count so that a reader sees how full the balls are.  Needs a GPU; there is no fallback.

    python tools/ball_query_bench.py [--launches 60] [--warmup 10] [--quick]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return {"median_us": round(us[len(us) // 2], 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}


def torch_ball_query(radius, nsample, x1, x2):
    """cdist + mask + sort: the nsample lowest hit indices, padded with the first (not bit-exact at the radius: cdist's
    own rounding) -- the formulation a user writes without the library."""
    n = x1.shape[1]
    d = torch.cdist(x2, x1)
    key = torch.where(d < radius, torch.arange(n, device=x1.device).expand_as(d), torch.full_like(d, n, dtype=torch.long))
    idx = key.sort(dim=-1).values[..., :nsample]
    cnt = (idx < n).sum(-1)
    idx = torch.where(idx < n, idx, idx[..., :1])
    return idx.int(), cnt.int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=60, help="timed launches per entry (>= 50)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="skip the torch formulation (it allocates b*m*n*8 bytes a launch)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ball_query_bench needs a GPU")
    from dh3d_amd import _lib as L, ops, pm
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2024)
    cube = torch.from_numpy(rng.uniform(-1, 1, (8, 8192, 3)).astype(np.float32)).to(dev)
    picks = ops.farthest_point_sample(1024, cube).long()
    fps_q = torch.gather(cube, 1, picks[..., None].expand(-1, -1, 3)).contiguous()
    demo = np.load(os.path.join(ROOT, "tests", "golden", "demo_clouds.npz"))
    cases = [("cube_m1024_r0.1_k32", cube, fps_q, 0.1, 32), ("cube_m1024_r0.2_k32", cube, fps_q, 0.2, 32),
             ("cube_m1024_r0.4_k64", cube, fps_q, 0.4, 64), ("cube_m8192_r0.1_k32", cube, cube, 0.1, 32)]
    for name in ("global_c", "local_268"):
        x = torch.from_numpy(np.ascontiguousarray(demo[name][None].repeat(8, 0))).to(dev)
        q = torch.gather(x, 1, ops.farthest_point_sample(x.shape[1] // 8, x).long()[..., None].expand(-1, -1, 3)).contiguous()
        # radius in metres: the first of the ladder whose median ball holds 8-64 points (counted up to 128)
        fits = [(r, float(pm.ball_query_scan(r, 128, x, q)[1].float().median())) for r in (0.5, 0.75, 1.0, 1.5, 2.0, 3.0)]
        radius = next((r for r, med in fits if 8 <= med <= 64), None)
        assert radius is not None, "%s: no radius of the ladder gives a median ball of 8-64 points: %s" % (name, fits)
        cases.append(("demo_%s_r%g_k32" % (name, radius), x, q, radius, 32))
    out = {"tool": "ball_query_bench", "device": torch.cuda.get_device_name(0), "launches": args.launches, "cases": {}}
    lib, P, st = L.lib(), L.ptr, L.stream_ptr()
    for name, x1, x2, radius, k in cases:
        b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
        sort = pm.spatial_sort_cells(x1)
        ref = pm.ball_query_scan(radius, k, x1, x2)
        got = pm.ball_query_grid(radius, k, x1, x2, sort=sort)
        assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]), name
        # the timed calls are the C entry points on preallocated outputs: nothing but the launches lies between the events
        idx, cnt = torch.empty_like(ref[0]), torch.empty_like(ref[1])
        srt, gbox, cells = (torch.empty_like(t) for t in sort)
        rad = torch.full((1,), radius, dtype=torch.float32, device=dev)

        def scan():
            L.check(lib.dh3d_query_ball_point(b, n, m, radius, k, P(x1), P(x2), P(idx), P(cnt), st), "scan")

        def grid(s=sort):
            L.check(lib.dh3d_query_ball_point_grid(b, n, m, P(rad), 0, k, P(s[0]), P(s[1]), P(s[2]), P(x2), P(idx), P(cnt), st),
                    "grid")

        def sort_grid():
            L.check(lib.dh3d_spatial_sort_cells(P(x1), b, n, P(srt), P(gbox), P(cells), st), "sort")
            grid((srt, gbox, cells))

        e = {"b": b, "n": n, "m": m, "radius": radius, "nsample": k, "plan": pm.ball_query_plan(n, m, k),
             "median_pts_cnt": float(ref[1].float().median()), "full_rows": float((ref[1] == k).float().mean()),
             "scan": timed(scan, args.launches, args.warmup), "sort+grid": timed(sort_grid, args.launches, args.warmup),
             "grid": timed(grid, args.launches, args.warmup)}
        assert torch.equal(idx, ref[0]) and torch.equal(cnt, ref[1]), name
        if not args.quick:
            e["torch"] = timed(lambda: torch_ball_query(radius, k, x1, x2), max(args.launches, 50), 3)
        out["cases"][name] = e
    print(json.dumps(out))


if __name__ == "__main__":
    main()
