"""Times knn_point two ways and prints ONE JSON line:
  knn_point   ops.knn_point (dh3d_knn_point: the fused kernel for c = 3, k <= 64)
  torch       the composition a user has without it: the [b,m,n] squared-distance matrix (broadcast difference, square,
              sum over c) followed by torch.topk(k, largest=False, sorted=True)
on uniform clouds in [0, 1]^3 at (b, n, m, k) = (8, 8192, 1024, 32), (8, 8192, 8192, 8), (8, 16384, 2048, 64) and the
reference demo's (32, 512, 128, 64).  Per entry: median / min / max in microseconds of --launches calls after --warmup,
each between a pair of device events on the current stream, and the peak extra device memory of one call.  Before timing,
the two are compared on the rows whose k + 1 smallest distances are distinct (elsewhere topk's tie order is its own).
Needs a GPU; there is no fallback.

    python tools/knn_point_bench.py [--launches 60] [--warmup 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((8, 8192, 1024, 32), (8, 8192, 8192, 8), (8, 16384, 2048, 64), (32, 512, 128, 64))


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


def peak_extra_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(peak)


def torch_knn_point(k, x1, x2):
    d = ((x1[:, None, :, :] - x2[:, :, None, :]) ** 2).sum(-1)      # [b,m,n]
    val, idx = torch.topk(d, k, dim=-1, largest=False, sorted=True)
    return val, idx.int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=60, help="timed calls per entry (>= 50)")
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_point_bench needs a GPU")
    from dh3d_amd import ops, pm
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2025)
    out = {"tool": "knn_point_bench", "device": torch.cuda.get_device_name(0), "launches": args.launches, "cases": {}}
    for b, n, m, k in SHAPES:
        x1 = torch.from_numpy(rng.random((b, n, 3), dtype=np.float32)).to(dev)
        x2 = torch.from_numpy(rng.random((b, m, 3), dtype=np.float32)).to(dev)
        val, idx = ops.knn_point(k, x1, x2)
        tval, tidx = torch_knn_point(k + 1, x1[:1], x2[:1])
        judge = (tval[0, :, 1:] > tval[0, :, :-1]).all(-1)
        agree = float((idx[0][judge] == tidx[0][judge][:, :k]).all(-1).float().mean())
        assert float(judge.float().mean()) > 0.9 and agree > 0.99, (b, n, m, k, agree)   # (torch rounds the sum its own way)
        del tval, tidx
        e = {"b": b, "n": n, "m": m, "k": k, "plan": pm.knn_point_plan(n, m, 3, k), "rows_agreeing_with_torch": agree,
             "knn_point": timed(lambda: ops.knn_point(k, x1, x2), args.launches, args.warmup),
             "knn_point_peak_extra_bytes": peak_extra_bytes(lambda: ops.knn_point(k, x1, x2)),
             "torch": timed(lambda: torch_knn_point(k, x1, x2), args.launches, min(args.warmup, 3)),
             "torch_peak_extra_bytes": peak_extra_bytes(lambda: torch_knn_point(k, x1, x2))}
        e["torch_over_knn_point"] = round(e["torch"]["median_us"] / e["knn_point"]["median_us"], 2)
        out["cases"]["b%d_n%d_m%d_k%d" % (b, n, m, k)] = e
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
