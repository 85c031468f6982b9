"""Times prepare_clouds (voxel grid 0.2, radius outliers 1.0 / 4, crop or pad) and prints ONE JSON line.  Per case
(B, Nraw, targetnum) = (8, 32768, 8192) and (8, 65536, 16384), on synthetic street scenes in metres (tests/prepare_reference.py
street_scene, one seed per cloud; the larger case joins two scenes 60 m apart):
  prepare      utils.prepare_clouds on the batch: median / min / max in microseconds of --launches calls after --warmup,
               each between a pair of device events on the current stream
  forward      the local (detection_config) forward of the batch it produced, DH3D.forward(points, num_valid=...), timed
               the same way in the same process
  restatement  the numpy restatement of the same batch on the host, one cloud after the other (host clock, one pass)
and the counts the batch went through.  Before timing, the op's output is compared with the restatement, bit for bit.
Needs a GPU; there is no fallback.

    python tools/prepare_bench.py [--launches 60] [--warmup 10] [--out profiles/prepare_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = ((8, 32768, 8192), (8, 65536, 16384))


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


def scene(seed, n):
    import prepare_reference as R
    a = R.street_scene(seed)
    if n > a.shape[0]:
        b = R.street_scene(seed + 1000)
        b[:, 0] += np.float32(60.0)
        a = np.concatenate([a, b], axis=0)
    return np.ascontiguousarray(a[:n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--prepare-only", action="store_true", help="time the op alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prepare_bench needs a GPU")
    import prepare_reference as R
    from dh3d_amd import ConfigFactory, utils
    from dh3d_amd.model import DH3D
    dev = torch.device("cuda:0")
    model = None if args.prepare_only else DH3D(ConfigFactory("detection_config").getconfig()).init_synthetic(0).to(dev).eval().prepare()
    out = {"tool": "prepare_bench", "device": torch.cuda.get_device_name(0), "launches": args.launches, "cases": {}}
    for B, N, T in CASES:
        clouds = [scene(100 + b, N) for b in range(B)]
        raw = torch.from_numpy(np.stack(clouds)).to(dev)
        num = torch.full((B,), N, dtype=torch.int32, device=dev)
        points, nv, counts, cen = utils.prepare_clouds(raw, num, T)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = [R.prepare_cloud(c, T) for c in clouds]
        cpu_s = time.perf_counter() - t0
        for b, c in enumerate(clouds):
            exp = R.prepare_cloud(c, T, centroid=cen[b].cpu().numpy())
            assert np.array_equal(points[b].cpu().numpy(), exp["points"]) and int(nv[b]) == exp["num_valid"], b
        e = {"B": B, "Nraw": N, "targetnum": T, "counts": counts.cpu().tolist(), "num_valid": nv.cpu().tolist(),
             "prepare": timed(lambda: utils.prepare_clouds(raw, num, T), args.launches, args.warmup),
             "restatement_cpu_ms": round(cpu_s * 1e3, 1)}
        if model is not None:
            with torch.no_grad():
                e["forward"] = timed(lambda: model(points, num_valid=nv), args.launches, args.warmup)
            e["prepare_over_forward"] = round(e["prepare"]["median_us"] / e["forward"]["median_us"], 3)
        out["cases"]["B%d_Nraw%d_target%d" % (B, N, T)] = e
        del host
        torch.cuda.empty_cache()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
