"""Times the training-batch builders of dh3d_amd.pairs next to the steps they feed and prints ONE JSON line.
  local   make_local_pairs for 10 sources (12000 points each) -> 20 clouds of 8192 points with 256 nodes, its four stages
          one by one (resample_clouds, augment_clouds, rotate_pairs, sample_pair_nodes), and one LocalTrainer step
          (basic_config, 10 pairs of 8192 points, 256 nodes) on the batch it built
  global  make_global_batch for 22 sources (6000 points each) -> 22 clouds of 4096 points, its two stages, and one
          QuadrupletTrainer step (1 query + 2 positives + 18 negatives + 1 other negative) on the batch it built
Every builder and stage is timed twice: `eager` (the Python call between a pair of device events: launches, allocations
and the host code included) and `graph` (replays of the call captured once, the seed read from its device tensor: the
device time of the kernels alone); median / min / max in microseconds of --launches runs after --warmup.
`restatement_cpu_ms` is the numpy restatement of the same batch (tests/pairs_reference.py) arranged as the reference's
loader runs it: cloud after cloud on the host, the sampler's Python loop per pick, and for the positive nodes
scipy.spatial.cKDTree when scipy is importable, else the brute-force argmin (`restatement_nn` says which).  One pass,
host clock.  Before timing, the device batch is compared with the restatement (nodes exactly, points within one ulp).
Needs a GPU; there is no fallback.

    python tools/pairs_bench.py [--launches 40] [--warmup 5] [--out profiles/pairs_bench.json] [--no-steps]
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


def _stats(us):
    us = sorted(us)
    return {"median_us": round(us[len(us) // 2], 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2)}


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
    return _stats([a.elapsed_time(b) * 1e3 for a, b in ev])


def both_ways(fn, launches, warmup):
    """fn() eager, and the replay of fn() captured once."""
    out = {"eager": timed(fn, launches, warmup)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = fn()
    out["graph"] = timed(graph.replay, launches, warmup)
    del keep, graph
    return out


def sources(B, nsrc, seed, dev):
    rng = np.random.default_rng(seed)
    src = (rng.random((B, nsrc, 3), dtype=np.float32) * np.float32(30.0))
    return src, torch.from_numpy(src).to(dev), torch.full((B,), nsrc, dtype=torch.int32, device=dev)


def one_ulp(got, exp):
    return bool((np.abs(got.astype(np.float64) - exp.astype(np.float64)) <= np.spacing(np.maximum(np.abs(got), np.abs(exp)))).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--no-steps", action="store_true", help="time the builders alone (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pairs_bench needs a GPU")
    import pairs_reference as R
    from dh3d_amd import ConfigFactory, pairs
    from dh3d_amd.model import DH3D
    from dh3d_amd.training import LocalTrainer, QuadrupletTrainer
    try:
        import scipy.spatial  # noqa: F401
        nn = "kdtree"
    except ImportError:
        nn = "brute"
    dev = torch.device("cuda:0")
    seed = 2024
    sd = torch.tensor([seed], dtype=torch.int64, device=dev)
    L, W = args.launches, args.warmup
    out = {"tool": "pairs_bench", "device": torch.cuda.get_device_name(0), "launches": L, "restatement_nn": nn}

    # ---- stage 1: 10 sources -> 20 clouds of 8192 points, 256 nodes
    B, nsrc, N, M = 10, 12000, 8192, 256
    src_np, src, num = sources(B, nsrc, 1, dev)
    batch = pairs.make_local_pairs(src, num, numpts=N, sample_nodes=M, seed=sd)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    exp = R.make_local_pairs(src_np, [nsrc] * B, N, M, seed, nn=nn)
    cpu_s = time.perf_counter() - t0
    idx = batch["sample_idx"].cpu().numpy()
    assert np.array_equal(idx[:B], exp["sample_idx"][:B]), "anchors differ from the restatement"
    if nn == "brute":
        assert np.array_equal(idx[B:], exp["sample_idx"][B:]), "positives differ from the restatement"
    assert one_ulp(batch["points"].cpu().numpy(), exp["points"]), "points differ from the restatement"
    drawn, _ = pairs.resample_clouds(torch.cat([src, src]), torch.cat([num, num]), N, seed=sd)
    both, _ = pairs.augment_clouds(drawn, ("Jitter",), seed=sd)
    pc1, pc2 = both[:B].contiguous(), both[B:].contiguous()
    src2, num2 = torch.cat([src, src]), torch.cat([num, num])
    e = {"sources": B, "nsrc": nsrc, "numpts": N, "sample_nodes": M, "restatement_cpu_ms": round(cpu_s * 1e3, 1),
         "make_local_pairs": both_ways(lambda: pairs.make_local_pairs(src, num, numpts=N, sample_nodes=M, seed=sd), L, W),
         "stages": {
             "resample_clouds": both_ways(lambda: pairs.resample_clouds(src2, num2, N, seed=sd), L, W),
             "augment_clouds": both_ways(lambda: pairs.augment_clouds(drawn, ("Jitter",), seed=sd), L, W),
             "rotate_pairs": both_ways(lambda: pairs.rotate_pairs(pc2, seed=sd), L, W),
             "sample_pair_nodes": both_ways(lambda: pairs.sample_pair_nodes(pc1, pc2, M, seed=sd), L, W)}}
    if not args.no_steps:
        cfg = ConfigFactory("basic_config").getconfig()
        cfg.num_points, cfg.batch_size, cfg.sampled_kpnum = N, B, M
        tr = LocalTrainer(DH3D(cfg).init_synthetic(0).to(dev).eval().prepare())
        e["local_trainer_step"] = timed(lambda: tr.step(batch["points"], batch["R"], batch["sample_idx"], sync=False), L, max(W, 5))
        e["build_over_step"] = round(e["make_local_pairs"]["graph"]["median_us"] / e["local_trainer_step"]["median_us"], 4)
        del tr
    out["local"] = e
    torch.cuda.empty_cache()

    # ---- global stage: 22 clouds of 4096 points
    B, nsrc, N = 22, 6000, 4096
    src_np, src, num = sources(B, nsrc, 2, dev)
    pts = pairs.make_global_batch(src, num, N, seed=sd)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    exp = R.make_global_batch(src_np, [nsrc] * B, N, seed)
    cpu_s = time.perf_counter() - t0
    assert one_ulp(pts.cpu().numpy(), exp), "the global batch differs from the restatement"
    drawn, _ = pairs.resample_clouds(src, num, N, seed=sd)
    aug = ("Jitter", "RotateSmall", "Shift", "Rotate1D")
    e = {"clouds": B, "nsrc": nsrc, "numpts": N, "restatement_cpu_ms": round(cpu_s * 1e3, 1),
         "make_global_batch": both_ways(lambda: pairs.make_global_batch(src, num, N, seed=sd), L, W),
         "stages": {"resample_clouds": both_ways(lambda: pairs.resample_clouds(src, num, N, seed=sd), L, W),
                    "augment_clouds": both_ways(lambda: pairs.augment_clouds(drawn, aug, seed=sd), L, W)}}
    if not args.no_steps:
        cfg = ConfigFactory("global_config").getconfig()
        cfg.batch_size, cfg.num_pos, cfg.num_neg, cfg.num_points = 1, 2, 18, N
        tr = QuadrupletTrainer(DH3D(cfg).init_synthetic(0).to(dev).eval().prepare())
        e["quadruplet_trainer_step"] = timed(lambda: tr.step(pts, sync=False), L, max(W, 5))
        e["build_over_step"] = round(e["make_global_batch"]["graph"]["median_us"] / e["quadruplet_trainer_step"]["median_us"], 4)
    out["global"] = e

    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
