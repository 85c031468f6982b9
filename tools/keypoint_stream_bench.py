"""Keypoint-only fetch vs the dense map over the host link (cfg 5: detection_config, B = 4, N = 16384, depth-4 Pipeline).

    python tools/keypoint_stream_bench.py [--steps 60] [--warmup 10] [--clouds real|uniform] [--out FILE]

Every step takes a pinned host batch in (staging kernel on the slot's stream) and, per mode:
  a  full     : fetch the whole xyz_feat_att [4, 16384, 132] (34.6 MB) to pinned host       -- what --perform_nms needs today
  b  keypoints: fetch kp_count + xyz_feat_att_nms [4, 512, 132] (1.08 MB) to pinned host     -- NMS on the device
  c  none     : the dense map computed, nothing fetched                                     -- the device-only bound
  c_kp        : the keypoints computed, nothing fetched                                     -- (c_kp - c) = NMS in flight
and the serial (one captured step at a time) cost of the dense forward with and without the keypoint outputs.
Clouds/s = B * steps / wall time, median of three blocks.  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of `--steps 20 --modes b`.  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KP = ("kp_count", "xyz_feat_att_nms")


def clouds(kind, B, N, seed):
    if kind == "real":
        from dh3d_amd.utils import get_fixednum_pcd
        z = np.load(os.path.join(ROOT, "tests", "golden", "demo_clouds.npz"))
        src = [z["local_268"], z["local_642"]]
        return np.stack([np.ascontiguousarray(get_fixednum_pcd(src[b % 2], N, rng=np.random.default_rng(seed + b))[0],
                                              np.float32) for b in range(B)])
    return np.random.default_rng(seed).random((B, N, 3), dtype=np.float32)


def run_mode(model, host_batches, outputs, fetch, depth, steps, warmup, dev):
    """clouds/s and ms per step of a depth-`depth` pipeline fed pinned host batches; fetch: output names copied to pinned
    host buffers (one set per slot)."""
    pipe = model.pipeline(host_batches[0].to(dev), depth=depth, outputs=outputs)
    outs0 = pipe._runs[0].outputs
    bufs = [{n: torch.empty(outs0[n].shape, dtype=outs0[n].dtype).pin_memory() for n in fetch} for _ in range(depth)]
    B = host_batches[0].shape[0]

    def block(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tickets = []
        for i in range(n):
            if len(tickets) >= depth:
                tickets[-depth].event.synchronize()  # the slot's host buffers are about to be reused
            tickets.append(pipe.submit(host_batches[i % len(host_batches)], fetch_to=bufs[i % depth] or None))
        for t in tickets[-depth:]:
            t.event.synchronize()
        return time.perf_counter() - t0

    block(warmup)
    dts = sorted(block(steps) for _ in range(3))
    dt = dts[1]
    fetched = sum(bufs[0][n].numel() * bufs[0][n].element_size() for n in fetch)
    return {"clouds_per_s": B * steps / dt, "ms_per_step": dt / steps * 1e3, "blocks_ms_per_step":
            [d / steps * 1e3 for d in dts], "bytes_fetched_per_step": fetched}


def serial_ms(model, batch, outputs, steps, warmup):
    f = model.graphed(batch, outputs=outputs)
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    res = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            f()
        e1.record()
        e1.synchronize()
        res.append(e0.elapsed_time(e1) / steps)
    return sorted(res)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--clouds", default="real", choices=("real", "uniform"))
    ap.add_argument("--modes", default="a,b,c,c_kp,serial")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from dh3d_amd import ConfigFactory
    from dh3d_amd.model import DH3D
    dev = torch.device("cuda:0")
    B, N = 4, 16384
    cfg = ConfigFactory("detection_config").getconfig()
    cfg.num_points = N
    model = DH3D(cfg).init_synthetic(0).to(dev).eval().prepare()
    host = [torch.from_numpy(clouds(a.clouds, B, N, 5005 + 10 * i)).pin_memory() for i in range(4)]
    modes = a.modes.split(",")
    res = {"workload": "cfg5 detection_config B=%d N=%d, %s clouds, depth %d, pinned host batches in" % (B, N, a.clouds, a.depth),
           "steps": a.steps, "nms": {"radius": 0.5, "min_ratio": 0.01, "max_kp": 512, "knn": 50}}
    with torch.no_grad():
        spec = {"a": (("xyz_feat_att",), ("xyz_feat_att",)), "b": (KP, KP), "c": (("xyz_feat_att",), ()), "c_kp": (KP, ())}
        for m in modes:
            if m in spec:
                outputs, fetch = spec[m]
                res[m] = run_mode(model, host, outputs, fetch, a.depth, a.steps, a.warmup, dev)
                res[m]["outputs"], res[m]["fetched"] = list(outputs), list(fetch)
        if "serial" in modes:
            x = host[0].to(dev)
            dense = serial_ms(model, x, ("xyz_feat_att",), a.steps, a.warmup)
            kp = serial_ms(model, x, ("xyz_feat_att",) + KP, a.steps, a.warmup)
            res["serial"] = {"dense_ms": dense, "dense_plus_keypoints_ms": kp, "nms_ms": kp - dense}
        if "c" in res and "c_kp" in res:
            res["nms_in_flight_ms_per_step"] = res["c_kp"]["ms_per_step"] - res["c"]["ms_per_step"]
        if "a" in res and "b" in res:
            res["b_over_a"] = res["b"]["clouds_per_s"] / res["a"]["clouds_per_s"]
        count = model(host[0].to(dev), fetch=KP)["kp_count"]
        res["kp_count_first_batch"] = count.tolist()
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
