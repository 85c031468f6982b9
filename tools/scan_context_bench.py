"""Time Scan Context (csrc/scan_context.hip, dh3d_amd/scancontext.py) with device events around back-to-back calls after a
warm-up, and in the same run a tensor-op statement of each kernel:
  build      scan_context at 64 x 8192 and 1 x 131072 points (synthetic street scenes, 20 x 60 bins, radius 40) against
             sqrt / atan2 / floor bin ids + scatter_reduce("amax") -- the same image up to points that sit within rounding of a
             bin edge ("bins_equal" says how many bins agree); the floor is the rows read once over the copy bandwidth
             measured here
  distance   scan_context_distance at Q = 4096, C = 10 against a map of R = 65536 random images against
             gather + einsum (the Ns x Ns column Gram matrix of every pair in float64) + a diagonal gather + min; "flop" counts
             2 Nr Ns^2 per pair
  search     ScanContextIndex.search of 64 clouds of 8192 points in that map (k = 1, 10 candidates): image, ring-key top-k,
             distance, the gathers
  relocalize relocalize_scan_context of 8 turned, shifted, noisy, permuted copies against a map of 64 stored scenes, without
             and with the dense ICP, and the yaw / translation errors of both poses
These are WARM numbers: every iteration reads the same inputs.  Prints one JSON line and writes it to
profiles/scan_context_bench.json.

    python tools/scan_context_bench.py [--iters 20] [--kernel-iters 200] [--queries 4096] [--map 65536]
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
from dh3d_amd import scancontext as sc  # noqa: E402

NR, NS, RADIUS, Z0 = 20, 60, 40.0, 2.0


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


def scene(rng, n, extent=40.0):
    """Random wall segments up to a random top over a noisy ground plane, the sensor 2 m above it: [n, 3] float32."""
    walls, per = 24, n // 48
    parts = []
    for _ in range(walls):
        a, b = rng.uniform(-extent, extent, 2), rng.uniform(-extent, extent, 2)
        xy = a + rng.random((per, 1)) * (b - a) + rng.normal(0.0, 0.02, (per, 2))
        parts.append(np.concatenate([xy, (-2.0 + rng.random(per) * rng.uniform(1.0, 8.0))[:, None]], 1))
    m = n - walls * per
    parts.append(np.concatenate([rng.uniform(-extent, extent, (m, 2)), -2.0 + np.abs(rng.normal(0.0, 0.03, (m, 1))) + 0.01], 1))
    return rng.permutation(np.concatenate(parts, 0)).astype(np.float32)


def build_tensor_ops(x):
    """The image by tensor ops: float32 polar coordinates, floor to bin ids, one scatter_reduce."""
    P = x.shape[0]
    h = x[:, :, 2] + Z0
    r = torch.sqrt(x[:, :, 0] * x[:, :, 0] + x[:, :, 1] * x[:, :, 1])
    ring = torch.floor(r * (NR / RADIUS)).long()
    theta = torch.atan2(x[:, :, 1], x[:, :, 0])
    sector = torch.floor(torch.where(theta < 0, theta + 2.0 * math.pi, theta) * (NS / (2.0 * math.pi))).long().clamp_(0, NS - 1)
    ok = (r < RADIUS) & (h > 0)
    idx = torch.where(ok, ring * NS + sector, torch.zeros_like(ring))
    desc = torch.zeros((P, NR * NS), dtype=torch.float32, device=x.device)
    desc.scatter_reduce_(1, idx, torch.where(ok, h, torch.zeros_like(h)), "amax", include_self=True)
    return desc.view(P, NR, NS)


def distance_tensor_ops(q, mp, cand, diag):
    """dist and shift by tensor ops: unit columns in float64, the Gram matrix of every pair, its wrapped diagonals."""
    def unit(d):
        d = d.double()
        w = (d * d).sum(1, keepdim=True)
        return torch.where(w > 0, d / w.sqrt().clamp_min(1e-300), torch.zeros_like(d)), (w[:, 0] > 0).double()
    qn, qz = unit(q)
    cn, cz = unit(mp.index_select(0, cand.reshape(-1).long()))
    Q, C = cand.shape
    gram = torch.einsum("qij,qcik->qcjk", qn, cn.view(Q, C, NR, NS))           # [Q, C, Ns(j), Ns(k)]
    both = qz[:, None, :, None] * cz.view(Q, C, 1, NS)
    ix = diag.view(1, 1, NS, NS).expand(Q, C, NS, NS)                          # ix[j, n] = (j + n) % Ns
    s = gram.gather(3, ix).sum(2)                                              # [Q, C, n]
    m = both.gather(3, ix).sum(2)
    d = torch.where(m > 0, 1.0 - s / m.clamp_min(1.0), torch.ones_like(s))
    return d.min(2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--map", type=int, default=65536)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    res = dict(rings=NR, sectors=NS, max_radius=RADIUS, iters=a.iters, kernel_iters=a.kernel_iters, warm=True)

    big = torch.empty((256 << 20,), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(big)
    copy_us = timed(lambda: dst.copy_(big), a.kernel_iters)
    bw = 2.0 * big.numel() / (copy_us * 1e-6)             # bytes per second, read + write
    res["copy_gbps"] = bw / 1e9
    del big, dst

    scenes = np.stack([scene(rng, 8192) for _ in range(64)])
    for label, x in (("build_64x8192", torch.from_numpy(scenes).to(dev)),
                     ("build_1x131072", torch.from_numpy(scene(rng, 131072)[None]).to(dev))):
        P, N = x.shape[:2]
        kern = sc.scan_context(x, None, None, NR, NS, RADIUS, Z0)["desc"]
        ops = build_tensor_ops(x)
        res[label] = dict(us=timed(lambda: sc.scan_context(x, None, None, NR, NS, RADIUS, Z0), a.kernel_iters),
                          tensor_ops_us=timed(lambda: build_tensor_ops(x), a.kernel_iters),
                          floor_us=12.0 * P * N / bw * 1e6, bytes=12 * P * N, workgroups=P * ((N + 2047) // 2048),
                          occupied=float((kern > 0).float().mean()), bins_equal=float((kern == ops).float().mean()))

    Q, R, C = a.queries, a.map, 10
    mp = torch.relu(torch.randn((R, NR, NS), device=dev, generator=torch.Generator(dev).manual_seed(1)) + 0.3) * 3.0
    qd = torch.relu(torch.randn((Q, NR, NS), device=dev, generator=torch.Generator(dev).manual_seed(2)) + 0.3) * 3.0
    cand = torch.randint(0, R, (Q, C), device=dev, generator=torch.Generator(dev).manual_seed(3)).to(torch.int32)
    diag = ((torch.arange(NS, device=dev)[:, None] + torch.arange(NS, device=dev)[None, :]) % NS)
    dist, shift, _ = sc.scan_context_distance(qd, mp, cand)
    od, os_ = distance_tensor_ops(qd, mp, cand, diag)
    flop = 2.0 * NR * NS * NS * Q * C
    us = timed(lambda: sc.scan_context_distance(qd, mp, cand), a.iters)
    res["distance"] = dict(Q=Q, C=C, R=R, us=us, tensor_ops_us=timed(lambda: distance_tensor_ops(qd, mp, cand, diag), max(2, a.iters // 4)),
                           flop=flop, gflops=flop / us * 1e-3, gather_bytes=4 * NR * NS * Q * C * 2,
                           gather_floor_us=4.0 * NR * NS * Q * C * 2 / bw * 1e6,
                           max_abs_diff_to_tensor_ops=float((dist - od).abs().max()), shifts_equal=float((shift == os_).float().mean()))
    del od, os_

    index = sc.ScanContextIndex(capacity=R, num_rings=NR, num_sectors=NS, max_radius=RADIUS, z_offset=Z0, device=dev)
    index.desc.copy_(mp)                                   # a full map without 65536 clouds: the buffers filled directly
    index.places.desc.copy_(mp.double().mean(2).float())
    index.places.count.fill_(R)
    xq = torch.from_numpy(scenes).to(dev)
    res["search"] = dict(queries=64, points=8192, R=R, k=1, candidates=C, us=timed(lambda: index.search(xq, k=1, candidates=C), a.iters))
    del index, mp, qd

    index = sc.ScanContextIndex(capacity=64, points=8192, num_rings=NR, num_sectors=NS, max_radius=RADIUS, z_offset=Z0, device=dev)
    index.add(xq)
    yaw = rng.uniform(-math.pi, math.pi, 8)
    tr = rng.uniform(-0.3, 0.3, (8, 2))
    moved = np.zeros((8, 8192, 3), np.float32)
    for p in range(8):
        c, s = math.cos(yaw[p]), math.sin(yaw[p])
        pts = scenes[p].astype(np.float64)                 # place = Rz(yaw) query + t
        pts[:, :2] = (pts[:, :2] - tr[p]) @ np.array([[c, -s], [s, c]])
        moved[p] = (pts + rng.normal(0.0, 0.02, pts.shape))[rng.permutation(8192)]
    y = torch.from_numpy(moved).to(dev)
    for label, kw in (("relocalize", {}), ("relocalize_refined", dict(refine=True))):
        us = timed(lambda: sc.relocalize_scan_context(index, y, k=1, candidates=C, **kw), a.iters)
        out = sc.relocalize_scan_context(index, y, k=1, candidates=C, **kw)
        Rt = out["Rt"].cpu().numpy()
        dyaw = np.degrees(np.abs((np.arctan2(Rt[:, 1, 0], Rt[:, 0, 0]) - yaw + math.pi) % (2 * math.pi) - math.pi))
        dt = np.linalg.norm(Rt[:, :2, 3] - tr, axis=1)
        row = dict(queries=8, places=64, points=8192, us=us, found=int((out["place"][:, 0].cpu().numpy() == np.arange(8)).sum()),
                   yaw_err_deg_mean=float(dyaw.mean()), yaw_err_deg_max=float(dyaw.max()), t_err_mean=float(dt.mean()),
                   t_err_max=float(dt.max()), sector_deg=360.0 / NS)
        if "fitness" in out:
            row["fitness_mean"], row["rmse_mean"] = float(out["fitness"].mean()), float(out["rmse"].mean())
        res[label] = row
    line = json.dumps(res)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "scan_context_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
