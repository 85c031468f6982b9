"""flex_convolution_transpose (FlexDeconv) timings: section A (the reference formulation), section A' (inverted neighbour
lists + GEMM) and flex_convolution's own A' at the same shape, forward and forward + backward, in one process.  On a
uniform cube and on the demo clouds' stored kNN lists (tests/golden/demo_clouds.npz: global_c, 8192 points, as 8 clouds;
local_268, 16384 points, as 4), next to the uniform cube of the same size.  Median and maximum of per-call HIP-event times
after warm-up; the in-degree (median / max) of each neighbourhood beside them.

    python tools/flex_deconv_bench.py [--iters 20]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from dh3d_amd import ops  # noqa: E402


def times_ms(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), float(np.max(out))


def clouds(dev, name, B, N, K):
    """positions [B, 3, N], neighbourhoods [B, K, N] int32"""
    if name == "cube":
        pos = torch.rand((B, 3, N), generator=torch.Generator().manual_seed(1)).to(dev)
        nn_, _ = ops.knn_bruteforce(pos, K)
        return pos, nn_.transpose(1, 2).contiguous()
    d = np.load(os.path.join(ROOT, "tests", "golden", "demo_clouds.npz"))
    xyz, knn = d[name], d[name + "/knn"]
    assert xyz.shape[0] == N and knn.shape[1] == K
    pos = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(xyz.T[None], (B, 3, N)))).to(dev)
    nbr = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(knn.T[None], (B, K, N))).astype(np.int32)).to(dev)
    return pos, nbr


def indegree(nbr):
    B, K, N = nbr.shape
    deg = torch.zeros((B, N), dtype=torch.int64, device=nbr.device)
    deg.scatter_add_(1, nbr.reshape(B, K * N).long(), torch.ones((B, K * N), dtype=torch.int64, device=nbr.device))
    deg = deg.cpu().numpy()
    return int(np.median(deg)), int(deg.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = 8
    print("%-10s %2s x %5s %3s->%-3s %7s | %-26s %-26s %-26s" % ("cloud", "B", "N", "Din", "Dout", "in-deg",
          "A fwd / fwd+bwd (med,max)", "A' fwd / fwd+bwd", "flex_conv A' fwd / fwd+bwd"))
    for name, B, N in (("cube", 8, 8192), ("global_c", 8, 8192), ("cube", 4, 16384), ("local_268", 4, 16384)):
        pos, nbr = clouds(dev, name, B, N, K)
        dmed, dmax = indegree(nbr)
        for Din, Dout in ((64, 64), (32, 64)):
            g = torch.Generator().manual_seed(2)
            f = torch.randn((B, Din, N), generator=g).to(dev).requires_grad_()
            th = (0.1 * torch.randn((3, Din, Dout), generator=g)).to(dev).requires_grad_()
            bi = (0.1 * torch.randn((Din, Dout), generator=g)).to(dev).requires_grad_()
            gout = torch.randn((B, Dout, N), generator=g).to(dev)
            cols = []
            for op, fast in ((ops.flex_convolution_transpose, False), (ops.flex_convolution_transpose, True),
                             (ops.flex_convolution, True)):
                ops.FAST_PATH = fast
                iters = args.iters if fast else 3

                def fwd():
                    with torch.no_grad():
                        op(f, pos, nbr, th, bi)

                def fwd_bwd():
                    torch.autograd.grad(op(f, pos, nbr, th, bi), (f, th, bi), gout)

                a, b = times_ms(fwd, iters), times_ms(fwd_bwd, iters)
                cols.append("%7.3f,%7.3f / %7.3f,%7.3f" % (a + b))
            ops.FAST_PATH = True
            print("%-10s %2d x %5d %3d->%-3d %3d/%-3d | %s" % (name, B, N, Din, Dout, dmed, dmax, "  ".join(cols)),
                  flush=True)
    print("(ms; per column: median,max of the forward / of forward + backward)")


if __name__ == "__main__":
    main()
