"""Time place retrieval (csrc/retrieval.hip) against the tensor-op path it can replace: retrieval.search_descriptors and
evaluation.retrieval(backend="torch") on the SAME device tensors, D = 256, k = 25, unit-norm descriptors, for (Q, R) =
(32, 65536) a few queries against a city-scale map, (4096, 65536) a whole traversal against it, and (400, 400) one Oxford
traversal pair.  Device events around `iters` back-to-back calls after a warm-up; the two paths' ids are compared once.
Prints one JSON line.

    python tools/retrieval_bench.py [--iters 10]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dh3d_amd import evaluation, retrieval  # noqa: E402

SIZES = ((32, 65536), (4096, 65536), (400, 400))


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
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    D, k = 256, 25
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = dict(dim=D, k=k, iters=a.iters, sizes=[])
    for Q, R in SIZES:
        ref = torch.nn.functional.normalize(torch.randn((R, D), device="cuda", generator=gen), dim=1)
        qry = torch.nn.functional.normalize(torch.randn((Q, D), device="cuda", generator=gen), dim=1)
        S, slice_rows = retrieval.retrieve_plan(Q, R, D, k)
        hip_us = timed(lambda: retrieval.search_descriptors(ref, qry, k), a.iters)
        torch_us = timed(lambda: evaluation.retrieval(ref, qry, k, backend="torch"), a.iters)
        same = (retrieval.search_descriptors(ref, qry, k)[0].long() == evaluation.retrieval(ref, qry, k)).float().mean()
        res["sizes"].append(dict(Q=Q, R=R, slices=S, slice_rows=slice_rows, hip_us=hip_us, torch_us=torch_us,
                                 speedup=torch_us / hip_us, ids_equal_share=float(same)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
