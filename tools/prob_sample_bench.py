"""Times dh3d_prob_sample and its seeded form (dh3d_amd.pm.prob_sample, dh3d_amd.utils.sample_by_weight) next to the
tensor-op path a user would write instead -- torch.cumsum + torch.searchsorted, which gives OTHER ids on rows whose
reference sums are not monotone and other sums in most entries -- and prints ONE JSON line.  Shapes (rows x weights, draws a
row): 64 x 8192 with m = 512 and m = 8192, and 8 x 131072 with m = 8192; uniform weights.
  hip            pm.prob_sample(weights, draws): the cumulative sums and the walks, two kernels
  hip_seeded     utils.sample_by_weight(weights, m, count, seed): the same with the draws made in the search kernel
  torch          cumsum, one multiply, searchsorted, clamp, to int32 on given draws
  torch_rand     torch.rand for the draws, then the same
Every call is timed twice: `eager` (the Python call between a pair of device events) and `graph` (replays of the call
captured once: the device time of the kernels alone); median / min / max in microseconds of --launches runs after --warmup.
The two paths alternate over --rounds rounds in this one process; a shape's figure is the median of the rounds' medians, the
rounds' medians are kept next to it as the spread.  Before timing, rows of the device result are compared with the numpy
restatement (tests/prob_sample_reference.py).  Needs a GPU; there is no fallback.

    python tools/prob_sample_bench.py [--launches 300] [--warmup 20] [--rounds 3] [--out FILE (default profiles/prob_sample_bench.json)]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pairs_bench import both_ways  # noqa: E402

SHAPES = ((64, 8192, 512), (64, 8192, 8192), (8, 131072, 8192))


def tensor_op_path(w, r):
    cum = torch.cumsum(w, dim=1)
    q = r * cum[:, -1:]
    return torch.searchsorted(cum, q).clamp_(max=w.shape[1] - 1).to(torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prob_sample_bench.json"), help="the JSON line is also written here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prob_sample_bench needs a GPU")
    import prob_sample_reference as R
    from dh3d_amd import pm, utils
    dev = torch.device("cuda:0")
    seed = 2024
    sd = torch.tensor([seed], dtype=torch.int64, device=dev)
    L, W = args.launches, args.warmup
    out = {"tool": "prob_sample_bench", "device": torch.cuda.get_device_name(0), "launches": L, "rounds": args.rounds, "shapes": {}}

    for b, n, m in SHAPES:
        rng = np.random.default_rng(n + m)
        w_np = rng.random((b, n), dtype=np.float32)
        r_np = rng.random((b, m), dtype=np.float32)
        w, r = torch.from_numpy(w_np).to(dev), torch.from_numpy(r_np).to(dev)
        count = torch.full((b,), n, dtype=torch.int32, device=dev)

        # the device results are the restatement's, on the first and the last row
        ids, cum = pm.prob_sample(w, r)
        ids_s = utils.sample_by_weight(w, m, count=count, seed=sd)
        for row in (0, b - 1):
            c = R.cumsum(w_np[row])
            assert np.array_equal(cum[row].cpu().numpy().view(np.int32), c.view(np.int32)), "sums differ from the restatement"
            assert np.array_equal(ids[row].cpu().numpy(), R.walk(c, r_np[row])), "ids differ from the restatement"
            assert np.array_equal(ids_s[row].cpu().numpy(), R.sample_row(w_np[row], n, m, seed, row)), "seeded ids differ"
        t_ids = tensor_op_path(w, r)
        e = {"tensor_op_ids_that_differ": int((t_ids != ids).sum()),
             "tensor_op_sums_that_differ": int((torch.cumsum(w, dim=1) != cum).sum())}

        paths = {"hip": lambda: pm.prob_sample(w, r), "hip_seeded": lambda: utils.sample_by_weight(w, m, count=count, seed=sd),
                 "torch": lambda: tensor_op_path(w, r),
                 "torch_rand": lambda: tensor_op_path(w, torch.rand((b, m), dtype=torch.float32, device=dev))}
        rounds = {k: [] for k in paths}
        for _ in range(args.rounds):            # the paths alternate: a drift of the machine meets all of them
            for k, fn in paths.items():
                rounds[k].append(both_ways(fn, L, W))
        for k, rs in rounds.items():
            e[k] = {mode: {"median_us": round(float(np.median([x[mode]["median_us"] for x in rs])), 2),
                           "round_medians_us": [x[mode]["median_us"] for x in rs],
                           "min_us": min(x[mode]["min_us"] for x in rs)} for mode in ("eager", "graph")}
        e["torch_over_hip_graph"] = round(e["torch"]["graph"]["median_us"] / e["hip"]["graph"]["median_us"], 3)
        e["torch_rand_over_hip_seeded_graph"] = round(e["torch_rand"]["graph"]["median_us"] / e["hip_seeded"]["graph"]["median_us"], 3)
        out["shapes"]["%dx%d_m%d" % (b, n, m)] = e
        del w, r, count, ids, cum, ids_s, t_ids
        torch.cuda.empty_cache()

    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
