"""Times the training-tuple kernels of dh3d_amd.tuples next to the host loop they replace and the step they feed, and prints
ONE JSON line.  Maps of M = 21711 (the reference's training set) and 65536 places: 44 noisy traversals of one route at 4 m
steps, at UTM-sized offsets, a 256-float descriptor and a 4096-point cloud per place.  Per map:
  tuple_counts            the O(M^2) pass, once per map
  tuples                  draw_queries + sample_tuples at (num_pos, num_neg) = (2, 18) with the other negative, for Q = 1 and
                          Q = 2048 query slots, without and with hard mining (6 hard of 18, pool_fraction 0.1, D = 256);
                          for Q = 2048 also without the other negative and at (1, 1): what pass 2 and the list folds cost
  make_quadruplet_batch   bank -> queries -> tuples -> gather -> make_global_batch for one quadruplet (22 clouds of 4096)
  host_loop               a host loader mining one tuple at a time with Python sets over the whole map, as the reference's
                          global training loader does (core/datasets.py:208-232), on the same positions in this process:
                          two set differences against all M ids, two draws and a shuffle per tuple; the per-place id lists
                          it looks up are built beforehand
Every device call is timed twice: `eager` (the Python call between a pair of device events) and `graph` (replays of the call
captured once, the seed read from its device tensor: the device time of the kernels alone); median / min / max in
microseconds of --launches runs after --warmup.  Before timing, the device tuples are compared with the numpy restatement
(tests/tuples_reference.py) on a few slots.  One QuadrupletTrainer step (22 clouds of 4096 points) is timed in the same run.
Needs a GPU; there is no fallback.

    python tools/tuples_bench.py [--launches 40] [--warmup 5] [--out FILE (default profiles/tuples_bench.json)] [--no-steps]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pairs_bench import both_ways, timed  # noqa: E402

P, NG, HARD, FRACTION, D, NPTS = 2, 18, 6, 0.1, 256, 4096


def route_map(M, seed):
    """M places: traversals of ceil(M / 44) places each along one route (4 m steps, a gentle curve), 1 m Gaussian noise."""
    rng = np.random.default_rng(seed)
    per = -(-M // 44)
    s = 4.0 * (np.arange(M) % per)
    xy = np.stack([s, 300.0 * np.sin(s / 700.0)], axis=1) + rng.standard_normal((M, 2))
    return np.array([5735000.0, 620000.0]) + xy


class SetMiner:
    """The host baseline: a loader that mines one tuple at a time with Python sets over the whole map, which is what the
    reference's global training loader pays -- per tuple, two set differences against all M place ids (the places far enough
    to be negatives; the places near neither the query nor a drawn negative), one draw without replacement from each of the
    first two candidate lists and a Python shuffle of the last.  The near / not-far id lists of a place are what the
    reference reads from its tuple pickles; here they come from the restatement's distances and are cached, so the timed
    pass only looks them up."""

    def __init__(self, pos, restatement):
        self.pos, self.R = pos, restatement
        self.everyone = dict.fromkeys(range(len(pos)))   # (a dict: the baseline makes a set of its keys for every tuple)
        self.cache = {}

    def lists(self, place):
        """(ids within the positive radius, the place excepted; ids within the negative radius) as Python lists."""
        if place not in self.cache:
            d2 = self.R.d2_from(self.pos, place, len(self.pos))
            rp2, rn2 = self.R.radii2(10.0, 50.0)
            near = np.flatnonzero(d2 <= rp2)
            self.cache[place] = (near[near != place].tolist(), np.flatnonzero(d2 <= rn2).tolist())
        return self.cache[place]

    def mine(self, query, draw, shuffler):
        near, not_far = self.lists(query)
        if len(near) < P:
            return None
        chosen_pos = [near[k] for k in draw.choice(len(near), size=P, replace=False)]
        far = list(set(self.everyone.keys()) - set(not_far))
        chosen_neg = [far[k] for k in draw.choice(len(far), size=NG, replace=False)]
        barred = set(near)
        for g in chosen_neg:
            barred.update(self.lists(g)[0])
        free = list(set(self.everyone.keys()) - barred)
        shuffler.shuffle(free)
        return query, chosen_pos, chosen_neg, free[0]

    def seconds_per_tuple(self, queries):
        """Median over `queries`.  Two passes from the same random state: the first fills the cache, the second is timed."""
        for _ in range(2):
            draw, shuffler = np.random.default_rng(5), random.Random(5)
            took = []
            for q in queries:
                t0 = time.perf_counter()
                self.mine(q, draw, shuffler)
                took.append(time.perf_counter() - t0)
        return sorted(took)[len(took) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tuples_bench.json"), help="the JSON line is also written here")
    ap.add_argument("--no-steps", action="store_true", help="time the tuple kernels alone (for a kernel trace)")
    ap.add_argument("--maps", type=int, nargs="+", default=[21711, 65536])
    ap.add_argument("--host-tuples", type=int, default=24)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tuples_bench needs a GPU")
    import tuples_reference as R
    from dh3d_amd import ConfigFactory, tuples
    from dh3d_amd.model import DH3D
    from dh3d_amd.retrieval import PlaceIndex
    from dh3d_amd.training import QuadrupletTrainer
    dev = torch.device("cuda:0")
    seed = 2024
    sd = torch.tensor([seed], dtype=torch.int64, device=dev)
    L, W = args.launches, args.warmup
    out = {"tool": "tuples_bench", "device": torch.cuda.get_device_name(0), "launches": L, "num_pos": P, "num_neg": NG,
           "num_hard": HARD, "pool_fraction": FRACTION, "D": D, "maps": {}}

    step_us = None
    if not args.no_steps:
        cfg = ConfigFactory("global_config").getconfig()
        cfg.batch_size, cfg.num_pos, cfg.num_neg, cfg.num_points = 1, P, NG, NPTS
        tr = QuadrupletTrainer(DH3D(cfg).init_synthetic(0).to(dev).eval().prepare())
        pts = torch.rand((1 + P + NG + 1, NPTS, 3), device=dev) * 30.0
        out["quadruplet_trainer_step"] = timed(lambda: tr.step(pts, sync=False), L, max(W, 5))
        step_us = out["quadruplet_trainer_step"]["median_us"]
        del tr, pts
        torch.cuda.empty_cache()

    for M in args.maps:
        pos_np = route_map(M, M)
        gen = torch.Generator(device=dev).manual_seed(M)
        bank = PlaceIndex(dim=D, capacity=M, device=dev, points=NPTS)
        bank.pos.copy_(torch.from_numpy(pos_np))
        bank.desc.copy_(torch.randn((M, D), generator=gen, device=dev))
        bank.cloud.copy_(torch.rand((M, NPTS, 3), generator=gen, device=dev) * 30.0)
        bank.cloud_count.fill_(NPTS)
        bank.count.fill_(M)
        pos, desc = bank.pos, bank.desc
        n_pos, n_neg = tuples.tuple_counts(pos, bank.count)
        hard = dict(desc=desc, num_hard=HARD, pool_fraction=FRACTION)

        # the device tuples are the restatement's, on a few slots
        queries, ok = tuples.draw_queries(n_pos, n_neg, 4, P, NG, count=bank.count, seed=sd)
        got = tuples.sample_tuples(pos, queries, P, NG, count=bank.count, seed=sd, **hard)
        exp = R.sample_tuples(pos_np, queries.cpu().numpy(), P, NG, desc=desc.cpu().numpy(), num_hard=HARD, pool_fraction=FRACTION,
                              seed=seed)
        for k in ("pos", "neg", "other", "valid"):
            assert np.array_equal(got[k].cpu().numpy(), exp[k]), "%s differs from the restatement" % k
        assert int(ok) == 1 and exp["valid"].all()

        def draw_and_sample(Q, num_pos=P, num_neg=NG, **kw):
            def fn():
                qs, _ = tuples.draw_queries(n_pos, n_neg, Q, num_pos, num_neg, count=bank.count, seed=sd)
                return tuples.sample_tuples(pos, qs, num_pos, num_neg, count=bank.count, seed=sd, **kw)
            return fn

        e = {"valid_queries": int(((n_pos >= P) & (n_neg >= NG)).sum()), "mean_positives": round(float(n_pos.float().mean()), 1),
             "mean_negatives": round(float(n_neg.float().mean()), 1),
             "tuple_counts": both_ways(lambda: tuples.tuple_counts(pos, bank.count), max(L // 4, 5), 2), "tuples": {}}
        for Q in (1, 2048):
            e["tuples"]["Q%d" % Q] = both_ways(draw_and_sample(Q), L, W)
            e["tuples"]["Q%d_hard" % Q] = both_ways(draw_and_sample(Q, **hard), L, W)
        e["tuples"]["Q2048_no_other"] = both_ways(draw_and_sample(2048, other_neg=False), L, W)
        e["tuples"]["Q2048_one_one"] = both_ways(draw_and_sample(2048, 1, 1), L, W)
        e["tuples"]["Q1_draw_queries"] = both_ways(
            lambda: tuples.draw_queries(n_pos, n_neg, 1, P, NG, count=bank.count, seed=sd), L, W)
        e["tuples"]["Q2048_draw_queries"] = both_ways(
            lambda: tuples.draw_queries(n_pos, n_neg, 2048, P, NG, count=bank.count, seed=sd), L, W)
        counts = (n_pos, n_neg)
        e["make_quadruplet_batch"] = both_ways(
            lambda: tuples.make_quadruplet_batch(bank, 1, P, NG, numpts=NPTS, counts=counts, seed=sd), L, W)
        e["make_quadruplet_batch_hard"] = both_ways(
            lambda: tuples.make_quadruplet_batch(bank, 1, P, NG, numpts=NPTS, counts=counts, seed=sd, **{k: hard[k] for k in ("num_hard", "pool_fraction")}), L, W)
        host = SetMiner(pos_np, R)
        valid = np.nonzero(((n_pos >= P) & (n_neg >= NG)).cpu().numpy())[0]
        host_s = host.seconds_per_tuple([int(i) for i in np.random.default_rng(3).choice(valid, args.host_tuples, replace=False)])
        e["host_loop_ms_per_tuple"] = round(host_s * 1e3, 3)
        per_tuple_us = e["tuples"]["Q2048"]["graph"]["median_us"] / 2048
        e["host_over_device_Q1"] = round(host_s * 1e6 / e["tuples"]["Q1"]["graph"]["median_us"], 1)
        e["host_over_device_Q2048_per_tuple"] = round(host_s * 1e6 / per_tuple_us, 1)
        if step_us:
            e["tuples_Q1_over_step"] = round(e["tuples"]["Q1"]["graph"]["median_us"] / step_us, 4)
            e["tuples_Q1_hard_over_step"] = round(e["tuples"]["Q1_hard"]["graph"]["median_us"] / step_us, 4)
            e["make_quadruplet_batch_over_step"] = round(e["make_quadruplet_batch"]["graph"]["median_us"] / step_us, 4)
        out["maps"]["M%d" % M] = e
        del bank, pos, desc, host
        torch.cuda.empty_cache()

    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
