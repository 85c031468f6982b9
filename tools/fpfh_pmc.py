"""Launches the two FPFH kernels (csrc/fpfh.hip: spfh_counts_kernel, fpfh_kernel) a few times at 64 x 8192 points, K = 32, on
random subsets of a demo cloud with the device's own kNN ids and normals; run under `rocprofv3 --pmc <counters>
--kernel-trace -- python tools/fpfh_pmc.py`, one counter set per run, and under `rocprofv3 --kernel-trace --stats` in a run
of its own for the kernel times (profiles/fpfh_pmc.txt holds both).  `--summary FILE.db PATTERN` prints the average of
every counter over the kernels whose name matches the SQL pattern."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(db, pattern):
    import sqlite3
    c = sqlite3.connect(db)
    for row in c.execute("select name, counter_name, avg(counter_value), count(*) from pmc_events where name like ? "
                         "group by name, counter_name", (pattern,)):
        print("%-40s %-30s %16.0f (n=%d)" % (row[0].replace("(anonymous namespace)::", "")[:40], row[1], row[2], row[3]))


def main():
    import numpy as np
    import torch
    from dh3d_amd import registration as reg
    from dh3d_amd.utils import batched_knn
    P, N, K = 64, 8192, 32
    rng = np.random.default_rng(0)
    cloud = np.load(os.path.join(ROOT, "tests", "golden", "demo_clouds.npz"))["local_642"]
    x = torch.from_numpy(np.stack([cloud[rng.permutation(len(cloud))[:N]] for _ in range(P)]).astype(np.float32)).cuda()
    nrm = reg.estimate_normals(x, k=16)["normals"]
    nbr = batched_knn(x, K)[0]
    for _ in range(6):
        reg.compute_fpfh(x, nrm, nbr=nbr)
    torch.cuda.synchronize()
    print("done")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--summary":
        summary(sys.argv[2], sys.argv[3])
    else:
        main()
