"""Launches the ordered three_nn a few times at the local step's shape (8 x 8192 fine points against 8 x 1024 samples) and the
global step's (32 x 4096 against 512), through the candidate groups' boxes and through the sampled set's cell table; run
under rocprofv3 --pmc ... (tools/gpu_three_nn_pmc.sh; tools/rocpd_summary.py --pmc lists the two kernels side by side)."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from dh3d_amd import pm
import bench
dev = torch.device("cuda")
for B, N in ((8, 8192), (32, 4096)):
    xyz = bench.synthetic_clouds(B, N, 2002, dev, 0)
    srt, gbox, cells = pm.spatial_sort_cells(xyz)
    _, xyz_s, srt2, gbox2, cells2 = pm.fps_sorted_ordered(srt, gbox, N // 8, cells=cells)
    for _ in range(6):
        pm.three_nn_sorted(srt, gbox, srt2, gbox2)
        pm.three_nn_sorted(srt, gbox, srt2, gbox2, cells2=cells2)
    torch.cuda.synchronize()
print("done")
