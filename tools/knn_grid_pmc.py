"""Dev: the launches a counter run of knn_grid_kernel profiles, `knn_grid_pmc.py [B N]` on the bench's cube.  Without arguments:
8 x 8192, three launches each of the pruned scan and the cell lists (tools/gpu_knn_grid_pmc.sh); with B N: four of pm.knn_grid."""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch, bench
from dh3d_amd import pm
dev = torch.device("cuda")
shape = [int(a) for a in sys.argv[1:3]]
B, N = shape if len(shape) == 2 else (8, 8192)
pts = bench.synthetic_clouds(B, N, 2002, dev, 0)
srt, gbox, cells = pm.spatial_sort_cells(pts)
for _ in range(4 if shape else 3):
    if not shape:
        pm.knn_sorted(srt, gbox, 8)
    pm.knn_grid(srt, gbox, cells, 8)
torch.cuda.synchronize()
