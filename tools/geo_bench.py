"""Dev micro-benchmark of the geometry kernels (PYTHONPATH=. python tools/geo_bench.py)."""
import torch
from dh3d_amd import pm, ops
dev = torch.device("cuda")


def ev(fn, iters=20):
    for _ in range(3):
        fn()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / iters


for B, N in ((1, 8192), (8, 8192), (32, 4096), (8, 1024), (32, 512)):
    xyz = torch.rand(B, N, 3, device=dev)
    srt, gbox = pm.spatial_sort(xyz)
    m = max(N // 8, 1)
    samp = torch.gather(xyz, 1, pm.fps_sorted(srt, gbox, m).long()[:, :, None].expand(-1, -1, 3)).contiguous()
    srt2, gbox2 = pm.spatial_sort(samp)
    print(B, N, "sort %.3f knn_bf %.3f knn_sorted %.3f fps_bf %.3f fps_sorted %.3f three_nn %.3f three_nn_sorted %.3f" % (
        ev(lambda: pm.spatial_sort(xyz)), ev(lambda: pm.knn_xyz(xyz, 8)), ev(lambda: pm.knn_sorted(srt, gbox, 8)),
        ev(lambda: ops.farthest_point_sample(m, xyz)), ev(lambda: pm.fps_sorted(srt, gbox, m)),
        ev(lambda: ops.three_nn(xyz, samp)), ev(lambda: pm.three_nn_sorted(srt, gbox, srt2, gbox2))))
