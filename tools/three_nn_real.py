"""Dev: the ordered three_nn alone on the bench's uniform clouds, the scene-like clouds and the demo (real) clouds -- through the
candidate groups' boxes and through the sampled set's cell table (the FPS kernel's cells_s).   python tools/three_nn_real.py"""
import sys; sys.path.insert(0, ".")
import torch, bench
from dh3d_amd import pm
dev = torch.device("cuda")
for B, N in ((8, 8192), (32, 4096)):
    for name, p in (("real", bench.real_oxford_clouds(B, N, dev)), ("scene", bench.scene_like_clouds(B, N, 2002, dev)[..., :3].contiguous()),
                    ("cube", bench.synthetic_clouds(B, N, 1234, dev)[..., :3].contiguous())):
        srt, gbox, cells = pm.spatial_sort_cells(p)
        _, xyz_s, srt_s, gbox_s, cells_s = pm.fps_sorted_ordered(srt, gbox, N // 8, cells=cells)
        a, b = pm.three_nn_sorted(srt, gbox, srt_s, gbox_s), pm.three_nn_sorted(srt, gbox, srt_s, gbox_s, cells2=cells_s)
        same = bool(torch.equal(a[1], b[1])) and bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)))
        for rep in range(3):  # (repeated: the spread of the launches is the yardstick)
            t = bench.event_time_ms(lambda: pm.three_nn_sorted(srt, gbox, srt_s, gbox_s), iters=20, warm=3) * 1e3
            tc = bench.event_time_ms(lambda: pm.three_nn_sorted(srt, gbox, srt_s, gbox_s, cells2=cells_s), iters=20, warm=3) * 1e3
            print("%2d x %5d %-5s three_nn boxes %.1f us  cells %.1f us  crowded %d / %d  same %s" % (
                B, N, name, t, tc, int((cells_s[:, 4106] != 0).sum()), B, same), flush=True)
