"""Dev: long randomised comparison of the ordered three_nn (128 <= m <= 1024 samples: candidate groups pruned by their boxes,
and the candidates read off the set's cell table; three_nn_sorted_kernel otherwise) with the plain op -- indices AND squared distances bit for
bit (uniform, blobs, planes, lines, lattices with exact ties, duplicated / coincident points; samples = a random subset,
an FPS subset or unrelated points).   python tools/three_nn_fuzz.py [cases] [seed]"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from dh3d_amd import ops, pm
dev = torch.device("cuda")
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 4242)
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 300
KINDS = ("uniform", "blobs", "plane", "line", "grid", "dups", "shell", "twoscale", "same")
def cloud(B, N, kind):
    if kind == "uniform": x = rng.random((B, N, 3))
    elif kind == "blobs":
        c = rng.random((B, 6, 3)); x = c[:, rng.integers(0, 6, N)] + 0.01 * rng.standard_normal((B, N, 3))
    elif kind == "plane": x = rng.random((B, N, 3)); x[..., 2] *= 1e-3
    elif kind == "line": x = rng.random((B, N, 1)) * np.array([1.0, 0.5, 0.25]) + 1e-4 * rng.standard_normal((B, N, 3))
    elif kind == "grid":
        g = int(np.ceil(N ** (1 / 3))) + 1
        pts = np.stack(np.meshgrid(*[np.arange(g)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
        x = np.stack([pts[rng.permutation(len(pts))[:N]] for _ in range(B)]) * 0.25
    elif kind == "dups":
        h = rng.random((B, (N + 1) // 2, 3)); x = np.concatenate([h, h], 1)[:, :N]; x = np.stack([xx[rng.permutation(N)] for xx in x])
    elif kind == "shell":
        v = rng.standard_normal((B, N, 3)); x = v / np.linalg.norm(v, axis=2, keepdims=True) * 10
    elif kind == "same": x = np.broadcast_to(rng.random((B, 1, 3)), (B, N, 3)).copy()
    else:
        x = rng.random((B, N, 3)); x[:, : N // 2] = x[:, : N // 2] * 1e-3 + 0.5
    return np.ascontiguousarray(x.astype(np.float32))
bad = 0
for it in range(cases):
    N = int(rng.choice([64, 65, 100, 513, 1000, 1024, 2049, 4096, 5000, 8192, 16384]))
    B = int(rng.choice([1, 2, 3, 8])) if N <= 8192 else int(rng.choice([1, 2]))
    m = int(rng.choice([3, 5, 64, 127, 128, 129, 200, 256, 500, 512, 700, 1000, 1024, 1025, 2048]))
    m = min(m, N)
    kind = KINDS[int(rng.integers(0, len(KINDS)))]
    x = cloud(B, N, kind)
    how = int(rng.integers(0, 3))
    if how == 0:
        s2 = np.stack([xx[rng.permutation(N)[:m]] for xx in x])
    elif how == 1:
        s2 = cloud(B, m, KINDS[int(rng.integers(0, len(KINDS)))])
    else:
        t0 = torch.from_numpy(x).to(dev)
        s2 = torch.gather(t0, 1, ops.farthest_point_sample(m, t0).long()[:, :, None].expand(-1, -1, 3)).cpu().numpy()
    t, s2 = torch.from_numpy(x).to(dev), torch.from_numpy(np.ascontiguousarray(s2)).to(dev)
    srt, gbox = pm.spatial_sort(t)
    srt2, gbox2, cells2 = pm.spatial_sort_cells(s2)
    d0, i0 = ops.three_nn(t, s2)
    ok = True
    for d, i in (pm.three_nn_sorted(srt, gbox, srt2, gbox2), pm.three_nn_sorted(srt, gbox, srt2, gbox2, cells2=cells2)):
        ok = ok and bool(torch.equal(i, i0)) and bool(torch.equal(d.view(torch.int32), d0.view(torch.int32)))
    if not ok:
        bad += 1
        print("MISMATCH", it, B, N, m, kind, how, flush=True)
print("cases %d mismatches %d" % (cases, bad))
