"""Point-major ([B,N,C]) fused kernels used by the model path (section B of include/dh3d_hip.h).

Thin, allocation-only wrappers: each function validates shapes, allocates the output with torch and
enqueues one C-ABI call on the current stream.  No function here has a CPU or eager-torch fallback.
"""

import ctypes

import torch

from . import _lib as L

ACT_NONE, ACT_RELU, ACT_SIGMOID = L.ACT_NONE, L.ACT_RELU, L.ACT_SIGMOID


def _knn_out(what, out, B, N, k, device):
    """The (nn, dist) a kNN wrapper writes: fresh tensors, or the caller's `out` pair after validation."""
    if out is None:
        return (torch.empty((B, N, k), dtype=torch.int32, device=device),
                torch.empty((B, N, k), dtype=torch.float32, device=device))
    nn, dist = out
    for t, dt, name in ((nn, torch.int32, "nn"), (dist, torch.float32, "dist")):
        if tuple(t.shape) != (B, N, k) or t.dtype != dt or t.device != device or not t.is_contiguous():
            raise ValueError("%s: out %s must be contiguous %s [%d, %d, %d] on %s, got %s %s on %s"
                             % (what, name, dt, B, N, k, device, t.dtype, tuple(t.shape), t.device))
    return nn, dist


def knn_xyz(xyz, k, out=None):
    """xyz [B,N,3] -> (nbr [B,N,K] int32, dist [B,N,K]); same function as ops.knn_bruteforce.
    out: optional (nn int32 [B,N,K], dist float32 [B,N,K]), contiguous on the device, to write into."""
    x = L.require_cuda_f32(xyz, "xyz", 3)
    B, N, _ = x.shape
    nn, dist = _knn_out("knn_xyz", out, B, N, k, x.device)
    L.check(L.lib().dh3d_knn_bruteforce_xyz(L.ptr(x), B, N, k, L.ptr(nn), L.ptr(dist), L.stream_ptr()), "knn_xyz")
    return nn, dist


KNN_FAMILIES = {1: "small", 2: "lane", 3: "anydp"}


def knn_plan(B, N, k, Dp=3):
    """The kernel knn_xyz / ops.knn_bruteforce run for B clouds of N points in Dp dimensions (host only;
    dh3d_knn_bruteforce_plan): ("small", CPL, Q) a wave per query, CPL candidates per lane and Q queries per wave
    (N <= 2048); ("lane", KMAX) a lane per query with a K-list of KMAX; ("anydp", KMAX) the kernel for Dp != 3.  None where
    the entry refuses the shape."""
    r = L.lib().dh3d_knn_bruteforce_plan(int(B), int(Dp), int(N), int(k))
    if r < 0:
        return None
    family, a, b = KNN_FAMILIES[r >> 16], (r >> 8) & 255, r & 255
    return (family, a, b) if family == "small" else (family, b)


def spatial_sort(xyz):
    """xyz [B,N,3] -> (sorted [B,N,4] Morton-ordered records (x,y,z,bits(orig idx)), gbox [B,ceil(N/64),8])."""
    x = L.require_cuda_f32(xyz, "xyz", 3)
    B, N, _ = x.shape
    srt = torch.empty((B, N, 4), dtype=torch.float32, device=x.device)
    gbox = torch.empty((B, (N + 63) // 64, 8), dtype=torch.float32, device=x.device)
    L.check(L.lib().dh3d_spatial_sort(L.ptr(x), B, N, L.ptr(srt), L.ptr(gbox), L.stream_ptr()), "spatial_sort")
    return srt, gbox


CELL_INTS = 4112   # include/dh3d_hip.h DH3D_CELL_INTS
CELL_FLAG = 4106   # csrc/cell_grid.h kCellFlag: 1 = a crowded cloud, knn_grid serves it with the pruned scan
CELL_SCHED = 4107  # csrc/cell_grid.h kCellSched: the grid's bit schedule (0x186186 = a cube's z y x z y x ...)


def spatial_sort_cells(xyz):
    """spatial_sort + the 16^3 cell table of every cloud: (sorted, gbox, cells [B, CELL_INTS] int32)."""
    x = L.require_cuda_f32(xyz, "xyz", 3)
    B, N, _ = x.shape
    srt = torch.empty((B, N, 4), dtype=torch.float32, device=x.device)
    gbox = torch.empty((B, (N + 63) // 64, 8), dtype=torch.float32, device=x.device)
    cells = torch.empty((B, CELL_INTS), dtype=torch.int32, device=x.device)
    L.check(L.lib().dh3d_spatial_sort_cells(L.ptr(x), B, N, L.ptr(srt), L.ptr(gbox), L.ptr(cells), L.stream_ptr()),
            "spatial_sort_cells")
    return srt, gbox, cells


def knn_grid(srt, gbox, cells, k, out=None):
    """kNN by cell lists on the three outputs of spatial_sort_cells(); same (nbr [B,N,K], dist) as knn_xyz bit for bit.
    K <= 8.  out: optional (nn int32 [B,N,K], dist float32 [B,N,K]), contiguous on the device, to write into."""
    B, N, _ = srt.shape
    nn, dist = _knn_out("knn_grid", out, B, N, k, srt.device)
    L.check(L.lib().dh3d_knn_grid(L.ptr(srt), L.ptr(gbox), L.ptr(cells), B, N, k, L.ptr(nn), L.ptr(dist), L.stream_ptr()), "knn_grid")
    return nn, dist


def knn_grid_plan(B, N, k):
    """The launch plan knn_grid makes for B clouds of N points and K neighbours (host only): (code, D).  code 4 / 2: the
    crowded clouds' pruned scan runs inside knn_grid_kernel<4, code> (G = B * ceil(N / 64) <= 1280 / <= 4096); 0: the cell
    lists, then the knn_sorted kernel gated on the crowded flag in a second launch.  D: grid bits dropped for small sets.
    None where knn_grid refuses the shape."""
    r = L.lib().dh3d_knn_grid_plan(int(B), int(N), int(k))
    return None if r < 0 else (r % 16, r // 16)


def knn_sorted(srt, gbox, k, out=None):
    """kNN from spatial_sort() output; same (nbr [B,N,K], dist) as knn_xyz, original indexing.
    out: optional (nn int32 [B,N,K], dist float32 [B,N,K]), contiguous on the device, to write into."""
    B, N, _ = srt.shape
    nn, dist = _knn_out("knn_sorted", out, B, N, k, srt.device)
    L.check(L.lib().dh3d_knn_sorted(L.ptr(srt), L.ptr(gbox), B, N, k, L.ptr(nn), L.ptr(dist), L.stream_ptr()),
            "knn_sorted")
    return nn, dist


def knn_sorted_plan(B, N, k):
    """The kernel knn_sorted launches for B clouds of N points and K neighbours (host only; dh3d_knn_sorted_plan):
    (S, KMAX).  S = 8 / 4 / 2: knn_split_kernel<KMAX, S>, S waves per 64-query group (G = B * ceil(N / 64) <= 256 / 1280 /
    4096 and K <= 16); S = 0: the one-wave knn_sorted_kernel<KMAX>.  None where knn_sorted refuses the shape."""
    r = L.lib().dh3d_knn_sorted_plan(int(B), int(N), int(k))
    return None if r < 0 else (r // 256, r % 256)


def _ball_args(radius, nsample, xyz1, xyz2, what):
    """The checks both ball-query kernels share -> (x1, x2, radii tensor or None, b, n, m)."""
    # the operator's own refusals first (tf_grouping.cpp:90-104), then where the tensors live: the two kinds of error do
    # not mask each other
    if int(nsample) <= 0:
        raise ValueError("%s expects positive nsample" % what)
    if not isinstance(radius, torch.Tensor) and not float(radius) > 0.0:
        raise ValueError("%s expects positive radius" % what)
    if all(isinstance(t, torch.Tensor) and t.dim() == 3 for t in (xyz1, xyz2)):
        if xyz1.shape[2] != 3 or xyz2.shape[2] != 3:
            raise ValueError("%s expects (batch_size,ndataset,3) xyz1 and (batch_size,npoint,3) xyz2" % what)
        if xyz1.shape[0] != xyz2.shape[0]:
            raise ValueError("%s: batch(xyz1/xyz2) mismatch: %d vs %d" % (what, xyz1.shape[0], xyz2.shape[0]))
    x1 = L.require_cuda_f32(xyz1, "xyz1", 3)
    x2 = L.require_cuda_f32(xyz2, "xyz2", 3)
    if x1.device != x2.device:
        raise ValueError("%s: xyz1 and xyz2 live on different devices" % what)
    b, n, m = x1.shape[0], x1.shape[1], x2.shape[1]
    if b <= 0 or n <= 0 or m <= 0:
        raise ValueError("%s: empty xyz1 %s or xyz2 %s" % (what, tuple(x1.shape), tuple(x2.shape)))
    if isinstance(radius, torch.Tensor):
        rad = L.require_cuda_f32(radius, "radii", 2)
        if tuple(rad.shape) != (b, m) or rad.device != x1.device:
            raise ValueError("%s: radii must be [%d, %d] on %s, got %s on %s" % (what, b, m, x1.device, tuple(rad.shape),
                                                                             rad.device))
    else:
        rad = None
    return x1, x2, rad, b, n, m


def ball_query_scan(radius, nsample, xyz1, xyz2):
    """query_ball_point by the scan kernel (any shape): xyz1 [b,n,3] dataset, xyz2 [b,m,3] queries -> (idx [b,m,nsample]
    int32, pts_cnt [b,m] int32).  radius: a positive float, or a float32 tensor [b,m] of per-query radii
    (query_ball_point2; a radius <= 0 or NaN has no hits).  Row format: include/dh3d_hip.h dh3d_query_ball_point."""
    x1, x2, rad, b, n, m = _ball_args(radius, nsample, xyz1, xyz2, "ball_query_scan")
    idx = torch.empty((b, m, int(nsample)), dtype=torch.int32, device=x1.device)
    cnt = torch.empty((b, m), dtype=torch.int32, device=x1.device)
    with torch.cuda.device(x1.device):
        if rad is None:
            st = L.lib().dh3d_query_ball_point(b, n, m, float(radius), int(nsample), L.ptr(x1), L.ptr(x2), L.ptr(idx),
                                               L.ptr(cnt), L.stream_ptr())
        else:
            st = L.lib().dh3d_query_ball_point2(b, n, m, int(nsample), L.ptr(x1), L.ptr(x2), L.ptr(rad), L.ptr(idx),
                                                L.ptr(cnt), L.stream_ptr())
    L.check(st, "ball_query_scan")
    return idx, cnt


def ball_query_grid(radius, nsample, xyz1, xyz2, sort=None):
    """The same (idx, pts_cnt) bit for bit by cell lists (n <= 16384).  sort: the (sorted, gbox, cells) of
    spatial_sort_cells(xyz1) when the caller holds them already; None: sorted here."""
    x1, x2, rad, b, n, m = _ball_args(radius, nsample, xyz1, xyz2, "ball_query_grid")
    if n > 16384:
        raise ValueError("ball_query_grid: n = %d is beyond the spatial sort (16384)" % n)
    with torch.cuda.device(x1.device):
        srt, gbox, cells = spatial_sort_cells(x1) if sort is None else sort
        if tuple(srt.shape) != (b, n, 4) or tuple(cells.shape) != (b, CELL_INTS) or tuple(gbox.shape) != (b, (n + 63) // 64, 8):
            raise ValueError("ball_query_grid: sort is not spatial_sort_cells() of a [%d, %d, 3] cloud" % (b, n))
        r = rad if rad is not None else torch.full((1,), float(radius), dtype=torch.float32, device=x1.device)
        idx = torch.empty((b, m, int(nsample)), dtype=torch.int32, device=x1.device)
        cnt = torch.empty((b, m), dtype=torch.int32, device=x1.device)
        L.check(L.lib().dh3d_query_ball_point_grid(b, n, m, L.ptr(r), int(rad is not None), int(nsample), L.ptr(srt),
                                                   L.ptr(gbox), L.ptr(cells), L.ptr(x2), L.ptr(idx), L.ptr(cnt),
                                                   L.stream_ptr()), "ball_query_grid")
    return idx, cnt


BALL_GRID_MIN_N, BALL_GRID_MAX_N = 1 << 30, 16384  # csrc/ball_query.hip kGridMinN (no shape yet: not measured), the sort's limit


def ball_query_plan(n, m, nsample):
    """The dispatcher's one rule, on shapes alone (= dh3d_query_ball_point_plan): 1 sort + cell lists, 0 the scan."""
    if n <= 0 or m <= 0 or nsample <= 0:
        return -1
    return 1 if BALL_GRID_MIN_N <= n <= BALL_GRID_MAX_N else 0


KNN_POINT_FUSED_MAX_K, KNN_POINT_MAX_K = 64, 1024  # csrc/knn_point.hip kFusedMaxK, kRowMaxK


def knn_point_plan(n, m, c, k):
    """The kernel dh3d_knn_point runs for a shape (= dh3d_knn_point_plan): 1 the fused kernel (c = 3, k <= 64), 0 the
    generic one (a workgroup per query, any c, k <= 1024), -1 a shape it refuses.  Never the batch or the data."""
    if n <= 0 or m <= 0 or c <= 0 or k <= 0 or k > n:
        return -1
    if c == 3 and k <= KNN_POINT_FUSED_MAX_K:
        return 1
    return 0 if k <= KNN_POINT_MAX_K else -1


def select_top_k(k, dist):
    """dist [b,m,n] float32 -> (idx [b,m,n] int32, dist_out [b,m,n]): every row the reference's partial selection sort of
    its first k entries, whole row returned (include/dh3d_hip.h dh3d_select_top_k: ROW FORMAT, TIE ORDER)."""
    k = int(k)
    if k < 1 or (isinstance(dist, torch.Tensor) and dist.dim() == 3 and k > dist.shape[2]):
        raise ValueError("SelectionSort expects 1 <= k <= n")
    if isinstance(dist, torch.Tensor) and dist.dim() != 3:
        raise ValueError("SelectionSort expects rank 3: (b,m,n) dist shape")  # tf_grouping.cpp:181
    d = L.require_cuda_f32(dist, "dist", 3)
    b, m, n = d.shape
    if b <= 0 or m <= 0:
        raise ValueError("SelectionSort: empty dist %s" % (tuple(d.shape),))
    idx = torch.empty((b, m, n), dtype=torch.int32, device=d.device)
    out = torch.empty((b, m, n), dtype=torch.float32, device=d.device)
    with torch.cuda.device(d.device):
        L.check(L.lib().dh3d_select_top_k(b, n, m, k, L.ptr(d), L.ptr(idx), L.ptr(out), L.stream_ptr()), "select_top_k")
    return idx, out


def knn_point(k, xyz1, xyz2):
    """xyz1 [b,n,c] dataset, xyz2 [b,m,c] queries -> (val [b,m,k] squared distances, idx [b,m,k] int32): the first k columns
    of select_top_k on the squared-distance matrix, which is never formed (include/dh3d_hip.h dh3d_knn_point)."""
    k = int(k)
    # the operator's own refusals first, then where the tensors live (as _ball_args)
    if k < 1:
        raise ValueError("SelectionSort expects 1 <= k <= n")
    if all(isinstance(t, torch.Tensor) for t in (xyz1, xyz2)):
        if xyz1.dim() == 3 and xyz2.dim() == 3:
            if k > xyz1.shape[1]:
                raise ValueError("SelectionSort expects 1 <= k <= n")
            if xyz1.shape[0] != xyz2.shape[0]:
                raise ValueError("knn_point: batch(xyz1/xyz2) mismatch: %d vs %d" % (xyz1.shape[0], xyz2.shape[0]))
            if xyz1.shape[2] != xyz2.shape[2] or xyz1.shape[2] < 1:
                raise ValueError("knn_point: c(xyz1/xyz2) mismatch: %d vs %d" % (xyz1.shape[2], xyz2.shape[2]))
        else:
            raise ValueError("knn_point expects rank 3: (batch_size,ndataset,c) xyz1 and (batch_size,npoint,c) xyz2")
    x1 = L.require_cuda_f32(xyz1, "xyz1", 3)
    x2 = L.require_cuda_f32(xyz2, "xyz2", 3)
    if x1.device != x2.device:
        raise ValueError("knn_point: xyz1 and xyz2 live on different devices")
    (b, n, c), m = x1.shape, x2.shape[1]
    if b <= 0 or m <= 0:
        raise ValueError("knn_point: empty xyz1 %s or xyz2 %s" % (tuple(x1.shape), tuple(x2.shape)))
    if knn_point_plan(n, m, c, k) < 0:
        raise ValueError("knn_point: k = %d is beyond the kernels (%d)" % (k, KNN_POINT_MAX_K))
    val = torch.empty((b, m, k), dtype=torch.float32, device=x1.device)
    idx = torch.empty((b, m, k), dtype=torch.int32, device=x1.device)
    with torch.cuda.device(x1.device):
        L.check(L.lib().dh3d_knn_point(b, n, m, c, k, L.ptr(x1), L.ptr(x2), L.ptr(val), L.ptr(idx), L.stream_ptr()),
                "knn_point")
    return val, idx


PROB_SAMPLE_MAX_N, PROB_SAMPLE_MAX_M = 1 << 20, 1 << 20  # csrc/prob_sample.hip kMaxN, kMaxM


def _prob_rows(inp, what):
    """The checks ProbSample's weights go through, the operator's own refusal first (tf_sampling.cpp:76)."""
    if isinstance(inp, torch.Tensor) and inp.dim() != 2:
        raise ValueError("ProbSample expects (batch_size,num_choices) inp shape")
    p = L.require_cuda_f32(inp, "inp", 2)
    if p.shape[0] < 1 or p.shape[1] < 1:
        raise ValueError("%s: empty inp %s" % (what, tuple(p.shape)))
    if p.shape[1] > PROB_SAMPLE_MAX_N:
        raise ValueError("%s: num_choices = %d is beyond the kernels (%d)" % (what, p.shape[1], PROB_SAMPLE_MAX_N))
    return p


def prob_sample(inp, inpr):
    """inp [b,n] float32 weights, inpr [b,m] float32 draws -> (ids [b,m] int32, cum [b,n] float32 the reference's cumulative
    sums, its `temp`): include/dh3d_hip.h dh3d_prob_sample."""
    if isinstance(inp, torch.Tensor) and inp.dim() != 2:
        raise ValueError("ProbSample expects (batch_size,num_choices) inp shape")  # tf_sampling.cpp:76
    if isinstance(inp, torch.Tensor) and isinstance(inpr, torch.Tensor) and (inpr.dim() != 2 or inpr.shape[0] != inp.shape[0]):
        raise ValueError("ProbSample expects (batch_size,num_points) inpr shape")  # tf_sampling.cpp:79
    p = _prob_rows(inp, "prob_sample")
    r = L.require_cuda_f32(inpr, "inpr", 2)
    if p.device != r.device:
        raise ValueError("prob_sample: inp and inpr live on different devices")
    (b, n), m = p.shape, r.shape[1]
    if m < 1 or m > PROB_SAMPLE_MAX_M:
        raise ValueError("prob_sample: num_points = %d is outside 1 .. %d" % (m, PROB_SAMPLE_MAX_M))
    cum = torch.empty((b, n), dtype=torch.float32, device=p.device)
    ids = torch.empty((b, m), dtype=torch.int32, device=p.device)
    with torch.cuda.device(p.device):
        L.check(L.lib().dh3d_prob_sample(b, n, m, L.ptr(p), L.ptr(r), L.ptr(cum), L.ptr(ids), L.stream_ptr()), "prob_sample")
    return ids, cum


def prob_sample_seeded(inp, m, count, seed):
    """inp [b,n] float32 weights, count [b] int32 or None, seed a 1-element int64 GPU tensor -> (ids [b,m] int32, cum [b,n]):
    include/dh3d_hip.h dh3d_prob_sample_seeded.  cum holds the sums of a row's first count[b] entries, zeros behind them."""
    p = _prob_rows(inp, "prob_sample_seeded")
    m = int(m)
    if m < 1 or m > PROB_SAMPLE_MAX_M:
        raise ValueError("prob_sample_seeded: m = %d is outside 1 .. %d" % (m, PROB_SAMPLE_MAX_M))
    b, n = p.shape
    c = None
    if count is not None:
        c = L.require_cuda_i32(count, "count", 1)
        if c.shape[0] != b:
            raise ValueError("prob_sample_seeded expects (batch_size) count = (%d,), got %s" % (b, tuple(c.shape)))
    cum = torch.empty((b, n), dtype=torch.float32, device=p.device)
    ids = torch.empty((b, m), dtype=torch.int32, device=p.device)
    with torch.cuda.device(p.device):
        L.check(L.lib().dh3d_prob_sample_seeded(b, n, m, L.ptr(p), L.ptr(c), L.ptr(seed), L.ptr(cum), L.ptr(ids),
                                                L.stream_ptr()), "prob_sample_seeded")
    return ids, cum


PREPARE_MAX_N, PREPARE_MAX_TARGET = 131072, 1 << 20  # csrc/prepare.hip kMaxN, kMaxTarget


def prepare_clouds(raw, num_raw, targetnum, voxel_size=0.2, radius=1.0, nb_points=4, sortby_dis=True):
    """raw [B,Nraw,3] float32, num_raw [B] int32 -> (points [B,targetnum,3], num_valid [B] int32, counts [B,3] int32,
    centroid [B,3] float64): voxel grid, radius-outlier removal and crop / pad of every cloud on the device, no host sync
    (dh3d_prepare_clouds in include/dh3d_hip.h holds the semantics).  voxel_size / radius None: that stage is skipped."""
    targetnum, nb_points = int(targetnum), int(nb_points)
    vox = 0.0 if voxel_size is None else float(voxel_size)
    rad = 0.0 if radius is None else float(radius)
    if targetnum < 1:
        raise ValueError("prepare_clouds expects targetnum >= 1")
    if (voxel_size is not None and not 0.0 < vox < float("inf")) or (radius is not None and not 0.0 < rad < float("inf")):
        raise ValueError("prepare_clouds expects a positive finite voxel_size and radius (or None to skip the stage)")
    if nb_points < 0:
        raise ValueError("prepare_clouds expects nb_points >= 0")
    if all(isinstance(t, torch.Tensor) for t in (raw, num_raw)):
        if raw.dtype != torch.float32 or num_raw.dtype != torch.int32:
            raise ValueError("prepare_clouds expects float32 raw and int32 num_raw, got %s and %s" % (raw.dtype, num_raw.dtype))
        if raw.dim() != 3 or raw.shape[2] != 3 or raw.shape[0] < 1 or raw.shape[1] < 1:
            raise ValueError("prepare_clouds expects (batch_size,nraw,3) raw, got %s" % (tuple(raw.shape),))
        if num_raw.dim() != 1 or num_raw.shape[0] != raw.shape[0]:
            raise ValueError("prepare_clouds expects (batch_size) num_raw = (%d,), got %s" % (raw.shape[0], tuple(num_raw.shape)))
        if raw.shape[1] > PREPARE_MAX_N or targetnum > PREPARE_MAX_TARGET:
            raise ValueError("prepare_clouds: nraw = %d / targetnum = %d is beyond the kernels (%d / %d)"
                             % (raw.shape[1], targetnum, PREPARE_MAX_N, PREPARE_MAX_TARGET))
    x = L.require_cuda_f32(raw, "raw", 3)
    n = L.require_cuda_i32(num_raw, "num_raw", 1)
    if x.device != n.device:
        raise ValueError("prepare_clouds: raw and num_raw live on different devices")
    B, N, _ = x.shape
    points = torch.empty((B, targetnum, 3), dtype=torch.float32, device=x.device)
    num_valid = torch.empty((B,), dtype=torch.int32, device=x.device)
    counts = torch.empty((B, 3), dtype=torch.int32, device=x.device)
    centroid = torch.empty((B, 3), dtype=torch.float64, device=x.device)
    nbytes = L.lib().dh3d_prepare_clouds_workspace(B, N, targetnum)
    if nbytes == 0:
        raise ValueError("prepare_clouds: shape B = %d, nraw = %d, targetnum = %d is beyond the kernels" % (B, N, targetnum))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        L.check(L.lib().dh3d_prepare_clouds(B, N, targetnum, L.ptr(x), L.ptr(n), vox, rad, nb_points, int(bool(sortby_dis)),
                                            L.ptr(points), L.ptr(num_valid), L.ptr(counts), L.ptr(centroid), L.ptr(ws),
                                            nbytes, L.stream_ptr()), "prepare_clouds")
    return points, num_valid, counts, centroid


KEYPOINT_MAX = 4096  # include/dh3d_hip.h dh3d_keypoint_nms: M limit


def keypoint_nms(scores, nn, dist, nms_radius, min_response_ratio, max_keypoints, remove_noise=True, num_valid=None,
                 invert=False):
    """Keypoint NMS of a batch (dh3d_keypoint_nms): scores [B,N] float32 (a strided view such as xyz_feat_att[:, :, 131] is
    read in place), nn / dist [B,N,K] from knn_xyz / knn_sorted, num_valid [B] int32 or None, invert: the score is
    1 - scores.  -> (count [B] int32, inds [B, max_keypoints] int32, -1 padded), on the device, no host sync."""
    if not isinstance(scores, torch.Tensor) or scores.dtype != torch.float32 or not scores.is_cuda or scores.dim() != 2:
        raise ValueError("scores must be a float32 [B, N] tensor on the GPU")
    B, N = scores.shape
    if scores.stride(1) < 1 or scores.stride(0) != N * scores.stride(1):
        scores = scores.contiguous()
    nn = L.require_cuda_i32(nn, "nn", 3)
    dist = L.require_cuda_f32(dist, "dist", 3)
    K = nn.shape[2]
    if tuple(nn.shape) != (B, N, K) or tuple(dist.shape) != (B, N, K):
        raise ValueError("nn / dist must be [%d, %d, K], got %s / %s" % (B, N, tuple(nn.shape), tuple(dist.shape)))
    if num_valid is not None:
        num_valid = L.require_cuda_i32(num_valid, "num_valid", 1)
        if num_valid.shape[0] != B:
            raise ValueError("num_valid must be [%d], got %s" % (B, tuple(num_valid.shape)))
    M = int(max_keypoints)
    if not 1 <= M <= KEYPOINT_MAX:
        raise ValueError("max_keypoints must be in [1, %d], got %d" % (KEYPOINT_MAX, M))
    ws_bytes = L.lib().dh3d_keypoint_nms_workspace_bytes(B, N, M)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=scores.device)
    count = torch.empty((B,), dtype=torch.int32, device=scores.device)
    inds = torch.empty((B, M), dtype=torch.int32, device=scores.device)
    L.check(L.lib().dh3d_keypoint_nms(L.ptr(scores), scores.stride(1), int(bool(invert)), L.ptr(nn), L.ptr(dist),
                                      L.ptr(num_valid), B, N, K, float(nms_radius), float(min_response_ratio), M,
                                      int(bool(remove_noise)), L.ptr(count), L.ptr(inds), L.ptr(ws), ws_bytes,
                                      L.stream_ptr()), "keypoint_nms")
    return count, inds


def gather_rows(src, inds, count):
    """src [B,N,C] float32, inds [B,M] / count [B] int32 (keypoint_nms) -> [B,M,C]: the rows src[b, inds[b, j]] for
    j < count[b], zero rows after that (dh3d_gather_rows)."""
    x = L.require_cuda_f32(src, "src", 3)
    ix = L.require_cuda_i32(inds, "inds", 2)
    cnt = L.require_cuda_i32(count, "count", 1)
    B, N, C = x.shape
    if ix.shape[0] != B or cnt.shape[0] != B:
        raise ValueError("inds [%d, M] / count [%d] expected, got %s / %s" % (B, B, tuple(ix.shape), tuple(cnt.shape)))
    M = ix.shape[1]
    out = torch.empty((B, M, C), dtype=torch.float32, device=x.device)
    L.check(L.lib().dh3d_gather_rows(L.ptr(x), B, N, C, L.ptr(ix), L.ptr(cnt), M, L.ptr(out), L.stream_ptr()),
            "gather_rows")
    return out


def fps_sorted(srt, gbox, npoint, with_xyz=False, xyz=None):
    """FPS from spatial_sort() output; same idx [B,npoint] (original indexing) as ops.farthest_point_sample.
    with_xyz: also the sampled coordinates [B,npoint,3], written by the same kernel.
    xyz: the cloud the records came from -- required where the LDS coordinate table does not fit (above 12288 points, or
    fps_sorted_fits(N, npoint) false)."""
    B, N, _ = srt.shape
    out = torch.empty((B, npoint), dtype=torch.int32, device=srt.device)
    xyz_s = torch.empty((B, npoint, 3), dtype=torch.float32, device=srt.device) if with_xyz else None
    if xyz is not None:
        x = L.require_cuda_f32(xyz, "xyz", 3)
        L.check(L.lib().dh3d_fps_sorted_cloud(L.ptr(srt), L.ptr(gbox), L.ptr(x), B, N, npoint, L.ptr(out), L.ptr(xyz_s),
                                              L.stream_ptr()), "fps_sorted_cloud")
    elif with_xyz:
        L.check(L.lib().dh3d_fps_sorted_xyz(L.ptr(srt), L.ptr(gbox), B, N, npoint, L.ptr(out), L.ptr(xyz_s),
                                            L.stream_ptr()), "fps_sorted_xyz")
    else:
        L.check(L.lib().dh3d_fps_sorted(L.ptr(srt), L.ptr(gbox), B, N, npoint, L.ptr(out), L.stream_ptr()),
                "fps_sorted")
    return (out, xyz_s) if with_xyz else out


def fps_sorted_fits(N, npoint, ordered=False, with_cloud=False):
    """Does the sorted FPS kernel take N points -> npoint picks?  ordered: fps_sorted_ordered; with_cloud: fps_sorted(xyz=);
    neither: fps_sorted without the cloud (the LDS coordinate table).  Host-side query of the launcher's LDS budget."""
    return L.lib().dh3d_fps_sorted_fits(int(N), int(npoint), int(bool(ordered)), int(bool(with_cloud))) == 1


def fps_sorted_ordered(srt, gbox, npoint, cells=None):
    """fps_sorted(with_xyz=True) + the sampled set in the cloud's Morton order out of the same launch: returns
    (idx [B,m], xyz_s [B,m,3], srt_s [B,m,4], gbox_s [B,ceil(m/64),8], cells_s [B,CELL_INTS] or None) -- srt_s / gbox_s /
    cells_s are what spatial_sort_cells(xyz_s) would hand to three_nn_sorted / knn_grid (cells_s only when the cloud's
    own table `cells` is given).  N <= 8192 and fps_sorted_fits(N, npoint, ordered=True)."""
    B, N, _ = srt.shape
    dev = srt.device
    out = torch.empty((B, npoint), dtype=torch.int32, device=dev)
    xyz_s = torch.empty((B, npoint, 3), dtype=torch.float32, device=dev)
    srt_s = torch.empty((B, npoint, 4), dtype=torch.float32, device=dev)
    gbox_s = torch.empty((B, (npoint + 63) // 64, 8), dtype=torch.float32, device=dev)
    cells_s = torch.empty((B, CELL_INTS), dtype=torch.int32, device=dev) if cells is not None else None
    L.check(L.lib().dh3d_fps_sorted_ordered(L.ptr(srt), L.ptr(gbox), L.ptr(cells), B, N, npoint, L.ptr(out), L.ptr(xyz_s),
                                            L.ptr(srt_s), L.ptr(gbox_s), L.ptr(cells_s), L.stream_ptr()), "fps_sorted_ordered")
    return out, xyz_s, srt_s, gbox_s, cells_s


def three_nn_sorted(srt1, gbox1, srt2, gbox2, cells2=None):
    """three_nn from spatial_sort() outputs of the query cloud and of the candidate set: same (dist [B,n,3] squared,
    idx [B,n,3]) as ops.three_nn, original indexing on both sides.  cells2: the candidate set's cell table [B,CELL_INTS]
    (fps_sorted_ordered's cells_s, or spatial_sort_cells of the set) -- a query group then visits only the samples of the
    cells it can reach (128 <= m <= 1024; other sizes ignore the table)."""
    B, n, _ = srt1.shape
    m = srt2.shape[1]
    d3 = torch.empty((B, n, 3), dtype=torch.float32, device=srt1.device)
    i3 = torch.empty((B, n, 3), dtype=torch.int32, device=srt1.device)
    if cells2 is not None:
        c2 = L.require_cuda_i32(cells2, "cells2", 2)
        if tuple(c2.shape) != (B, CELL_INTS):
            raise ValueError("three_nn_sorted: cells2 is not the cell table of a batch of %d sets" % B)
        L.check(L.lib().dh3d_three_nn_cells(B, n, m, L.ptr(srt1), L.ptr(gbox1), L.ptr(srt2), L.ptr(gbox2), L.ptr(c2),
                                            L.ptr(d3), L.ptr(i3), L.stream_ptr()), "three_nn_cells")
        return d3, i3
    L.check(L.lib().dh3d_three_nn_sorted(B, n, m, L.ptr(srt1), L.ptr(gbox1), L.ptr(srt2), L.ptr(gbox2), L.ptr(d3),
                                         L.ptr(i3), L.stream_ptr()), "three_nn_sorted")
    return d3, i3


def pack_weight(W):
    """W [Kd, Dout] row-major -> MFMA fragment order (see mfma_gemm.h)."""
    W = L.require_cuda_f32(W, "W", 2)
    out = torch.empty_like(W)
    L.check(L.lib().dh3d_pack_weight(L.ptr(W), W.shape[0], W.shape[1], L.ptr(out), L.stream_ptr()), "pack_weight")
    return out


def pack_flex_weight(theta, bias):
    """theta [3,Din,Dout], bias [Din,Dout] -> packed [4*Din, Dout] = [bias; theta_x; theta_y; theta_z]."""
    t = L.require_cuda_f32(theta, "theta", 3)
    b = L.require_cuda_f32(bias, "bias", 2)
    if t.shape[0] != 3:
        raise ValueError("point-major flex_conv needs Dp == 3")
    Din, Dout = b.shape
    out = torch.empty((4 * Din, Dout), dtype=torch.float32, device=t.device)
    L.check(L.lib().dh3d_pack_flex_weight(L.ptr(t), L.ptr(b), Din, Dout, L.ptr(out), L.stream_ptr()),
            "pack_flex_weight")
    return out


def flex_conv(features, xyz, nbr, wpacked, Dout, pre_bias=None, scale=None, shift=None, act=ACT_NONE, remap=None):
    """Fused factorised flex_conv (exact-f32 MFMA).  remap [B,N] int32 (optional): `features` is the [B,Nsrc,Din] map of
    the level above and point j of this level is its row remap[b,j] -- group_point fused into the neighbour gather."""
    f = L.require_cuda_f32(features, "features", 3)
    x = L.require_cuda_f32(xyz, "xyz", 3)
    nb = L.require_cuda_i32(nbr, "nbr", 3)
    B, N = x.shape[0], x.shape[1]
    Din = f.shape[2]
    K = nb.shape[2]
    rm = None
    if remap is not None:
        rm = L.require_cuda_i32(remap, "remap", 2)
        if tuple(rm.shape) != (B, N) or f.shape[0] != B:
            raise ValueError("flex_conv: remap must be [B,N] and features [B,Nsrc,Din]")
    elif tuple(f.shape[:2]) != (B, N):
        raise ValueError("flex_conv: xyz/nbr do not match features [B,N,*]")
    if tuple(x.shape) != (B, N, 3) or tuple(nb.shape[:2]) != (B, N):
        raise ValueError("flex_conv: xyz/nbr do not match [B,N,*]")
    out = torch.empty((B, N, Dout), dtype=torch.float32, device=f.device)
    ep = L.make_epilogue(pre_bias, scale, shift, act)
    L.check(L.lib().dh3d_flex_conv_pm_gather_fwd(L.ptr(f), L.ptr(rm), f.shape[1], L.ptr(x), L.ptr(nb), L.ptr(wpacked), B,
                                                 N, K, Din, Dout, ep, L.ptr(out), L.stream_ptr()), "flex_conv_pm")
    return out


def flex_tile_x6_supported(Din, Dout, K):
    """Shapes served by the 32-point-tile bf16x6 flex_conv (csrc/flex_tx6.hip): the sampled levels, cfg 5's K = 12."""
    return (Din, Dout, K) in ((64, 128, 8), (128, 128, 8), (128, 256, 8), (128, 128, 12))


def flex_conv_tile_x6(features, xyz, nbr, wpacked_x3, Dout, pre_bias=None, scale=None, shift=None, act=ACT_NONE,
                      wpost_packed=None, Dpost=0):
    """flex_conv on 32-point tiles, tile GEMM on the bf16 matrix pipe at f32 accuracy.  With wpost_packed (a packed
    [Dout, 64] weight; 128 -> 256, K = 8): returns (out, out @ Wpost) from the same launch."""
    f = L.require_cuda_f32(features, "features", 3)
    x = L.require_cuda_f32(xyz, "xyz", 3)
    nb = L.require_cuda_i32(nbr, "nbr", 3)
    B, N, Din = f.shape
    if tuple(x.shape) != (B, N, 3) or tuple(nb.shape[:2]) != (B, N):
        raise ValueError("flex_conv_tile_x6: xyz/nbr do not match features [B,N,*]")
    out = torch.empty((B, N, Dout), dtype=torch.float32, device=f.device)
    out2 = torch.empty((B, N, Dpost), dtype=torch.float32, device=f.device) if wpost_packed is not None else None
    ep = L.make_epilogue(pre_bias, scale, shift, act)
    L.check(L.lib().dh3d_flex_conv_pm_tile_x6_fwd(L.ptr(f), L.ptr(x), L.ptr(nb), L.ptr(wpacked_x3), B, N, nb.shape[2], Din,
                                                  Dout, ep, L.ptr(out), L.ptr(wpost_packed), int(Dpost), L.ptr(out2),
                                                  L.stream_ptr()), "flex_conv_pm_tile_x6")
    return out if wpost_packed is None else (out, out2)


def flex_x6_supported(Din, Dout, K):
    """Shapes served by the persistent bf16x6 flex_conv (csrc/flex_x6.hip)."""
    return K == 8 and (Din, Dout) in ((32, 64), (64, 64))


def pack_flex_weight_x3(theta, bias):
    """[bias; theta_x; theta_y; theta_z] as three exact bf16 chunk planes in MFMA fragment order."""
    t = L.require_cuda_f32(theta, "theta", 3)
    b = L.require_cuda_f32(bias, "bias", 2)
    if t.shape[0] != 3:
        raise ValueError("point-major flex_conv needs Dp == 3")
    Din, Dout = b.shape
    out = torch.empty((3 * 4 * Din * Dout,), dtype=torch.int16, device=t.device)
    L.check(L.lib().dh3d_pack_flex_weight_x3(L.ptr(t), L.ptr(b), Din, Dout, L.ptr(out), L.stream_ptr()),
            "pack_flex_weight_x3")
    return out


def flex_conv_x6(features, xyz, nbr, wpacked_x3, Dout, pre_bias=None, scale=None, shift=None, act=ACT_NONE,
                 reserve_cus_per_xcd=0):
    """flex_conv on the bf16 matrix pipe at f32 accuracy (full-resolution layers, K == 8).
    reserve_cus_per_xcd: placement hint -- CUs per XCD another stream's kernel holds (speed only, see the header)."""
    f = L.require_cuda_f32(features, "features", 3)
    x = L.require_cuda_f32(xyz, "xyz", 3)
    nb = L.require_cuda_i32(nbr, "nbr", 3)
    B, N, Din = f.shape
    K = nb.shape[2]
    if tuple(x.shape) != (B, N, 3) or tuple(nb.shape[:2]) != (B, N):
        raise ValueError("flex_conv_x6: xyz/nbr do not match features [B,N,*]")
    out = torch.empty((B, N, Dout), dtype=torch.float32, device=f.device)
    ep = L.make_epilogue(pre_bias, scale, shift, act)
    L.check(L.lib().dh3d_flex_conv_pm_x6_fwd_r(L.ptr(f), L.ptr(x), L.ptr(nb), L.ptr(wpacked_x3), B, N, K, Din, Dout, ep,
                                               int(reserve_cus_per_xcd), L.ptr(out), L.stream_ptr()), "flex_conv_pm_x6")
    return out


def flex_pool(features, nbr, want_argmax=False):
    f = L.require_cuda_f32(features, "features", 3)
    nb = L.require_cuda_i32(nbr, "nbr", 3)
    B, N, C = f.shape
    K = nb.shape[2]
    out = torch.empty_like(f)
    argmax = torch.empty((B, N, C), dtype=torch.int32, device=f.device) if want_argmax else None
    L.check(L.lib().dh3d_flex_pool_pm_fwd(L.ptr(f), L.ptr(nb), B, N, K, C, L.ptr(out), L.ptr(argmax),
                                          L.stream_ptr()), "flex_pool_pm")
    return (out, argmax) if want_argmax else out


def flex_avg(features, nbr, scale=1.0):
    """Flex_Avg (core/layers.py:342-436): scale * sum_k features[nbr[n,k]]; backbones.py:80-82 uses scale = 1/knn."""
    f = L.require_cuda_f32(features, "features", 3)
    nb = L.require_cuda_i32(nbr, "nbr", 3)
    B, N, C = f.shape
    out = torch.empty_like(f)
    L.check(L.lib().dh3d_flex_avg_pm_fwd(L.ptr(f), L.ptr(nb), B, N, nb.shape[2], C, float(scale), L.ptr(out),
                                         L.stream_ptr()), "flex_avg_pm")
    return out


def conv_pointset_xyz(xyz, nbr, theta, bias, pre_bias=None, scale=None, shift=None, act=ACT_NONE):
    x = L.require_cuda_f32(xyz, "xyz", 3)
    nb = L.require_cuda_i32(nbr, "nbr", 3)
    B, N, _ = x.shape
    K = nb.shape[2]
    Dout = theta.shape[1]
    out = torch.empty((B, N, Dout), dtype=torch.float32, device=x.device)
    ep = L.make_epilogue(pre_bias, scale, shift, act)
    L.check(L.lib().dh3d_conv_pointset_pm_fwd(L.ptr(x), L.ptr(nb), L.ptr(theta), L.ptr(bias), B, N, K, Dout, ep,
                                              L.ptr(out), L.stream_ptr()), "conv_pointset_pm")
    return out


def conv_pointset_pool_xyz(xyz, nbr, theta, bias, pre_bias=None, scale=None, shift=None, act=ACT_NONE):
    """flex_pool(epilogue(conv_pointset(xyz))) over the same neighbourhoods [B,N,8] in two small launches; the
    [B,N,Dout] map between the two operators is not materialised (core/backbones.py:107-110)."""
    x = L.require_cuda_f32(xyz, "xyz", 3)
    nb = L.require_cuda_i32(nbr, "nbr", 3)
    B, N, _ = x.shape
    Dout = theta.shape[1]
    out = torch.empty((B, N, Dout), dtype=torch.float32, device=x.device)
    scratch = torch.empty((B, N, 4), dtype=torch.float32, device=x.device)
    ep = L.make_epilogue(pre_bias, scale, shift, act)
    L.check(L.lib().dh3d_conv_pointset_pool_pm_fwd(L.ptr(x), L.ptr(nb), L.ptr(theta), L.ptr(bias), B, N, nb.shape[2], Dout,
                                                   ep, L.ptr(scratch), L.ptr(out), L.stream_ptr()), "conv_pointset_pool_pm")
    return out


def linear(x1, wpacked, Dout, x2=None, pre_bias=None, scale=None, shift=None, act=ACT_NONE, residual=None):
    """out = epilogue([x1 | x2] @ W) (+ residual); x* are [..., C] with identical leading dims."""
    a = L.require_cuda_f32(x1, "x1")
    lead = a.shape[:-1]
    C1 = a.shape[-1]
    R = a.numel() // C1
    C2 = 0
    b = None
    if x2 is not None:
        b = L.require_cuda_f32(x2, "x2")
        C2 = b.shape[-1]
        if b.shape[:-1] != lead:
            raise ValueError("linear: x1/x2 leading dims differ")
    res = None
    if residual is not None:
        res = L.require_cuda_f32(residual, "residual")
    out = torch.empty(lead + (Dout,), dtype=torch.float32, device=a.device)
    ep = L.make_epilogue(pre_bias, scale, shift, act)
    L.check(L.lib().dh3d_linear_pm_fwd(L.ptr(a), C1, L.ptr(b), C2, L.ptr(wpacked), R, Dout, ep, L.ptr(res),
                                       L.ptr(out), L.stream_ptr()), "linear_pm")
    return out


def se_res(x, pool, W1, b1, W2, b2):
    a = L.require_cuda_f32(x, "x")
    p = L.require_cuda_f32(pool, "pool")
    C = a.shape[-1]
    R = a.numel() // C
    out = torch.empty_like(a)
    L.check(L.lib().dh3d_se_res_pm_fwd(L.ptr(a), L.ptr(p), L.ptr(W1), L.ptr(b1), L.ptr(W2), L.ptr(b2), R, C,
                                       L.ptr(out), L.stream_ptr()), "se_res_pm")
    return out


def se_res_pack(W1, b1, W2):
    """W1 [C,C/4], b1 [C/4], W2 [C/4,C] -> (w1packed, b1pad, w2packed) for se_res_packed (zero padding to 32)."""
    C, Cq = W1.shape
    W1p = torch.zeros((C, 32), dtype=torch.float32, device=W1.device)
    W1p[:, :Cq] = W1
    b1p = torch.zeros((32,), dtype=torch.float32, device=W1.device)
    b1p[:Cq] = b1
    W2p = torch.zeros((32, C), dtype=torch.float32, device=W1.device)
    W2p[:Cq] = W2
    return pack_weight(W1p), b1p, pack_weight(W2p)


def se_res_packed(x, pool, w1packed, b1pad, w2packed, b2):
    """se_res on the matrix pipe (csrc/dense.hip se_res_mfma_kernel)."""
    a = L.require_cuda_f32(x, "x")
    p = L.require_cuda_f32(pool, "pool")
    C = a.shape[-1]
    R = a.numel() // C
    out = torch.empty_like(a)
    L.check(L.lib().dh3d_se_res_pm_packed_fwd(L.ptr(a), L.ptr(p), L.ptr(w1packed), L.ptr(b1pad), L.ptr(w2packed),
                                              L.ptr(b2), R, C, L.ptr(out), L.stream_ptr()), "se_res_pm_packed")
    return out


def se_res_pool_packed(x, nbr, w1packed, b1pad, w2packed, b2):
    """se_res_packed(x, flex_pool(x, nbr)) in one launch (the pooled rows are formed while staging).  x [B,N,C], nbr
    [B,N,K] int32, C = 64 or 128."""
    a = L.require_cuda_f32(x, "x", 3)
    nb = L.require_cuda_i32(nbr, "nbr", 3)
    B, N, C = a.shape
    out = torch.empty_like(a)
    L.check(L.lib().dh3d_se_res_pool_pm_packed_fwd(L.ptr(a), L.ptr(nb), B, N, nb.shape[2], L.ptr(w1packed), L.ptr(b1pad),
                                                   L.ptr(w2packed), L.ptr(b2), C, L.ptr(out), L.stream_ptr()),
            "se_res_pool_pm_packed")
    return out


def se_res_pool_conv(x, nbr, w1packed, b1pad, w2packed, b2, conv_wp, conv_b, conv_scale, conv_shift, act=ACT_RELU):
    """(y, act(bn(y @ Wconv + b))) with y = se_res_packed(x, flex_pool(x, nbr)), one launch; x [B,N,C], conv C -> C
    (conv_wp = pack_weight of its [C,C] matrix), C = 64 or 128; conv_b / conv_scale / conv_shift may be None."""
    a = L.require_cuda_f32(x, "x", 3)
    nb = L.require_cuda_i32(nbr, "nbr", 3)
    B, N, C = a.shape
    out, out2 = torch.empty_like(a), torch.empty((B, N, C), dtype=torch.float32, device=a.device)
    ep = L.make_epilogue(conv_b, conv_scale, conv_shift, act)
    L.check(L.lib().dh3d_se_res_pool_conv_pm_fwd(L.ptr(a), L.ptr(nb), B, N, nb.shape[2], L.ptr(w1packed), L.ptr(b1pad),
                                                 L.ptr(w2packed), L.ptr(b2), C, L.ptr(out), L.ptr(conv_wp), ep, C,
                                                 L.ptr(out2), L.stream_ptr()), "se_res_pool_conv_pm")
    return out, out2


def three_interpolate_idw(points, idx, dist):
    p = L.require_cuda_f32(points, "points", 3)
    ix = L.require_cuda_i32(idx, "idx", 3)
    d = L.require_cuda_f32(dist, "dist", 3)
    b, m, c = p.shape
    n = ix.shape[1]
    out = torch.empty((b, n, c), dtype=torch.float32, device=p.device)
    L.check(L.lib().dh3d_three_interpolate_idw_fwd(b, m, c, n, L.ptr(p), L.ptr(ix), L.ptr(d), L.ptr(out),
                                                   L.stream_ptr()), "three_interpolate_idw")
    return out


def l2norm_concat(x, eps, prefix=None):
    a = L.require_cuda_f32(x, "x")
    C = a.shape[-1]
    R = a.numel() // C
    P = 0
    pf = None
    if prefix is not None:
        pf = L.require_cuda_f32(prefix, "prefix")
        P = pf.shape[-1]
    out = torch.empty(a.shape[:-1] + (P + C,), dtype=torch.float32, device=a.device)
    L.check(L.lib().dh3d_l2norm_concat_fwd(L.ptr(a), R, C, float(eps), L.ptr(pf), P, L.ptr(out), L.stream_ptr()),
            "l2norm_concat")
    return out


def mlp_head(h, wpacked, H, w_fc, b_fc, pre_bias=None, scale=None, shift=None, act=ACT_RELU):
    a = L.require_cuda_f32(h, "h")
    C = a.shape[-1]
    R = a.numel() // C
    out = torch.empty(a.shape[:-1] + (1,), dtype=torch.float32, device=a.device)
    ep = L.make_epilogue(pre_bias, scale, shift, act)
    L.check(L.lib().dh3d_mlp_head_pm_fwd(L.ptr(a), R, C, L.ptr(wpacked), H, ep, L.ptr(w_fc), float(b_fc),
                                         L.ptr(out), L.stream_ptr()), "mlp_head_pm")
    return out


def linear_x6(x1, wpacked_x3, Dout, x2=None, pre_bias=None, scale=None, shift=None, act=ACT_NONE, residual=None):
    """linear() on the bf16 pipe at f32 accuracy (tiled bf16x6 GEMM); Dout in {128, 256}, C1/C2 multiples of 32."""
    a = L.require_cuda_f32(x1, "x1")
    lead = a.shape[:-1]
    C1 = a.shape[-1]
    R = a.numel() // C1
    C2 = 0
    b = None
    if x2 is not None:
        b = L.require_cuda_f32(x2, "x2")
        C2 = b.shape[-1]
        if b.shape[:-1] != lead:
            raise ValueError("linear_x6: x1/x2 leading dims differ")
    res = None
    if residual is not None:
        res = L.require_cuda_f32(residual, "residual")
    out = torch.empty(lead + (Dout,), dtype=torch.float32, device=a.device)
    ep = L.make_epilogue(pre_bias, scale, shift, act)
    L.check(L.lib().dh3d_linear_pm_x6_fwd(L.ptr(a), C1, L.ptr(b), C2, L.ptr(wpacked_x3), R, Dout, ep, L.ptr(res),
                                          L.ptr(out), L.stream_ptr()), "linear_pm_x6")
    return out


def upsample_linear_x6(points, idx, dist, wpacked_x3, Dout, x2=None, pre_bias=None, scale=None, shift=None,
                       act=ACT_NONE, residual=None, l2cat=None):
    """linear_x6([three_interpolate_idw(points, idx, dist) | x2]) without materialising the up-sampled tensor.
    points [B,m,C1], idx/dist [B,n,3], x2 [B,n,C2].  l2cat = (prefix [B,n,3], eps): return
    [prefix | l2_normalize(result, eps)] [B,n,3+Dout] instead (Dout == 128), the result itself is not written."""
    p = L.require_cuda_f32(points, "points", 3)
    ix = L.require_cuda_i32(idx, "idx", 3)
    d = L.require_cuda_f32(dist, "dist", 3)
    B, m, C1 = p.shape
    n = ix.shape[1]
    C2 = 0
    b = None
    if x2 is not None:
        b = L.require_cuda_f32(x2, "x2", 3)
        C2 = b.shape[-1]
        if tuple(b.shape[:2]) != (B, n):
            raise ValueError("upsample_linear_x6: x2 must be [B,n,C2]")
    res = None
    if residual is not None:
        res = L.require_cuda_f32(residual, "residual", 3)
    ep = L.make_epilogue(pre_bias, scale, shift, act)
    if l2cat is not None:
        pf = L.require_cuda_f32(l2cat[0], "prefix", 3)
        if tuple(pf.shape) != (B, n, 3):
            raise ValueError("upsample_linear_x6: prefix must be [B,n,3]")
        out = torch.empty((B, n, 3 + Dout), dtype=torch.float32, device=p.device)
        L.check(L.lib().dh3d_upsample_linear_l2cat_pm_x6_fwd(L.ptr(p), L.ptr(ix), L.ptr(d), B, n, m, C1, L.ptr(b), C2,
                                                             L.ptr(wpacked_x3), Dout, ep, L.ptr(res), L.ptr(pf),
                                                             float(l2cat[1]), L.ptr(out), L.stream_ptr()),
                "upsample_linear_l2cat_pm_x6")
        return out
    out = torch.empty((B, n, Dout), dtype=torch.float32, device=p.device)
    L.check(L.lib().dh3d_upsample_linear_pm_x6_fwd(L.ptr(p), L.ptr(ix), L.ptr(d), B, n, m, C1, L.ptr(b), C2,
                                                   L.ptr(wpacked_x3), Dout, ep, L.ptr(res), L.ptr(out), L.stream_ptr()),
            "upsample_linear_pm_x6")
    return out


def upsample_linear_shortcut_x6(points, idx, dist, wstacked_x3, Dout, x2, x3, ep_main, ep_shortcut, l2cat=None):
    """act(BN([three_interpolate_idw(points, idx, dist) | x2] W)) + act_sc(BN_sc(x3 W_sc)) in one kernel (Dout == 128);
    wstacked_x3 = pack_weight_x3([W; W_sc]); ep_* = (pre_bias, scale, shift, act).  l2cat as in upsample_linear_x6."""
    p = L.require_cuda_f32(points, "points", 3)
    ix = L.require_cuda_i32(idx, "idx", 3)
    d = L.require_cuda_f32(dist, "dist", 3)
    B, m, C1 = p.shape
    n = ix.shape[1]
    b = L.require_cuda_f32(x2, "x2", 3)
    c = L.require_cuda_f32(x3, "x3", 3)
    if tuple(b.shape[:2]) != (B, n) or tuple(c.shape[:2]) != (B, n):
        raise ValueError("upsample_linear_shortcut_x6: x2 / x3 must be [B,n,*]")
    pf = None
    width = Dout
    if l2cat is not None:
        pf = L.require_cuda_f32(l2cat[0], "prefix", 3)
        if tuple(pf.shape) != (B, n, 3):
            raise ValueError("upsample_linear_shortcut_x6: prefix must be [B,n,3]")
        width = 3 + Dout
    out = torch.empty((B, n, width), dtype=torch.float32, device=p.device)
    e1, e2 = L.make_epilogue(*ep_main), L.make_epilogue(*ep_shortcut)
    L.check(L.lib().dh3d_upsample_linear_shortcut_pm_x6_fwd(
        L.ptr(p), L.ptr(ix), L.ptr(d), B, n, m, C1, L.ptr(b), b.shape[-1], L.ptr(c), c.shape[-1], L.ptr(wstacked_x3),
        Dout, e1, e2, L.ptr(pf), float(l2cat[1]) if l2cat is not None else 0.0, L.ptr(out), L.stream_ptr()),
        "upsample_linear_shortcut_pm_x6")
    return out


def interp_combine(coarse_w, idx, dist, partial=None, pre_bias=None, scale=None, shift=None, act=ACT_NONE, residual=None,
                   l2cat=None):
    """act(BN(interp3(coarse_w) + partial + pre_bias)) + residual -> [B,N,128]; l2cat = (prefix [B,N,3], eps) returns
    [prefix | l2_normalize(.)] [B,N,131] instead (the tail of a concat conv commuted through the up-sampling)."""
    cw = L.require_cuda_f32(coarse_w, "coarse_w", 3)
    ix = L.require_cuda_i32(idx, "idx", 3)
    d = L.require_cuda_f32(dist, "dist", 3)
    B, M, C = cw.shape
    N = ix.shape[1]
    pf, eps = (L.require_cuda_f32(l2cat[0], "prefix", 3), float(l2cat[1])) if l2cat is not None else (None, 0.0)
    out = torch.empty((B, N, C + (3 if pf is not None else 0)), dtype=torch.float32, device=cw.device)
    ep = L.make_epilogue(pre_bias, scale, shift, act)
    L.check(L.lib().dh3d_interp_combine_fwd(L.ptr(cw), L.ptr(ix), L.ptr(d), L.ptr(partial), B, N, M, C, ep,
                                            L.ptr(residual), L.ptr(pf), eps, L.ptr(out), L.stream_ptr()),
            "interp_combine")
    return out


def local_tail_fused(x1, x2, wp3_shortcut, wp3_lower, ep_shortcut, ep_concat, coarse_w, idx, dist, prefix, l2_eps):
    """[prefix | l2_normalize(relu(BN_c(interp3(coarse_w) + x2 W_lower + b_c)) + relu(BN_s(x1 W_s + b_s)))] [B,N,131] in one
    launch (csrc/dense_tail.hip): interp_combine with the lower-block and shortcut GEMMs done on the fly.
    ep_* = (bias, scale, shift) tuples (activation ReLU)."""
    a = L.require_cuda_f32(x1, "x1", 3)
    b = L.require_cuda_f32(x2, "x2", 3)
    cw = L.require_cuda_f32(coarse_w, "coarse_w", 3)
    ix = L.require_cuda_i32(idx, "idx", 3)
    d = L.require_cuda_f32(dist, "dist", 3)
    pf = L.require_cuda_f32(prefix, "prefix", 3) if prefix is not None else None   # None: the plain [B,N,128] sum
    B, N, C = a.shape
    if C != 64 or b.shape != a.shape or cw.shape[2] != 128 or N % 32:
        raise ValueError("local_tail_fused: x1 / x2 [B,N,64], coarse_w [B,M,128], N % 32 == 0")
    out = torch.empty((B, N, 131 if pf is not None else 128), dtype=torch.float32, device=a.device)
    e1, e2 = L.make_epilogue(*ep_shortcut, ACT_RELU), L.make_epilogue(*ep_concat, ACT_RELU)
    L.check(L.lib().dh3d_local_tail_fused_fwd(L.ptr(a), L.ptr(b), L.ptr(wp3_shortcut), L.ptr(wp3_lower), e1, e2, L.ptr(cw),
                                              L.ptr(ix), L.ptr(d), L.ptr(pf), float(l2_eps), B, N, cw.shape[1], L.ptr(out),
                                              L.stream_ptr()), "local_tail_fused")
    return out


def pack_weight_x3(W):
    """W [Kd, Dout] f32 -> three exact bf16 chunk planes in MFMA fragment order (csrc/dense_x6.hip)."""
    W = L.require_cuda_f32(W, "W", 2)
    out = torch.empty((3 * W.shape[0] * W.shape[1],), dtype=torch.int16, device=W.device)
    L.check(L.lib().dh3d_pack_weight_x3(L.ptr(W), W.shape[0], W.shape[1], L.ptr(out), L.stream_ptr()),
            "pack_weight_x3")
    return out


def mlp_head_x6(h, wpacked_x3, H, w_fc, b_fc, pre_bias=None, scale=None, shift=None, act=ACT_RELU):
    """mlp_head with the 256 -> 1024 GEMM on the bf16 pipe at f32 accuracy (six exact-chunk products)."""
    a = L.require_cuda_f32(h, "h")
    C = a.shape[-1]
    R = a.numel() // C
    out = torch.empty(a.shape[:-1] + (1,), dtype=torch.float32, device=a.device)
    ep = L.make_epilogue(pre_bias, scale, shift, act)
    L.check(L.lib().dh3d_mlp_head_pm_x6_fwd(L.ptr(a), R, C, L.ptr(wpacked_x3), H, ep, L.ptr(w_fc), float(b_fc),
                                            L.ptr(out), L.stream_ptr()), "mlp_head_pm_x6")
    return out


def interp_head(coarse, idx, dist, wslices_x3, Hd, w_fc, b_fc, pre_bias=None, scale=None, shift=None, act=ACT_RELU,
                order=None):
    """mlp_head_x6(three_interpolate_idw(coarse, idx, dist), ...) with the wide conv commuted through the interpolation:
    the [C, Hd] GEMM runs on the coarse rows (its 256-column slices in one launch, `wslices_x3` = their packed images
    back to back), a gather kernel
    interpolates the Hd-wide rows and finishes bias + BN + act + w_fc + sigmoid.  coarse [B,m,C], idx/dist [B,n,3].
    order: spatial_sort records [B,n,4] of the fine cloud -> the LDS-staged kernel (m <= 1024)."""
    x = L.require_cuda_f32(coarse, "coarse", 3)
    ix = L.require_cuda_i32(idx, "idx", 3)
    d = L.require_cuda_f32(dist, "dist", 3)
    B, m, C = x.shape
    n = ix.shape[1]
    ns = Hd // 256
    H = torch.empty((ns, B * m, 256), dtype=torch.float32, device=x.device)
    L.check(L.lib().dh3d_linear_slices_pm_x6_fwd(L.ptr(x), C, L.ptr(wslices_x3), B * m, ns, L.ptr(H), L.stream_ptr()),
            "linear_slices_pm_x6")
    out = torch.empty((B, n, 1), dtype=torch.float32, device=x.device)
    ep = L.make_epilogue(pre_bias, scale, shift, act)
    if order is not None and m <= 1024:
        # fine points in Morton order (`order` = spatial_sort records of the fine cloud), coarse rows staged in LDS
        L.check(L.lib().dh3d_interp_head_sorted_fwd(L.ptr(H), Hd, L.ptr(ix), L.ptr(d), L.ptr(order), B, n, m, ep,
                                                    L.ptr(w_fc), float(b_fc), L.ptr(out), L.stream_ptr()),
                "interp_head_sorted")
        return out
    L.check(L.lib().dh3d_interp_head_fwd(L.ptr(H), Hd, L.ptr(ix), L.ptr(d), B, n, m, ep, L.ptr(w_fc), float(b_fc),
                                         L.ptr(out), L.stream_ptr()), "interp_head")
    return out


def netvlad_aggregate(x, att, wc_packed, bn_scale, bn_shift, W2):
    a = L.require_cuda_f32(x, "x", 3)
    B, N, D = a.shape
    Cl = W2.shape[-1]
    t = L.require_cuda_f32(att, "att").reshape(B, N)
    ws_bytes = L.lib().dh3d_netvlad_workspace_bytes(B, N, D, Cl)
    if ws_bytes == 0:
        raise ValueError("netvlad_aggregate: unsupported shape D=%d Cl=%d" % (D, Cl))
    ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=a.device)
    vlad = torch.empty((B, D * Cl), dtype=torch.float32, device=a.device)
    L.check(L.lib().dh3d_netvlad_aggregate_fwd(L.ptr(a), L.ptr(t), L.ptr(wc_packed), L.ptr(bn_scale),
                                               L.ptr(bn_shift), L.ptr(W2), B, N, D, Cl, L.ptr(ws), ws_bytes,
                                               L.ptr(vlad), L.stream_ptr()), "netvlad_aggregate")
    return vlad


def netvlad_fused(x, att, wc_packed, bn_scale, bn_shift, W2, Wh, bn1_scale, bn1_shift, Wg, bn2_scale, bn2_shift,
                  l2_eps=0.0):
    """netvlad_head(netvlad_aggregate(...), ...) in one C call, without the separate whole-vector normalisation kernel."""
    xx = L.require_cuda_f32(x, "x", 3)
    B, N, D = xx.shape
    Cl, O = W2.shape[1], Wh.shape[1]
    a = L.require_cuda_f32(att, "att").reshape(B, N).contiguous()
    ws_bytes = L.lib().dh3d_netvlad_fused_workspace_bytes(B, N, D, Cl, O)
    if ws_bytes == 0:
        raise ValueError("netvlad_fused: unsupported shape D=%d Cl=%d O=%d" % (D, Cl, O))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=xx.device)
    out = torch.empty((B, O), dtype=torch.float32, device=xx.device)
    L.check(L.lib().dh3d_netvlad_fused_fwd(L.ptr(xx), L.ptr(a), L.ptr(wc_packed), L.ptr(bn_scale), L.ptr(bn_shift),
                                           L.ptr(W2), L.ptr(Wh), L.ptr(bn1_scale), L.ptr(bn1_shift), L.ptr(Wg),
                                           L.ptr(bn2_scale), L.ptr(bn2_shift), B, N, D, Cl, O, float(l2_eps), L.ptr(ws),
                                           ws_bytes, L.ptr(out), L.stream_ptr()), "netvlad_fused")
    return out


def walk_plan(idx, dist, order, m):
    """The slot tables of pm.global_tail's walk, built ahead of it (csrc/dense_x6.hip walk_plan_kernel): idx / dist [B,n,3]
    from three_nn against m <= 1024 sampled points, order = spatial_sort records [B,n,4] of the fine cloud (or None).
    Returns an opaque int32 tensor, valid for exactly these inputs."""
    ix = L.require_cuda_i32(idx, "idx", 3)
    d = L.require_cuda_f32(dist, "dist", 3)
    B, n, _ = ix.shape
    nbytes = L.lib().dh3d_walk_plan_bytes(B, n)
    plan = torch.empty((nbytes // 4,), dtype=torch.int32, device=ix.device)
    L.check(L.lib().dh3d_walk_plan(L.ptr(ix), L.ptr(d), L.ptr(order), B, n, int(m), L.ptr(plan), L.stream_ptr()), "walk_plan")
    return plan


def global_tail_accum_size(B, m):
    """floats of global_tail's accumulator block [ A' B*m*64 | asum B*64 ]."""
    return B * m * 64 + B * 64


def global_tail(coarse, idx, dist, order, wslices_x3, Hd, w_fc, b_fc, att_ep, wc_packed, cl_scale, cl_shift, W2, Wh,
                bn1_scale, bn1_shift, Wg, bn2_scale, bn2_shift, l2_eps=0.0, want_att=False, accum=None, cw=None, plan=None):
    """three_interpolate -> attention head -> NetVLAD + gating, with the up-sampling commuted through both consumers: the
    fine points are walked once (csrc/dense_x6.hip VladTail), everything else runs on the coarse rows.
    coarse [B,m,256], idx/dist [B,n,3], order = spatial_sort records [B,n,4] of the fine cloud, att_ep =
    (pre_bias, scale, shift, act) of the attention's hidden layer.  accum (optional): a ZEROED float32 tensor of
    global_tail_accum_size(B, m) elements (the caller's fill, issued off the critical chain); cw (optional):
    coarse @ cluster_weights if the caller has it already; plan (optional): walk_plan(idx, dist, order, m) of exactly these
    inputs, built off the critical chain.  Returns the descriptor [B,O] (, att [B,n,1])."""
    x = L.require_cuda_f32(coarse, "coarse", 3)
    ix = L.require_cuda_i32(idx, "idx", 3)
    d = L.require_cuda_f32(dist, "dist", 3)
    B, m, C = x.shape
    n = ix.shape[1]
    ns = Hd // 256
    H = torch.empty((ns, B * m, 256), dtype=torch.float32, device=x.device)
    L.check(L.lib().dh3d_linear_slices_pm_x6_fwd(L.ptr(x), C, L.ptr(wslices_x3), B * m, ns, L.ptr(H), L.stream_ptr()),
            "linear_slices_pm_x6")
    if cw is None:   # (the caller may have it already: pm.flex_conv_tile_x6 computes it in the flex_conv's launch)
        cw = linear(x, wc_packed, 64)                                              # coarse @ cluster_weights
    att = torch.empty((B, n, 1), dtype=torch.float32, device=x.device) if want_att else None
    zero_here = accum is None
    if accum is None:
        accum = torch.empty((global_tail_accum_size(B, m),), dtype=torch.float32, device=x.device)
    elif accum.numel() != global_tail_accum_size(B, m) or accum.dtype != torch.float32 or not accum.is_cuda:
        raise ValueError("global_tail: accum must be a zeroed float32 GPU tensor of global_tail_accum_size(B, m) elements")
    ep = L.make_epilogue(*att_ep)
    if plan is not None and (plan.dtype != torch.int32 or plan.numel() * 4 != L.lib().dh3d_walk_plan_bytes(B, n)):
        raise ValueError("global_tail: plan is not walk_plan(idx, dist, order, m) of these shapes")
    L.check(L.lib().dh3d_global_walk_planned_fwd(L.ptr(H), Hd, L.ptr(x), L.ptr(cw), L.ptr(ix), L.ptr(d), L.ptr(order), L.ptr(plan),
                                                 B, n, m, ep, L.ptr(w_fc), float(b_fc), L.ptr(cl_scale), L.ptr(cl_shift),
                                                 L.ptr(att), L.ptr(accum), 1 if zero_here else 0, L.stream_ptr()), "global_walk")
    apart, asum = accum[:B * m * 64], accum[B * m * 64:]
    O = Wh.shape[1]
    ws_bytes = L.lib().dh3d_netvlad_tail_workspace_bytes(B, C, 64, O)
    if ws_bytes == 0:
        raise ValueError("global_tail: unsupported NetVLAD shape")
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=x.device)
    out = torch.empty((B, O), dtype=torch.float32, device=x.device)
    # V = A'^T coarse is formed inside the finalize kernel (no batched GEMM launch)
    L.check(L.lib().dh3d_netvlad_tail_assign_fwd(L.ptr(apart), L.ptr(x), L.ptr(asum), m, L.ptr(W2), L.ptr(Wh), L.ptr(bn1_scale),
                                                 L.ptr(bn1_shift), L.ptr(Wg), L.ptr(bn2_scale), L.ptr(bn2_shift), B, C, 64, O,
                                                 float(l2_eps), L.ptr(ws), ws_bytes, L.ptr(out), L.stream_ptr()),
            "netvlad_tail_assign")
    return (out, att) if want_att else out


def netvlad_head(vlad, Wh, bn1_scale, bn1_shift, Wg, bn2_scale, bn2_shift, l2_eps=0.0):
    v = L.require_cuda_f32(vlad, "vlad", 2)
    B, Kd = v.shape
    O = Wh.shape[1]
    if Kd % 8 != 0:
        raise ValueError("netvlad_head: unsupported shape Kd=%d (vlad's width must be a multiple of 8)" % Kd)
    ws_bytes = L.lib().dh3d_netvlad_head_workspace_bytes(B, Kd, O)
    if ws_bytes == 0:
        raise ValueError("netvlad_head: unsupported output dim %d" % O)
    ws = torch.empty((ws_bytes // 4,), dtype=torch.float32, device=v.device)
    out = torch.empty((B, O), dtype=torch.float32, device=v.device)
    L.check(L.lib().dh3d_netvlad_head_fwd(L.ptr(v), L.ptr(Wh), L.ptr(bn1_scale), L.ptr(bn1_shift), L.ptr(Wg),
                                          L.ptr(bn2_scale), L.ptr(bn2_shift), B, Kd, O, float(l2_eps), L.ptr(ws),
                                          ws_bytes, L.ptr(out), L.stream_ptr()), "netvlad_head")
    return out


# --------------------------------------------------------------------------------------------- backward / training
def flex_conv_bwd(features, xyz, nbr, theta, bias, grad_out, center_rank0=False, need_grad_features=True):
    """Factorised flex_conv backward (csrc/flex_bwd.hip): features [B,N,Din], xyz [B,N,3], nbr [B,N,K] int32,
    theta [3,Din,Dout], bias [Din,Dout], grad_out [B,N,Dout] -> (grad_features [B,N,Din] or None, grad_theta, grad_bias)."""
    f = L.require_cuda_f32(features, "features", 3)
    x = L.require_cuda_f32(xyz, "xyz", 3)
    nb = L.require_cuda_i32(nbr, "nbr", 3)
    t = L.require_cuda_f32(theta, "theta", 3)
    bi = L.require_cuda_f32(bias, "bias", 2)
    g = L.require_cuda_f32(grad_out, "grad_out", 3)
    B, N, Din = f.shape
    K, Dout = nb.shape[2], t.shape[2]
    if t.shape[0] != 3 or tuple(bi.shape) != (Din, Dout) or tuple(g.shape) != (B, N, Dout):
        raise ValueError("flex_conv_bwd: inconsistent shapes")
    ws_bytes = L.lib().dh3d_flex_conv_pm_bwd_workspace_bytes(B, N, Din, Dout)
    if ws_bytes == 0:
        raise ValueError("flex_conv_bwd: Din and Dout must be multiples of 4")
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=f.device)
    gf = torch.empty_like(f) if need_grad_features else None
    gt, gb = torch.empty_like(t), torch.empty_like(bi)
    L.check(L.lib().dh3d_flex_conv_pm_bwd(L.ptr(f), L.ptr(x), L.ptr(nb), L.ptr(t), L.ptr(bi), L.ptr(g), B, N, K, Din,
                                          Dout, 1 if center_rank0 else 0, L.ptr(ws), ws_bytes, L.ptr(gf), L.ptr(gt),
                                          L.ptr(gb), L.stream_ptr()), "flex_conv_pm_bwd")
    return gf, gt, gb


GEMM_KERNELS = {1: "rows1", 2: "rows2", 3: "rows3", 4: "rows4", 5: "shortk", 6: "f32_narrow", 7: "f32_wide",
                8: "x6_narrow", 9: "x6_wide"}   # include/dh3d_hip.h DH3D_GEMM_*


def gemm_plan(ta, M, N, K, batch=1, bias=False):
    """The kernel of csrc/gemm.hip that gemm_tn (ta) / gemm_nn and their batched forms take for a shape, and its cut of the
    reduction (host only): (kernel name, chunks, kchunk, stage) -- dh3d_gemm_plan.  None where they refuse the shape."""
    c, kc, st = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    r = L.lib().dh3d_gemm_plan(1 if ta else 0, int(M), int(N), int(K), int(batch), 1 if bias else 0, ctypes.byref(c),
                               ctypes.byref(kc), ctypes.byref(st))
    return None if r == 0 else (GEMM_KERNELS[r], c.value, kc.value, st.value)


def gemm_tn(A, B, out=None, accumulate=False):
    """C[M,N] (+)= A[K,M]^T @ B[K,N], f32-accurate (exact-f32 MFMA for small products, bf16x6 with both operands split on
    the fly from 2^26 multiply-adds; csrc/gemm.hip) -- weight gradients: the reduction runs over rows."""
    A = L.require_cuda_f32(A, "A", 2)
    B = L.require_cuda_f32(B, "B", 2)
    K, M = A.shape
    if B.shape[0] != K:
        raise ValueError("gemm_tn: row counts differ")
    N = B.shape[1]
    if out is None and _ZERO_ARENA[0] is not None and L.lib().dh3d_gemm_is_split(1, M, N, K, 1):
        out, accumulate = zeros((M, N), torch.float32, A.device), True   # split reduction: the arena's zeros, no fill
    C = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=A.device)
    L.check(L.lib().dh3d_gemm_tn_f32(L.ptr(A), L.ptr(B), K, M, N, 1 if accumulate else 0, L.ptr(C), L.stream_ptr()),
            "gemm_tn")
    return C


def gemm_nn(A, B, out=None, accumulate=False, bias=None):
    """C[M,N] (+)= A[M,K] @ B[K,N] (+ bias[N]), f32-accurate (see gemm_tn)."""
    A = L.require_cuda_f32(A, "A", 2)
    B = L.require_cuda_f32(B, "B", 2)
    M, K = A.shape
    if B.shape[0] != K:
        raise ValueError("gemm_nn: inner dimensions differ")
    N = B.shape[1]
    if out is None and bias is None and _ZERO_ARENA[0] is not None and L.lib().dh3d_gemm_is_split(0, M, N, K, 1):
        out, accumulate = zeros((M, N), torch.float32, A.device), True
    C = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=A.device)
    L.check(L.lib().dh3d_gemm_nn_f32(L.ptr(A), L.ptr(B), L.ptr(bias), M, K, N, 1 if accumulate else 0, L.ptr(C),
                                     L.stream_ptr()), "gemm_nn")
    return C


def stage_copy(src, dst):
    """dst <- src on the current stream by a kernel (dh3d_stage_copy): each side a contiguous CUDA tensor or a contiguous
    PINNED CPU tensor (device-addressable), same byte count.  The serving loop's host <-> slot-buffer hand-over
    (engine.Pipeline.submit): no copy engine, no engine-to-engine dependency on the step's chain."""
    for t, nm in ((src, "src"), (dst, "dst")):
        if not (t.is_cuda or t.is_pinned()):
            raise ValueError("stage_copy: %s must be a CUDA tensor or a pinned CPU tensor" % nm)
        if not t.is_contiguous():
            raise ValueError("stage_copy: %s must be contiguous" % nm)
    nbytes = src.numel() * src.element_size()
    if nbytes != dst.numel() * dst.element_size():
        raise ValueError("stage_copy: %d bytes into %d" % (nbytes, dst.numel() * dst.element_size()))
    L.check(L.lib().dh3d_stage_copy(src.data_ptr(), dst.data_ptr(), nbytes, int(src.is_cuda and dst.is_cuda),
                                    L.stream_ptr()), "stage_copy")
    return dst


def transpose_last2(x):
    """[..., R, C] -> [..., C, R] (32-bit elements) through LDS tiles."""
    if not x.is_cuda or x.element_size() != 4:
        raise ValueError("transpose_last2: 32-bit GPU tensors only")
    x = x.contiguous()
    R, C = x.shape[-2], x.shape[-1]
    Bt = x.numel() // (R * C)
    out = torch.empty(tuple(x.shape[:-2]) + (C, R), dtype=x.dtype, device=x.device)
    L.check(L.lib().dh3d_transpose32(L.ptr(x), Bt, R, C, L.ptr(out), L.stream_ptr()), "transpose32")
    return out


def colsum(x, out=None, accumulate=False):
    """x [R, C] -> [C] column sums (bias gradients)."""
    x = L.require_cuda_f32(x, "x", 2)
    R, C = x.shape
    o = out if out is not None else torch.empty((C,), dtype=torch.float32, device=x.device)
    L.check(L.lib().dh3d_colsum_f32(L.ptr(x), R, C, 1 if accumulate else 0, L.ptr(o), L.stream_ptr()), "colsum")
    return o


def _mask_u8(mask):
    return None if mask is None else mask.to(torch.uint8).contiguous()


_ITEMSIZE = {torch.float32: 4, torch.float64: 8, torch.int32: 4, torch.int64: 8, torch.uint8: 1}


class ZeroArena(object):
    """One zeroed device buffer per training step for the accumulators its kernels add into (statistics partials, scatter
    targets: include/dh3d_hip.h "zeroed by the CALLER").  `begin()` clears it with ONE fill and rewinds; `zeros()` below
    hands out views while the arena is active (`with pm.zero_arena(a): ...`) and falls back to torch.zeros otherwise or
    when the arena is too small -- the demand of a step is recorded, the next `begin()` outside a graph capture grows
    the buffer to it.  Views are only valid until the next `begin()`.  Two kinds of tensors that leave a step DO come
    from here and inherit that lifetime: the loss never does, but the parameter gradients of split-reduction GEMMs
    (`gemm_tn` / `gemm_nn` below: dW of the attention head and of NetVLAD's assignment) are arena views -- `p.grad` is
    valid until the next step begins, which is what an optimiser step needs; code that keeps gradients across steps
    (gradient accumulation, inspection) must clone them (QuadrupletTrainer.keep_grads does).

    A buffer is never freed or replaced while a captured hipGraph may still replay into it: an arena built with
    `fixed_bytes` (one per captured step graph, owned by that graph's entry) never reallocates -- `take()` falls back
    to torch.zeros (inside a capture: the graph's own pool) when it is too small; only the growing arena of the eager
    steps reallocates, and no graph records its address."""

    def __init__(self, fixed_bytes=None, device=None):
        self.buf, self.off, self.demand, self.peak = None, 0, 0, 0
        self.fixed = fixed_bytes is not None
        if self.fixed and fixed_bytes > 0:
            self.buf = torch.empty((int(fixed_bytes),), dtype=torch.uint8, device=device)

    def begin(self, device):
        self.peak = max(self.peak, self.demand)
        capturing = torch.cuda.is_current_stream_capturing() if torch.cuda.is_available() else False
        if (not self.fixed and self.peak and not capturing
                and (self.buf is None or self.buf.numel() < self.peak or self.buf.device != device)):
            self.buf = torch.empty((self.peak,), dtype=torch.uint8, device=device)
        if self.buf is not None:
            self.buf.zero_()
        self.off, self.demand = 0, 0

    def take(self, shape, dtype, device):
        n = 1
        for d in shape:
            n *= int(d)
        nbytes = n * _ITEMSIZE[dtype]
        span = (nbytes + 255) // 256 * 256
        self.demand += span
        if self.buf is None or self.buf.device != device or self.off + span > self.buf.numel():
            return torch.zeros(shape, dtype=dtype, device=device)
        # a tensor of its own on the arena's storage (NOT a view of `buf`: autograd would tie every accumulator that
        # leaves a custom Function to the arena's version counter, which the next begin() bumps)
        esz = nbytes // max(n, 1) if n else 1
        v = torch.empty((0,), dtype=dtype, device=device).set_(self.buf.untyped_storage(), self.off // esz, tuple(shape))
        self.off += span
        return v


_ZERO_ARENA = [None]


class zero_arena(object):
    """Context: accumulators come out of `arena` (a ZeroArena, already begun) instead of one torch.zeros each."""

    def __init__(self, arena):
        self.arena, self.prev = arena, None

    def __enter__(self):
        self.prev, _ZERO_ARENA[0] = _ZERO_ARENA[0], self.arena
        return self.arena

    def __exit__(self, *exc):
        _ZERO_ARENA[0] = self.prev
        return False


def zeros(shape, dtype, device):
    """A zeroed accumulator: a view of the active ZeroArena, or torch.zeros."""
    a = _ZERO_ARENA[0]
    return a.take(tuple(shape), dtype, device) if a is not None else torch.zeros(tuple(shape), dtype=dtype, device=device)


def bn_colstats(x, mask=None, rows_per_cloud=0, out=None):
    """x [R,C] -> (sum [C], sumsq [C]) float64 (views of `out` [>= 2C] if given); mask [clouds] bool excludes padding
    clouds of rows_per_cloud rows."""
    x = L.require_cuda_f32(x, "x", 2)
    R, C = x.shape
    buf = out if out is not None else zeros((2 * C,), torch.float64, x.device)   # `out` must be zeroed by the caller
    s1, s2 = buf[:C], buf[C:2 * C]
    m = _mask_u8(mask)
    L.check(L.lib().dh3d_bn_colstats(L.ptr(x), R, C, L.ptr(m), int(rows_per_cloud), L.ptr(s1), L.ptr(s2),
                                     L.stream_ptr()), "bn_colstats")
    return s1, s2


def bn_finalize(s1, s2, cnt, gamma, beta, eps, momentum, run_mean, run_var, unbiased=True):
    """(sum, sumsq, count) -> [mean, rstd, scale, shift] as rows of one [4, C] float32 tensor; running buffers updated
    (unbiased: the moving variance takes the Bessel-corrected batch variance, as tf.nn.fused_batch_norm feeds it)."""
    C = gamma.numel()
    o = torch.empty((4, C), dtype=torch.float32, device=gamma.device)
    L.check(L.lib().dh3d_bn_finalize(L.ptr(s1), L.ptr(s2), L.ptr(cnt), L.ptr(gamma), L.ptr(beta), float(eps),
                                     float(momentum), 1 if unbiased else 0, L.ptr(run_mean), L.ptr(run_var), C, L.ptr(o[0]), L.ptr(o[1]),
                                     L.ptr(o[2]), L.ptr(o[3]), L.stream_ptr()), "bn_finalize")
    return o


def bn_bwd_finalize(S1, S2, cnt, mean, rstd, gamma):
    """-> [k2, k3] rows of a [2, C] tensor (coefficients of bn_bwd_apply)."""
    C = gamma.numel()
    o = torch.empty((2, C), dtype=torch.float32, device=gamma.device)
    L.check(L.lib().dh3d_bn_bwd_finalize(L.ptr(S1), L.ptr(S2), L.ptr(cnt), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), C,
                                         L.ptr(o[0]), L.ptr(o[1]), L.stream_ptr()), "bn_bwd_finalize")
    return o


def bn_finalize_parts(part, cnt, gamma, beta, eps, momentum, run_mean, run_var, unbiased=True):
    """bn_finalize from per-cloud partial rows part [2, P, C] float64 (sum | sumsq), the reduction over P included."""
    _, P, C = part.shape
    o = torch.empty((4, C), dtype=torch.float32, device=gamma.device)
    L.check(L.lib().dh3d_bn_finalize_parts(L.ptr(part), P, L.ptr(cnt), L.ptr(gamma), L.ptr(beta), float(eps),
                                           float(momentum), 1 if unbiased else 0, L.ptr(run_mean), L.ptr(run_var), C,
                                           L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), L.ptr(o[3]), L.stream_ptr()),
            "bn_finalize_parts")
    return o


def bn_bwd_finalize_parts(part, cnt, mean, rstd, gamma):
    """part [nk, P, C] float64 per-cloud partial sums (nk = 2 or 3) -> ([k2, k3] rows of a [2, C] tensor, grads [nk, C]
    float32 = their sums over P: dbeta, dgamma(, d w_fc)) in one launch."""
    nk, P, C = part.shape
    o = torch.empty((2, C), dtype=torch.float32, device=part.device)
    grads = torch.empty((nk, C), dtype=torch.float32, device=part.device)
    L.check(L.lib().dh3d_bn_bwd_finalize_parts(L.ptr(part), nk, P, L.ptr(cnt), L.ptr(mean), L.ptr(rstd), L.ptr(gamma), C,
                                               L.ptr(o[0]), L.ptr(o[1]), L.ptr(grads), L.stream_ptr()),
            "bn_bwd_finalize_parts")
    return o, grads


def sigmoid_bwd(datt, att, mask=None, rows_per_cloud=0):
    """-> (dlogit = datt*att*(1-att), 0 on the rows of masked clouds; its sum as a [1] tensor)."""
    datt, att = datt.contiguous(), att.contiguous()
    dlogit = torch.empty_like(att)
    tot = torch.zeros((1,), dtype=torch.float32, device=att.device)   # (a parameter gradient: not from the step arena)
    L.check(L.lib().dh3d_sigmoid_bwd(L.ptr(datt), L.ptr(att), L.ptr(_mask_u8(mask)), int(rows_per_cloud), att.numel(),
                                     L.ptr(dlogit), L.ptr(tot), L.stream_ptr()), "sigmoid_bwd")
    return dlogit, tot


def scale_shift_act(x, scale, shift, relu, out=None, residual=None):
    """y = act(x * scale[c] + shift[c]) (+ residual, added after the activation)."""
    x = L.require_cuda_f32(x, "x", 2)
    R, C = x.shape
    y = out if out is not None else torch.empty_like(x)
    if residual is not None:
        r = L.require_cuda_f32(residual, "residual", 2)
        if r.shape != x.shape:
            raise ValueError("scale_shift_act: residual shape differs")
        L.check(L.lib().dh3d_scale_shift_act_res(L.ptr(x), R, C, L.ptr(scale), L.ptr(shift), 1 if relu else 0, L.ptr(r),
                                                 L.ptr(y), L.stream_ptr()), "scale_shift_act_res")
        return y
    L.check(L.lib().dh3d_scale_shift_act(L.ptr(x), R, C, L.ptr(scale), L.ptr(shift), 1 if relu else 0, L.ptr(y),
                                         L.stream_ptr()), "scale_shift_act")
    return y


def row_logit_sigmoid(h, scale, shift, w, b):
    """att[r] = sigmoid(sum_c relu(h*scale+shift)[r,c]*w[c] + b); b: device tensor holding the scalar."""
    h = L.require_cuda_f32(h, "h", 2)
    R, C = h.shape
    att = torch.empty((R,), dtype=torch.float32, device=h.device)
    L.check(L.lib().dh3d_row_logit_sigmoid(L.ptr(h), R, C, L.ptr(scale), L.ptr(shift), L.ptr(w), L.ptr(b), L.ptr(att),
                                           L.stream_ptr()), "row_logit_sigmoid")
    return att


def bn_bwd_sums(x, mean, rstd, gamma, beta, relu, dy=None, rowscale=None, colvec=None, mask=None, rows_per_cloud=0):
    """-> S [3, C] float64: S[0] = sum dz, S[1] = sum dz*xhat, S[2] = sum rowscale*y (rank-one form only; else unused)."""
    x = L.require_cuda_f32(x, "x", 2)
    R, C = x.shape
    S = zeros((3, C), torch.float64, x.device)
    m = _mask_u8(mask)
    L.check(L.lib().dh3d_bn_bwd_sums(L.ptr(x), L.ptr(dy), L.ptr(rowscale), L.ptr(colvec), R, C, L.ptr(mean), L.ptr(rstd),
                                     L.ptr(gamma), L.ptr(beta), 1 if relu else 0, L.ptr(m), int(rows_per_cloud),
                                     L.ptr(S[0]), L.ptr(S[1]), L.ptr(S[2]), L.stream_ptr()), "bn_bwd_sums")
    return S


def bn_bwd_apply(x, scale, shift, k2, k3, relu, dy=None, rowscale=None, colvec=None, mask=None, rows_per_cloud=0,
                 out=None):
    """dx = scale*dz - k2 - k3*x (see include/dh3d_hip.h); out may be x (in place)."""
    x = L.require_cuda_f32(x, "x", 2)
    R, C = x.shape
    dx = out if out is not None else torch.empty_like(x)
    m = _mask_u8(mask)
    L.check(L.lib().dh3d_bn_bwd_apply(L.ptr(x), L.ptr(dy), L.ptr(rowscale), L.ptr(colvec), R, C, L.ptr(scale),
                                      L.ptr(shift), L.ptr(k2), L.ptr(k3), 1 if relu else 0, L.ptr(m),
                                      int(rows_per_cloud), L.ptr(dx), L.stream_ptr()), "bn_bwd_apply")
    return dx


# ---- attention head, training mode, conv commuted through the up-sampling (csrc/interp_train.hip)
def _g_layout(G, idx):
    """G: [ns, B*m, 256] slices or [B*m, Hd] row-major -> (Hd, row_major flag, m)."""
    B = idx.shape[0]
    if G.dim() == 3:
        return G.shape[0] * 256, 0, G.shape[1] // B
    return G.shape[1], 1, G.shape[0] // B


def interp_bn_colstats(G, idx, dist, order, mask=None, out=None, parts=False):
    """G = coarse @ W + b as [ns, B*m, 256] slices or as [B*m, Hd]; idx/dist [B,n,3]; order = spatial_sort records
    [B,n,4] or None -> (sum, sumsq) [Hd] float64 of the virtual rows three_interpolate(G) (views of `out` if given)."""
    Hd, rm, m = _g_layout(G, idx)
    B, n = idx.shape[0], idx.shape[1]
    part = zeros((2, B, Hd), torch.float64, G.device)
    L.check(L.lib().dh3d_interp_bn_colstats(L.ptr(G), Hd, rm, L.ptr(idx), L.ptr(dist), L.ptr(order), B, n, m,
                                            L.ptr(_mask_u8(mask)), L.ptr(part), L.stream_ptr()), "interp_bn_colstats")
    if parts:
        return part
    buf = out if out is not None else torch.empty((2 * Hd,), dtype=torch.float64, device=G.device)
    torch.sum(part, dim=1, out=buf[:2 * Hd].view(2, Hd))
    return buf[:Hd], buf[Hd:2 * Hd]


def interp_head_rows(G, idx, dist, order, scale, shift, w_fc, b_fc_dev):
    """att [B*n] = sigmoid(relu(three_interpolate(G) * scale + shift) . w_fc + b_fc), b_fc a device scalar."""
    Hd, rm, m = _g_layout(G, idx)
    B, n = idx.shape[0], idx.shape[1]
    out = torch.empty((B * n,), dtype=torch.float32, device=G.device)
    ep = L.make_epilogue(None, scale, shift, ACT_RELU)
    L.check(L.lib().dh3d_interp_head_sorted_fwd_dev(L.ptr(G), Hd, rm, L.ptr(idx), L.ptr(dist), L.ptr(order), B, n, m, ep,
                                                    L.ptr(w_fc), L.ptr(b_fc_dev), L.ptr(out), L.stream_ptr()),
            "interp_head_sorted_dev")
    return out


def interp_bn_bwd_sums(G, idx, dist, order, dlogit, w_fc, mean, rstd, gamma, beta, mask=None, parts=False):
    """-> S [3, Hd] float64 (parts: the per-cloud partials [3, B, Hd] for bn_bwd_finalize_parts)."""
    Hd, rm, m = _g_layout(G, idx)
    B, n = idx.shape[0], idx.shape[1]
    part = zeros((3, B, Hd), torch.float64, G.device)
    L.check(L.lib().dh3d_interp_bn_bwd_sums(L.ptr(G), Hd, rm, L.ptr(idx), L.ptr(dist), L.ptr(order), B, n, m,
                                            L.ptr(_mask_u8(mask)), L.ptr(dlogit), L.ptr(w_fc), L.ptr(mean), L.ptr(rstd),
                                            L.ptr(gamma), L.ptr(beta), L.ptr(part), L.stream_ptr()), "interp_bn_bwd_sums")
    return part if parts else part.sum(1)


def interp_bn_bwd_apply(G, idx, dist, order, dlogit, w_fc, scale, shift, k2, k3, mask=None):
    """-> dG (the layout of G) = interp^T(scale*dz - k2 - k3*h)."""
    Hd, rm, m = _g_layout(G, idx)
    B, n = idx.shape[0], idx.shape[1]
    dG = zeros(G.shape, torch.float32, G.device)
    L.check(L.lib().dh3d_interp_bn_bwd_apply(L.ptr(G), Hd, rm, L.ptr(idx), L.ptr(dist), L.ptr(order), B, n, m,
                                             L.ptr(_mask_u8(mask)), L.ptr(dlogit), L.ptr(w_fc), L.ptr(scale),
                                             L.ptr(shift), L.ptr(k2), L.ptr(k3), L.ptr(dG), L.stream_ptr()),
            "interp_bn_bwd_apply")
    return dG


# ---- NetVLAD's assignment, training mode, rows commuted through the up-sampling (csrc/netvlad_train.hip)
def nv_commuted_fwd_stats(c, cw, idx, dist, order, mask=None, out=None, parts=False):
    """c [B*m,256], cw = c @ Wc [B*m,64] -> s [B*n,64], rinv [B*n] (by original point index) and (sum, sumsq) [64]
    float64 of the columns of s (views of `out` if given)."""
    B, n = idx.shape[0], idx.shape[1]
    m = c.shape[0] // B
    s = torch.empty((B * n, 64), dtype=torch.float32, device=c.device)
    rinv = torch.empty((B * n,), dtype=torch.float32, device=c.device)
    part = zeros((2, B, 64), torch.float64, c.device)
    L.check(L.lib().dh3d_netvlad_commuted_fwd_stats(L.ptr(c), L.ptr(cw), L.ptr(idx), L.ptr(dist), L.ptr(order), B, n, m,
                                                    L.ptr(_mask_u8(mask)), L.ptr(s), L.ptr(rinv), L.ptr(part),
                                                    L.stream_ptr()), "netvlad_commuted_fwd_stats")
    if parts:
        return s, rinv, part
    buf = out if out is not None else torch.empty((128,), dtype=torch.float64, device=c.device)
    torch.sum(part, dim=1, out=buf[:128].view(2, 64))
    return s, rinv, buf[:64], buf[64:128]


def nv_commuted_fwd_assign(s, rinv, att, scale, shift, idx, dist, order, m, mask=None):
    """-> p [B*n,64] = softmax(s*scale + shift), asum [B,64] = sum_n p*att, Ap [B*m,64] = interp^T(p*att*rinv)."""
    B, n = idx.shape[0], idx.shape[1]
    p = torch.empty_like(s)
    asum = zeros((B, 64), torch.float32, s.device)
    Ap = zeros((B * m, 64), torch.float32, s.device)
    L.check(L.lib().dh3d_netvlad_commuted_fwd_assign(L.ptr(s), L.ptr(rinv), L.ptr(att), L.ptr(scale), L.ptr(shift),
                                                     L.ptr(idx), L.ptr(dist), L.ptr(order), B, n, m, L.ptr(_mask_u8(mask)),
                                                     L.ptr(p), L.ptr(asum), L.ptr(Ap), L.stream_ptr()),
            "netvlad_commuted_fwd_assign")
    return p, asum, Ap


def nv_commuted_bwd_sums(E, p, s, att, rinv, dasum, mean, rstd, idx, dist, order, mask=None, parts=False):
    """-> dz [B*n,64], datt [B*n], t2 [B*n], S [2,64] float64 (sum dz, sum dz*shat)."""
    B, n = idx.shape[0], idx.shape[1]
    m = E.shape[0] // B
    dz = torch.empty_like(s)
    datt = torch.empty((B * n,), dtype=torch.float32, device=s.device)
    t2 = torch.empty((B * n,), dtype=torch.float32, device=s.device)
    part = zeros((2, B, 64), torch.float64, s.device)
    L.check(L.lib().dh3d_netvlad_commuted_bwd_sums(L.ptr(E), L.ptr(p), L.ptr(s), L.ptr(att), L.ptr(rinv), L.ptr(dasum),
                                                   L.ptr(mean), L.ptr(rstd), L.ptr(idx), L.ptr(dist), L.ptr(order), B, n, m,
                                                   L.ptr(_mask_u8(mask)), L.ptr(dz), L.ptr(datt), L.ptr(t2), L.ptr(part),
                                                   L.stream_ptr()), "netvlad_commuted_bwd_sums")
    return dz, datt, t2, (part if parts else part.sum(1))


def nv_commuted_bwd_apply(dz, s, rinv, t2, k1, k2, k3, idx, dist, order, m, mask=None):
    """-> q [B*n], dcw [B*m,64] = interp^T(rinv * (k1*dz - k2 - k3*s))."""
    B, n = idx.shape[0], idx.shape[1]
    q = torch.empty((B * n,), dtype=torch.float32, device=s.device)
    dcw = zeros((B * m, 64), torch.float32, s.device)
    L.check(L.lib().dh3d_netvlad_commuted_bwd_apply(L.ptr(dz), L.ptr(s), L.ptr(rinv), L.ptr(t2), L.ptr(k1), L.ptr(k2),
                                                    L.ptr(k3), L.ptr(idx), L.ptr(dist), L.ptr(order), B, n, m,
                                                    L.ptr(_mask_u8(mask)), L.ptr(q), L.ptr(dcw), L.stream_ptr()),
            "netvlad_commuted_bwd_apply")
    return q, dcw


def interp_scatter_scaled(c, q, idx, dist, order, dc, mask=None):
    """dc [B*m,256] += interp^T(-q * interp(c)) in place."""
    B, n = idx.shape[0], idx.shape[1]
    m = c.shape[0] // B
    L.check(L.lib().dh3d_interp_scatter_scaled(L.ptr(c), L.ptr(q), L.ptr(idx), L.ptr(dist), L.ptr(order), B, n, m,
                                               L.ptr(_mask_u8(mask)), L.ptr(dc), L.stream_ptr()), "interp_scatter_scaled")
    return dc


def netvlad_assign_rows(s, scale, shift, att, rows_per_cloud=0):
    """a = softmax(s*scale + shift) * att; with rows_per_cloud (% 64 == 0) also (a, asum [clouds, 64]) -- the per-cloud
    column sums of a from the same pass."""
    s = L.require_cuda_f32(s, "s", 2)
    a = torch.empty_like(s)
    asum = None
    if rows_per_cloud:
        asum = torch.empty((s.shape[0] // rows_per_cloud, s.shape[1]), dtype=torch.float32, device=s.device)
    L.check(L.lib().dh3d_netvlad_assign_rows(L.ptr(s), s.shape[0], s.shape[1], L.ptr(scale), L.ptr(shift), L.ptr(att),
                                             L.ptr(a), L.ptr(asum), int(rows_per_cloud), L.stream_ptr()),
            "netvlad_assign_rows")
    return (a, asum) if rows_per_cloud else a


def idw_weights(dist):
    """three_nn distances [..., 3] -> inverse-distance weights (core/backbones.py:92-95), one launch."""
    dist = L.require_cuda_f32(dist, "dist", dist.dim())
    w = torch.empty_like(dist)
    L.check(L.lib().dh3d_idw_weights(L.ptr(dist), dist.numel() // 3, L.ptr(w), L.stream_ptr()), "idw_weights")
    return w


def context_gate(v, g):
    v, g = L.require_cuda_f32(v, "v", v.dim()), L.require_cuda_f32(g, "g", g.dim())
    y = torch.empty_like(v)
    L.check(L.lib().dh3d_context_gate_fwd(L.ptr(v), L.ptr(g), v.numel(), L.ptr(y), L.stream_ptr()), "context_gate")
    return y


def context_gate_bwd(v, g, dy):
    dv, dg = torch.empty_like(v), torch.empty_like(v)
    L.check(L.lib().dh3d_context_gate_bwd(L.ptr(v), L.ptr(g), L.ptr(dy), v.numel(), L.ptr(dv), L.ptr(dg), L.stream_ptr()),
            "context_gate_bwd")
    return dv, dg


def netvlad_assign_rows_bwd(s, scale, shift, att, da):
    s = L.require_cuda_f32(s, "s", 2)
    dz = torch.empty_like(s)
    datt = torch.empty((s.shape[0],), dtype=torch.float32, device=s.device)
    L.check(L.lib().dh3d_netvlad_assign_rows_bwd(L.ptr(s), s.shape[0], s.shape[1], L.ptr(scale), L.ptr(shift),
                                                 L.ptr(att), L.ptr(da), L.ptr(dz), L.ptr(datt), L.stream_ptr()),
            "netvlad_assign_rows_bwd")
    return dz, datt


def l2norm_rows_bwd(x, dxn, eps):
    x = L.require_cuda_f32(x, "x", 2)
    dx = torch.empty_like(x)
    L.check(L.lib().dh3d_l2norm_rows_bwd(L.ptr(x), L.ptr(dxn), x.shape[0], x.shape[1], float(eps), L.ptr(dx),
                                         L.stream_ptr()), "l2norm_rows_bwd")
    return dx


def gemm_tn_batched(A, B):
    """A [b,K,M], B [b,K,N] -> C [b,M,N] = A^T B per batch entry."""
    A = L.require_cuda_f32(A, "A", 3)
    B = L.require_cuda_f32(B, "B", 3)
    b, K, M = A.shape
    N = B.shape[2]
    C = torch.empty((b, M, N), dtype=torch.float32, device=A.device)
    L.check(L.lib().dh3d_gemm_tn_f32_batched(L.ptr(A), L.ptr(B), b, K, M, N, L.ptr(C), L.stream_ptr()), "gemm_tn_batched")
    return C


def gemm_nn_batched(A, B, bias=None):
    """A [b,M,K], B [b,K,N] (+ bias [b,N]) -> C [b,M,N]."""
    A = L.require_cuda_f32(A, "A", 3)
    B = L.require_cuda_f32(B, "B", 3)
    b, M, K = A.shape
    N = B.shape[2]
    C = torch.empty((b, M, N), dtype=torch.float32, device=A.device)
    L.check(L.lib().dh3d_gemm_nn_f32_batched(L.ptr(A), L.ptr(B), L.ptr(bias), b, M, K, N, L.ptr(C), L.stream_ptr()),
            "gemm_nn_batched")
    return C
