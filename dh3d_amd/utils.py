"""Host-side helpers either side of the hot path: keypoint NMS on the device, raw .bin clouds and
descriptors, fixed-size clouds, weighted random choice.  Mirrors core/utils.py:15-43 (single_nms), :87-110 (get_fixednum_pcd),
:139-153 (load_descriptor_bin / load_single_pcfile / write_to_bin)."""
import numpy as np
import torch

from . import pairs, pm


def single_nms(xyz, attention, nms_radius, min_response_ratio, max_keypoints, remove_noise=True, knn=50):
    """Keypoint non-maximum suppression on the GPU (core/utils.py:15-43, used by localdesc_extract.py:92-102).

    xyz [N,3] / attention [N] CUDA float32.  A point survives if its response is the (first) maximum among its `knn`
    nearest neighbours inside `nms_radius` (rank 0 = the point itself), exceeds min_response_ratio * max response,
    and -- remove_noise -- its 8th neighbour lies within 2.0 (sparse outliers are muted first).  Survivors are
    ordered by (response, index) descending and cut to max_keypoints.  Returns (num_keypoints, indices [num] int64).

    The 50-NN query is the kNN kernel of the hot path (exact; float32 distances where the reference's scikit-learn
    ball tree computes in float64 -- a point exactly on the 2.0 / nms_radius shell may fall on the other side)."""
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz must be [N,3]")
    N = xyz.shape[0]
    k = min(knn, N)
    att = attention.reshape(N).to(torch.float32).clone()
    nn, dist = pm.knn_xyz(xyz.reshape(1, N, 3).contiguous(), k)
    nn, dist = nn[0].long(), dist[0]
    if remove_noise and k > 7:
        att[dist[:, 7] > 2.0] = 0.0
    knn_att = att[nn]
    knn_att[dist > nms_radius] = 0.0
    is_max = knn_att.argmax(dim=1) == 0  # torch.argmax, like numpy's, returns the first maximal index
    thresh = att.max() * min_response_ratio
    keep = torch.nonzero(is_max & (att > thresh)).reshape(-1)
    if keep.numel() > 0:
        # sorted(..., reverse=True) on (attention, index) tuples: response descending, then index descending
        order = torch.argsort(keep, descending=True)
        keep = keep[order]
        keep = keep[torch.argsort(att[keep], descending=True, stable=True)]
    keep = keep[:max_keypoints]
    return int(keep.numel()), keep


def batched_knn(xyz, knn=50):
    """The k-NN batched_nms runs on: (nn [B,N,k] int32, dist [B,N,k]), k = min(knn, N).  The Morton-ordered search up to
    16384 points, the brute-force kernel beyond; both give the ids and distance bits of pm.knn_xyz (single_nms's)."""
    N = xyz.shape[1]
    k = min(int(knn), N)
    if N <= 16384:
        srt, gbox = pm.spatial_sort(xyz)
        return pm.knn_sorted(srt, gbox, k)
    return pm.knn_xyz(xyz, k)


def batched_nms(xyz, scores, nms_radius, min_response_ratio, max_keypoints, remove_noise=True, knn=50, num_valid=None,
                invert=False):
    """single_nms for a batch, on the device end to end (HIP: dh3d_keypoint_nms), no host sync -- graph-capturable.

    xyz [B,N,3], scores [B,N] float32 on the GPU (invert=True: the score is 1 - scores, e.g. scores =
    xyz_feat_att[:, :, 131], read in place).  Returns (count [B] int32, inds [B, max_keypoints] int32 padded with -1):
    cloud b's keypoints are inds[b, :count[b]], the ids single_nms(xyz[b], scores[b]) returns, in its order, bit for bit.

    num_valid [B] int32 (optional): cloud b holds num_valid[b] real points followed by padding; padded points are never
    kept, take no part in the maximum response and count as outside every ball.  That equals single_nms on the cropped
    cloud xyz[b, :num_valid[b]] whenever no real point has a padded one among its k nearest neighbours -- the case of
    get_fixednum_pcd(randsample=False) (dummies at 1e5, >= 50 real points).  Padding by re-drawn duplicates
    (randsample=True) is not covered: the duplicates change the real points' neighbourhoods."""
    x = xyz if xyz.is_contiguous() else xyz.contiguous()
    if x.dim() != 3 or x.shape[2] != 3:
        raise ValueError("xyz must be [B,N,3]")
    if scores.dim() != 2 or tuple(scores.shape) != tuple(x.shape[:2]):
        raise ValueError("scores must be [B,N] = %s, got %s" % (tuple(x.shape[:2]), tuple(scores.shape)))
    nn, dist = batched_knn(x, knn)
    return pm.keypoint_nms(scores, nn, dist, nms_radius, min_response_ratio, max_keypoints, remove_noise=remove_noise,
                           num_valid=num_valid, invert=invert)


def sample_by_weight(weights, m, count=None, seed=0):
    """m ids a row drawn WITH replacement, id i of row b with probability weights[b, i] / sum(weights[b]), on the device, no
    host sync -- graph-capturable (HIP: dh3d_prob_sample_seeded; the reference's ProbSample with the draws made on the device).

    weights [B,n] float32 on the GPU, non-negative and finite.  count [B] int32 (optional): row b is its first count[b]
    entries, held to 0 .. n; the entries behind them are never read.  Returns ids [B,m] int32; a row without entries or with
    a total that is not > 0 is all -1.  An id of weight 0 is never drawn as long as the sums before it are exact.

    seed is an int or a 1-element int64 tensor on the GPU, as pairs.py takes it: the kernels read the tensor, so a captured
    graph draws afresh on every replay once the caller changes it.  The ids feed ops.gather_point / ops.group_point, e.g.
    keypoints in proportion to the detector's attention:
        ids = sample_by_weight(attention, 256, count=num_valid, seed=seed)
        xyz = ops.gather_point(points, ids)"""
    if isinstance(weights, torch.Tensor) and weights.dim() != 2:
        raise ValueError("sample_by_weight expects (batch_size,num_choices) weights, got %s" % (tuple(weights.shape),))
    if isinstance(weights, torch.Tensor) and not weights.is_cuda:
        raise ValueError("weights must live on the GPU (the HIP path has no CPU fallback)")
    sd = pairs.seed_tensor(seed, weights.device if isinstance(weights, torch.Tensor) else None)
    with torch.no_grad():
        return pm.prob_sample_seeded(weights, m, count, sd)[0]


def load_descriptor_bin(filename, dim=131, dtype=np.float32):
    """Raw little-endian float32 rows of `dim` values: [x, y, z, 128-d descriptor(, score)]."""
    return np.fromfile(filename, dtype=dtype).reshape(-1, dim)


def load_single_pcfile(filename, dim=3, dtype=np.float32):
    """Raw float32 cloud with `dim` values per point; the first three are the coordinates."""
    pc = np.fromfile(filename, dtype=dtype)
    return pc.reshape(pc.shape[0] // dim, dim)[:, 0:3]


def write_to_bin(points, filename):
    np.ascontiguousarray(points).tofile(filename)


def get_fixednum_pcd(cloud, targetnum, randsample=True, sortby_dis=True, rng=None):
    """Crop (nearest to the centroid first, then a random permutation) or pad (random re-draws, or far-away
    dummies) a cloud to exactly `targetnum` points; returns (cloud, number of original points kept).  One cloud, on the
    host, without the voxel down-sampling / outlier removal the reference runs first (open3d): prepare_clouds() below does
    those two steps and the randsample=False crop / pad for a batch of raw clouds on the device."""
    rng = np.random.default_rng() if rng is None else rng
    cloud = np.asarray(cloud)
    n = cloud.shape[0]
    if n > targetnum:
        if sortby_dis:
            d = ((cloud - cloud.mean(axis=0)) ** 2).sum(axis=1)
            cloud = cloud[np.argsort(d)[:targetnum], :3]
        cloud = cloud[rng.choice(cloud.shape[0], targetnum, replace=False)]
        return cloud, targetnum
    pad = targetnum - n
    if randsample:
        extra = cloud[rng.choice(n, size=pad, replace=True)]
    else:
        extra = np.full((pad, 3), 100000.0, dtype=np.float32)
    return np.concatenate([cloud, extra], axis=0), n


def prepare_clouds(raw, num_raw, targetnum, voxel_size=0.2, radius=1.0, nb_points=4, randsample=False, sortby_dis=True,
                   check=False):
    """get_fixednum_pcd(need_downsample=True, randsample=False) of the reference (core/utils.py:87-110, the test-set reader
    core/datasets.py:85) for B raw clouds of different sizes, on the GPU, no host sync, graph-capturable (HIP:
    dh3d_prepare_clouds; include/dh3d_hip.h holds the exact semantics, DESIGN.md the points INFERRED from open3d).

    raw [B,Nraw,3] float32 and num_raw [B] int32 on the GPU: cloud b is raw[b, :num_raw[b]], finite rows, Nraw <= 131072.
      1. voxel grid of `voxel_size` (None: skipped): a voxel's point is the float32 mean of its members; the voxels come in
         the order of their first member.
      2. radius outliers (radius None: skipped): a point stays iff more than `nb_points` points, itself included, lie
         strictly inside `radius`.
      3. m survivors: m <= targetnum pads with rows of 100000.0 (num_valid = m); m > targetnum keeps the targetnum points
         nearest the centroid (sortby_dis) or the first targetnum.  The reference then shuffles the kept points with an
         unseeded random permutation; here they stay in index order, which nothing downstream depends on.
    Returns (points [B,targetnum,3], num_valid [B] int32, counts [B,3] int32 = raw points / voxels / survivors, centroid
    [B,3] float64): points and num_valid are what DH3D.forward(num_valid=...), batched_nms and register_clouds take.

    randsample=True (padding by re-drawn points) is not on the device: get_fixednum_pcd does it on the host.  A cloud
    wider than 2^21 cells on an axis comes back void (num_valid 0, counts [b, 1:] = -1); check=True reads counts back (a
    host sync, not capturable) and raises ValueError for it."""
    if randsample:
        raise NotImplementedError("prepare_clouds pads with far-away dummies only (randsample=False); padding by re-drawn "
                                  "points is utils.get_fixednum_pcd(randsample=True) on the host")
    out = pm.prepare_clouds(raw, num_raw, targetnum, voxel_size=voxel_size, radius=radius, nb_points=nb_points,
                            sortby_dis=sortby_dis)
    if check and bool((out[2][:, 1] < 0).any()):
        raise ValueError("prepare_clouds: a cloud spans 2^21 cells or more on an axis (voxel_size / radius too small for it)")
    return out
