"""Training batches on the device: what core/datasets.py builds on the host, one cloud at a time, between the prepared
clouds and the trainers (HIP: csrc/pairs.hip; include/dh3d_hip.h "Training batches" holds the exact semantics).

    resample_clouds    get_fixednum_pcd(randsample=True, sortby_dis=False): a random choice of, or a padding by re-drawn
                       points to, a fixed number of points
    augment_clouds     core/augment.py: Rotate1D, Jitter, Scale, RotateSmall, Shift as one float64 chain, rounded once
    sample_pair_nodes  the second half of loadPair: farthest-point nodes in a random half of pc1, their 1-NN in pc2
    make_local_pairs   Local_train_dataset_selfpair.loadPair for B sources: the arguments of LocalTrainer.step
    make_global_batch  Global_train_dataset_triplet.loadPC for the clouds of a quadruplet: QuadrupletTrainer.step's input

numpy's random streams cannot be reproduced; every draw is a counter-based function of (seed, stream, cloud, element)
through splitmix64, restated exactly in the header.  `seed` is an int or a 1-element int64 tensor on the GPU: the kernels
read it from device memory, so a captured graph draws a fresh batch on every replay once the caller changes that tensor
(an int is copied to the device on every call, which a capture cannot hold).  Nothing here synchronises with the host."""
import math

import torch

from . import _lib as L

AUGMENTATIONS = ("Rotate1D", "Jitter", "Scale", "RotateSmall", "Shift")  # the order of get_augmentations_from_list
_AUG_BITS = {"Rotate1D": 1, "Jitter": 2, "Scale": 4, "RotateSmall": 8, "Shift": 16}  # include/dh3d_hip.h DH3D_AUG_*
RESAMPLE_MAX_N, RESAMPLE_MAX_TARGET = 131072, 1 << 20  # include/dh3d_hip.h dh3d_resample_clouds
PAIR_MAX_N = 16384                                      # include/dh3d_hip.h dh3d_sample_pair_nodes


def aug_mask(aug):
    """The DH3D_AUG_* bit set of a collection of augmentation names (None: no augmentation); ValueError for another name."""
    mask = 0
    for name in (aug or ()):
        if name not in _AUG_BITS:
            raise ValueError("unknown augmentation %r: expected a subset of %s" % (name, AUGMENTATIONS))
        mask |= _AUG_BITS[name]
    return mask


def seed_tensor(seed, device):
    """The device scalar the kernels read: a 1-element int64 tensor is passed through (its 64 bits are the uint64 seed); an
    int is reduced mod 2^64 and copied to the device."""
    if isinstance(seed, torch.Tensor):
        if seed.dtype != torch.int64 or seed.numel() != 1:
            raise ValueError("seed must be an int or a 1-element int64 tensor, got %s %s" % (seed.dtype, tuple(seed.shape)))
        if not seed.is_cuda:
            raise ValueError("a seed tensor must live on the GPU (the kernels read it)")
        return seed
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return torch.tensor([s - (1 << 64) if s >= 1 << 63 else s], dtype=torch.int64, device=device)


def _clouds(points, name):
    if isinstance(points, torch.Tensor) and (points.dim() != 3 or points.shape[2] != 3 or points.shape[0] < 1 or points.shape[1] < 1):
        raise ValueError("%s must be (batch_size,npoints,3), got %s" % (name, tuple(points.shape)))
    return L.require_cuda_f32(points, name, 3)


def resample_clouds(points, num_valid, targetnum, seed=0):
    """points [B,Nsrc,3] float32, num_valid [B] int32 -> (out [B,targetnum,3], num_orig [B] int32 = min(n, targetnum)).

    get_fixednum_pcd(randsample=True, sortby_dis=False) (core/utils.py:87-110) after its outlier removal, which
    utils.prepare_clouds(voxel_size=None) does.  Cloud b is the first n = num_valid[b] rows; rows behind them are never
    read.  n >= targetnum: a random choice of targetnum rows, in index order; 0 < n < targetnum: the rows, then re-drawn
    ones; n == 0: rows of 100000.0.  The crop to the points nearest the centroid of the global loader (sortby_dis=True) is
    prepare_clouds' own: prepare_clouds(sortby_dis=True) followed by this function restates loadPC's draw."""
    targetnum = int(targetnum)
    if targetnum < 1:
        raise ValueError("resample_clouds expects targetnum >= 1")
    if isinstance(points, torch.Tensor) and points.dim() == 3 and (points.shape[1] > RESAMPLE_MAX_N or targetnum > RESAMPLE_MAX_TARGET):
        raise ValueError("resample_clouds: nsrc = %d / targetnum = %d is beyond the kernels (%d / %d)"
                         % (points.shape[1], targetnum, RESAMPLE_MAX_N, RESAMPLE_MAX_TARGET))
    x = _clouds(points, "points")
    n = L.require_cuda_i32(num_valid, "num_valid", 1)
    B, N, _ = x.shape
    if n.shape[0] != B:
        raise ValueError("resample_clouds expects (batch_size) num_valid = (%d,), got %s" % (B, tuple(n.shape)))
    sd = seed_tensor(seed, x.device)
    out = torch.empty((B, targetnum, 3), dtype=torch.float32, device=x.device)
    num_orig = torch.empty((B,), dtype=torch.int32, device=x.device)
    nbytes = L.lib().dh3d_resample_clouds_ws_bytes(B, N, targetnum)
    if nbytes == 0:
        raise ValueError("resample_clouds: shape B = %d, nsrc = %d, targetnum = %d is beyond the kernels" % (B, N, targetnum))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        L.check(L.lib().dh3d_resample_clouds(B, N, targetnum, L.ptr(x), L.ptr(n), L.ptr(sd), L.ptr(out), L.ptr(num_orig),
                                             L.ptr(ws), nbytes, L.stream_ptr()), "resample_clouds")
    return out, num_orig


def augment_clouds(points, aug, seed=0, sigma=0.05, clip=0.1, scale_low=0.8, scale_high=1.25, angle_sigma=0.06,
                   angle_clip=0.18, shift_range=0.1):
    """core/augment.py on the device: points [B,N,3] float32 -> (out [B,N,3] float32, params).

    `aug` is a subset of AUGMENTATIONS; whatever its order, the augmentations run in the order of
    get_augmentations_from_list (Rotate1D about z, Jitter, Scale, RotateSmall, Shift) as one float64 chain that is rounded
    once to float32.  params holds the per-cloud transform in float64: rot1d [B,3,3], scale [B], rot_small [B,3,3], shift
    [B,3] (identity / 1 / 0 for what is off); rows are multiplied from the left, data @ R, as in the reference."""
    mask = aug_mask(aug)
    x = _clouds(points, "points")
    B, N, _ = x.shape
    sd = seed_tensor(seed, x.device)
    out = torch.empty_like(x)
    f64 = dict(dtype=torch.float64, device=x.device)
    params = {"rot1d": torch.empty((B, 3, 3), **f64), "scale": torch.empty((B,), **f64),
              "rot_small": torch.empty((B, 3, 3), **f64), "shift": torch.empty((B, 3), **f64)}
    with torch.cuda.device(x.device):
        L.check(L.lib().dh3d_augment_clouds(B, N, L.ptr(x), mask, float(sigma), float(clip), float(scale_low), float(scale_high),
                                            float(angle_sigma), float(angle_clip), float(shift_range), L.ptr(sd), L.ptr(out),
                                            L.ptr(params["rot1d"]), L.ptr(params["scale"]), L.ptr(params["rot_small"]),
                                            L.ptr(params["shift"]), L.stream_ptr()), "augment_clouds")
    return out, params


def rotate_pairs(pc2, rot_maxv=math.pi, seed=0, out=None):
    """loadPair's rotation of the second clouds: pc2 [B,N,3] -> (pc2 @ Rot in float64 rounded once [B,N,3], Rot [B,3,3]
    float32), Rot = [[c,s,0],[-s,c,0],[0,0,1]] of a uniform angle in [-rot_maxv, rot_maxv).  out: where to write the clouds."""
    x = _clouds(pc2, "pc2")
    B, N, _ = x.shape
    sd = seed_tensor(seed, x.device)
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device:
        raise ValueError("rotate_pairs: out must be a contiguous float32 tensor of pc2's shape on its device")
    R = torch.empty((B, 3, 3), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        L.check(L.lib().dh3d_pair_rotate(B, N, L.ptr(x), float(rot_maxv), L.ptr(sd), L.ptr(out), L.ptr(R), L.stream_ptr()),
                "rotate_pairs")
    return out, R


def sample_pair_nodes(pc1, pc2, sample_nodes, seed=0):
    """pc1, pc2 [B,N,3] float32 -> (anc [B,M], pos [B,M] int32), M = sample_nodes: loadPair's nodes (core/datasets.py:142-150).

    A random half of pc1 (N // 2 rows, in index order), FarthestSampler.sample over it from a random first pick (running
    minimum of the float64 squared distance, next pick = the first maximum), anc = the picks as rows of pc1, pos = each
    anchor's nearest row of pc2 (lowest index on ties).  N <= 16384 and 1 <= sample_nodes <= N // 2."""
    M = int(sample_nodes)
    if isinstance(pc1, torch.Tensor) and pc1.dim() == 3:
        if pc1.shape[1] > PAIR_MAX_N:
            raise ValueError("sample_pair_nodes: npoints = %d is beyond the kernel (%d)" % (pc1.shape[1], PAIR_MAX_N))
        if not 1 <= M <= pc1.shape[1] // 2:
            raise ValueError("sample_pair_nodes expects 1 <= sample_nodes <= npoints // 2 = %d, got %d" % (pc1.shape[1] // 2, M))
    a = _clouds(pc1, "pc1")
    b = _clouds(pc2, "pc2")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("sample_pair_nodes: pc1 %s and pc2 %s must have one shape and device" % (tuple(a.shape), tuple(b.shape)))
    B, N, _ = a.shape
    sd = seed_tensor(seed, a.device)
    anc = torch.empty((B, M), dtype=torch.int32, device=a.device)
    pos = torch.empty((B, M), dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        L.check(L.lib().dh3d_sample_pair_nodes(B, N, M, L.ptr(a), L.ptr(b), L.ptr(sd), L.ptr(anc), L.ptr(pos), L.stream_ptr()),
                "sample_pair_nodes")
    return anc, pos


def make_local_pairs(src, num_valid, numpts=8192, sample_nodes=256, rot_maxv=math.pi, aug=("Jitter",), seed=0):
    """Local_train_dataset_selfpair.loadPair (core/datasets.py:119-151) for B source clouds src [B,Nsrc,3] / num_valid [B]
    (utils.prepare_clouds' outputs): every source is drawn twice (clouds b and B + b of a stacked batch: resample_clouds,
    then augment_clouds), the second draw is rotated about z by a uniform angle in [-rot_maxv, rot_maxv), and the nodes come
    from sample_pair_nodes on the first draw and the UNROTATED second, as upstream.  Returns a dict:
        points [2B,numpts,3] = [pc1 | pc2_trans], R [B,3,3] float32, sample_idx [2B,sample_nodes] int32 = [anc | pos]
            -- the arguments of LocalTrainer.step --
        pc2 [B,numpts,3]  the second draws before the rotation."""
    aug_mask(aug)  # (an unknown name is refused before anything is launched)
    x = _clouds(src, "src")
    n = L.require_cuda_i32(num_valid, "num_valid", 1)
    B = x.shape[0]
    sd = seed_tensor(seed, x.device)
    drawn, _ = resample_clouds(torch.cat([x, x], dim=0), torch.cat([n, n], dim=0), numpts, seed=sd)
    both, _ = augment_clouds(drawn, aug, seed=sd)
    pc1, pc2 = both[:B], both[B:]
    points = torch.empty_like(both)
    points[:B].copy_(pc1)
    _, R = rotate_pairs(pc2, rot_maxv, seed=sd, out=points[B:])
    anc, pos = sample_pair_nodes(pc1, pc2, sample_nodes, seed=sd)
    return {"points": points, "R": R, "sample_idx": torch.cat([anc, pos], dim=0), "pc2": pc2}


def make_global_batch(clouds, num_valid, numpts=8192, aug=("Jitter", "RotateSmall", "Shift", "Rotate1D"), seed=0):
    """Global_train_dataset_triplet.loadPC (core/datasets.py:184-191) for the clouds of a quadruplet, in their role order:
    resample_clouds, then augment_clouds.  clouds [B,Nsrc,3] / num_valid [B] come from utils.prepare_clouds(sortby_dis=True),
    the step before this one: its crop to the points nearest the centroid is loadPC's sortby_dis=True.  Returns points
    [B,numpts,3], the input of QuadrupletTrainer.step."""
    aug_mask(aug)
    x = _clouds(clouds, "clouds")
    sd = seed_tensor(seed, x.device)
    drawn, _ = resample_clouds(x, num_valid, numpts, seed=sd)
    return augment_clouds(drawn, aug, seed=sd)[0]
