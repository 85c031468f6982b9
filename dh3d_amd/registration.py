"""Registration of cloud pairs from keypoints: descriptor matching and RANSAC rigid fits on the device, for many pairs per
call (csrc/registration.hip), plus the reference evaluation's error metrics on the host.

The reference does this step in MATLAB, one pair at a time (evaluate/local_eval/matlab_code: local_align_demo.m,
eval_align.m): pdist2(pos_desc, anc_desc, 'smallest', 1), ransacfitRt with a 1.0 m threshold, then compareTransform /
GetEulerAngles and a success / inlier-ratio / trial / RTE / RRE summary.  Here a batch of pairs stays on the GPU until a
[P, 3, 4] pose and a few counts per pair come out; include/dh3d_hip.h dh3d_ransac_rigid states every rule (the splitmix64
sampler replaces randsample, whose stream cannot be reproduced).  Beside RANSAC stands a deterministic estimator on the same
correspondences, gnc_rigid (dh3d_gnc_rigid: graduated non-convexity on the Geman-McClure objective by re-weighted float64
fits): no seed, and a fit count that depends on the extent of the correspondences and the threshold, not on the inlier
share (the time follows it within a few per cent: the eigen-solve of a fit sweeps until it has converged).  It is a local
method with a good track record, not a guarantee.  estimator="gnc" selects it in register, register_clouds and
register_fpfh (and through their keywords in PlaceIndex.localize and relocalize_clouds); the default stays "ransac".
relocalize_scan_context has no keypoint fit to select: its pose comes from the Scan Context yaw and ICP.

    match, dist = match_descriptors(anchor_desc, anchor_count, positive_desc, positive_count)
    m2 = match_descriptors2(anchor_desc, anchor_count, positive_desc, positive_count, ratio=0.9, mutual=True)  # nn1, nn2, match, ...
    res = register(anchor_rows, anchor_count, positive_rows, positive_count, match={"ratio": 0.9, "mutual": True})
    res = ransac_rigid(anchor_xyz, positive_xyz, match, anchor_count)       # Rt, valid, inliers, ... (no host sync)
    res = gnc_rigid(anchor_xyz, positive_xyz, match, anchor_count, threshold=0.5)  # the same keys + weights, iterations
    res = register(anchor_rows, anchor_count, positive_rows, positive_count, estimator="gnc", threshold=0.5)
    res = register(anchor_rows, anchor_count, positive_rows, positive_count)  # rows as xyz_feat_att_nms / _nms_res.bin
    res = register_clouds(model, anchor_points, positive_points)              # forward (config.detection) + register
    res = refine_icp(anchor_points, positive_points, res["Rt"], res["valid"])  # dense ICP: Rt, fitness, rmse, nn, ...
    res = register_clouds(model, anchor_points, positive_points, refine=True)  # ... with the refined pose as Rt
    nrm = estimate_normals(anchor_points, k=16)                               # PCA normals, curvature, the ids used
    res = refine_icp_plane(anchor_points, positive_points, res["Rt"], res["valid"])  # point-to-plane: + num_plane, rmse_plane
    res = register_clouds(model, anchor_points, positive_points, refine={"method": "plane", "iterations": 5})
    res = refine_icp_gicp(anchor_points, positive_points, res["Rt"], res["valid"])  # generalized ICP: + num_planar, rmse_gicp
    f = compute_fpfh(anchor_points, k=32)                                     # fpfh [P, N, 36], counts, normals, nbr
    res = register_fpfh(anchor_points, positive_points, refine=True)          # no model: normals -> FPFH -> match -> RANSAC -> ICP
    kp = iss_keypoints(anchor_points, salient_radius=2.0, non_max_radius=1.5) # ISS detector: ids, count, saliency, ...
    res = register_fpfh(anchor_points, positive_points, keypoints={"method": "iss"})  # ... in front of the FPFH registration
    dt, ddeg = transform_errors(T_gt, res["Rt"], res["valid"])                # compareTransform, host float64
    summary = summarize_registration(dt, ddeg, res["inlier_ratio"], res["trials"])
"""
import numpy as np
import torch

from . import _lib as L
from .pm import KEYPOINT_MAX

DESC_MAX = 256  # descriptor length limit of dh3d_match_descriptors


def _rows(t, name, min_cols):
    """A float32 [P, M, C] GPU tensor whose rows can be read with one element stride (a column slice of a contiguous map is
    read in place); anything else is made contiguous."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.dim() != 3:
        raise ValueError("%s must be a float32 [P, M, C] tensor on the GPU" % name)
    if t.shape[2] < min_cols:
        raise ValueError("%s needs at least %d columns, got shape %s" % (name, min_cols, tuple(t.shape)))
    if t.shape[0] == 0 or t.shape[1] == 0:
        raise ValueError("%s must not be empty, got shape %s" % (name, tuple(t.shape)))
    if t.stride(2) != 1 or t.stride(0) != t.shape[1] * t.stride(1) or t.stride(1) < t.shape[2]:
        t = t.contiguous()
    return t


def _count(c, name, P, device):
    c = L.require_cuda_i32(c, name, 1)
    if c.shape[0] != P or c.device != device:
        raise ValueError("%s must be int32 [%d] on %s, got %s on %s" % (name, P, device, tuple(c.shape), c.device))
    return c


def _check_m(M, name):
    if M > KEYPOINT_MAX:
        raise ValueError("%s: at most %d keypoints per cloud, got %d" % (name, KEYPOINT_MAX, M))


def _descriptor_pair(anchor_desc, anchor_count, positive_desc, positive_count):
    """The checked inputs of match_descriptors / match_descriptors2 and their shape: a, ac, b, bc, P, Ma, Mb, D."""
    a = _rows(anchor_desc, "anchor_desc", 1)
    b = _rows(positive_desc, "positive_desc", 1)
    P, Ma, D = a.shape
    if b.shape[0] != P or b.shape[2] != D or b.device != a.device:
        raise ValueError("positive_desc must be [%d, Mb, %d] on %s, got %s" % (P, D, a.device, tuple(b.shape)))
    Mb = b.shape[1]
    if D > DESC_MAX or D % 4:
        raise ValueError("descriptor length must be a multiple of 4 up to %d, got %d" % (DESC_MAX, D))
    _check_m(Ma, "anchor_desc")
    _check_m(Mb, "positive_desc")
    ac = _count(anchor_count, "anchor_count", P, a.device)
    bc = _count(positive_count, "positive_count", P, a.device)
    return a, ac, b, bc, P, Ma, Mb, D


def match_descriptors(anchor_desc, anchor_count, positive_desc, positive_count):
    """Nearest positive descriptor of every anchor keypoint (pdist2(pos, anc, 'smallest', 1)): anchor_desc [P, Ma, D] and
    positive_desc [P, Mb, D] float32 (column views such as rows[:, :, 3:131] are read in place), counts [P] int32 ->
    (match [P, Ma] int32, the lowest positive id at the smallest distance, -1 past anchor_count or when the pair has no
    positive; dist [P, Ma] float32, +inf there).  D <= 256, a multiple of 4; Ma, Mb <= 4096."""
    a, ac, b, bc, P, Ma, Mb, D = _descriptor_pair(anchor_desc, anchor_count, positive_desc, positive_count)
    match = torch.empty((P, Ma), dtype=torch.int32, device=a.device)
    dist = torch.empty((P, Ma), dtype=torch.float32, device=a.device)
    L.check(L.lib().dh3d_match_descriptors(L.ptr(a), a.stride(1), L.ptr(ac), L.ptr(b), b.stride(1), L.ptr(bc), P, Ma, Mb, D,
                                           L.ptr(match), L.ptr(dist), L.stream_ptr()), "match_descriptors")
    return match, dist


def match_descriptors2(anchor_desc, anchor_count, positive_desc, positive_count, ratio=None, mutual=False):
    """match_descriptors with the second neighbour, Lowe's ratio test and the mutual check (include/dh3d_hip.h
    dh3d_match_descriptors2 states every rule).  Inputs and limits as match_descriptors.  ratio: None (no test) or a number
    in (0, 1]: a row is kept when S1 < float32(ratio * ratio) * S2 on the float32 sums of squares (strict: ratio = 1 rejects
    exact ties; a lone candidate is kept).  mutual: keep a row only when its positive's nearest anchor is that row.
    Returns a dict of device tensors: nn1 / nn2 [P, Ma] int32 and dist1 / dist2 [P, Ma] float32 (the two nearest positives,
    ties to the lowest id; -1 / +inf where there is none; nn1 / dist1 are match_descriptors' results bit for bit), match
    [P, Ma] int32 (nn1 where the row is kept, else -1), num_kept [P] int32, and with mutual=True rev [P, Mb] int32 /
    rev_dist [P, Mb] float32 (every positive's nearest anchor; without mutual the reverse search is not run).  No host
    sync: graph-capturable."""
    a, ac, b, bc, P, Ma, Mb, D = _descriptor_pair(anchor_desc, anchor_count, positive_desc, positive_count)
    ratio2 = 0.0
    if ratio is not None:
        ratio = float(ratio)
        if not 0.0 < ratio <= 1.0:
            raise ValueError("ratio must be None or in (0, 1], got %r" % (ratio,))
        ratio2 = float(np.float32(ratio * ratio))
    mutual = bool(mutual)
    dev = a.device
    new = lambda M, dtype: torch.empty((P, M), dtype=dtype, device=dev)
    out = dict(nn1=new(Ma, torch.int32), dist1=new(Ma, torch.float32), nn2=new(Ma, torch.int32), dist2=new(Ma, torch.float32),
               match=new(Ma, torch.int32), num_kept=torch.empty((P,), dtype=torch.int32, device=dev))
    if mutual:
        out["rev"], out["rev_dist"] = new(Mb, torch.int32), new(Mb, torch.float32)
    with torch.cuda.device(dev):
        L.check(L.lib().dh3d_match_descriptors2(L.ptr(a), a.stride(1), L.ptr(ac), L.ptr(b), b.stride(1), L.ptr(bc), P, Ma, Mb, D,
                                                ratio2, int(mutual), L.ptr(out["nn1"]), L.ptr(out["dist1"]), L.ptr(out["nn2"]),
                                                L.ptr(out["dist2"]), L.ptr(out.get("rev")), L.ptr(out.get("rev_dist")),
                                                L.ptr(out["match"]), L.ptr(out["num_kept"]), L.stream_ptr()),
                "match_descriptors2")
    return out


def _corr_inputs(anchor_xyz, positive_xyz, match, anchor_count):
    """The checked inputs of ransac_rigid / gnc_rigid and their shape: ax, bx, m, ac, P, Ma, Mb."""
    ax = _rows(anchor_xyz, "anchor_xyz", 3)
    bx = _rows(positive_xyz, "positive_xyz", 3)
    P, Ma = ax.shape[:2]
    if bx.shape[0] != P or bx.device != ax.device:
        raise ValueError("positive_xyz must be [%d, Mb, >=3] on %s, got %s" % (P, ax.device, tuple(bx.shape)))
    Mb = bx.shape[1]
    _check_m(Ma, "anchor_xyz")
    _check_m(Mb, "positive_xyz")
    m = L.require_cuda_i32(match, "match", 2)
    if tuple(m.shape) != (P, Ma) or m.device != ax.device:
        raise ValueError("match must be int32 [%d, %d] on %s, got %s" % (P, Ma, ax.device, tuple(m.shape)))
    ac = _count(anchor_count, "anchor_count", P, ax.device)
    return ax, bx, m, ac, P, Ma, Mb


def ransac_rigid(anchor_xyz, positive_xyz, match, anchor_count, threshold=1.0, confidence=0.99, max_trials=10000, seed=0):
    """ransacfitRt on every pair: correspondences anchor_xyz[p, i] <-> positive_xyz[p, match[p, i]] for i < anchor_count[p]
    with 0 <= match < Mb; the model maps positive into anchor coordinates (anchor ~ R positive + t).  anchor_xyz [P, Ma, >=3]
    and positive_xyz [P, Mb, >=3] float32 (the first three columns are read; keypoint rows are read in place).  Returns a
    dict of device tensors: Rt [P, 3, 4] float64 (NaN where not valid), valid [P] bool, inliers [P, Ma] bool (the winning
    hypothesis' mask), num_inliers [P] int32, inlier_ratio [P] float64 (num_inliers / n, 0 when n = 0), trials [P] int32,
    num_corr [P] int32 (n).  No host sync: graph-capturable."""
    ax, bx, m, ac, P, Ma, Mb = _corr_inputs(anchor_xyz, positive_xyz, match, anchor_count)
    threshold, confidence, max_trials, seed = float(threshold), float(confidence), int(max_trials), int(seed)
    if not threshold > 0.0 or not 0.0 < confidence < 1.0 or not 0 <= max_trials < (1 << 30):
        raise ValueError("need threshold > 0, 0 < confidence < 1 and 0 <= max_trials < 2^30, got %r, %r, %r"
                         % (threshold, confidence, max_trials))
    if not 0 <= seed < (1 << 64):
        raise ValueError("seed must be a uint64, got %r" % seed)
    dev = ax.device
    Rt = torch.empty((P, 3, 4), dtype=torch.float64, device=dev)
    valid = torch.empty((P,), dtype=torch.int32, device=dev)
    inliers = torch.empty((P, Ma), dtype=torch.bool, device=dev)
    num_inliers = torch.empty((P,), dtype=torch.int32, device=dev)
    trials = torch.empty((P,), dtype=torch.int32, device=dev)
    num_corr = torch.empty((P,), dtype=torch.int32, device=dev)
    L.check(L.lib().dh3d_ransac_rigid(L.ptr(ax), ax.stride(1), L.ptr(bx), bx.stride(1), L.ptr(m), L.ptr(ac), P, Ma, Mb,
                                      threshold, confidence, max_trials, seed, L.ptr(Rt), L.ptr(valid), L.ptr(inliers),
                                      L.ptr(num_inliers), L.ptr(trials), L.ptr(num_corr), L.stream_ptr()), "ransac_rigid")
    ratio = num_inliers.to(torch.float64) / num_corr.clamp(min=1).to(torch.float64)
    return dict(Rt=Rt, valid=valid.bool(), inliers=inliers, num_inliers=num_inliers, inlier_ratio=ratio, trials=trials,
                num_corr=num_corr)


GNC_MAX_ITERATIONS = 1024  # csrc/registration.hip kGncMaxIter


def gnc_rigid(anchor_xyz, positive_xyz, match, anchor_count, threshold=1.0, division=1.4, settle=8, max_iterations=64):
    """A deterministic robust fit of every pair, beside ransac_rigid and on its inputs: graduated non-convexity on the
    Geman-McClure objective (Fast Global Registration's, solved by re-weighted closed-form float64 fits; include/dh3d_hip.h
    dh3d_gnc_rigid states every rule).  No sampling and no seed; the number of fits depends only on the extent of the
    correspondences and the threshold, not on the inlier share (RANSAC's trial count, and with it its time, does).  It is a local method with a
    good track record, not a guarantee: from the least-squares start it can settle on a wrong pose when outliers dominate.
    threshold: the residual scale the weights end at, and the inlier distance (ransac_rigid's meaning and default);
    division > 1: the factor mu shrinks by per fit; settle >= 0: further fits once mu has reached threshold^2;
    1 <= max_iterations <= 1024 ends the schedule early (1: the plain least-squares fit).  Returns ransac_rigid's keys --
    Rt [P, 3, 4] float64 (NaN where not valid), valid [P] bool, inliers [P, Ma] bool (residual < threshold under Rt),
    num_inliers, inlier_ratio, num_corr -- plus weights [P, Ma] float64 (the weights of the last fit in anchor row order, 0
    for rows that are no correspondence) and iterations [P] int32 (the fits run).  trials is the same tensor as iterations:
    summarize_registration(..., res["trials"]) and other callers read a count of model fits from either estimator.  No
    host sync, no workspace: graph-capturable."""
    ax, bx, m, ac, P, Ma, Mb = _corr_inputs(anchor_xyz, positive_xyz, match, anchor_count)
    threshold, division, settle, max_iterations = float(threshold), float(division), int(settle), int(max_iterations)
    if not threshold > 0.0 or not division > 1.0 or settle < 0 or not 1 <= max_iterations <= GNC_MAX_ITERATIONS:
        raise ValueError("need threshold > 0, division > 1, settle >= 0 and 1 <= max_iterations <= %d, got %r, %r, %r, %r"
                         % (GNC_MAX_ITERATIONS, threshold, division, settle, max_iterations))
    dev = ax.device
    Rt = torch.empty((P, 3, 4), dtype=torch.float64, device=dev)
    weights = torch.empty((P, Ma), dtype=torch.float64, device=dev)
    valid = torch.empty((P,), dtype=torch.int32, device=dev)
    inliers = torch.empty((P, Ma), dtype=torch.bool, device=dev)
    num_inliers = torch.empty((P,), dtype=torch.int32, device=dev)
    num_corr = torch.empty((P,), dtype=torch.int32, device=dev)
    iterations = torch.empty((P,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().dh3d_gnc_rigid(L.ptr(ax), ax.stride(1), L.ptr(bx), bx.stride(1), L.ptr(m), L.ptr(ac), P, Ma, Mb,
                                       threshold, division, settle, max_iterations, L.ptr(Rt), L.ptr(weights), L.ptr(valid),
                                       L.ptr(inliers), L.ptr(num_inliers), L.ptr(num_corr), L.ptr(iterations), L.stream_ptr()),
                "gnc_rigid")
        ratio = num_inliers.to(torch.float64) / num_corr.clamp(min=1).to(torch.float64)
        return dict(Rt=Rt, valid=valid.bool(), inliers=inliers, num_inliers=num_inliers, inlier_ratio=ratio, trials=iterations,
                    num_corr=num_corr, weights=weights, iterations=iterations)


_ESTIMATORS = {"ransac": (ransac_rigid, ("threshold", "confidence", "max_trials", "seed")),
               "gnc": (gnc_rigid, ("threshold", "division", "settle", "max_iterations"))}


def _estimator(fit_kw):
    """The estimator of register / register_fpfh / register_clouds out of their keywords: pops estimator= ("ransac", the
    default, or "gnc") and returns (the fit, the remaining keywords), which must be that estimator's own."""
    kw = dict(fit_kw)
    name = kw.pop("estimator", "ransac")
    if name not in _ESTIMATORS:
        raise ValueError('estimator must be "ransac" or "gnc", got %r' % (name,))
    fn, names = _ESTIMATORS[name]
    bad = sorted(set(kw) - set(names))
    if bad:
        raise ValueError('estimator="%s" takes the keywords %s, got %s' % (name, ", ".join(names), ", ".join(bad)))
    return fn, kw


def _match_options(match):
    """register's / register_fpfh's match=: None (dh3d_match_descriptors) or a dict of match_descriptors2's ratio / mutual."""
    if match is None:
        return None
    if not isinstance(match, dict) or set(match) - {"ratio", "mutual"}:
        raise ValueError("match must be None or a dict with the keys ratio and mutual, got %r" % (match,))
    return dict(match)


def _match_and_fit(desc_a, anchor_count, desc_b, positive_count, xyz_a, xyz_b, match, ransac_kw):
    """Descriptors to poses: match_descriptors (match None) or match_descriptors2 (a dict of its options, whose outputs join
    the result), then on the ids the estimator that ransac_kw names (estimator="ransac", the default: ransac_rigid;
    "gnc": gnc_rigid) with the rest of ransac_kw, which must be that estimator's keywords."""
    fit, fit_kw = _estimator(ransac_kw)
    opts = _match_options(match)
    if opts is None:
        ids, dist = match_descriptors(desc_a, anchor_count, desc_b, positive_count)
        more = {}
    else:
        more = match_descriptors2(desc_a, anchor_count, desc_b, positive_count, **opts)
        ids, dist = more["match"], more["dist1"]
    out = fit(xyz_a, xyz_b, ids, anchor_count, **fit_kw)
    out.update(more)
    out["match"], out["dist"] = ids, dist
    return out


def register(anchor_rows, anchor_count, positive_rows, positive_count, desc_dim=128, match=None, **ransac_kw):
    """Keypoint rows in, poses out: rows [P, M, C >= 3 + desc_dim] float32 as the model's xyz_feat_att_nms (C = 132) or a
    _nms_res.bin (utils.load_descriptor_bin) give them -- [x, y, z, descriptor(, score)] -- with counts [P] int32.  Matches
    every anchor keypoint to its nearest positive descriptor, then ransac_rigid (keyword arguments threshold, confidence,
    max_trials, seed).  Returns ransac_rigid's dict plus match / dist; everything stays on the device, no host sync.
    estimator="gnc" (default "ransac") fits with gnc_rigid instead: the keywords are then its threshold, division, settle,
    max_iterations, and the result gains weights / iterations; a keyword of the other estimator is a ValueError.
    match: None, or a dict of match_descriptors2's options, e.g. {"ratio": 0.9, "mutual": True} ({}: that entry, no
    filter): RANSAC then sees only the kept rows, match is the filtered list, dist is dist1 (of every row, kept or not) and
    match_descriptors2's other outputs (nn1, nn2, dist1, dist2, num_kept, with mutual rev / rev_dist) join the result."""
    _estimator(ransac_kw)  # (a wrong estimator or keyword is refused before anything is launched)
    a = _rows(anchor_rows, "anchor_rows", 3 + int(desc_dim))
    b = _rows(positive_rows, "positive_rows", 3 + int(desc_dim))
    return _match_and_fit(a[:, :, 3:3 + desc_dim], anchor_count, b[:, :, 3:3 + desc_dim], positive_count, a, b, match, ransac_kw)


ICP_MAX_POINTS, ICP_MAX_ITERATIONS, ICP_GRID_MAX = 131072, 256, 16384  # csrc/icp.hip kMaxPoints, kMaxIter, kGridMaxNa
_ICP_WS = {}  # (device, P, Na, Nb) -> the uint8 workspace of dh3d_icp_refine (its content carries nothing between calls)


def icp_plan(Na, Nb):
    """How refine_icp(path=0) associates a shape: "scan", "grid", or None for a shape the call refuses."""
    return {1: "scan", 2: "grid"}.get(L.lib().dh3d_icp_plan(int(Na), int(Nb)))


def refine_icp(anchor_points, positive_points, Rt, valid=None, anchor_count=None, positive_count=None, max_dist=1.0,
               iterations=20, path=0):
    """Dense point-to-point ICP of every pair from the pose Rt [P, 3, 4] float64 (anchor ~ R positive + t, ransac_rigid's
    convention): `iterations` times { nearest anchor point of every moved positive point within max_dist, float64
    least-squares fit over those pairs }, then one last association that describes the returned pose
    (include/dh3d_hip.h dh3d_icp_refine states every rule).  anchor_points [P, Na, >=3] and positive_points [P, Nb, >=3]
    float32 (the first three columns are read; column views are read in place); valid [P] bool / int32 or None (all);
    counts [P] int32 or None (all rows; prepare_clouds' num_valid).  path: 0 the plan's choice, 1 scan, 2 cell lists
    (Na <= 16384) -- the same result either way.  Returns a dict of device tensors: Rt [P, 3, 4] float64, valid [P] bool
    (the input's, and False where Rt had a non-finite entry; such pairs come back with Rt NaN, nn -1, num_corr 0, fitness 0,
    rmse NaN), nn [P, Nb] int32 (the anchor of every positive point under the returned pose, -1: none within max_dist),
    num_corr [P] int32, fitness [P] float64 (num_corr / positive count) and rmse [P] float64 (over the pairs of nn; NaN
    without any).  iterations = 0 evaluates the given pose.  No host sync: graph-capturable.  The workspace is kept per
    (device, P, Na, Nb) and carries nothing between calls; calls of one shape share it, so they belong on one stream (or on
    streams ordered against each other)."""
    return _icp_call(anchor_points, positive_points, Rt, valid, anchor_count, positive_count, max_dist, iterations, path, None)


def _icp_call(anchor_points, positive_points, Rt, valid, anchor_count, positive_count, max_dist, iterations, path, normals,
              positive_normals=None, epsilon=None):
    """The checks, the workspace and the call of refine_icp (normals None: dh3d_icp_refine), refine_icp_plane and
    refine_icp_gicp (positive_normals and epsilon given: dh3d_icp_refine_gicp)."""
    a = _rows(anchor_points, "anchor_points", 3)
    b = _rows(positive_points, "positive_points", 3)
    P, Na = a.shape[:2]
    dev = a.device
    if b.shape[0] != P or b.device != dev:
        raise ValueError("positive_points must be [%d, Nb, >=3] on %s, got %s on %s" % (P, dev, tuple(b.shape), b.device))
    Nb = b.shape[1]
    if not isinstance(Rt, torch.Tensor) or Rt.dtype != torch.float64 or not Rt.is_cuda or tuple(Rt.shape) != (P, 3, 4) \
            or Rt.device != dev:
        raise ValueError("Rt must be a float64 [%d, 3, 4] tensor on %s" % (P, dev))
    rt0 = Rt.contiguous()
    if valid is not None:
        if not isinstance(valid, torch.Tensor) or valid.dtype not in (torch.bool, torch.int32) or not valid.is_cuda \
                or tuple(valid.shape) != (P,) or valid.device != dev:
            raise ValueError("valid must be a bool or int32 [%d] tensor on %s" % (P, dev))
        valid = valid.to(torch.int32).contiguous()
    ac = None if anchor_count is None else _count(anchor_count, "anchor_count", P, dev)
    bc = None if positive_count is None else _count(positive_count, "positive_count", P, dev)
    max_dist, iterations, path = float(max_dist), int(iterations), int(path)
    if not 0.0 < max_dist < float("inf") or not 0 <= iterations <= ICP_MAX_ITERATIONS or path not in (0, 1, 2):
        raise ValueError("need a positive finite max_dist, 0 <= iterations <= %d and path 0, 1 or 2, got %r, %r, %r"
                         % (ICP_MAX_ITERATIONS, max_dist, iterations, path))
    if Na > ICP_MAX_POINTS or Nb > ICP_MAX_POINTS or (path == 2 and Na > ICP_GRID_MAX):
        raise ValueError("refine_icp: at most %d points per cloud (%d anchor points on path 2), got %d / %d"
                         % (ICP_MAX_POINTS, ICP_GRID_MAX, Na, Nb))
    lib = L.lib()
    key = (dev, P, Na, Nb)
    ws = _ICP_WS.get(key)
    if ws is None:
        nbytes = lib.dh3d_icp_refine_ws_bytes(P, Na, Nb)
        if nbytes == 0:
            raise ValueError("refine_icp: shape P = %d, Na = %d, Nb = %d is not served" % (P, Na, Nb))
        ws = _ICP_WS[key] = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    out_rt = torch.empty((P, 3, 4), dtype=torch.float64, device=dev)
    nn = torch.empty((P, Nb), dtype=torch.int32, device=dev)
    num_corr = torch.empty((P,), dtype=torch.int32, device=dev)
    fitness = torch.empty((P,), dtype=torch.float64, device=dev)
    rmse = torch.empty((P,), dtype=torch.float64, device=dev)
    ok = torch.empty((P,), dtype=torch.int32, device=dev)
    # per method: the entry, what it takes between anchor_count and the positive and behind `path`, its two extra outputs
    nrm = lambda t: (L.ptr(t), t.stride(1))
    if normals is None:
        what, entry, more, tail, extra = "refine_icp", lib.dh3d_icp_refine, (), (), ()
    elif positive_normals is None:
        what, entry, more, tail = "refine_icp_plane", lib.dh3d_icp_refine_plane, nrm(normals), ()
        extra = ("num_plane", "rmse_plane")
    else:
        what, entry, more, tail = "refine_icp_gicp", lib.dh3d_icp_refine_gicp, nrm(normals) + nrm(positive_normals), (epsilon,)
        extra = ("num_planar", "rmse_gicp")
    res = dict(Rt=out_rt, valid=ok, nn=nn, num_corr=num_corr, fitness=fitness, rmse=rmse)
    for name, dtype in zip(extra, (torch.int32, torch.float64)):
        res[name] = torch.empty((P,), dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        L.check(entry(L.ptr(a), a.stride(1), L.ptr(ac), *more, L.ptr(b), b.stride(1), L.ptr(bc), L.ptr(rt0), L.ptr(valid), P, Na, Nb,
                      max_dist, iterations, path, *tail, L.ptr(out_rt), L.ptr(nn), L.ptr(num_corr), L.ptr(fitness), L.ptr(rmse),
                      L.ptr(ok), *(L.ptr(res[name]) for name in extra), L.ptr(ws), ws.numel(), L.stream_ptr()), what)
    res["valid"] = ok.bool()
    return res


NORMALS_MAX_K = 64  # csrc/normals.hip kMaxK


def _viewpoint(viewpoint):
    v = [float(c) for c in viewpoint] if np.ndim(viewpoint) == 1 else []
    if len(v) != 3 or not all(np.isfinite(v)):
        raise ValueError("viewpoint must be three finite numbers, got %r" % (viewpoint,))
    return (L.c_double * 3)(*v)


def estimate_normals(points, num_valid=None, k=16, viewpoint=(0., 0., 0.), nbr=None):
    """Surface normals by PCA of every point's k nearest neighbours, flipped towards `viewpoint` (the reference's
    external/findPointNormals.m; include/dh3d_hip.h dh3d_estimate_normals states every rule).  points [P, N, >=3] float32
    on the GPU (the first three columns are read; column views are read in place), num_valid [P] int32 or None (all rows).
    nbr [P, N, K] int32, K <= 64: the neighbour ids of every point; None takes them from utils.batched_knn(points, k), whose
    lists hold the point itself.  Ids outside 0 .. num_valid - 1 are skipped, so, as batched_nms says of its padding, rows
    behind num_valid never enter a valid point's neighbourhood when the padding lies far away (prepare_clouds' rows of
    100000.0) and the cloud has at least k points: that equals the normals of the cropped cloud.  Returns a dict of device
    tensors: normals [P, N, 3] float32 (zero where fewer than 3 usable neighbours, coincident neighbours, or a row behind
    num_valid), curvature [P, N] float32 (smallest eigenvalue / their sum) and nbr (the ids used).  No host sync:
    graph-capturable."""
    x = _rows(points, "points", 3)
    P, N = x.shape[:2]
    dev = x.device
    cnt = None if num_valid is None else _count(num_valid, "num_valid", P, dev)
    if nbr is None:
        k = int(k)
        if not 1 <= k <= NORMALS_MAX_K:
            raise ValueError("estimate_normals: need 1 <= k <= %d, got %d" % (NORMALS_MAX_K, k))
        from .utils import batched_knn
        with torch.cuda.device(dev):
            nbr = batched_knn(x[:, :, :3].contiguous(), k)[0]
    nbr = L.require_cuda_i32(nbr, "nbr", 3)
    if nbr.shape[0] != P or nbr.shape[1] != N or nbr.device != dev or not 1 <= nbr.shape[2] <= NORMALS_MAX_K:
        raise ValueError("nbr must be int32 [%d, %d, 1..%d] on %s, got %s on %s"
                         % (P, N, NORMALS_MAX_K, dev, tuple(nbr.shape), nbr.device))
    if N > ICP_MAX_POINTS:
        raise ValueError("estimate_normals: at most %d points per cloud, got %d" % (ICP_MAX_POINTS, N))
    vp = _viewpoint(viewpoint)
    normals = torch.empty((P, N, 3), dtype=torch.float32, device=dev)
    curvature = torch.empty((P, N), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.lib().dh3d_estimate_normals(L.ptr(x), x.stride(1), L.ptr(cnt), L.ptr(nbr), P, N, nbr.shape[2], vp,
                                              L.ptr(normals), L.ptr(curvature), L.stream_ptr()), "estimate_normals")
    return dict(normals=normals, curvature=curvature, nbr=nbr)


def refine_icp_plane(anchor_points, positive_points, Rt, valid=None, anchor_count=None, positive_count=None, max_dist=1.0,
                     iterations=20, path=0, anchor_normals=None, normals_k=16, viewpoint=(0., 0., 0.)):
    """Dense point-to-plane ICP: refine_icp's inputs, association, loop and outputs with the fit that minimises the
    residuals along the anchor's normals (a linearised 6 x 6 solve per iteration; include/dh3d_hip.h dh3d_icp_refine_plane
    states every rule).  On street scenes it reaches in about 5 iterations what the point-to-point fit has not reached in
    20, because walls and ground no longer hold the pose back along themselves.  anchor_normals [P, Na, >=3] float32 is read
    in place (zero normals drop out of the fit); None computes it with estimate_normals(anchor_points, anchor_count,
    normals_k, viewpoint).  The result is refine_icp's dict -- rmse stays the point-to-point one, so the two methods
    compare -- plus num_plane [P] int32 (pairs with a normal in the last association) and rmse_plane [P] float64 (the rms
    residual along the normals; NaN without pairs).  No host sync: graph-capturable; the workspace is refine_icp's."""
    a = _rows(anchor_points, "anchor_points", 3)
    nrm = _normals_of(a, anchor_normals, anchor_count, "anchor_normals", normals_k, viewpoint)
    return _icp_call(a, positive_points, Rt, valid, anchor_count, positive_count, max_dist, iterations, path, nrm)


def _normals_of(points, normals, count, name, normals_k, viewpoint):
    """The normals [P, N, >=3] of a cloud batch: the caller's, read in place, or estimate_normals' when None."""
    if normals is None:
        normals = estimate_normals(points, count, normals_k, viewpoint)["normals"]
    nrm = _rows(normals, name, 3)
    if tuple(nrm.shape[:2]) != tuple(points.shape[:2]) or nrm.device != points.device:
        raise ValueError("%s must be [%d, %d, >=3] on %s, got %s on %s"
                         % (name, points.shape[0], points.shape[1], points.device, tuple(nrm.shape), nrm.device))
    return nrm


def refine_icp_gicp(anchor_points, positive_points, Rt, valid=None, anchor_count=None, positive_count=None, max_dist=1.0,
                    iterations=20, path=0, anchor_normals=None, normals_k=16, viewpoint=(0., 0., 0.), positive_normals=None,
                    epsilon=1e-3):
    """Dense generalized (plane-to-plane) ICP, Segal, Haehnel & Thrun 2009: refine_icp's inputs, association, loop and
    outputs with the fit that models both surfaces -- every point carries a covariance that is 1 across its normal and
    `epsilon` (0 < epsilon <= 1) along it, and every pair is weighted by the inverse of the anchor's covariance plus the moved
    positive's (a linearised 6 x 6 solve per iteration; include/dh3d_hip.h dh3d_icp_refine_gicp states every rule).
    anchor_normals [P, Na, >=3] and positive_normals [P, Nb, >=3] float32 are read in place; None computes that cloud's with
    estimate_normals(points, its count, normals_k, viewpoint).  Sign and length of a normal do not matter; a zero normal makes
    its point isotropic and keeps it in the fit, so with all normals zero (or epsilon = 1) this is a linearised point-to-point
    step.  The result is refine_icp's dict -- rmse stays the point-to-point one, so the three methods compare -- plus
    num_planar [P] int32 (pairs of the last association whose normals are both non-zero) and rmse_gicp [P] float64 (the rms
    of the weighted residual sqrt(d . M d); NaN without pairs).  No host sync: graph-capturable; the workspace is
    refine_icp's."""
    a = _rows(anchor_points, "anchor_points", 3)
    b = _rows(positive_points, "positive_points", 3)
    epsilon = float(epsilon)
    if not 0.0 < epsilon <= 1.0:
        raise ValueError("refine_icp_gicp: need 0 < epsilon <= 1, got %r" % (epsilon,))
    an = _normals_of(a, anchor_normals, anchor_count, "anchor_normals", normals_k, viewpoint)
    pn = _normals_of(b, positive_normals, positive_count, "positive_normals", normals_k, viewpoint)
    return _icp_call(a, b, Rt, valid, anchor_count, positive_count, max_dist, iterations, path, an, pn, epsilon)


FPFH_MAX_K, FPFH_COLS = 64, 36  # csrc/fpfh.hip kMaxK, kRow: 33 bins and three zero columns


def _max_dist(max_dist, what):
    d = 0.0 if max_dist is None else float(max_dist)
    if max_dist is not None and not 0.0 < d < float("inf"):
        raise ValueError("%s: max_dist must be None or positive and finite, got %r" % (what, max_dist))
    return d


def compute_fpfh(points, normals=None, num_valid=None, k=32, max_dist=None, nbr=None, ids=None, normals_k=16,
                 viewpoint=(0., 0., 0.)):
    """FPFH descriptors (Fast Point Feature Histograms, Rusu et al. 2009) from normals and neighbour lists: per point three
    11-bin histograms of the angles between its normal, its neighbours' normals and the lines to them (stage 1, the SPFH
    counts), then the 1 / d^2 weighted sum of the neighbours' histograms (stage 2); include/dh3d_hip.h dh3d_spfh_counts /
    dh3d_fpfh state every rule.  points [P, N, >=3] float32 on the GPU (the first three columns are read; column views are
    read in place), num_valid [P] int32 or None (all rows).  normals [P, N, >=3] float32, read in place and used as given
    (zero normals take their pairs out of the histograms); None computes them with estimate_normals(points, num_valid,
    normals_k, viewpoint).  nbr [P, N, K] int32, K <= 64: the neighbour ids of every point; None takes them from
    utils.batched_knn(points, k), whose lists hold the point itself (it never pairs with itself) -- with padding far away
    and at least k valid points no padded row enters a valid point's list, as estimate_normals says.  max_dist: None, or the
    radius beyond which a listed neighbour is left out.  ids [P, M] int32 or None: the points to describe (keypoints); an id
    outside 0 .. num_valid - 1 gives a zero row.  Returns a dict of device tensors: fpfh [P, M or N, 36] float32 (33 bins,
    a block of 11 sums to 200 when the point and one of its near neighbours have usable pairs, to 100 when only one of the
    two has, else to 0; columns 33-35 are zero so that match_descriptors reads the rows in place),
    counts [P, N, 36] uint8 (the SPFH counts of every point, byte 33 the number of pairs), normals and nbr as used.  No host
    sync: graph-capturable."""
    x = _rows(points, "points", 3)
    P, N = x.shape[:2]
    dev = x.device
    cnt = None if num_valid is None else _count(num_valid, "num_valid", P, dev)
    r = _max_dist(max_dist, "compute_fpfh")
    if N > ICP_MAX_POINTS:
        raise ValueError("compute_fpfh: at most %d points per cloud, got %d" % (ICP_MAX_POINTS, N))
    if nbr is None:
        k = int(k)
        if not 1 <= k <= FPFH_MAX_K:
            raise ValueError("compute_fpfh: need 1 <= k <= %d, got %d" % (FPFH_MAX_K, k))
        from .utils import batched_knn
        with torch.cuda.device(dev):
            nbr = batched_knn(x[:, :, :3].contiguous(), k)[0]
    nbr = L.require_cuda_i32(nbr, "nbr", 3)
    if nbr.shape[0] != P or nbr.shape[1] != N or nbr.device != dev or not 1 <= nbr.shape[2] <= FPFH_MAX_K:
        raise ValueError("nbr must be int32 [%d, %d, 1..%d] on %s, got %s on %s"
                         % (P, N, FPFH_MAX_K, dev, tuple(nbr.shape), nbr.device))
    if normals is None:
        normals = estimate_normals(x, cnt, normals_k, viewpoint)["normals"]
    nrm = _rows(normals, "normals", 3)
    if tuple(nrm.shape[:2]) != (P, N) or nrm.device != dev:
        raise ValueError("normals must be [%d, %d, >=3] on %s, got %s on %s" % (P, N, dev, tuple(nrm.shape), nrm.device))
    M = N
    if ids is not None:
        ids = L.require_cuda_i32(ids, "ids", 2)
        if ids.shape[0] != P or ids.shape[1] < 1 or ids.shape[1] > ICP_MAX_POINTS or ids.device != dev:
            raise ValueError("ids must be int32 [%d, 1..%d] on %s, got %s on %s"
                             % (P, ICP_MAX_POINTS, dev, tuple(ids.shape), ids.device))
        M = ids.shape[1]
    K = nbr.shape[2]
    counts = torch.empty((P, N, FPFH_COLS), dtype=torch.uint8, device=dev)
    fpfh = torch.empty((P, M, FPFH_COLS), dtype=torch.float32, device=dev)
    lib = L.lib()
    with torch.cuda.device(dev):
        L.check(lib.dh3d_spfh_counts(L.ptr(x), x.stride(1), L.ptr(nrm), nrm.stride(1), L.ptr(cnt), L.ptr(nbr), P, N, K, r,
                                     L.ptr(counts), L.stream_ptr()), "compute_fpfh (counts)")
        L.check(lib.dh3d_fpfh(L.ptr(x), x.stride(1), L.ptr(cnt), L.ptr(nbr), L.ptr(counts), L.ptr(ids), P, N, K, M, r,
                              L.ptr(fpfh), L.stream_ptr()), "compute_fpfh")
    return dict(fpfh=fpfh, counts=counts, normals=nrm, nbr=nbr)


ISS_MAX_POINTS = 16384  # csrc/iss.hip kMaxN (the cell table of dh3d_spatial_sort_cells); its kMaxKeep is KEYPOINT_MAX
_ISS_WS = {}  # (device, P, N, M) -> the uint8 workspace of dh3d_iss_keypoints (its content carries nothing between calls)


def cloud_resolution(points, num_valid=None):
    """The resolution of every cloud, [P] float32 on the device: the float64 mean over the valid rows of the distance to the
    nearest other row (column 1 of utils.batched_knn(points, 2); with padding far away no padded row is a valid row's nearest),
    0 for fewer than 2 valid rows.  points [P, N, >=3] float32 on the GPU, num_valid [P] int32 or None (all rows).  No host
    sync."""
    x = _rows(points, "points", 3)
    P, N = x.shape[:2]
    dev = x.device
    cnt = None if num_valid is None else _count(num_valid, "num_valid", P, dev)
    if N < 2:
        return torch.zeros((P,), dtype=torch.float32, device=dev)
    from .utils import batched_knn
    with torch.cuda.device(dev):
        near = batched_knn(x[:, :, :3].contiguous(), 2)[1][:, :, 1].to(torch.float64)
    n = torch.full((P,), N, dtype=torch.int64, device=dev) if cnt is None else cnt.clamp(0, N).to(torch.int64)
    inside = torch.arange(N, device=dev)[None, :] < n[:, None]
    mean = torch.where(inside, near, torch.zeros_like(near)).sum(dim=1) / n.clamp(min=1).to(torch.float64)
    return torch.where(n >= 2, mean, torch.zeros_like(mean)).to(torch.float32)


def _iss_radius(r, name, P, dev):
    """A radius of iss_keypoints as a [P] float32 device tensor: a number for all clouds, or the caller's tensor."""
    if isinstance(r, torch.Tensor):
        if r.dtype != torch.float32 or not r.is_cuda or tuple(r.shape) != (P,) or r.device != dev:
            raise ValueError("%s must be a number or a float32 [%d] tensor on %s" % (name, P, dev))
        return r
    return torch.full((P,), float(r), dtype=torch.float32, device=dev)


def iss_keypoints(points, num_valid=None, salient_radius=None, non_max_radius=None, gamma_21=0.975, gamma_32=0.975,
                  min_neighbors=5, max_keypoints=4096, saliency=None, eigenvalues=False):
    """ISS keypoints (Intrinsic Shape Signatures, Zhong 2009; Open3D's compute_iss_keypoints) of every cloud, on the device:
    a point is salient where the float64 scatter of all points within salient_radius has eigenvalues l1 >= l2 >= l3 with l2 <
    gamma_21 * l1 and l3 < gamma_32 * l2, its saliency being l3; it is a keypoint where no point within non_max_radius is more
    salient (ties to the lowest index) and both balls hold at least min_neighbors points (include/dh3d_hip.h
    dh3d_iss_keypoints states every rule).  points [P, N, >=3] float32 on the GPU (the first three columns are read; column
    views are read in place), N <= 16384; num_valid [P] int32 or None (all rows).  A radius is a number, a [P] float32 device
    tensor, or None: 6 x (salient) and 4 x (non-max) cloud_resolution(points, num_valid), computed on the device.
    saliency [P, N] float32: the caller's saliencies in place of the eigenvalue rule (the suppression and the selection
    alone).  Returns a dict of device tensors: ids [P, max_keypoints] int32 (the most salient first, -1 behind them: what
    register_fpfh(keypoint_ids=...) takes), count [P] int32, saliency [P, N] float32, num_neighbors [P, N, 2] int32 (the
    points within the salient and the non-max radius, the point itself counted), eigenvalues [P, N, 3] float64 (l1 l2 l3;
    None unless asked for) and radii [P, 2] float32 as used.  No host sync: graph-capturable.  The workspace is kept per
    (device, P, N, max_keypoints) and carries nothing between calls; calls of one shape belong on one stream."""
    x = _rows(points, "points", 3)
    P, N = x.shape[:2]
    dev = x.device
    cnt = None if num_valid is None else _count(num_valid, "num_valid", P, dev)
    gamma_21, gamma_32, min_neighbors, M = float(gamma_21), float(gamma_32), int(min_neighbors), int(max_keypoints)
    if not 0.0 < gamma_21 <= 1.0 or not 0.0 < gamma_32 <= 1.0:
        raise ValueError("iss_keypoints: gamma_21 and gamma_32 must lie in (0, 1], got %r, %r" % (gamma_21, gamma_32))
    if min_neighbors < 1:
        raise ValueError("iss_keypoints: min_neighbors must be at least 1, got %d" % min_neighbors)
    if N > ISS_MAX_POINTS:
        raise ValueError("iss_keypoints: at most %d points per cloud, got %d" % (ISS_MAX_POINTS, N))
    if not 1 <= M <= KEYPOINT_MAX:
        raise ValueError("iss_keypoints: max_keypoints must lie in 1 .. %d, got %d" % (KEYPOINT_MAX, M))
    sal_in = None
    if saliency is not None:
        sal_in = L.require_cuda_f32(saliency, "saliency", 2)
        if tuple(sal_in.shape) != (P, N) or sal_in.device != dev:
            raise ValueError("saliency must be float32 [%d, %d] on %s, got %s on %s" % (P, N, dev, tuple(sal_in.shape), sal_in.device))
    if salient_radius is None or non_max_radius is None:
        res = cloud_resolution(x, cnt)
    rs = res * 6.0 if salient_radius is None else _iss_radius(salient_radius, "salient_radius", P, dev)
    rn = res * 4.0 if non_max_radius is None else _iss_radius(non_max_radius, "non_max_radius", P, dev)
    radii = torch.stack((rs, rn), dim=1).contiguous()
    lib = L.lib()
    key = (dev, P, N, M)
    ws = _ISS_WS.get(key)
    if ws is None:
        nbytes = lib.dh3d_iss_keypoints_ws_bytes(P, N, M)
        if nbytes == 0:
            raise ValueError("iss_keypoints: shape P = %d, N = %d, max_keypoints = %d is not served" % (P, N, M))
        ws = _ISS_WS[key] = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    sal = torch.empty((P, N), dtype=torch.float32, device=dev)
    nbr = torch.empty((P, N, 2), dtype=torch.int32, device=dev)
    lam = torch.empty((P, N, 3), dtype=torch.float64, device=dev) if eigenvalues else None
    ids = torch.empty((P, M), dtype=torch.int32, device=dev)
    count = torch.empty((P,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.dh3d_iss_keypoints(L.ptr(x), x.stride(1), L.ptr(cnt), L.ptr(radii), L.ptr(sal_in), P, N, gamma_21, gamma_32,
                                       min_neighbors, M, L.ptr(sal), L.ptr(nbr), L.ptr(lam), L.ptr(ids), L.ptr(count), L.ptr(ws),
                                       ws.numel(), L.stream_ptr()), "iss_keypoints")
    return dict(ids=ids, count=count, saliency=sal, num_neighbors=nbr, eigenvalues=lam, radii=radii)


def _fpfh_keypoints(x, cnt, keypoints, keypoint_ids, name):
    """The keypoints of register_fpfh on one batch of clouds: (ids [P, M] int32 or None for all points, count [P] int32)."""
    P, N = x.shape[:2]
    dev = x.device
    full = torch.full((P,), N, dtype=torch.int32, device=dev) if cnt is None else cnt.clamp(0, N)
    if isinstance(keypoints, dict):  # a detector: {"method": "iss", ...iss_keypoints' keywords}
        kw = dict(keypoints)
        method = kw.pop("method", None)
        if method != "iss":
            raise ValueError('%s keypoints: method must be "iss", got %r' % (name, method))
        if keypoint_ids is not None:
            raise ValueError("%s: give a keypoint detector or keypoint_ids, not both" % name)
        res = iss_keypoints(x, cnt, **kw)
        return res["ids"], res["count"]
    if keypoint_ids is not None:
        ids = L.require_cuda_i32(keypoint_ids, name + " keypoint_ids", 2)
        if ids.shape[0] != P or ids.device != dev:
            raise ValueError("%s keypoint_ids must be int32 [%d, M] on %s, got %s" % (name, P, dev, tuple(ids.shape)))
        _check_m(ids.shape[1], name + " keypoint_ids")
        return ids, (ids >= 0).sum(dim=1).to(torch.int32)       # (-1 padding at the tail, as batched_nms / FPS give it)
    if keypoints is None and N <= KEYPOINT_MAX:
        return None, full
    M = KEYPOINT_MAX if keypoints is None else int(keypoints)
    if M < 1:
        raise ValueError("keypoints must be at least 1, got %r" % (keypoints,))
    _check_m(M, name + " keypoints")
    r = torch.arange(M, dtype=torch.int64, device=dev)
    ids = ((r[None, :] * full[:, None].to(torch.int64)) // M).to(torch.int32)    # ids[p, r] = (r * n_p) // M, on the device
    return ids, torch.where(full > 0, torch.full_like(full, M), torch.zeros_like(full))


def register_fpfh(anchor_points, positive_points, num_valid=None, keypoints=None, keypoint_ids=None, k=32, max_dist=None,
                  refine=None, **ransac_kw):
    """Registration of cloud pairs from geometry alone, no model and no weights: compute_fpfh on both batches (normals by
    estimate_normals at k = 16, the k nearest neighbours of utils.batched_knn, max_dist as compute_fpfh's), match_descriptors
    on the 36-column rows of the keypoints, ransac_rigid (its keywords threshold, confidence, max_trials, seed; or with
    estimator="gnc" gnc_rigid and its keywords, as register takes them), and refine_pose exactly as register_clouds wires it.  anchor_points [P, Na, >=3] and positive_points [P, Nb, >=3] float32 on
    the GPU.  num_valid: None, one int32 [P] tensor for both batches, or a pair (anchor, positive).  The keypoints of a cloud:
    every point when it has at most 4096 rows and nothing is asked; otherwise `keypoints` = M (default 4096) of them spread
    over the valid rows, ids[p, r] = (r * n_p) // M, computed on the device; or the caller's keypoint_ids -- one int32 [P, M]
    tensor or a pair (anchor, positive), e.g. farthest-point picks, -1 padded at the tail.  keypoints may be a pair too, and
    in place of a number a detector: {"method": "iss", ...iss_keypoints' keywords} runs iss_keypoints on the cloud (N <= 16384)
    and goes on as with its ids as keypoint_ids.
    match (a keyword beside ransac_rigid's): None, or a dict of match_descriptors2's options as register takes it
    ({"ratio": 0.9, "mutual": True}); a pair the filters leave fewer than three correspondences comes back valid=False.
    refine: None, True or a dict of refine_pose keywords, on the full clouds.  Returns register_clouds' keys: ransac_rigid's
    dict plus match / dist (indices into the keypoint lists), and with refine Rt_ransac, fitness, rmse, num_corr_icp, nn (and
    num_plane, rmse_plane with method="plane"; num_planar, rmse_gicp with method="gicp"); plus anchor_ids / positive_ids (the
    keypoint ids, None: all points).  No host sync."""
    rkw = _refine_kw(refine)
    match = ransac_kw.pop("match", None)
    _estimator(ransac_kw)  # (a wrong estimator or keyword is refused before normals and FPFH are launched)
    pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    nv, kp, kid = pair(num_valid), pair(keypoints), pair(keypoint_ids)
    rows, cnts, idl = [], [], []
    for s, (pts, name) in enumerate(((anchor_points, "anchor"), (positive_points, "positive"))):
        x = _rows(pts, name + "_points", 3)
        c = None if nv[s] is None else _count(nv[s], "num_valid", x.shape[0], x.device)
        ids, kc = _fpfh_keypoints(x, c, kp[s], kid[s], name)
        desc = compute_fpfh(x, None, c, k=k, max_dist=max_dist, ids=ids)["fpfh"]
        if ids is None:
            xyz = x
        else:
            from .pm import gather_rows
            xyz = gather_rows(x[:, :, :3], ids, kc)
        rows.append((xyz, desc))
        cnts.append(kc)
        idl.append(ids)
    out = _match_and_fit(rows[0][1], cnts[0], rows[1][1], cnts[1], rows[0][0], rows[1][0], match, ransac_kw)
    out["anchor_ids"], out["positive_ids"] = idl
    if rkw is not None:
        _merge_refinement(out, refine_pose(anchor_points, positive_points, out["Rt"], out["valid"], anchor_count=nv[0],
                                           positive_count=nv[1], **rkw))
    return out


def _merge_refinement(out, icp, before="Rt_ransac", dense=True):
    """A refine_pose result `icp` into the registration result `out`, in place: Rt becomes the refined pose and the pose so
    far moves to `before`; fitness and rmse, and the method's own rmse_plane / rmse_gicp.  dense (register_fpfh,
    register_clouds): also num_corr_icp, nn and the method's count num_plane / num_planar."""
    out[before], out["Rt"] = out["Rt"], icp["Rt"]
    names = dict(fitness="fitness", rmse="rmse", rmse_plane="rmse_plane", rmse_gicp="rmse_gicp")
    if dense:
        names.update(num_corr="num_corr_icp", nn="nn", num_plane="num_plane", num_planar="num_planar")
    out.update((names[k], v) for k, v in icp.items() if k in names)


def refine_pose(anchor_points, positive_points, Rt, valid=None, anchor_count=None, positive_count=None, method="point", **kw):
    """The dense refinement behind register_clouds / PlaceIndex.localize(refine=...): method "point" is refine_icp (its
    keywords max_dist, iterations, path), "plane" is refine_icp_plane (those plus anchor_normals, normals_k, viewpoint),
    "gicp" is refine_icp_gicp (those plus positive_normals, epsilon)."""
    fns = {"point": refine_icp, "plane": refine_icp_plane, "gicp": refine_icp_gicp}
    if method not in fns:
        raise ValueError('method must be "point", "plane" or "gicp", got %r' % (method,))
    fn = fns[method]
    return fn(anchor_points, positive_points, Rt, valid, anchor_count=anchor_count, positive_count=positive_count, **kw)


def _refine_kw(refine):
    """refine: None / False (no refinement), True (refine_icp's defaults) or a dict of refine_pose keywords: refine_icp's,
    or method="plane" and refine_icp_plane's, or method="gicp" and refine_icp_gicp's."""
    if refine is None or refine is False:
        return None
    if refine is True:
        return {}
    if isinstance(refine, dict):
        return dict(refine)
    raise ValueError("refine must be None, True or a dict of refine_icp keywords, got %r" % (refine,))


def register_clouds(model, anchor_points, positive_points, num_valid=None, refine=None, **kw):
    """Both batches of clouds [P, N, 3] through model.forward(fetch=("kp_count", "xyz_feat_att_nms")) (config.detection),
    then register on the keypoints.  num_valid: None, one int32 [P] tensor for both batches, or a pair (anchor, positive).
    refine: None, True or a dict of refine_icp keywords -- the RANSAC pose is then refined by dense ICP of the full clouds
    (num_valid as the counts): Rt is the refined pose and the result gains Rt_ransac (the keypoint fit), fitness, rmse,
    num_corr_icp and nn; valid stays the RANSAC fit's.  A dict with method="plane" (and refine_icp_plane's keywords) refines
    point-to-plane instead and adds num_plane and rmse_plane; method="gicp" (and refine_icp_gicp's keywords) refines by
    generalized ICP and adds num_planar and rmse_gicp.  Other keywords go to register: desc_dim, match={"ratio": ...,
    "mutual": ...}, estimator= and that estimator's (ransac_rigid's by default)."""
    if not getattr(model.config, "detection", False):
        raise ValueError("register_clouds needs a model with config.detection (the keypoint outputs)")
    rkw = _refine_kw(refine)
    _estimator({k: v for k, v in kw.items() if k not in ("desc_dim", "match")})  # (refused before the forwards run)
    nv_a, nv_b = num_valid if isinstance(num_valid, (tuple, list)) else (num_valid, num_valid)
    fetch = ("kp_count", "xyz_feat_att_nms")
    oa = model.forward(anchor_points, fetch=fetch, num_valid=nv_a)
    ob = model.forward(positive_points, fetch=fetch, num_valid=nv_b)
    out = register(oa["xyz_feat_att_nms"], oa["kp_count"], ob["xyz_feat_att_nms"], ob["kp_count"], **kw)
    if rkw is not None:
        _merge_refinement(out, refine_pose(anchor_points, positive_points, out["Rt"], out["valid"], anchor_count=nv_a,
                                           positive_count=nv_b, **rkw))
    return out


def _host64(t):
    return t.detach().cpu().numpy().astype(np.float64) if isinstance(t, torch.Tensor) else np.asarray(t, np.float64)


def transform_errors(T_gt, T_est, valid=None):
    """compareTransform (common/Utils.m) with GetEulerAngles, float64 on the host.  T_gt, T_est [P, 3 or 4, 4] (tensors or
    arrays), valid [P] (None: all).  delta_t = |t_gt - t_est|; dR = R_gt^T R_est, ry = asin(dR[0, 2]), rz = acos(dR[0, 0] /
    cos ry), rx = acos(dR[2, 2] / cos ry) evaluated in complex128 with abs taken, as MATLAB does when rounding pushes an
    argument past +-1; delta_deg = (|rx| + |ry| + |rz|) * 180 / pi.  Pairs without an estimate get (3, 6), eval_align.m's
    catch.  Returns (delta_t [P], delta_deg [P]) float64."""
    G = _host64(T_gt)[:, :3, :]
    E = _host64(T_est)[:, :3, :]
    if G.shape != E.shape or G.shape[1:] != (3, 4):
        raise ValueError("T_gt and T_est must be [P, 3 or 4, 4], got %s / %s" % (G.shape, E.shape))
    ok = np.ones(len(G), bool) if valid is None else _host64(valid).astype(bool)
    ok &= np.isfinite(E).all(axis=(1, 2))
    dt = np.linalg.norm(G[:, :, 3] - E[:, :, 3], axis=1)
    dR = np.einsum("pki,pkj->pij", G[:, :, :3], E[:, :, :3]).astype(np.complex128)
    with np.errstate(invalid="ignore", divide="ignore"):  # (pairs without an estimate are NaN here; replaced below)
        ry = np.arcsin(dR[:, 0, 2])
        rz = np.arccos(dR[:, 0, 0] / np.cos(ry))
        rx = np.arccos(dR[:, 2, 2] / np.cos(ry))
    ddeg = (np.abs(rx) + np.abs(ry) + np.abs(rz)) * 180.0 / np.pi
    return np.where(ok, dt, 3.0), np.where(ok, ddeg, 6.0)


def summarize_registration(delta_t, delta_deg, inlier_ratio, trials):
    """eval_align.m's summary: a pair fails when delta_t > 2 or delta_deg > 5; over the successful pairs only, the mean
    inlier ratio, the mean trial count and mean / std (N - 1) of RTE (delta_t) and RRE (delta_deg)."""
    dt, dd = _host64(delta_t), _host64(delta_deg)
    ir, tr = _host64(inlier_ratio), _host64(trials)
    ok = ~((dt > 2) | (dd > 5))
    n_ok = int(ok.sum())

    def std(v):
        return float(np.std(v, ddof=1)) if len(v) > 1 else float("nan")
    return dict(num_pairs=len(dt), num_failed=len(dt) - n_ok, success_rate=100.0 * n_ok / max(len(dt), 1),
                mean_inlier_ratio=float(ir[ok].mean()) if n_ok else float("nan"),
                mean_trials=float(tr[ok].mean()) if n_ok else float("nan"),
                rte_mean=float(dt[ok].mean()) if n_ok else float("nan"), rte_std=std(dt[ok]),
                rre_mean=float(dd[ok].mean()) if n_ok else float("nan"), rre_std=std(dd[ok]))
