"""Place retrieval on the device: the exact float64 top-k search of global descriptors (csrc/retrieval.hip), a
fixed-capacity map of places whose fill level lives on the device, and the relocalisation loop on top of it.

The reference retrieves with scipy's cKDTree on the host (evaluate/global_eval/evaluation_retrieval.py:37-40).  Here the
search is one call that forms no [Q, R] matrix, ranks in float64 by (distance, map id) -- include/dh3d_hip.h dh3d_retrieve
states every rule -- and never tells the host how many places the map holds, so a captured graph keeps serving a map that
grows inside its capacity.

    idx, dist = search_descriptors(ref, qry, k)                   # int32 [Q, k] (-1 past the map's end), float64 [Q, k]
    idx, dist2 = search_descriptors_sq(ref, qry, k)               # the squared distances the ranks were made on
    index = PlaceIndex(dim=256, capacity=65536, device="cuda", keypoints=512)
    index.add(globaldesc, pos, kp_rows=xyz_feat_att_nms, kp_count=kp_count)
    idx, dist = index.search(query_desc, 25)
    res = index.localize(query_desc, query_rows, query_count, k=5)  # place [Q], Rt [Q, 3, 4], num_inliers, rank, ...
    res = relocalize_clouds(global_model, local_model, index, points, k=5)
    index = PlaceIndex(..., points=8192); index.add(..., cloud=points, cloud_count=num_valid)   # 12 * points bytes a place
    res = relocalize_clouds(global_model, local_model, index, points, k=5, refine=True)  # + dense ICP: Rt, fitness, rmse
"""
import torch

from . import _lib as L
from . import registration

DESC_MAX = 256  # descriptor length limit of dh3d_retrieve
K_MAX = 64      # neighbours per query


def retrieve_plan(Q, R, D, k):
    """(S, slice_rows) of dh3d_retrieve for a shape: the map is cut into S slices of slice_rows rows (the last may be
    shorter) that are scanned side by side; S = 1 is a single launch.  None for a shape the call refuses."""
    S = L.lib().dh3d_retrieve_plan(int(Q), int(R), int(D), int(k))
    if S < 0:
        return None
    tiles = (int(R) + 255) // 256
    return S, 256 * ((tiles + S - 1) // S)


def _rows2(t, name):
    """A float32 [n, D] GPU tensor whose rows can be read with one element stride (a column slice is read in place)."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2:
        raise ValueError("%s must be a float32 [n, D] tensor" % name)
    if not t.is_cuda:
        raise ValueError("%s must live on the GPU (the HIP path has no CPU fallback)" % name)
    if t.shape[0] == 0 or t.shape[1] == 0:
        raise ValueError("%s must not be empty, got shape %s" % (name, tuple(t.shape)))
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t


def search_descriptors(ref, qry, k, ref_count=None):
    """search_descriptors_sq with Euclidean distances: (idx int32 [Q, k], dist float64 [Q, k] = sqrt(dist2))."""
    idx, dist2 = search_descriptors_sq(ref, qry, k, ref_count)
    return idx, dist2.sqrt_()


def search_descriptors_sq(ref, qry, k, ref_count=None):
    """The k nearest rows of `ref` [R, D] for every row of `qry` [Q, D] (float32 on the GPU; column views with a
    contiguous last dimension are read in place), ascending by (float64 squared distance summed over the columns in
    order, map id).  ref_count: None or an int32 [1] device tensor -- only rows below clamp(ref_count, 0, R) exist and the
    others are never read.  Returns (idx int32 [Q, k], dist2 float64 [Q, k], the squared distances); entries past the map's end are -1 / +inf.
    D <= 256, a multiple of 4; k <= 64 (else ValueError).  No host sync: graph-capturable."""
    r = _rows2(ref, "ref")
    q = _rows2(qry, "qry")
    k = int(k)
    if q.shape[1] != r.shape[1] or q.device != r.device:
        raise ValueError("qry must be [Q, %d] on %s, got %s on %s" % (r.shape[1], r.device, tuple(q.shape), q.device))
    R, D, Q = r.shape[0], r.shape[1], q.shape[0]
    if D > DESC_MAX or D % 4 or not 0 < k <= K_MAX:
        raise ValueError("descriptor length must be a multiple of 4 up to %d and 1 <= k <= %d, got D = %d, k = %d"
                         % (DESC_MAX, K_MAX, D, k))
    if ref_count is not None:
        ref_count = L.require_cuda_i32(ref_count, "ref_count", 1)
        if ref_count.shape[0] != 1 or ref_count.device != r.device:
            raise ValueError("ref_count must be int32 [1] on %s" % (r.device,))
    lib = L.lib()
    ws_bytes = lib.dh3d_retrieve_ws_bytes(Q, R, D, k)
    if ws_bytes == 0:
        raise ValueError("search_descriptors: shape Q = %d, R = %d, D = %d, k = %d is not served" % (Q, R, D, k))
    with torch.cuda.device(r.device):
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=r.device)
        idx = torch.empty((Q, k), dtype=torch.int32, device=r.device)
        dist2 = torch.empty((Q, k), dtype=torch.float64, device=r.device)
        L.check(lib.dh3d_retrieve(L.ptr(r), r.stride(0), L.ptr(ref_count), L.ptr(q), q.stride(0), Q, R, D, k, L.ptr(idx),
                                  L.ptr(dist2), L.ptr(ws), ws_bytes, L.stream_ptr()), "search_descriptors")
    return idx, dist2


class PlaceIndex:
    """A fixed-capacity map of places on the device: desc [capacity, dim] float32 global descriptors, pos [capacity, 2]
    float64 (northing, easting), count int32 [1] (the fill level, on the device), and with keypoints = M > 0 the places'
    keypoint rows kp_rows [capacity, M, row_dim] float32 ([x, y, z, descriptor(, score)] as the model's xyz_feat_att_nms)
    with kp_count [capacity] int32, and with points = N > 0 the places' clouds cloud [capacity, N, 3] float32 with
    cloud_count [capacity] int32 -- what localize(refine=...) runs the dense ICP against; it costs 12 * points bytes a
    place (96 KiB at 8192 points: 6 GiB for a map of 65536 places).  Buffers never move, so a graph captured around search / localize keeps serving the map
    while add() fills it."""

    def __init__(self, dim=256, capacity=4096, device="cuda", keypoints=0, row_dim=132, points=0):
        dim, capacity, keypoints, row_dim, points = int(dim), int(capacity), int(keypoints), int(row_dim), int(points)
        if dim <= 0 or dim > DESC_MAX or dim % 4 or capacity <= 0 or keypoints < 0 or points < 0:
            raise ValueError("need 0 < dim <= %d, a multiple of 4, capacity > 0, keypoints >= 0 and points >= 0" % DESC_MAX)
        if torch.device(device).type != "cuda":
            raise ValueError("PlaceIndex lives on the GPU (the HIP path has no CPU fallback), got %s" % (device,))
        self.dim, self.capacity, self.keypoints, self.row_dim, self.points = dim, capacity, keypoints, row_dim, points
        self.desc = torch.zeros((capacity, dim), dtype=torch.float32, device=device)
        self.device = self.desc.device  # with its index ("cuda" -> cuda:0): what the tensors handed to search / localize carry
        self.pos = torch.zeros((capacity, 2), dtype=torch.float64, device=self.device)
        self.count = torch.zeros((1,), dtype=torch.int32, device=self.device)
        self.kp_rows = self.kp_count = None
        if keypoints:
            self.kp_rows = torch.zeros((capacity, keypoints, row_dim), dtype=torch.float32, device=self.device)
            self.kp_count = torch.zeros((capacity,), dtype=torch.int32, device=self.device)
        self.cloud = self.cloud_count = None
        if points:
            self.cloud = torch.zeros((capacity, points, 3), dtype=torch.float32, device=self.device)
            self.cloud_count = torch.zeros((capacity,), dtype=torch.int32, device=self.device)
        self._n = 0  # host mirror of count: add() needs no device -> host copy

    def __len__(self):
        return self._n

    def add(self, desc, pos=None, kp_rows=None, kp_count=None, cloud=None, cloud_count=None):
        """Append n places: desc [n, dim]; pos [n, 2] (None: zeros); with keypoints, kp_rows [n, M' <= M, row_dim] and
        kp_count [n]; with points, cloud [n, N' <= N, 3] and cloud_count [n] (None: N' each).  Returns the ids (a range).  Raises when the map is full; no device -> host sync."""
        desc = torch.as_tensor(desc, dtype=torch.float32)
        if desc.dim() != 2 or desc.shape[1] != self.dim:
            raise ValueError("desc must be [n, %d], got %s" % (self.dim, tuple(desc.shape)))
        n, o = desc.shape[0], self._n
        if o + n > self.capacity:
            raise ValueError("PlaceIndex is full: %d places + %d > capacity %d" % (o, n, self.capacity))
        if self.keypoints and (kp_rows is None or kp_count is None):
            raise ValueError("this PlaceIndex holds keypoints: add() needs kp_rows and kp_count")
        if not self.keypoints and (kp_rows is not None or kp_count is not None):
            raise ValueError("this PlaceIndex was built with keypoints = 0")
        if self.keypoints:
            kp_rows = torch.as_tensor(kp_rows, dtype=torch.float32)
            kp_count = torch.as_tensor(kp_count, dtype=torch.int32)
            if kp_rows.dim() != 3 or kp_rows.shape[0] != n or kp_rows.shape[1] > self.keypoints or kp_rows.shape[2] != self.row_dim:
                raise ValueError("kp_rows must be [%d, <= %d, %d], got %s" % (n, self.keypoints, self.row_dim, tuple(kp_rows.shape)))
            if tuple(kp_count.shape) != (n,):
                raise ValueError("kp_count must be [%d], got %s" % (n, tuple(kp_count.shape)))
        if self.points and cloud is None:
            raise ValueError("this PlaceIndex holds clouds: add() needs cloud")
        if not self.points and (cloud is not None or cloud_count is not None):
            raise ValueError("this PlaceIndex was built with points = 0")
        if self.points:
            cloud = torch.as_tensor(cloud, dtype=torch.float32)
            if cloud.dim() != 3 or cloud.shape[0] != n or cloud.shape[1] > self.points or cloud.shape[2] != 3:
                raise ValueError("cloud must be [%d, <= %d, 3], got %s" % (n, self.points, tuple(cloud.shape)))
            if cloud_count is not None:
                cloud_count = torch.as_tensor(cloud_count, dtype=torch.int32)
                if tuple(cloud_count.shape) != (n,):
                    raise ValueError("cloud_count must be [%d], got %s" % (n, tuple(cloud_count.shape)))
        if pos is not None:
            pos = torch.as_tensor(pos, dtype=torch.float64)
            if tuple(pos.shape) != (n, 2):
                raise ValueError("pos must be [%d, 2], got %s" % (n, tuple(pos.shape)))
            self.pos[o:o + n].copy_(pos)
        if self.keypoints:
            m = kp_rows.shape[1]
            self.kp_rows[o:o + n, :m].copy_(kp_rows)
            self.kp_rows[o:o + n, m:].zero_()
            self.kp_count[o:o + n].copy_(kp_count.clamp(0, m))
        if self.points:
            m = cloud.shape[1]
            self.cloud[o:o + n, :m].copy_(cloud)
            self.cloud[o:o + n, m:].zero_()
            if cloud_count is None:
                self.cloud_count[o:o + n].fill_(m)
            else:
                self.cloud_count[o:o + n].copy_(cloud_count.clamp(0, m))
        self.desc[o:o + n].copy_(desc)
        self._n = o + n
        self.count.fill_(self._n)  # after the rows: a search ordered after this add sees complete places
        return range(o, o + n)

    def search(self, qry, k):
        """search_descriptors over the places added so far (the device count decides, not the host mirror)."""
        return search_descriptors(self.desc, qry, k, ref_count=self.count)

    def localize(self, query_desc, query_rows, query_count, k=5, desc_dim=128, refine=None, query_cloud=None,
                 query_cloud_count=None, **ransac_kw):
        """Retrieve k candidate places per query, register the query's keypoints against every candidate's in ONE batch of
        Q * k pairs (registration.register: anchor = the place's keypoints, positive = the query's, so Rt maps query
        coordinates into the place's frame, place ~ R query + t) and keep, per query, the candidate with the most inliers;
        ties go to the better retrieval rank; candidates with idx == -1 or without a valid fit never win.
        query_desc [Q, dim], query_rows [Q, Mq, row_dim], query_count [Q] int32.  Returns a dict of device tensors: place [Q]
        int32 (-1: no candidate is valid), rank [Q] int32 (the winner's retrieval rank, -1), Rt [Q, 3, 4] float64 (NaN where
        place is -1), num_inliers [Q] int32 (0 there), inlier_ratio [Q] float64, inliers [Q, M] bool (the winner's mask over
        the place's keypoints), pos [Q, 2] float64 (the place's position, NaN there), idx / dist [Q, k] (the retrieval).
        refine: None, True or a dict of registration.refine_icp keywords -- after the vote the winner's pose (and only the
        winner's) is refined by dense ICP of query_cloud [Q, N, >=3] (query_cloud_count [Q] int32 or None) against the
        winner's stored cloud, gathered by place id on the device; a query without a winner goes in as invalid.  Rt is then
        the refined pose and the result gains Rt_ransac (the keypoint fit), fitness and rmse (the dense overlap: the check on
        the retrieved place); a dict with method="plane" refines point-to-plane (registration.refine_icp_plane's keywords;
        the winner's normals are computed per call) and adds rmse_plane; method="gicp" refines by generalized ICP
        (registration.refine_icp_gicp's keywords; both clouds' normals are computed per call) and adds rmse_gicp.  Needs an index built with points > 0 (else
        ValueError).  Other keywords go to registration.register: ransac_rigid's, and match={"ratio": ..., "mutual": ...} (the
        ratio test and the mutual check ahead of RANSAC); estimator="gnc" and gnc_rigid's keywords fit every candidate with
        the deterministic estimator instead.  No host sync."""
        if not self.keypoints:
            raise ValueError("localize needs a PlaceIndex built with keypoints > 0")
        rkw = registration._refine_kw(refine)
        if rkw is not None:
            if not self.points:
                raise ValueError("localize(refine=...) needs a PlaceIndex built with points > 0 (the places' clouds)")
            if query_cloud is None:
                raise ValueError("localize(refine=...) needs query_cloud")
        k = int(k)
        idx, dist = self.search(query_desc, k)
        Q = idx.shape[0]
        qr = registration._rows(query_rows, "query_rows", 3 + int(desc_dim))
        qc = registration._count(query_count, "query_count", Q, self.device)
        if qr.shape[0] != Q:
            raise ValueError("query_rows must be [%d, Mq, C], got %s" % (Q, tuple(qr.shape)))
        found = idx >= 0
        safe = idx.clamp(min=0).long().view(-1)
        cand_rows = self.kp_rows.index_select(0, safe)                                     # [Q*k, M, row_dim]
        cand_count = torch.where(found.view(-1), self.kp_count.index_select(0, safe), torch.zeros_like(safe, dtype=torch.int32))
        pair_rows = qr[:, None].expand(Q, k, qr.shape[1], qr.shape[2]).reshape(Q * k, qr.shape[1], qr.shape[2])
        pair_count = qc[:, None].expand(Q, k).reshape(Q * k)
        res = registration.register(cand_rows, cand_count, pair_rows, pair_count, desc_dim=desc_dim, **ransac_kw)
        ok = found & res["valid"].view(Q, k)
        ninl = res["num_inliers"].view(Q, k).long()
        # most inliers, then the better rank: one key, unique per row
        key = torch.where(ok, ninl * k + (k - 1 - torch.arange(k, device=self.device)), torch.full_like(ninl, -1))
        best = key.argmax(dim=1)
        any_ok = key.gather(1, best[:, None])[:, 0] >= 0
        pair = torch.arange(Q, device=self.device) * k + best
        nan = float("nan")
        place = torch.where(any_ok, idx.gather(1, best[:, None])[:, 0], torch.full_like(best, -1, dtype=torch.int32))
        out = dict(
            place=place, rank=torch.where(any_ok, best, torch.full_like(best, -1)).to(torch.int32),
            Rt=torch.where(any_ok[:, None, None], res["Rt"].index_select(0, pair), torch.full_like(res["Rt"][:1], nan)),
            num_inliers=torch.where(any_ok, res["num_inliers"].index_select(0, pair), torch.zeros_like(place)),
            inlier_ratio=torch.where(any_ok, res["inlier_ratio"].index_select(0, pair), torch.zeros_like(dist[:, 0])),
            inliers=res["inliers"].index_select(0, pair) & any_ok[:, None],
            pos=torch.where(any_ok[:, None], self.pos.index_select(0, place.clamp(min=0).long()), torch.full_like(self.pos[:1], nan)),
            idx=idx, dist=dist)
        if rkw is not None:
            safe_place = place.clamp(min=0).long()
            icp = registration.refine_pose(self.cloud.index_select(0, safe_place), query_cloud, out["Rt"], any_ok,
                                           anchor_count=self.cloud_count.index_select(0, safe_place),
                                           positive_count=query_cloud_count, **rkw)
            registration._merge_refinement(out, icp, dense=False)
        return out


def relocalize_clouds(global_model, local_model, index, points, k=5, num_valid=None, refine=None, **kw):
    """Clouds [Q, N, 3] in, place ids and poses out: globaldesc from `global_model` (config.extract_global), kp_count /
    xyz_feat_att_nms from `local_model` (config.detection) -- two models, as the reference has two checkpoints -- then
    index.localize.  num_valid: None or int32 [Q].  refine: None, True or a dict of registration.refine_icp keywords (or
    method="plane" / "gicp" and registration.refine_icp_plane's / refine_icp_gicp's) -- the winner's pose is refined by dense ICP of `points` against the
    place's stored cloud (PlaceIndex(points=...)).  Other keywords go to index.localize and from there to
    registration.register: match={"ratio": ..., "mutual": ...} filters the correspondences ahead of RANSAC."""
    if not getattr(global_model.config, "extract_global", False):
        raise ValueError("relocalize_clouds needs a global_model with config.extract_global (the globaldesc output)")
    if not getattr(local_model.config, "detection", False):
        raise ValueError("relocalize_clouds needs a local_model with config.detection (the keypoint outputs)")
    if registration._refine_kw(refine) is not None and not index.points:
        raise ValueError("relocalize_clouds(refine=...) needs a PlaceIndex built with points > 0 (the places' clouds)")
    g = global_model.forward(points, fetch=("globaldesc",), num_valid=num_valid)
    o = local_model.forward(points, fetch=("kp_count", "xyz_feat_att_nms"), num_valid=num_valid)
    if refine is not None:
        kw = dict(kw, refine=refine, query_cloud=points, query_cloud_count=num_valid)
    return index.localize(g["globaldesc"], o["xyz_feat_att_nms"], o["kp_count"], k=k, **kw)
