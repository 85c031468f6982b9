"""Scan Context on the device (Kim & Kim, IROS 2018): place recognition and relocalisation of raw clouds without a model.

A cloud becomes a rings x sectors polar height image and a ring key (csrc/scan_context.hip; include/dh3d_hip.h
dh3d_scan_context states every rule -- the image is bit-defined).  A map of places is searched in two steps: the exact top-k
search of retrieval.py on the rotation-invariant ring keys gives a short list, the column-shifted cosine distance
(dh3d_scan_context_distance) ranks it, and the best shift is the yaw between query and place: the start pose of the dense ICP
of registration.py against the place's stored cloud.  No trained weights anywhere on the way.

    sc = scan_context(points, num_valid)                          # desc [P, 20, 60], ring_key [P, 20]
    dist, shift, order = scan_context_distance(sc["desc"], map_desc, cand)   # [Q, C] each; order: slots by (dist, id, slot)
    index = ScanContextIndex(capacity=65536, points=8192)
    index.add(points, num_valid, pos=pos)
    res = index.search(points, k=1, candidates=10)                # place, dist, shift, yaw [Q, k]
    res = relocalize_scan_context(index, points, refine=True)     # + Rt [Q, 3, 4] (place ~ R query + t), fitness, rmse

Direction of the shift: if the place's cloud is Rz(theta) applied to the query's, the best shift is theta / (2 pi / Ns), so
place ~ Rz(2 pi shift / Ns) query."""
import math

import numpy as np
import torch

from . import _lib as L
from . import registration
from .retrieval import PlaceIndex, search_descriptors_sq

RINGS_MAX, SECTORS_MAX, CANDIDATES_MAX = 32, 128, 64  # csrc/scan_context.hip

_TABLES = {}  # (device, Nr, Ns, max_radius) -> (sector_dir, ring_edge2) on the device


def _grid(num_rings, num_sectors, max_radius=1.0):
    Nr, Ns, radius = int(num_rings), int(num_sectors), float(max_radius)
    if not 4 <= Nr <= RINGS_MAX or Nr % 4 or not 8 <= Ns <= SECTORS_MAX or Ns % 4:
        raise ValueError("need num_rings in 4 .. %d and num_sectors in 8 .. %d, multiples of 4, got %d, %d"
                         % (RINGS_MAX, SECTORS_MAX, Nr, Ns))
    if not 0.0 < radius < float("inf"):
        raise ValueError("max_radius must be positive and finite, got %r" % (max_radius,))
    return Nr, Ns, radius


def tables(num_rings, num_sectors, max_radius):
    """The two float64 tables dh3d_scan_context reads, as numpy arrays: sector_dir [Ns/2 - 1, 2] = (cos, sin)(2 pi k / Ns)
    for k = 1 .. Ns/2 - 1 and ring_edge2 [Nr + 1] = (i * max_radius / Nr)^2.  Made once on the host: the kernel and a
    restatement that reads them see identical bits."""
    Nr, Ns, radius = _grid(num_rings, num_sectors, max_radius)
    ang = 2.0 * np.pi * np.arange(1, Ns // 2, dtype=np.float64) / Ns
    edge = np.arange(Nr + 1, dtype=np.float64) * radius / Nr
    return np.stack([np.cos(ang), np.sin(ang)], axis=1), edge * edge


def _device_tables(device, Nr, Ns, radius):
    key = (device, Nr, Ns, radius)
    t = _TABLES.get(key)
    if t is None:
        sector_dir, ring_edge2 = tables(Nr, Ns, radius)
        t = _TABLES[key] = (torch.from_numpy(sector_dir).to(device), torch.from_numpy(ring_edge2).to(device))
    return t


def _center(center, P, device):
    if center is None:
        return None
    if not isinstance(center, torch.Tensor) or center.dtype != torch.float32 or not center.is_cuda \
            or tuple(center.shape) != (P, 2) or center.device != device:
        raise ValueError("center must be a float32 [%d, 2] tensor on %s" % (P, device))
    return center.contiguous()


def scan_context(points, num_valid=None, center=None, num_rings=20, num_sectors=60, max_radius=80.0, z_offset=2.0):
    """The Scan Context of every cloud: points [P, N, >=3] float32 on the GPU (the first three columns are read; a column
    view is read in place), num_valid None or int32 [P] (rows past it are never read), center None (the origin) or float32
    [P, 2].  A bin holds the largest z + z_offset > 0 of the points of its ring and sector within max_radius, 0 when it has
    none; non-finite points are skipped.  Returns {"desc": float32 [P, num_rings, num_sectors], "ring_key": float32
    [P, num_rings], the rings' means}.  No host sync: graph-capturable once the grid's tables are on the device (the first
    call with a grid puts them there)."""
    x = registration._rows(points, "points", 3)
    Nr, Ns, radius = _grid(num_rings, num_sectors, max_radius)
    P, N, dev = x.shape[0], x.shape[1], x.device
    cnt = None if num_valid is None else registration._count(num_valid, "num_valid", P, dev)
    ctr = _center(center, P, dev)
    with torch.cuda.device(dev):
        sector_dir, ring_edge2 = _device_tables(dev, Nr, Ns, radius)
        desc = torch.empty((P, Nr, Ns), dtype=torch.float32, device=dev)
        ring_key = torch.empty((P, Nr), dtype=torch.float32, device=dev)
        L.check(L.lib().dh3d_scan_context(L.ptr(x), x.stride(1), L.ptr(cnt), L.ptr(ctr), L.ptr(sector_dir), L.ptr(ring_edge2),
                                          P, N, Nr, Ns, float(z_offset), L.ptr(desc), L.ptr(ring_key), L.stream_ptr()),
                "scan_context")
    return dict(desc=desc, ring_key=ring_key)


def _images(t, name):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 3:
        raise ValueError("%s must be a float32 [n, num_rings, num_sectors] tensor" % name)
    if not t.is_cuda:
        raise ValueError("%s must live on the GPU (the HIP path has no CPU fallback)" % name)
    if 0 in t.shape:
        raise ValueError("%s must not be empty, got shape %s" % (name, tuple(t.shape)))
    return t.contiguous()


def scan_context_distance(qry_desc, map_desc, cand, map_count=None):
    """The column-shifted cosine distance of every query image qry_desc [Q, Nr, Ns] to its candidates cand [Q, C <= 64]
    int32, ids into map_desc [R, Nr, Ns] (search_descriptors_sq's idx: -1 past the map's end).  map_count: None or int32 [1]
    on the device -- only rows below it exist.  Returns (dist float64 [Q, C], shift int32 [Q, C] -- the smallest column shift
    that attains dist; map ~ Rz(2 pi shift / Ns) query --, order int32 [Q, C]: the slots sorted by (dist, id, slot)).  An id
    outside the map gives +inf / -1.  No host sync: graph-capturable."""
    q = _images(qry_desc, "qry_desc")
    m = _images(map_desc, "map_desc")
    if m.shape[1:] != q.shape[1:] or m.device != q.device:
        raise ValueError("map_desc must be [R, %d, %d] on %s, got %s on %s"
                         % (q.shape[1], q.shape[2], q.device, tuple(m.shape), m.device))
    c = L.require_cuda_i32(cand, "cand", 2)
    Q, C, dev = q.shape[0], c.shape[1], q.device
    if c.shape[0] != Q or not 0 < C <= CANDIDATES_MAX or c.device != dev:
        raise ValueError("cand must be int32 [%d, 1 .. %d] on %s, got %s on %s" % (Q, CANDIDATES_MAX, dev, tuple(c.shape), c.device))
    if map_count is not None:
        map_count = L.require_cuda_i32(map_count, "map_count", 1)
        if map_count.shape[0] != 1 or map_count.device != dev:
            raise ValueError("map_count must be int32 [1] on %s" % (dev,))
    with torch.cuda.device(dev):
        dist = torch.empty((Q, C), dtype=torch.float64, device=dev)
        shift = torch.empty((Q, C), dtype=torch.int32, device=dev)
        order = torch.empty((Q, C), dtype=torch.int32, device=dev)
        L.check(L.lib().dh3d_scan_context_distance(L.ptr(q), L.ptr(m), L.ptr(map_count), L.ptr(c), Q, m.shape[0], C, q.shape[1],
                                                   q.shape[2], L.ptr(dist), L.ptr(shift), L.ptr(order), L.stream_ptr()),
                "scan_context_distance")
    return dist, shift, order


class ScanContextIndex:
    """A fixed-capacity map of places found by their Scan Context: a PlaceIndex over the ring keys (`places`: keys
    [capacity, num_rings], pos, the fill level on the device, and with points = N > 0 the places' clouds [capacity, N, 3]
    for the dense refinement) plus desc [capacity, num_rings, num_sectors] and center [capacity, 2] float32.  Buffers never
    move: a graph captured around search keeps serving the map while add() fills it."""

    def __init__(self, capacity, points=0, num_rings=20, num_sectors=60, max_radius=80.0, z_offset=2.0, device="cuda"):
        self.num_rings, self.num_sectors, self.max_radius = _grid(num_rings, num_sectors, max_radius)
        self.z_offset = float(z_offset)
        self.places = PlaceIndex(dim=self.num_rings, capacity=capacity, device=device, points=points)
        self.capacity, self.points, self.device = self.places.capacity, self.places.points, self.places.device
        self.desc = torch.zeros((self.capacity, self.num_rings, self.num_sectors), dtype=torch.float32, device=self.device)
        self.center = torch.zeros((self.capacity, 2), dtype=torch.float32, device=self.device)

    def __len__(self):
        return len(self.places)

    def _scan(self, points, num_valid, center):
        return scan_context(points, num_valid, center, self.num_rings, self.num_sectors, self.max_radius, self.z_offset)

    def add(self, points, num_valid=None, pos=None, center=None):
        """Append the places of n clouds: points [n, N', >=3] (N' <= points where the index stores clouds), num_valid None
        or int32 [n], pos None or [n, 2] (northing, easting), center None or float32 [n, 2].  Returns the ids (a range).
        Raises when the map is full; no device -> host sync."""
        points = registration._rows(points, "points", 3)
        n, o = points.shape[0], len(self.places)
        if o + n > self.capacity:
            raise ValueError("ScanContextIndex is full: %d places + %d > capacity %d" % (o, n, self.capacity))
        if self.points and points.shape[1] > self.points:
            raise ValueError("this ScanContextIndex stores %d points a place, got clouds of %d" % (self.points, points.shape[1]))
        sc = self._scan(points, num_valid, center)
        self.desc[o:o + n].copy_(sc["desc"])
        if center is None:
            self.center[o:o + n].zero_()
        else:
            self.center[o:o + n].copy_(center)
        if self.points:   # the fill level moves last, inside PlaceIndex.add: a search ordered after this add sees whole places
            return self.places.add(sc["ring_key"], pos, cloud=points[:, :, :3], cloud_count=num_valid)
        return self.places.add(sc["ring_key"], pos)

    def search(self, points, num_valid=None, center=None, k=1, candidates=10):
        """The k best places of every query cloud: the `candidates` nearest ring keys (exact float64 top-k over the places
        added so far -- the device count decides), their shifted distances, then the first k by (dist, id).  Returns a dict
        of device tensors [Q, k]: place int32, dist float64, shift int32, yaw float64 = 2 pi shift / num_sectors (place ~
        Rz(yaw) query); -1 / +inf / -1 / NaN past the map's end.  No host sync."""
        k, C = int(k), int(candidates)
        if not 0 < k <= C <= CANDIDATES_MAX:
            raise ValueError("need 1 <= k <= candidates <= %d, got k = %d, candidates = %d" % (CANDIDATES_MAX, k, C))
        sc = self._scan(points, num_valid, center)
        cand, _ = search_descriptors_sq(self.places.desc, sc["ring_key"], C, ref_count=self.places.count)
        dist, shift, order = scan_context_distance(sc["desc"], self.desc, cand, map_count=self.places.count)
        top = order[:, :k].long()
        shift = shift.gather(1, top)
        yaw = torch.where(shift >= 0, shift.double() * (2.0 * math.pi) / self.num_sectors, torch.full_like(dist[:, :k], float("nan")))
        return dict(place=cand.gather(1, top), dist=dist.gather(1, top), shift=shift, yaw=yaw)


def relocalize_scan_context(index, points, num_valid=None, center=None, k=1, candidates=10, refine=None):
    """Clouds [Q, N, >=3] in, place ids and poses out, without a model: index.search, then the pose of the winner (rank 0)
    in ransac_rigid's convention with anchor = the place and positive = the query, place ~ R query + t:  R = Rz(yaw),
    t = c_place - R c_query with the centres as (cx, cy, 0).  Returns search's dict (place, dist, shift, yaw [Q, k]; column
    0 is the winner) plus Rt [Q, 3, 4] float64 (NaN where no place was found) and valid [Q] bool.  refine: None, True or a
    dict of registration.refine_pose keywords -- Rt is then refined by dense ICP of `points` against the winner's stored
    cloud (an index built with points > 0, else ValueError) and the result gains Rt_scan (the pose above), fitness and rmse
    (and rmse_plane with method="plane", rmse_gicp with method="gicp").  No host sync."""
    rkw = registration._refine_kw(refine)
    if rkw is not None and not index.points:
        raise ValueError("relocalize_scan_context(refine=...) needs a ScanContextIndex built with points > 0 (the places' clouds)")
    out = index.search(points, num_valid, center, k, candidates)
    place, yaw = out["place"][:, 0], out["yaw"][:, 0]
    valid = place >= 0
    safe = place.clamp(min=0).long()
    Q, dev = place.shape[0], place.device
    c, s = torch.cos(yaw), torch.sin(yaw)
    cm = index.center.index_select(0, safe).double()
    cq = torch.zeros((Q, 2), dtype=torch.float64, device=dev) if center is None else _center(center, Q, dev).double()
    zero, one = torch.zeros_like(c), torch.ones_like(c)
    Rt = torch.stack([c, -s, zero, cm[:, 0] - (c * cq[:, 0] - s * cq[:, 1]),
                      s, c, zero, cm[:, 1] - (s * cq[:, 0] + c * cq[:, 1]),
                      zero, zero, one, zero], dim=1).view(Q, 3, 4)
    out["Rt"] = torch.where(valid[:, None, None], Rt, torch.full_like(Rt, float("nan")))
    out["valid"] = valid
    if rkw is not None:
        icp = registration.refine_pose(index.places.cloud.index_select(0, safe), points, out["Rt"], valid,
                                       anchor_count=index.places.cloud_count.index_select(0, safe), positive_count=num_valid,
                                       **rkw)
        registration._merge_refinement(out, icp, before="Rt_scan", dense=False)
    return out
