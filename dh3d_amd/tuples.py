"""Training tuples on the device: which places of a map form a quadruplet (HIP: csrc/tuples.hip; include/dh3d_hip.h
"Training tuples" holds the exact semantics).  The reference decides this in Global_train_dataset_triplet.__iter__
(core/datasets.py:202-233) with Python set differences over the whole training set, per tuple and on the host.

    tuple_counts          |positives| and |negatives| of every place, from the positions: once per map
    draw_queries          the reference's shuffle plus its `continue` on too few positives: Q random places that can be queries
    sample_tuples         per query: random positives, hard (nearest in descriptor space) and random negatives, and one
                          "other negative" that is near neither the query nor any chosen negative
    make_quadruplet_batch bank of places -> tuple -> pairs.make_global_batch: the input of QuadrupletTrainer.step

    bank = PlaceIndex(dim=256, capacity=65536, points=8192); bank.add(desc, pos, cloud=clouds, cloud_count=num_valid)
    batch = make_quadruplet_batch(bank, cfg.batch_size, cfg.num_pos, cfg.num_neg, seed=seed_tensor)
    loss = trainer.step(batch["points"], sync=False)

Every draw is a counter-based function of (seed, stream, slot, place) as in pairs.py; `seed` is an int or a 1-element int64
tensor on the GPU, and with a tensor the whole chain is graph-capturable: nothing here synchronises with the host."""
import torch

from . import _lib as L
from . import pairs

MAX_PLACES, MAX_QUERIES, MAX_PICK, DESC_MAX = 1 << 20, 65535, 64, 256  # include/dh3d_hip.h "Training tuples" LIMITS
POS_RADIUS, NEG_RADIUS = 10.0, 50.0


def _radii(pos_radius, neg_radius):
    rp, rn = float(pos_radius), float(neg_radius)
    if not (0.0 < rp < float("inf") and 0.0 < rn < float("inf") and rn >= rp):
        raise ValueError("need finite radii with 0 < pos_radius <= neg_radius, got %r and %r" % (pos_radius, neg_radius))
    return rp, rn


def _picks(num_pos, num_neg):
    num_pos, num_neg = int(num_pos), int(num_neg)
    if not (1 <= num_pos <= MAX_PICK and 1 <= num_neg <= MAX_PICK):
        raise ValueError("need 1 <= num_pos <= %d and 1 <= num_neg <= %d, got %d and %d" % (MAX_PICK, MAX_PICK, num_pos, num_neg))
    return num_pos, num_neg


def _positions(pos, gpu=True):
    if not isinstance(pos, torch.Tensor) or pos.dtype != torch.float64 or pos.dim() != 2 or pos.shape[1] != 2 or pos.shape[0] < 1:
        raise ValueError("pos must be a float64 [M, 2] tensor of place positions")
    if pos.shape[0] > MAX_PLACES:
        raise ValueError("a map of %d places is beyond the kernels (%d)" % (pos.shape[0], MAX_PLACES))
    if gpu and not pos.is_cuda:
        raise ValueError("pos must live on the GPU (the HIP path has no CPU fallback)")
    return pos.contiguous()


def _count(count, device):
    if count is None:
        return None
    count = L.require_cuda_i32(count, "count", 1)
    if count.shape[0] != 1 or count.device != device:
        raise ValueError("count must be int32 [1] on %s" % (device,))
    return count


def _ids(t, name, n, device):
    t = L.require_cuda_i32(t, name, 1)
    if (n is not None and t.shape[0] != n) or t.shape[0] < 1 or t.device != device:
        raise ValueError("%s must be int32 [%s] on %s, got %s on %s" % (name, n if n is not None else "Q", device, tuple(t.shape), t.device))
    return t


def tuple_counts(pos, count=None, pos_radius=POS_RADIUS, neg_radius=NEG_RADIUS):
    """pos [M, 2] float64 (count: None or int32 [1] on the device, the live places) -> (n_pos [M], n_neg [M]) int32: how
    many places lie within pos_radius of each place (itself excepted) and how many beyond neg_radius; 0 for places at or
    beyond count.  Quadratic in the map: run it once per map, or whenever the map grows."""
    rp, rn = _radii(pos_radius, neg_radius)
    p = _positions(pos)
    count = _count(count, p.device)
    M = p.shape[0]
    n_pos = torch.empty((M,), dtype=torch.int32, device=p.device)
    n_neg = torch.empty((M,), dtype=torch.int32, device=p.device)
    with torch.cuda.device(p.device):
        L.check(L.lib().dh3d_tuple_counts(L.ptr(p), L.ptr(count), M, rp, rn, L.ptr(n_pos), L.ptr(n_neg), L.stream_ptr()),
                "tuple_counts")
    return n_pos, n_neg


def draw_queries(n_pos, n_neg, Q, num_pos, num_neg, count=None, seed=0):
    """Q random places with at least num_pos positives and num_neg negatives (tuple_counts' outputs), in random order ->
    (queries [Q] int32, ok [1] int32).  With fewer than Q such places the remaining entries are -1 and ok is 0."""
    num_pos, num_neg = _picks(num_pos, num_neg)
    Q = int(Q)
    if not 1 <= Q <= MAX_QUERIES:
        raise ValueError("need 1 <= Q <= %d, got %d" % (MAX_QUERIES, Q))
    if isinstance(n_pos, torch.Tensor) and n_pos.dim() == 1 and n_pos.shape[0] > MAX_PLACES:
        raise ValueError("a map of %d places is beyond the kernels (%d)" % (n_pos.shape[0], MAX_PLACES))
    a = L.require_cuda_i32(n_pos, "n_pos", 1)
    b = _ids(n_neg, "n_neg", a.shape[0], a.device)
    count = _count(count, a.device)
    M = a.shape[0]
    sd = pairs.seed_tensor(seed, a.device)
    queries = torch.empty((Q,), dtype=torch.int32, device=a.device)
    ok = torch.empty((1,), dtype=torch.int32, device=a.device)
    nbytes = L.lib().dh3d_draw_queries_ws_bytes(M, Q)
    if nbytes == 0:
        raise ValueError("draw_queries: shape M = %d, Q = %d is beyond the kernels" % (M, Q))
    with torch.cuda.device(a.device):
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=a.device)
        L.check(L.lib().dh3d_draw_queries(L.ptr(a), L.ptr(b), L.ptr(count), M, Q, num_pos, num_neg, L.ptr(sd), L.ptr(queries),
                                          L.ptr(ok), L.ptr(ws), nbytes, L.stream_ptr()), "draw_queries")
    return queries, ok


def sample_tuples(pos, queries, num_pos, num_neg, count=None, other_neg=True, desc=None, num_hard=0, pool_fraction=1.0,
                  pos_radius=POS_RADIUS, neg_radius=NEG_RADIUS, seed=0):
    """The tuple of every query place: pos [M, 2] float64, queries [Q] int32 (draw_queries' output; -1 or a place at or beyond
    count gives an invalid slot) -> a dict of int32 device tensors
        pos [Q, num_pos]    random positives (within pos_radius, the query excepted)
        neg [Q, num_neg]    [hard | random] negatives (beyond neg_radius)
        other [Q]           a place within pos_radius of neither the query nor any chosen negative, and none of them
                            (None with other_neg=False)
        valid [Q]           1 where every row above is filled; an unfilled row is all -1
    Hard negatives (num_hard > 0 and desc [M, D] float32, e.g. a PlaceIndex's descriptor cache): of a random pool_fraction
    of the negatives, the num_hard nearest to the query in descriptor space (exact float64, ties to the lower id) lead the
    row; the rest of the row is random among the remaining negatives."""
    num_pos, num_neg = _picks(num_pos, num_neg)
    num_hard, pool_fraction = int(num_hard), float(pool_fraction)
    if not 0 <= num_hard <= num_neg:
        raise ValueError("need 0 <= num_hard <= num_neg = %d, got %d" % (num_neg, num_hard))
    if not 0.0 <= pool_fraction <= 1.0:
        raise ValueError("need 0 <= pool_fraction <= 1, got %r" % (pool_fraction,))
    rp, rn = _radii(pos_radius, neg_radius)
    if isinstance(queries, torch.Tensor) and queries.dim() == 1 and queries.shape[0] > MAX_QUERIES:
        raise ValueError("%d query slots are beyond the kernels (%d)" % (queries.shape[0], MAX_QUERIES))
    M = _positions(pos, gpu=False).shape[0]  # (shapes are refused before anything looks at where the tensors live)
    if desc is not None and num_hard > 0:
        if not isinstance(desc, torch.Tensor) or desc.dtype != torch.float32 or desc.dim() != 2 or desc.shape[0] != M:
            raise ValueError("desc must be a float32 [%d, D] tensor" % M)
        if desc.shape[1] < 1 or desc.shape[1] > DESC_MAX or desc.shape[1] % 4:
            raise ValueError("descriptor length must be a multiple of 4 up to %d, got %d" % (DESC_MAX, desc.shape[1]))
        p = _positions(pos)
        if not desc.is_cuda or desc.device != p.device:
            raise ValueError("desc must live on the GPU, on pos's device")
        if desc.stride(1) != 1 or desc.stride(0) < desc.shape[1] or desc.stride(0) % 4 or desc.data_ptr() % 16:
            desc = desc.contiguous()
    else:
        desc, num_hard = None, 0
    p = _positions(pos)
    qs = _ids(queries, "queries", None, p.device)
    count = _count(count, p.device)
    Q = qs.shape[0]
    sd = pairs.seed_tensor(seed, p.device)
    i32 = dict(dtype=torch.int32, device=p.device)
    out = {"pos": torch.empty((Q, num_pos), **i32), "neg": torch.empty((Q, num_neg), **i32),
           "other": torch.empty((Q,), **i32) if other_neg else None, "valid": torch.empty((Q,), **i32)}
    with torch.cuda.device(p.device):
        L.check(L.lib().dh3d_sample_tuples(L.ptr(p), L.ptr(count), M, L.ptr(qs), Q, num_pos, num_neg, rp, rn, L.ptr(desc),
                                           desc.stride(0) if desc is not None else 0, desc.shape[1] if desc is not None else 0,
                                           num_hard, pool_fraction, L.ptr(sd), L.ptr(out["pos"]), L.ptr(out["neg"]),
                                           L.ptr(out["other"]), L.ptr(out["valid"]), L.stream_ptr()), "sample_tuples")
    return out


def make_quadruplet_batch(bank, batch_size, num_pos, num_neg, numpts=8192, counts=None, queries=None,
                          aug=("Jitter", "RotateSmall", "Shift", "Rotate1D"), seed=0, **sample_kw):
    """Global_train_dataset_triplet.__iter__ + loadPC for batch_size quadruplets drawn from a bank of places: anything with
    pos [M, 2] float64, count int32 [1], cloud [M, N, 3] float32, cloud_count [M] int32 and desc [M, D] float32 on the
    device -- a retrieval.PlaceIndex(points=N) is one.  The bank's clouds are expected as utils.prepare_clouds(sortby_dis=True)
    left them, as in pairs.make_global_batch: its crop to the points nearest the centroid is loadPC's sortby_dis=True.

    counts: tuple_counts' (n_pos, n_neg) of the bank (None: computed here, quadratic in the map -- pass them when the map
    does not change); queries: int32 [batch_size] (None: draw_queries); sample_kw: sample_tuples' keywords (other_neg,
    num_hard, pool_fraction, pos_radius, neg_radius; the bank's desc is the descriptor table).  Returns a dict of device
    tensors:
        points [batch_size * (1 + num_pos + num_neg (+ 1)), numpts, 3]   the argument of QuadrupletTrainer.step
        ids    the places behind the clouds, [queries | pos row-major | neg row-major | other] -- the role order
               losses._split expects -- with -1 (an unfilled row) clamped to place 0 so that the gather stays in bounds
        valid [batch_size], ok [1]   sample_tuples' and draw_queries' flags (ok = 1 with given queries)
    Neither flag is looked at on the host: a caller that cannot rule out an unfilled row masks the loss with `valid`."""
    pairs.aug_mask(aug)
    num_pos, num_neg = _picks(num_pos, num_neg)
    B = int(batch_size)
    if B < 1:
        raise ValueError("make_quadruplet_batch expects batch_size >= 1")
    if getattr(bank, "cloud", None) is None or getattr(bank, "cloud_count", None) is None:
        raise ValueError("make_quadruplet_batch needs a bank that holds the places' clouds (PlaceIndex(points=N))")
    pos = _positions(bank.pos)
    sd = pairs.seed_tensor(seed, pos.device)
    radii = {k: sample_kw[k] for k in ("pos_radius", "neg_radius") if k in sample_kw}
    if queries is None:
        n_pos, n_neg = counts if counts is not None else tuple_counts(pos, bank.count, **radii)
        queries, ok = draw_queries(n_pos, n_neg, B, num_pos, num_neg, count=bank.count, seed=sd)
    else:
        queries = _ids(queries, "queries", B, pos.device)
        ok = torch.ones((1,), dtype=torch.int32, device=pos.device)
    t = sample_tuples(pos, queries, num_pos, num_neg, count=bank.count, desc=bank.desc, seed=sd, **sample_kw)
    parts = [queries, t["pos"].reshape(-1), t["neg"].reshape(-1)] + ([t["other"]] if t["other"] is not None else [])
    ids = torch.cat(parts).clamp_(min=0)
    rows = ids.long()
    points = pairs.make_global_batch(bank.cloud.index_select(0, rows), bank.cloud_count.index_select(0, rows), numpts, aug=aug,
                                     seed=sd)
    return {"points": points, "ids": ids, "valid": t["valid"], "ok": ok}
