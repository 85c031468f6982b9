"""Plain numpy float32 restatement of select_top_k (the SelectionSort op), knn_point and gather_point
(include/dh3d_hip.h, csrc/knn_point.hip), written from the kernels' stated semantics -- the yardstick of the knn_point tests.

select_top_k(k, dist): per row the partial selection sort -- start from out = dist, idx = 0..n-1; for s = 0..k-1 find the
FIRST position t >= s holding the smallest value (strict <) and swap positions s and t in both arrays.  The whole row is
the result.  knn_point(k, xyz1, xyz2): the first k columns of that walk on D[b,j,i] = sum_c (xyz1[b,i,c] - xyz2[b,j,c])^2,
every difference and square rounded to float32 on its own, the squares added left to right over c.
"""
import numpy as np


def swap_walk_row(k, row):
    """One row -> (idx [n] int32, out [n] float32): the walk itself, one np.argmin (first minimum) per step."""
    out = np.array(row, np.float32, copy=True)
    n = out.shape[0]
    idx = np.arange(n, dtype=np.int32)
    for s in range(k):
        t = s + int(np.argmin(out[s:]))
        if t != s:
            out[s], out[t] = out[t], out[s]
            idx[s], idx[t] = idx[t], idx[s]
    return idx, out


def candidate_walk_row(k, row):
    """The same row by the candidate-set lemma the kernels rely on: the walk only ever moves the positions of
    C = {0..k-1} U {the k smallest by (value, position) among the positions >= k}; the k-step walk on C taken in position
    order, written back to the positions of C, is the whole row.  Nothing outside C moves."""
    row = np.asarray(row, np.float32)
    n = row.shape[0]
    tail = np.arange(k, n)
    if n - k > k:                                        # (only a speed-up: nothing above the k-th smallest value is chosen)
        tail = tail[row[k:] <= np.partition(row[k:], k - 1)[k - 1]]
    order = np.lexsort((tail, row[tail]))[:k]            # by value, then position
    cand = np.concatenate([np.arange(k), np.sort(tail[order])]).astype(np.int64)
    ci, cv = swap_walk_row(k, row[cand])
    idx, out = np.arange(n, dtype=np.int32), row.copy()
    idx[cand], out[cand] = cand[ci].astype(np.int32), cv
    return idx, out


def select_top_k(k, dist):
    """dist [b,m,n] float32 -> (idx [b,m,n] int32, dist_out [b,m,n] float32)."""
    dist = np.asarray(dist, np.float32)
    b, m, n = dist.shape
    if not 1 <= k <= n:
        raise ValueError("SelectionSort expects 1 <= k <= n")
    flat = dist.reshape(b * m, n)
    idx, out = np.empty(flat.shape, np.int32), np.empty(flat.shape, np.float32)
    for r in range(b * m):
        idx[r], out[r] = candidate_walk_row(k, flat[r]) if 4 * k < n else swap_walk_row(k, flat[r])
    return idx.reshape(b, m, n), out.reshape(b, m, n)


def sqdist(xyz1, xyz2):
    """xyz1 [b,n,c] dataset, xyz2 [b,m,c] queries -> D [b,m,n] float32 with the stated rounding."""
    x1, x2 = np.asarray(xyz1, np.float32), np.asarray(xyz2, np.float32)
    d = np.zeros((x1.shape[0], x2.shape[1], x1.shape[1]), np.float32)
    for c in range(x1.shape[2]):
        diff = (x1[:, None, :, c] - x2[:, :, None, c]).astype(np.float32)
        sq = (diff * diff).astype(np.float32)
        d = sq if c == 0 else (d + sq).astype(np.float32)
    return d


def knn_point(k, xyz1, xyz2, chunk=256):
    """-> (val [b,m,k] float32 squared distances, idx [b,m,k] int32), in the reference's order of outputs."""
    x1, x2 = np.asarray(xyz1, np.float32), np.asarray(xyz2, np.float32)
    b, m = x2.shape[0], x2.shape[1]
    if not 1 <= k <= x1.shape[1]:
        raise ValueError("SelectionSort expects 1 <= k <= n")
    val, idx = np.empty((b, m, k), np.float32), np.empty((b, m, k), np.int32)
    for j in range(0, m, chunk):                          # (bounded: never the whole [b,m,n] matrix)
        i, o = select_top_k(k, sqdist(x1, x2[:, j:j + chunk]))
        val[:, j:j + chunk], idx[:, j:j + chunk] = o[..., :k], i[..., :k]
    return val, idx


def gather_point(inp, idx):
    """inp [b,n,3], idx [b,m] -> [b,m,3]."""
    inp = np.asarray(inp, np.float32)
    return np.take_along_axis(inp, np.asarray(idx, np.int64)[..., None], 1)


def gather_point_grad(inp_shape, idx, grad_out):
    """The scatter-add of GatherPointGrad: grad_inp[b, idx[b,j]] += grad_out[b,j] (float64 accumulation)."""
    g = np.zeros(inp_shape, np.float64)
    for bi in range(inp_shape[0]):
        np.add.at(g[bi], np.asarray(idx[bi], np.int64), np.asarray(grad_out[bi], np.float64))
    return g
