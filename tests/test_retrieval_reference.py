"""CPU: the float64 restatement of dh3d_retrieve (tests/retrieval_reference.py) against the reference's recipe, scipy's
cKDTree (evaluation_retrieval.py:37-40); the case that tells a float64 rank from a float32 one; and the host-only half of
the C ABI (plan, workspace, status codes -- no compute calls here)."""
import ctypes

import numpy as np

import retrieval_reference as rr


def test_restatement_equals_the_kdtree_recipe():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    R, D, Q, k = 20000, 256, 64, 25
    ref = rr.clustered_map(rng, R, D)
    qry = rr.unit(ref[rng.integers(0, R, Q)] + 0.02 * rng.standard_normal((Q, D)))
    idx, d2 = rr.topk(ref, qry, k)
    dist, ind = cKDTree(ref).query(qry, k=k)
    assert (d2[:, 1:] > d2[:, :-1]).all()                 # tie-free data: the order is the distances' alone
    assert int((idx != ind).sum()) == 0                   # every one of the 1600 positions
    assert np.allclose(np.sqrt(d2), dist, rtol=1e-12, atol=0)


def test_float64_rank_differs_from_float32_on_the_near_tie():
    ref, qry = rr.near_tie_case()
    i32, d32 = rr.topk(ref, qry, 2, dtype=np.float32)
    i64, d64 = rr.topk(ref, qry, 2)
    assert d32[0, 0] == d32[0, 1] == 1.0 and i32[0].tolist() == [3, 7]     # float32: a tie, the lowest id first
    assert d64[0].tolist() == [1.0, 1.0 + 2.0 ** -26] and i64[0].tolist() == [7, 3]


def test_plan_is_refused_exactly_where_the_workspace_is_zero():
    from dh3d_amd import _lib
    lib = _lib.lib()
    plan, ws = lib.dh3d_retrieve_plan, lib.dh3d_retrieve_ws_bytes
    for shape in ((4, 100, 6, 5), (4, 100, 260, 5), (4, 100, 256, 65)):    # D % 4, D > 256, k > 64
        assert plan(*shape) == -1 and ws(*shape) == 0, shape
    for Q in (-1, 0, 1, 16, 17, 400, 4096, 100000):
        for R in (-1, 0, 1, 256, 257, 8192, 65536):
            for D in (0, 4, 6, 128, 256, 260):
                for k in (0, 1, 25, 64, 65):
                    S = plan(Q, R, D, k)
                    assert (S == -1) == (ws(Q, R, D, k) == 0), (Q, R, D, k)
                    ok = Q > 0 and R > 0 and D > 0 and k > 0 and D % 4 == 0 and D <= 256 and k <= 64
                    assert (S >= 1) == ok, (Q, R, D, k)
                    if ok:
                        assert S <= (R + 255) // 256          # never less than one tile of 256 rows per slice


def test_workspace_sizes_are_the_partial_lists():
    """Literal sizes, never computed by the code under test: the partial lists [S, Q, k] of 8-byte distance bits and 4-byte
    ids, each segment padded to 16 bytes (csrc/workspace.h carves them, so these numbers also pin the offsets)."""
    from dh3d_amd import _lib
    ws = _lib.lib().dh3d_retrieve_ws_bytes
    rows = [((1, 256, 256, 25), 320),                    # S = 1: 200 -> 208, 100 -> 112
            ((1, 257, 4, 1), 32),                        # S = 2
            ((400, 400, 256, 25), 240000),               # S = 2
            ((32, 65536, 256, 25), 2457600),             # S = 256
            ((4096, 65536, 256, 25), 2457600),           # S = 2
            ((4, 100, 6, 5), 0), ((4, 100, 260, 5), 0), ((4, 100, 256, 65), 0), ((0, 100, 256, 5), 0)]
    assert [(shape, ws(*shape)) for shape, _ in rows] == rows


def test_plan_splits_a_large_map_for_few_queries_only():
    from dh3d_amd import retrieval
    plan = retrieval.retrieve_plan
    assert plan(1, 256, 256, 25) == (1, 256)
    split = [R for R in range(1, 8193) if plan(1, R, 256, 25)[0] > 1]
    assert split and split[0] <= 8192
    assert plan(1, split[0] - 1, 256, 25)[0] == 1
    assert plan(32, 65536, 256, 25)[0] >= 128               # two blocks of queries fill the machine through the slices
    assert plan(100000, 65536, 256, 25)[0] == 1             # many queries do not split
    for Q, R in ((1, 257), (1, 5000), (33, 777), (32, 65536), (400, 400), (4096, 65536)):
        S, L = plan(Q, R, 256, 25)
        assert L % 256 == 0 and (S - 1) * L < R <= S * L, (Q, R, S, L)   # S slices of L rows cover the map, none empty
    assert plan(1, 100, 6, 5) is None


def test_status_codes_without_a_gpu():
    from dh3d_amd import _lib
    lib = _lib.lib()
    z, one = ctypes.c_void_p(0), ctypes.c_void_p(16)
    f = lib.dh3d_retrieve
    big = 1 << 30
    assert f(z, 8, z, one, 8, 1, 1, 8, 1, one, one, one, big, z) == 1        # NULL ref
    assert f(one, 8, z, z, 8, 1, 1, 8, 1, one, one, one, big, z) == 1        # NULL qry
    assert f(one, 8, z, one, 8, 1, 1, 8, 1, z, one, one, big, z) == 1        # NULL idx
    assert f(one, 8, z, one, 8, 1, 1, 8, 1, one, z, one, big, z) == 1        # NULL dist2
    for Q, R, D, k in ((0, 1, 8, 1), (1, 0, 8, 1), (1, 1, 0, 1), (1, 1, 8, 0), (-3, 1, 8, 1)):
        assert f(one, 8, z, one, 8, Q, R, D, k, one, one, one, big, z) == 1, (Q, R, D, k)
    assert f(one, 7, z, one, 8, 1, 1, 8, 1, one, one, one, big, z) == 1      # ref_stride < D
    assert f(one, 8, z, one, 4, 1, 1, 8, 1, one, one, one, big, z) == 1      # qry_stride < D
    assert f(one, 8, z, one, 8, 1, 1, 8, 1, one, one, z, big, z) == 1        # no workspace
    assert f(one, 8, z, one, 8, 1, 1, 8, 1, one, one, one, 1, z) == 1        # workspace too small
    assert f(one, 8, z, one, 8, 1, 1, 6, 1, one, one, one, big, z) == 2      # D % 4
    assert f(one, 260, z, one, 260, 1, 1, 260, 1, one, one, one, big, z) == 2  # D > 256
    assert f(one, 8, z, one, 8, 1, 100, 8, 65, one, one, one, big, z) == 2   # k > 64


def test_python_search_refuses_cpu_tensors_and_refused_shapes():
    import pytest
    import torch
    from dh3d_amd import evaluation, retrieval
    with pytest.raises(ValueError):
        retrieval.search_descriptors(torch.zeros(8, 4), torch.zeros(2, 4), 3)   # CPU tensors: no fallback
    with pytest.raises(ValueError):
        retrieval.PlaceIndex(dim=256, capacity=8, device="cpu")
    with pytest.raises(ValueError):
        evaluation.retrieval(np.zeros((5, 4), np.float32), np.zeros((2, 4), np.float32), 3, backend="hip")
    with pytest.raises(ValueError):
        evaluation.retrieval(np.zeros((5, 4), np.float32), np.zeros((2, 4), np.float32), 3, backend="faiss")
    # "torch" stays the default and today's code
    got = evaluation.retrieval(np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)[[2, 0]], 1)
    assert got.dtype == torch.int64 and got[:, 0].tolist() == [2, 0]
