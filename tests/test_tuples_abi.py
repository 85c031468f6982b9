"""CPU: the training-tuple entry points (include/dh3d_hip.h "Training tuples", csrc/tuples.hip) are declared, bound and
exported; every refusal is a status code before anything touches the GPU; the Python module refuses what the kernels do
not take before it looks at where the tensors live."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dh3d_tuple_counts", "dh3d_draw_queries_ws_bytes", "dh3d_draw_queries", "dh3d_sample_tuples")
P = 256  # a non-null, 16-byte-aligned fake pointer: every check below fails before a launch


def test_symbols_declared_bound_and_exported():
    from dh3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name), name
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION   # additions only
    section = header[header.index("Training tuples"):header.index("int dh3d_sample_tuples")]
    for word in ("POS(q)", "NEG(q)", "d2(q, j) <= rp2", "d2(q, j) > rn2", "j != q", "(dx*dx) + (dy*dy)", "never read",
                 "11 positive keys", "12 negative keys", "13 pool membership", "14 other-negative keys", "15 query keys",
                 "ASCENDING KEY order", "dh3d_resample_clouds emits", "DEVICE pointer", "graph-capturable", "every output element is written",
                 "not on Q", "M <= 2^20", "Q <= 65535", "pool_fraction", "bits of D2", "dh3d_retrieve's rule", "[hard | random]",
                 "BAR", "DEVIATION", "datasets.py:224-232", "ok[0] = 0", "pos_radius = 10.0", "neg_radius = 50.0"):
        assert word in section, word
    makefile = open(os.path.join(ROOT, "dh3d_amd", "csrc", "Makefile")).read()
    exact = [ln for ln in makefile.splitlines() if ln.startswith("EXACT :=")][0]
    assert "tuples.o" in exact                 # the -ffp-contract=off group: every id depends on d2's and D2's roundings


def test_workspace_size():
    from dh3d_amd import _lib
    f = _lib.lib().dh3d_draw_queries_ws_bytes
    for bad in ((0, 4), (4, 0), (-1, 4), ((1 << 20) + 1, 4), (100, 65536)):
        assert f(*bad) == 0, bad
    assert f(1 << 20, 65535) > 0
    # a key (8 bytes) and an id (4 bytes) per query slot, each segment padded to 16 bytes, and one padded counter
    for shape, size in (((10, 1), 16 + 16 + 16), ((602, 5), 48 + 32 + 16), ((65536, 2048), 16384 + 8192 + 16)):
        assert f(*shape) == size, shape


def _counts(lib, pos=P, count=None, M=100, rp=10.0, rn=50.0, n_pos=P, n_neg=P):
    return lib.dh3d_tuple_counts(pos, count, M, rp, rn, n_pos, n_neg, None)


def _draw(lib, n_pos=P, n_neg=P, count=None, M=100, Q=4, num_pos=2, num_neg=18, seed=P, queries=P, ok=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dh3d_draw_queries_ws_bytes(M, Q) or (1 << 40)
    return lib.dh3d_draw_queries(n_pos, n_neg, count, M, Q, num_pos, num_neg, seed, queries, ok, ws, ws_bytes, None)


def _sample(lib, pos=P, count=None, M=100, queries=P, Q=4, num_pos=2, num_neg=18, rp=10.0, rn=50.0, desc=None, stride=256,
            D=256, num_hard=0, fraction=1.0, seed=P, pos_idx=P, neg_idx=P, other=P, valid=P):
    return lib.dh3d_sample_tuples(pos, count, M, queries, Q, num_pos, num_neg, rp, rn, desc, stride, D, num_hard, fraction, seed,
                                  pos_idx, neg_idx, other, valid, None)


BAD_RADII = (dict(rp=0.0), dict(rp=-1.0), dict(rn=0.0), dict(rp=float("nan")), dict(rn=float("nan")), dict(rp=float("inf")),
             dict(rn=float("inf")), dict(rp=20.0, rn=10.0))


def test_bad_arguments_are_status_1():
    from dh3d_amd import _lib
    lib = _lib.lib()
    for kw in (dict(pos=None), dict(n_pos=None), dict(n_neg=None), dict(M=0), dict(M=-5), dict(pos=264)) + BAD_RADII:
        assert _counts(lib, **kw) == 1, kw
    small = lib.dh3d_draw_queries_ws_bytes(100, 4) - 1
    for kw in (dict(n_pos=None), dict(n_neg=None), dict(seed=None), dict(queries=None), dict(ok=None), dict(M=0), dict(Q=0),
               dict(Q=-1), dict(num_pos=0), dict(num_neg=0), dict(num_neg=-2), dict(ws=None), dict(ws=264), dict(ws_bytes=0),
               dict(ws_bytes=small)):
        assert _draw(lib, **kw) == 1, kw
    for kw in (dict(pos=None), dict(queries=None), dict(seed=None), dict(pos_idx=None), dict(neg_idx=None), dict(valid=None),
               dict(M=0), dict(Q=0), dict(num_pos=0), dict(num_neg=0), dict(num_hard=-1), dict(pos=264)) + BAD_RADII:
        assert _sample(lib, **kw) == 1, kw
    hard = dict(desc=P, num_hard=3)
    for kw in (dict(D=0), dict(D=-4), dict(stride=252), dict(stride=258), dict(desc=260), dict(fraction=-0.1), dict(fraction=1.5),
               dict(fraction=float("nan"))):
        assert _sample(lib, **dict(hard, **kw)) == 1, kw


def test_unsupported_shapes_are_status_2():
    from dh3d_amd import _lib
    lib = _lib.lib()
    assert _counts(lib, M=(1 << 20) + 1) == 2
    for kw in (dict(M=(1 << 20) + 1), dict(Q=65536), dict(num_pos=65), dict(num_neg=65)):
        assert _draw(lib, **kw) == 2, kw
    for kw in (dict(M=(1 << 20) + 1), dict(Q=65536), dict(num_pos=65), dict(num_neg=65), dict(num_hard=19),
               dict(desc=P, num_hard=3, D=260, stride=260), dict(desc=P, num_hard=3, D=6, stride=8)):
        assert _sample(lib, **kw) == 2, kw


def test_python_entry_point_refusals():
    from dh3d_amd import tuples
    pos = torch.zeros(50, 2, dtype=torch.float64)
    cnt = torch.zeros(50, dtype=torch.int32)
    qs = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="float64"):
        tuples.tuple_counts(pos.float())
    with pytest.raises(ValueError, match="float64"):
        tuples.sample_tuples(torch.zeros(50, 3, dtype=torch.float64), qs, 2, 18)
    with pytest.raises(ValueError, match="beyond the kernels"):
        tuples.tuple_counts(torch.zeros((1 << 20) + 1, 2, dtype=torch.float64))
    for bad in (dict(pos_radius=0.0), dict(neg_radius=float("nan")), dict(pos_radius=float("inf")), dict(pos_radius=60.0)):
        with pytest.raises(ValueError, match="radii"):
            tuples.tuple_counts(pos, **bad)
        with pytest.raises(ValueError, match="radii"):
            tuples.sample_tuples(pos, qs, 2, 18, **bad)
    for num_pos, num_neg in ((0, 18), (65, 18), (2, 0), (2, 65)):
        with pytest.raises(ValueError, match="num_pos"):
            tuples.draw_queries(cnt, cnt, 4, num_pos, num_neg)
        with pytest.raises(ValueError, match="num_pos"):
            tuples.sample_tuples(pos, qs, num_pos, num_neg)
    for Q in (0, 65536):
        with pytest.raises(ValueError, match="Q"):
            tuples.draw_queries(cnt, cnt, Q, 2, 18)
    with pytest.raises(ValueError, match="num_hard"):
        tuples.sample_tuples(pos, qs, 2, 18, num_hard=19)
    with pytest.raises(ValueError, match="num_hard"):
        tuples.sample_tuples(pos, qs, 2, 18, num_hard=-1)
    with pytest.raises(ValueError, match="pool_fraction"):
        tuples.sample_tuples(pos, qs, 2, 18, pool_fraction=1.5)
    with pytest.raises(ValueError, match="multiple of 4"):
        tuples.sample_tuples(pos, qs, 2, 18, desc=torch.zeros(50, 6), num_hard=2)
    with pytest.raises(ValueError, match="multiple of 4"):
        tuples.sample_tuples(pos, qs, 2, 18, desc=torch.zeros(50, 260), num_hard=2)
    with pytest.raises(ValueError, match=r"float32 \[50, D\]"):
        tuples.sample_tuples(pos, qs, 2, 18, desc=torch.zeros(49, 8), num_hard=2)
    with pytest.raises(ValueError, match="beyond the kernels"):
        tuples.sample_tuples(pos, torch.zeros(65536, dtype=torch.int32), 2, 18)

    class Bank:
        pass
    bank = Bank()
    bank.pos, bank.count, bank.desc = pos, torch.full((1,), 50, dtype=torch.int32), torch.zeros(50, 8)
    bank.cloud, bank.cloud_count = None, None
    with pytest.raises(ValueError, match="clouds"):
        tuples.make_quadruplet_batch(bank, 2, 2, 18)
    bank.cloud, bank.cloud_count = torch.zeros(50, 64, 3), torch.full((50,), 64, dtype=torch.int32)
    with pytest.raises(ValueError, match="unknown augmentation"):
        tuples.make_quadruplet_batch(bank, 2, 2, 18, aug=("Flip",))
    with pytest.raises(ValueError, match="batch_size"):
        tuples.make_quadruplet_batch(bank, 0, 2, 18)
    for call in (lambda: tuples.tuple_counts(pos), lambda: tuples.draw_queries(cnt, cnt, 4, 2, 18),
                 lambda: tuples.sample_tuples(pos, qs, 2, 18), lambda: tuples.make_quadruplet_batch(bank, 2, 2, 18, numpts=32)):
        with pytest.raises(ValueError, match="GPU"):
            call()
    assert "prepare_clouds(sortby_dis=True)" in tuples.make_quadruplet_batch.__doc__
    import inspect
    from dh3d_amd import pairs
    assert (inspect.signature(tuples.make_quadruplet_batch).parameters["aug"].default
            == inspect.signature(pairs.make_global_batch).parameters["aug"].default)
