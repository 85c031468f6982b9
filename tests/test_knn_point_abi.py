"""CPU: the knn_point / select_top_k entry points (include/dh3d_hip.h, csrc/knn_point.hip) are declared, bound and exported;
bad arguments give status codes before anything touches the GPU; the host-only plan is the Python rule and both kernels
occur; the three ops are part of the drop-in surface and refuse what the reference's ops refuse, with matchable messages."""
import ctypes
import os
import re

import pytest
import torch

NEW_SYMBOLS = ("dh3d_select_top_k", "dh3d_knn_point", "dh3d_knn_point_plan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_declared_bound_and_exported():
    from dh3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(handle, name), name
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION   # additions only
    section = header[header.index("SelectionSort (select_top_k) and KnnPoint"):header.index("int dh3d_knn_point_plan")]
    for word in ("TIE ORDER", "ROW FORMAT", "ROUNDING"):
        assert word in section, word
    assert "INFERRED" in section                                      # the summation order for c > 3


def test_bad_arguments_are_status_codes():
    from dh3d_amd import _lib
    lib = _lib.lib()
    z, p = None, 256  # (a non-null fake pointer: every check below fails before a launch)

    def knn(b=2, n=100, m=10, c=3, k=8, x1=p, x2=p, val=p, idx=p):
        return lib.dh3d_knn_point(b, n, m, c, k, x1, x2, val, idx, None)

    def sel(b=2, n=100, m=10, k=8, dist=p, outi=p, out=p):
        return lib.dh3d_select_top_k(b, n, m, k, dist, outi, out, None)

    for f in (knn, sel):
        for kw in (dict(b=0), dict(b=-1), dict(n=0), dict(n=-5), dict(m=0), dict(m=-1), dict(k=0), dict(k=-3), dict(k=101),
                   dict(k=100, n=99)):
            assert f(**kw) == 1, (f.__name__, kw)
    for kw in (dict(c=0), dict(c=-3), dict(x1=z), dict(x2=z), dict(val=z), dict(idx=z)):
        assert knn(**kw) == 1, kw
    for kw in (dict(dist=z), dict(outi=z), dict(out=z)):
        assert sel(**kw) == 1, kw
    assert knn(n=5000, k=1025) == 2 and knn(n=5000, k=1025, c=7) == 2   # beyond the generic kernel's list


def test_plan_is_the_python_rule_and_both_kernels_occur():
    from dh3d_amd import _lib, pm
    lib = _lib.lib()
    seen = set()
    for n in (-1, 0, 1, 63, 64, 65, 1000, 4096, 16384, 100000):
        for m in (0, 1, 64, 1000, 100000):
            for c in (-1, 0, 1, 2, 3, 4, 16, 64):
                for k in (-1, 0, 1, 3, 8, 32, 64, 65, 128, 1024, 1025, 5000):
                    r = lib.dh3d_knn_point_plan(n, m, c, k)
                    assert r == pm.knn_point_plan(n, m, c, k), (n, m, c, k)
                    assert r in (-1, 0, 1)
                    if n <= 0 or m <= 0 or c <= 0 or k <= 0 or k > n:
                        assert r == -1
                    elif k <= 1024:
                        assert r == (1 if c == 3 and k <= 64 else 0)
                    seen.add(r)
    assert seen == {-1, 0, 1}


def test_ops_surface_and_refusals():
    from dh3d_amd import ops
    for name in ("knn_point", "select_top_k", "gather_point"):
        assert name in ops.__all__ and callable(getattr(ops, name))
    x1, x2 = torch.zeros(2, 50, 3), torch.zeros(2, 7, 3)
    # the operator's own refusals come before the device check, so a CPU run tells them from the CPU-tensor refusal
    for k in (0, -1, 51):
        with pytest.raises(ValueError, match="SelectionSort expects 1 <= k <= n"):
            ops.knn_point(k, x1, x2)
        with pytest.raises(ValueError, match="SelectionSort expects 1 <= k <= n"):
            ops.select_top_k(k, torch.zeros(2, 7, 50))
    with pytest.raises(ValueError, match="batch"):
        ops.knn_point(8, x1, x2[:1])
    with pytest.raises(ValueError, match="c\\(xyz1/xyz2\\)"):
        ops.knn_point(8, x1, x2[..., :2])
    with pytest.raises(ValueError, match="rank 3"):
        ops.knn_point(8, x1[0], x2)
    with pytest.raises(ValueError, match="rank 3"):
        ops.select_top_k(3, torch.zeros(7, 50))
    with pytest.raises(ValueError, match="float32"):
        ops.knn_point(8, x1.double(), x2.double())
    with pytest.raises(ValueError, match="GPU"):
        ops.knn_point(8, x1, x2)
    with pytest.raises(ValueError, match="GPU"):
        ops.select_top_k(8, torch.zeros(2, 7, 50))
    idx = torch.zeros(2, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match="GatherPoint expects \\(batch_size,num_points,3\\) inp shape"):
        ops.gather_point(torch.zeros(2, 50, 4), idx)
    with pytest.raises(ValueError, match="GatherPoint expects \\(batch_size,num_points,3\\) inp shape"):
        ops.gather_point(torch.zeros(50, 3), idx)
    with pytest.raises(ValueError, match="GatherPoint expects \\(batch_size,num_result\\) idx shape"):
        ops.gather_point(x1, idx[:1])
    with pytest.raises(ValueError, match="GatherPoint expects \\(batch_size,num_result\\) idx shape"):
        ops.gather_point(x1, idx[0])
    with pytest.raises(ValueError, match="int32"):
        ops.gather_point(x1, idx.long())
    with pytest.raises(ValueError, match="GPU"):
        ops.gather_point(x1, idx)
