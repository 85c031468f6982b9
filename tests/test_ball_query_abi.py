"""CPU: the ball-query entry points (include/dh3d_hip.h, csrc/ball_query.hip) are declared, bound and exported; bad
arguments give status codes before anything touches the GPU; the host-only plan is the Python dispatcher's rule; the ops are
part of the drop-in surface and refuse what the reference's op refuses."""
import ctypes
import os
import re

import pytest
import torch

NEW_SYMBOLS = ("dh3d_query_ball_point", "dh3d_query_ball_point2", "dh3d_query_ball_point_grid",
               "dh3d_query_ball_point_plan")
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
    for word in ("EMPTY BALL", "ROW FORMAT", "ROUNDING"):
        assert word in header


def test_bad_arguments_are_status_codes():
    from dh3d_amd import _lib
    lib = _lib.lib()
    z, p = None, 256  # (a non-null fake pointer: every check below fails before a launch)

    def q1(b=2, n=100, m=10, r=0.5, k=8, x1=p, x2=p, idx=p, cnt=p):
        return lib.dh3d_query_ball_point(b, n, m, r, k, x1, x2, idx, cnt, None)

    def q2(b=2, n=100, m=10, k=8, x1=p, x2=p, rad=p, idx=p, cnt=p):
        return lib.dh3d_query_ball_point2(b, n, m, k, x1, x2, rad, idx, cnt, None)

    def qg(b=2, n=100, m=10, rad=p, per=0, k=8, srt=p, gbox=p, cells=p, x2=p, idx=p, cnt=p):
        return lib.dh3d_query_ball_point_grid(b, n, m, rad, per, k, srt, gbox, cells, x2, idx, cnt, None)

    for f in (q1, q2, qg):
        for kw in (dict(b=0), dict(n=0), dict(m=0), dict(k=0), dict(k=-3), dict(x2=z), dict(idx=z), dict(cnt=z)):
            assert f(**kw) == 1, (f.__name__, kw)
    assert q1(x1=z) == 1 and q2(x1=z) == 1 and q2(rad=z) == 1
    assert q1(r=0.0) == 1 and q1(r=-1.0) == 1 and q1(r=float("nan")) == 1
    assert qg(rad=z) == 1 and qg(srt=z) == 1 and qg(gbox=z) == 1 and qg(cells=z) == 1
    assert qg(n=16385) == 2   # beyond the spatial sort


def test_plan_is_the_dispatchers_rule():
    from dh3d_amd import _lib, pm
    lib = _lib.lib()
    seen = set()
    for n in (-1, 0, 1, 63, 64, 65, 1000, 2047, 2048, 2049, 4096, 8192, 16384, 16385, 20000, 100000):
        for m in (0, 1, 64, 1000, 8192, 100000):
            for k in (0, 1, 8, 32, 64, 128, 1000):
                r = lib.dh3d_query_ball_point_plan(n, m, k)
                assert r == pm.ball_query_plan(n, m, k), (n, m, k)
                assert r in (-1, 0, 1) and (r == -1) == (n <= 0 or m <= 0 or k <= 0)
                if n > 16384:
                    assert r != 1
                seen.add(r)
    assert seen >= {-1, 0}


def test_ops_surface_and_refusals():
    from dh3d_amd import ops
    assert "query_ball_point" in ops.__all__ and "query_ball_point2" in ops.__all__
    x1, x2 = torch.zeros(2, 50, 3), torch.zeros(2, 7, 3)
    with pytest.raises(ValueError):
        ops.query_ball_point(0.5, 8, x1, x2)                      # CPU tensors
    with pytest.raises(ValueError):
        ops.query_ball_point2(torch.ones(2, 7), 8, x1, x2)        # CPU tensors
    for bad_r in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            ops.query_ball_point(bad_r, 8, x1, x2)
    with pytest.raises(ValueError):
        ops.query_ball_point2(0.5, 8, x1, x2)                     # radii must be a tensor
    # the operator's own refusals come before the device check, so a CPU run tells them from the CPU-tensor refusal
    for k in (0, -1):
        with pytest.raises(ValueError, match="positive nsample"):
            ops.query_ball_point(0.5, k, x1, x2)
        with pytest.raises(ValueError, match="positive nsample"):
            ops.query_ball_point2(torch.ones(2, 7), k, x1, x2)
    with pytest.raises(ValueError, match="positive radius"):
        ops.query_ball_point(0.0, 8, x1, x2)
    with pytest.raises(ValueError, match="batch"):
        ops.query_ball_point(0.5, 8, x1, x2[:1])
    with pytest.raises(ValueError, match="batch"):
        ops.query_ball_point2(torch.ones(2, 7), 8, x1[:1], x2)
    with pytest.raises(ValueError, match="GPU"):
        ops.query_ball_point(0.5, 8, x1, x2)


@pytest.mark.gpu
def test_ops_refusals_on_device_tensors(dev):
    from dh3d_amd import ops
    x1, x2 = torch.zeros(2, 50, 3, device=dev), torch.zeros(2, 7, 3, device=dev)
    for call in (lambda: ops.query_ball_point(0.5, 0, x1, x2), lambda: ops.query_ball_point(0.5, -1, x1, x2),
                 lambda: ops.query_ball_point(0.0, 8, x1, x2),
                 lambda: ops.query_ball_point(0.5, 8, x1, x2[:1]),                    # mismatched batch
                 lambda: ops.query_ball_point(0.5, 8, x1.double(), x2),               # dtype
                 lambda: ops.query_ball_point(0.5, 8, x1[..., :2], x2),               # not xyz
                 lambda: ops.query_ball_point(0.5, 8, x1[0], x2),                     # rank
                 lambda: ops.query_ball_point2(torch.ones(2, 8, device=dev), 8, x1, x2),   # radii shape
                 lambda: ops.query_ball_point2(torch.ones(2, 7, device=dev), 0, x1, x2)):
        with pytest.raises(ValueError):
            call()
