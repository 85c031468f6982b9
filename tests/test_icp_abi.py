"""CPU: the ICP entry points (include/dh3d_hip.h "Dense point-to-point ICP", csrc/icp.hip) are declared, bound and
exported; every refusal is a status code before anything touches the GPU; the workspace is 0 exactly where the plan
refuses; the Python wrapper refuses what the kernels do not take."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dh3d_icp_plan", "dh3d_icp_refine_ws_bytes", "dh3d_icp_refine")
F = 256  # a non-null, 16-byte-aligned fake pointer: every check below fails before a launch


def test_symbols_declared_bound_and_exported():
    from dh3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name), name
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION   # an addition only
    section = header[header.index("Dense point-to-point ICP"):header.index("int dh3d_icp_plan")]
    for word in ("ASSOCIATION", "FIT", "LOOP", "strict", "lowest i", "ascending j", "No early exit", "Every element is written",
                 "graph-capturable", "no\n *   floating-point atomics"):
        assert word in section, word
    makefile = open(os.path.join(ROOT, "dh3d_amd", "csrc", "Makefile")).read()
    exact = [ln for ln in makefile.splitlines() if ln.startswith("EXACT :=")][0]
    assert "icp.o" in exact                    # the -ffp-contract=off group: the ids depend on d2's roundings
    assert "rigid_fit.h" in [ln for ln in makefile.splitlines() if ln.startswith("$(EXACT):")][0]
    # one copy of the fit: registration.hip and icp.hip include it, neither defines it
    csrc = os.path.join(ROOT, "dh3d_amd", "csrc")
    for f in ("registration.hip", "icp.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "rigid_fit.h"' in text and "void rotation_from_b(" not in text and "void accumulate_b(" not in text, f


def test_plan_and_workspace():
    from dh3d_amd import _lib
    lib = _lib.lib()
    plan, ws = lib.dh3d_icp_plan, lib.dh3d_icp_refine_ws_bytes
    assert plan(16384, 8192) == 2 and plan(16385, 8192) == 1 and plan(1, 1) == 2 and plan(131072, 131072) == 1
    for Na in (-1, 0, 1, 63, 64, 2048, 16384, 16385, 131072, 131073):
        for Nb in (-1, 0, 1, 8192, 131072, 131073):
            refused = plan(Na, Nb) == -1
            assert refused == (not (0 < Na <= 131072 and 0 < Nb <= 131072)), (Na, Nb)
            assert (ws(1, Na, Nb) == 0) == refused and (ws(65535, Na, Nb) == 0) == refused, (Na, Nb)
            assert ws(0, Na, Nb) == 0 and ws(-1, Na, Nb) == 0 and ws(65536, Na, Nb) == 0
    # the working pose always (96 bytes a pair); up to 16384 anchors also the sort's outputs (16 Na + 32 ceil(Na / 64) +
    # 4 * 4112 bytes a pair) and the anchor without its stride (12 Na), every segment padded to 16 bytes
    assert ws(1, 16385, 5) == 96 and ws(3, 131072, 131072) == 288
    assert ws(1, 64, 9) == 96 + 1024 + 32 + 16448 + 768 == ws(1, 64, 16385)
    assert ws(2, 2048, 2048) == 2 * (96 + 16 * 2048 + 32 * 32 + 16448 + 12 * 2048)
    assert all(ws(P, Na, 7) % 16 == 0 for P in (1, 3, 5) for Na in (1, 3, 65, 1000))


def _refine(lib, anchor=F, a_stride=3, a_count=F, positive=F, b_stride=3, b_count=F, Rt0=F, valid0=F, P=2, Na=1000, Nb=900,
            max_dist=1.0, iterations=20, path=0, Rt=F, nn=F, num_corr=F, fitness=F, rmse=F, valid=F, ws=F, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dh3d_icp_refine_ws_bytes(P, Na, Nb) or (1 << 40)
    return lib.dh3d_icp_refine(anchor, a_stride, a_count, positive, b_stride, b_count, Rt0, valid0, P, Na, Nb, max_dist,
                               iterations, path, Rt, nn, num_corr, fitness, rmse, valid, ws, ws_bytes, None)


def test_bad_arguments_are_status_1():
    from dh3d_amd import _lib
    lib = _lib.lib()
    small = lib.dh3d_icp_refine_ws_bytes(2, 1000, 900) - 1
    nan, inf = float("nan"), float("inf")
    for kw in (dict(anchor=None), dict(positive=None), dict(Rt0=None), dict(Rt=None), dict(nn=None), dict(num_corr=None),
               dict(fitness=None), dict(rmse=None), dict(valid=None), dict(P=0), dict(P=-1), dict(Na=0), dict(Nb=0), dict(Nb=-5),
               dict(a_stride=2), dict(b_stride=0), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=nan),
               dict(max_dist=inf), dict(iterations=-1), dict(path=3), dict(path=-1), dict(ws=None), dict(ws=264),
               dict(ws_bytes=0), dict(ws_bytes=small)):
        assert _refine(lib, **kw) == 1, kw


def test_unsupported_shapes_are_status_2():
    from dh3d_amd import _lib
    lib = _lib.lib()
    for kw in (dict(Na=131073), dict(Nb=131073), dict(P=65536), dict(iterations=257), dict(Na=16385, path=2)):
        assert _refine(lib, **kw) == 2, kw


def test_python_wrapper_refusals():
    from dh3d_amd import registration as reg
    from dh3d_amd import retrieval
    a, b = torch.zeros(2, 50, 3), torch.zeros(2, 40, 3)
    Rt = torch.zeros(2, 3, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU"):
        reg.refine_icp(a, b, Rt)                                  # CPU tensors: there is no CPU path
    with pytest.raises(ValueError, match="float32"):
        reg.refine_icp(a.double(), b, Rt)
    for bad in (a[0], a.reshape(2, 150), a.int()):               # wrong rank or dtype
        with pytest.raises(ValueError, match=r"\[P, M, C\]"):
            reg.refine_icp(bad, b, Rt)
        with pytest.raises(ValueError, match=r"\[P, M, C\]"):
            reg.refine_icp(a, bad, Rt)
    with pytest.raises(ValueError, match="refine must be"):
        reg._refine_kw("yes")
    assert reg._refine_kw(None) is None and reg._refine_kw(True) == {} and reg._refine_kw(dict(max_dist=2.0)) == dict(max_dist=2.0)
    import inspect
    sig = inspect.signature(reg.refine_icp)
    assert list(sig.parameters) == ["anchor_points", "positive_points", "Rt", "valid", "anchor_count", "positive_count",
                                    "max_dist", "iterations", "path"]
    assert (sig.parameters["max_dist"].default, sig.parameters["iterations"].default, sig.parameters["path"].default) == (1.0, 20, 0)
    assert inspect.signature(reg.register_clouds).parameters["refine"].default is None
    assert inspect.signature(retrieval.relocalize_clouds).parameters["refine"].default is None
    assert inspect.signature(retrieval.PlaceIndex.localize).parameters["refine"].default is None
    assert inspect.signature(retrieval.PlaceIndex.__init__).parameters["points"].default == 0
    assert "12 * points bytes" in retrieval.PlaceIndex.__doc__
    with pytest.raises(ValueError):
        retrieval.PlaceIndex(points=-1)
