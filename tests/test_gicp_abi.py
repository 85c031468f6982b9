"""CPU: the generalized ICP entry points (include/dh3d_hip.h, csrc/icp.hip) are declared, bound and exported; every refusal
is a status code before anything touches the GPU; the Python interface has the agreed signature and refuses what the kernels
do not take."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dh3d_icp_refine_gicp_ws_bytes", "dh3d_icp_refine_gicp")
F = 256  # a non-null, 16-byte-aligned fake pointer: every check below fails before a launch


def test_symbols_declared_bound_and_exported():
    from dh3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name), name
        assert header.index(name + "(") > header.index("int dh3d_scan_context_distance(")   # a new section, after all others
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION                          # an addition only
    assert _lib.lib().dh3d_icp_refine_gicp_ws_bytes.restype is ctypes.c_size_t
    makefile = open(os.path.join(ROOT, "dh3d_amd", "csrc", "Makefile")).read()
    exact = [ln for ln in makefile.splitlines() if ln.startswith("EXACT :=")][0]
    assert "icp.o" in exact                                                                # built without contraction
    section = header[header.index("Dense generalized (plane-to-plane) ICP refinement"):]
    for word in ("F_gicp", "every operation rounded on its own", "cof_00", "det = (W_00*cof_00 + W_01*cof_01) + W_02*cof_02",
                 "n_g < 3", "1e-12", "num_planar", "rmse_gicp", "xor 16", "graph-capturable", "Every element is written",
                 "does NOT take it out of the fit"):
        assert word in section, word
    src = open(os.path.join(ROOT, "dh3d_amd", "csrc", "icp.hip")).read()
    for kernel in ("icp_gicp_fit_kernel", "icp_gicp_stats_kernel"):
        assert "void %s(" % kernel in src, kernel
    assert src.count("Cholesky H = L L^T") == 1                                            # one solve for both linearised fits


def test_gicp_workspace_is_the_point_workspace():
    from dh3d_amd import _lib
    lib = _lib.lib()
    for P, Na, Nb in ((1, 64, 9), (2, 2048, 2048), (3, 16385, 5), (0, 5, 5), (1, 131073, 5), (65536, 5, 5), (1, 5, 0)):
        assert lib.dh3d_icp_refine_gicp_ws_bytes(P, Na, Nb) == lib.dh3d_icp_refine_ws_bytes(P, Na, Nb), (P, Na, Nb)
    assert lib.dh3d_icp_refine_gicp_ws_bytes(1, 131073, 5) == 0 and lib.dh3d_icp_refine_gicp_ws_bytes(1, 64, 9) > 0


def _gicp(lib, anchor=F, a_stride=3, a_count=F, a_normals=F, an_stride=3, b_normals=F, bn_stride=3, positive=F, b_stride=3,
          b_count=F, Rt0=F, valid0=F, P=2, Na=1000, Nb=900, max_dist=1.0, iterations=20, path=0, epsilon=1e-3, Rt=F, nn=F,
          num_corr=F, fitness=F, rmse=F, valid=F, num_planar=F, rmse_gicp=F, ws=F, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dh3d_icp_refine_gicp_ws_bytes(P, Na, Nb) or (1 << 40)
    return lib.dh3d_icp_refine_gicp(anchor, a_stride, a_count, a_normals, an_stride, b_normals, bn_stride, positive, b_stride,
                                    b_count, Rt0, valid0, P, Na, Nb, max_dist, iterations, path, epsilon, Rt, nn, num_corr,
                                    fitness, rmse, valid, num_planar, rmse_gicp, ws, ws_bytes, None)


def test_gicp_refusals():
    from dh3d_amd import _lib
    lib = _lib.lib()
    small = lib.dh3d_icp_refine_gicp_ws_bytes(2, 1000, 900) - 1
    nan = float("nan")
    for kw in (dict(a_normals=None), dict(b_normals=None), dict(an_stride=2), dict(bn_stride=2), dict(bn_stride=0),
               dict(num_planar=None), dict(rmse_gicp=None), dict(epsilon=0.0), dict(epsilon=-1e-3), dict(epsilon=1.5),
               dict(epsilon=nan), dict(epsilon=float("inf")),
               dict(anchor=None), dict(positive=None), dict(Rt0=None), dict(Rt=None), dict(nn=None), dict(num_corr=None),
               dict(fitness=None), dict(rmse=None), dict(valid=None), dict(P=0), dict(Na=0), dict(Nb=-5), dict(a_stride=2),
               dict(b_stride=0), dict(max_dist=0.0), dict(max_dist=nan), dict(iterations=-1), dict(path=3), dict(ws=None),
               dict(ws=264), dict(ws_bytes=0), dict(ws_bytes=small)):
        assert _gicp(lib, **kw) == 1, kw
    for kw in (dict(Na=131073), dict(Nb=131073), dict(P=65536), dict(iterations=257), dict(Na=16385, path=2)):
        assert _gicp(lib, **kw) == 2, kw


def test_python_interface():
    from dh3d_amd import registration as reg
    a, b = torch.zeros(2, 50, 3), torch.zeros(2, 40, 3)
    Rt = torch.zeros(2, 3, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU"):
        reg.refine_icp_gicp(a, b, Rt, anchor_normals=a, positive_normals=b)       # CPU tensors: there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        reg.refine_pose(a, b, Rt, method="gicp")                                  # ... and not "method must be"
    with pytest.raises(ValueError, match="method must be"):
        reg.refine_pose(a, b, Rt, method="generalized")
    gicp, plane = inspect.signature(reg.refine_icp_gicp), inspect.signature(reg.refine_icp_plane)
    assert list(gicp.parameters) == list(plane.parameters) + ["positive_normals", "epsilon"]
    assert all(gicp.parameters[k].default == plane.parameters[k].default for k in plane.parameters)
    assert (gicp.parameters["positive_normals"].default, gicp.parameters["epsilon"].default) == (None, 1e-3)
    assert inspect.signature(reg.refine_pose).parameters["method"].default == "point"
    for fn in (reg.refine_icp_gicp, reg.register_clouds, reg.register_fpfh):
        assert "rmse_gicp" in fn.__doc__ and "num_planar" in fn.__doc__, fn.__name__
    from dh3d_amd import retrieval, scancontext
    for fn in (retrieval.PlaceIndex.localize, scancontext.relocalize_scan_context):
        assert "rmse_gicp" in fn.__doc__, fn.__name__
