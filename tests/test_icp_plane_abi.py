"""CPU: the normals and point-to-plane ICP entry points (include/dh3d_hip.h, csrc/normals.hip, csrc/icp.hip) are declared,
bound and exported; every refusal is a status code before anything touches the GPU; the Python interface refuses what the
kernels do not take and leaves refine_icp as it was."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dh3d_estimate_normals", "dh3d_icp_refine_plane_ws_bytes", "dh3d_icp_refine_plane")
F = 256  # a non-null, 16-byte-aligned fake pointer: every check below fails before a launch


def test_symbols_declared_bound_and_exported():
    from dh3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name), name
        assert header.index(name + "(") > header.index("int dh3d_icp_refine(")       # after the point-to-point section
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION                   # an addition only
    makefile = open(os.path.join(ROOT, "dh3d_amd", "csrc", "Makefile")).read()
    exact = [ln for ln in makefile.splitlines() if ln.startswith("EXACT :=")][0]
    assert "normals.o" in exact and "icp.o" in exact                                # built without contraction
    csrc = os.path.join(ROOT, "dh3d_amd", "csrc")
    assert "smallest_eigenvector_3(" in open(os.path.join(csrc, "rigid_fit.h")).read()
    assert '#include "rigid_fit.h"' in open(os.path.join(csrc, "normals.hip")).read()
    for word in ("F_plane", "Cholesky", "1e-12", "n_pl < 6", "num_plane", "rmse_plane", "graph-capturable", "list order",
                 "first smallest", "Every element is written"):
        assert word in header[header.index("Surface normals from given neighbour lists"):], word


def test_plane_workspace_is_the_point_workspace():
    from dh3d_amd import _lib
    lib = _lib.lib()
    for P, Na, Nb in ((1, 64, 9), (2, 2048, 2048), (3, 16385, 5), (0, 5, 5), (1, 131073, 5), (65536, 5, 5), (1, 5, 0)):
        assert lib.dh3d_icp_refine_plane_ws_bytes(P, Na, Nb) == lib.dh3d_icp_refine_ws_bytes(P, Na, Nb), (P, Na, Nb)
    assert lib.dh3d_icp_refine_plane_ws_bytes(1, 131073, 5) == 0 and lib.dh3d_icp_refine_plane_ws_bytes(1, 64, 9) > 0


def _plane(lib, anchor=F, a_stride=3, a_count=F, normals=F, n_stride=3, positive=F, b_stride=3, b_count=F, Rt0=F, valid0=F, P=2,
           Na=1000, Nb=900, max_dist=1.0, iterations=20, path=0, Rt=F, nn=F, num_corr=F, fitness=F, rmse=F, valid=F, num_plane=F,
           rmse_plane=F, ws=F, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dh3d_icp_refine_plane_ws_bytes(P, Na, Nb) or (1 << 40)
    return lib.dh3d_icp_refine_plane(anchor, a_stride, a_count, normals, n_stride, positive, b_stride, b_count, Rt0, valid0, P,
                                     Na, Nb, max_dist, iterations, path, Rt, nn, num_corr, fitness, rmse, valid, num_plane,
                                     rmse_plane, ws, ws_bytes, None)


def test_plane_refusals():
    from dh3d_amd import _lib
    lib = _lib.lib()
    small = lib.dh3d_icp_refine_plane_ws_bytes(2, 1000, 900) - 1
    nan = float("nan")
    for kw in (dict(normals=None), dict(n_stride=2), dict(n_stride=0), dict(num_plane=None), dict(rmse_plane=None),
               dict(anchor=None), dict(positive=None), dict(Rt0=None), dict(Rt=None), dict(nn=None), dict(num_corr=None),
               dict(fitness=None), dict(rmse=None), dict(valid=None), dict(P=0), dict(Na=0), dict(Nb=-5), dict(a_stride=2),
               dict(b_stride=0), dict(max_dist=0.0), dict(max_dist=nan), dict(iterations=-1), dict(path=3), dict(ws=None),
               dict(ws=264), dict(ws_bytes=0), dict(ws_bytes=small)):
        assert _plane(lib, **kw) == 1, kw
    for kw in (dict(Na=131073), dict(Nb=131073), dict(P=65536), dict(iterations=257), dict(Na=16385, path=2)):
        assert _plane(lib, **kw) == 2, kw


def _normals(lib, xyz=F, stride=3, count=F, nbr=F, P=2, N=1000, K=16, view=True, normals=F, curvature=F):
    vp = (ctypes.c_double * 3)(0.0, 0.0, 0.0) if view else None
    return lib.dh3d_estimate_normals(xyz, stride, count, nbr, P, N, K, vp, normals, curvature, None)


def test_normals_refusals():
    from dh3d_amd import _lib
    lib = _lib.lib()
    for kw in (dict(xyz=None), dict(nbr=None), dict(view=False), dict(normals=None), dict(curvature=None), dict(stride=2),
               dict(P=0), dict(N=0), dict(N=-3), dict(K=0), dict(K=-1)):
        assert _normals(lib, **kw) == 1, kw
    for kw in (dict(K=65), dict(N=131073), dict(P=65536)):
        assert _normals(lib, **kw) == 2, kw


def test_python_interface_refusals():
    from dh3d_amd import registration as reg
    a, b = torch.zeros(2, 50, 3), torch.zeros(2, 40, 3)
    Rt = torch.zeros(2, 3, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="GPU"):
        reg.estimate_normals(a)                                   # CPU tensors: there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        reg.refine_icp_plane(a, b, Rt, anchor_normals=a)
    with pytest.raises(ValueError, match=r"\[P, M, C\]"):
        reg.estimate_normals(a[0])
    with pytest.raises(ValueError, match="method must be"):
        reg.refine_pose(a, b, Rt, method="planes")
    with pytest.raises(ValueError, match="viewpoint"):
        reg._viewpoint((0.0, 1.0))
    with pytest.raises(ValueError, match="viewpoint"):
        reg._viewpoint((0.0, 1.0, float("nan")))
    sig = inspect.signature(reg.estimate_normals)
    assert list(sig.parameters) == ["points", "num_valid", "k", "viewpoint", "nbr"]
    assert (sig.parameters["k"].default, sig.parameters["viewpoint"].default, sig.parameters["nbr"].default) == (16, (0., 0., 0.), None)
    plane, point = inspect.signature(reg.refine_icp_plane), inspect.signature(reg.refine_icp)
    assert list(plane.parameters) == list(point.parameters) + ["anchor_normals", "normals_k", "viewpoint"]
    assert all(plane.parameters[k].default == point.parameters[k].default for k in point.parameters)
    assert (plane.parameters["anchor_normals"].default, plane.parameters["normals_k"].default) == (None, 16)
    assert inspect.signature(reg.refine_pose).parameters["method"].default == "point"
    assert "num_valid" in reg.estimate_normals.__doc__ and "padding" in reg.estimate_normals.__doc__
