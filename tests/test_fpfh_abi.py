"""CPU: the FPFH entry points (include/dh3d_hip.h, csrc/fpfh.hip) are declared, bound and exported; every refusal is a status
code before anything touches the GPU; the count rows are an output, not a new workspace query; the Python interface
refuses what the kernels do not take and keeps the signatures the issue names."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dh3d_spfh_counts", "dh3d_fpfh")
F = 256  # a non-null, 16-byte-aligned fake pointer: every check below fails before a launch


def test_symbols_declared_bound_and_exported():
    from dh3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name), name
        assert header.index(name + "(") > header.index("int dh3d_estimate_normals(")   # after the normals it consumes
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION                     # an addition only
    makefile = open(os.path.join(ROOT, "dh3d_amd", "csrc", "Makefile")).read()
    exact = [ln for ln in makefile.splitlines() if ln.startswith("EXACT :=")][0]
    assert "fpfh.o" in exact                                                          # built without contraction
    said = header[header.index("FPFH descriptors from given normals"):header.index("int dh3d_fpfh(")]
    for word in ("NEAR", "USABLE", "|a1| < |a2|", "11 / (2 pi)", "floor(s)", "1.0 / d2", "list order", "ascending order",
                 "counts [P, N, 36] uint8", "columns 33-35 are zero", "INFERRED", "graph-capturable", "Every element is written"):
        assert word in said, word


def test_no_new_workspace_query():
    from dh3d_amd import _lib
    for name in _lib.EXPORTED_SYMBOLS:
        if "fpfh" in name or "spfh" in name:
            assert name in NEW_SYMBOLS, name
    assert not [s for s in NEW_SYMBOLS if s.endswith(("_workspace", "_workspace_bytes", "_ws_bytes"))]
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    said = header[header.index("FPFH descriptors from given normals"):header.index("int dh3d_fpfh(")]
    assert "workspace" not in said and "output of the caller's" in said


def _counts(lib, xyz=F, xs=3, normals=F, ns=3, count=F, nbr=F, P=2, N=1000, K=16, max_dist=0.0, counts=F):
    return lib.dh3d_spfh_counts(xyz, xs, normals, ns, count, nbr, P, N, K, max_dist, counts, None)


def _fpfh(lib, xyz=F, xs=3, count=F, nbr=F, counts=F, ids=F, P=2, N=1000, K=16, M=100, max_dist=0.0, out=F):
    return lib.dh3d_fpfh(xyz, xs, count, nbr, counts, ids, P, N, K, M, max_dist, out, None)


def test_refusals():
    from dh3d_amd import _lib
    lib = _lib.lib()
    for kw in (dict(xyz=None), dict(normals=None), dict(nbr=None), dict(counts=None), dict(counts=258), dict(xs=2), dict(ns=2),
               dict(ns=0), dict(P=0), dict(N=0), dict(N=-3), dict(K=0), dict(K=-1), dict(K=65)):
        assert _counts(lib, **kw) == 1, kw
    for kw in (dict(N=131073), dict(P=65536)):
        assert _counts(lib, **kw) == 2, kw
    for kw in (dict(xyz=None), dict(nbr=None), dict(counts=None), dict(counts=257), dict(out=None), dict(xs=2), dict(P=0),
               dict(N=0), dict(M=0), dict(M=-1), dict(K=0), dict(K=65), dict(ids=None, M=100), dict(ids=None, M=1001)):
        assert _fpfh(lib, **kw) == 1, kw
    for kw in (dict(N=131073), dict(M=131073), dict(P=65536)):
        assert _fpfh(lib, **kw) == 2, kw


def test_python_interface():
    from dh3d_amd import registration as reg
    a = torch.zeros(2, 50, 3)
    with pytest.raises(ValueError, match="GPU"):
        reg.compute_fpfh(a)                                       # CPU tensors: there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        reg.register_fpfh(a, a)
    with pytest.raises(ValueError, match=r"\[P, M, C\]"):
        reg.compute_fpfh(a[0])
    with pytest.raises(ValueError, match="max_dist"):
        reg._max_dist(0.0, "compute_fpfh")
    with pytest.raises(ValueError, match="max_dist"):
        reg._max_dist(float("inf"), "compute_fpfh")
    assert reg._max_dist(None, "x") == 0.0 and reg._max_dist(1.5, "x") == 1.5
    sig = inspect.signature(reg.compute_fpfh)
    assert list(sig.parameters) == ["points", "normals", "num_valid", "k", "max_dist", "nbr", "ids", "normals_k", "viewpoint"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["normals"], d["num_valid"], d["k"], d["max_dist"], d["nbr"], d["ids"], d["normals_k"], d["viewpoint"]) == \
        (None, None, 32, None, None, None, 16, (0., 0., 0.))
    sig = inspect.signature(reg.register_fpfh)
    assert list(sig.parameters) == ["anchor_points", "positive_points", "num_valid", "keypoints", "keypoint_ids", "k",
                                    "max_dist", "refine", "ransac_kw"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["num_valid"], d["keypoints"], d["keypoint_ids"], d["k"], d["max_dist"], d["refine"]) == (None, None, None, 32, None, None)
    assert reg.FPFH_COLS == 36 and reg.FPFH_COLS % 4 == 0 and reg.FPFH_COLS <= reg.DESC_MAX   # match_descriptors reads the rows
