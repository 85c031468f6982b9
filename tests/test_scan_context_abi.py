"""CPU: the Scan Context entry points (include/dh3d_hip.h, csrc/scan_context.hip) are declared, bound and exported; they add
no workspace query; every refusal is a status code before anything touches the GPU; the Python interface refuses what the
kernels do not take and keeps the signatures the module documents."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dh3d_scan_context", "dh3d_scan_context_distance")
F = 256  # a non-null, 16-byte-aligned fake pointer: every check below fails before a launch


def test_symbols_declared_bound_and_exported():
    from dh3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name), name
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION                     # an addition only
    makefile = open(os.path.join(ROOT, "dh3d_amd", "csrc", "Makefile")).read()
    exact = [ln for ln in makefile.splitlines() if ln.startswith("EXACT :=")][0]
    assert "scan_context.o" in exact.split()                                          # built without contraction
    said = header[header.index("Scan Context (csrc/scan_context.hip)"):header.index("int dh3d_scan_context(")]
    for word in ("rounded once in float32", "h > 0 strictly", "r2 >= ring_edge2[i]", "c_k * Y - s_k * X >= 0", "Y == 0 and X > 0",
                 "an empty bin holds 0", "bit-defined", "m_n == 0: d_n = 1.0", "smallest n", "+inf", "(j + n) % Ns",
                 "Every element", "graph-capturable", "no scratch memory"):
        assert word in said, word


def test_no_new_workspace_query():
    from dh3d_amd import _lib
    names = [n for n in _lib.EXPORTED_SYMBOLS if "scan_context" in n]
    assert sorted(names) == sorted(NEW_SYMBOLS)
    assert not [n for n in names if n.endswith(("_workspace", "_workspace_bytes", "_ws_bytes"))]


def _build(lib, xyz=F, stride=3, count=F, center=F, sector_dir=F, ring_edge2=F, P=2, N=1000, Nr=20, Ns=60, desc=F, key=F):
    return lib.dh3d_scan_context(xyz, stride, count, center, sector_dir, ring_edge2, P, N, Nr, Ns, 2.0, desc, key, None)


def _dist(lib, qry=F, mp=F, map_count=F, cand=F, Q=4, R=100, C=10, Nr=20, Ns=60, dist=F, shift=F, order=F):
    return lib.dh3d_scan_context_distance(qry, mp, map_count, cand, Q, R, C, Nr, Ns, dist, shift, order, None)


GRIDS_REFUSED = (dict(Nr=0), dict(Nr=3), dict(Nr=-4), dict(Nr=18), dict(Nr=36), dict(Ns=0), dict(Ns=4), dict(Ns=-8), dict(Ns=62),
                 dict(Ns=132))


def test_refusals():
    from dh3d_amd import _lib
    lib = _lib.lib()
    for kw in (dict(xyz=None), dict(sector_dir=None), dict(ring_edge2=None), dict(desc=None), dict(key=None), dict(stride=2),
               dict(stride=0), dict(P=0), dict(P=-1), dict(N=0), dict(N=-5)) + GRIDS_REFUSED:
        assert _build(lib, **kw) == 1, kw
    for kw in (dict(N=(1 << 20) + 1), dict(P=65536)):
        assert _build(lib, **kw) == 2, kw
    for kw in (dict(qry=None), dict(mp=None), dict(cand=None), dict(dist=None), dict(shift=None), dict(order=None), dict(Q=0),
               dict(Q=-1), dict(R=0), dict(R=-2), dict(C=0), dict(C=-1), dict(C=65)) + GRIDS_REFUSED:
        assert _dist(lib, **kw) == 1, kw
    for kw in (dict(Q=(1 << 20) + 1), dict(R=(1 << 24) + 1)):
        assert _dist(lib, **kw) == 2, kw
    assert _build(lib, N=(1 << 20) + 1, Nr=18) == 1 and _dist(lib, R=(1 << 24) + 1, C=65) == 1   # invalid before too large


def test_python_interface():
    from dh3d_amd import scancontext as sc
    a = torch.zeros(2, 50, 3)
    with pytest.raises(ValueError, match="GPU"):
        sc.scan_context(a)                                        # CPU tensors: there is no CPU path
    with pytest.raises(ValueError, match="GPU"):
        sc.scan_context_distance(torch.zeros(2, 20, 60), torch.zeros(3, 20, 60), torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="GPU"):
        sc.ScanContextIndex(8, device="cpu")
    with pytest.raises(ValueError, match=r"\[P, M, C\]"):
        sc.scan_context(a[0])
    for bad in ((18, 60), (36, 60), (20, 62), (20, 4), (20, 132)):
        with pytest.raises(ValueError, match="multiples of 4"):
            sc.tables(bad[0], bad[1], 80.0)
    with pytest.raises(ValueError, match="max_radius"):
        sc.tables(20, 60, 0.0)
    sig = inspect.signature(sc.scan_context)
    assert list(sig.parameters) == ["points", "num_valid", "center", "num_rings", "num_sectors", "max_radius", "z_offset"]
    assert [p.default for p in sig.parameters.values()][1:] == [None, None, 20, 60, 80.0, 2.0]
    sig = inspect.signature(sc.scan_context_distance)
    assert list(sig.parameters) == ["qry_desc", "map_desc", "cand", "map_count"] and sig.parameters["map_count"].default is None
    sig = inspect.signature(sc.ScanContextIndex.__init__)
    assert list(sig.parameters) == ["self", "capacity", "points", "num_rings", "num_sectors", "max_radius", "z_offset", "device"]
    assert [p.default for p in sig.parameters.values()][2:] == [0, 20, 60, 80.0, 2.0, "cuda"]
    sig = inspect.signature(sc.ScanContextIndex.add)
    assert list(sig.parameters) == ["self", "points", "num_valid", "pos", "center"]
    sig = inspect.signature(sc.ScanContextIndex.search)
    assert list(sig.parameters) == ["self", "points", "num_valid", "center", "k", "candidates"]
    assert [p.default for p in sig.parameters.values()][2:] == [None, None, 1, 10]
    sig = inspect.signature(sc.relocalize_scan_context)
    assert list(sig.parameters) == ["index", "points", "num_valid", "center", "k", "candidates", "refine"]
    assert [p.default for p in sig.parameters.values()][2:] == [None, None, 1, 10, None]
    assert sc.RINGS_MAX == 32 and sc.SECTORS_MAX == 128 and sc.CANDIDATES_MAX == 64
