"""CPU: the prepare_clouds entry points (include/dh3d_hip.h, csrc/prepare.hip) are declared, bound and exported; bad arguments
and oversize shapes give status codes before anything touches the GPU; the workspace size grows with the shape; the Python
entry point refuses what is not on the device before it looks at where the tensors live."""
import ctypes
import os
import re

import pytest
import torch

NEW_SYMBOLS = ("dh3d_prepare_clouds", "dh3d_prepare_clouds_workspace")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_declared_bound_and_exported():
    from dh3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert re.search(r"\bint\s+dh3d_prepare_clouds\s*\(", header)
    assert re.search(r"\bsize_t\s+dh3d_prepare_clouds_workspace\s*\(", header)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(handle, name), name
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION   # additions only
    section = header[header.index("Preparation of raw clouds"):header.index("size_t dh3d_prepare_clouds_workspace")]
    for word in ("STAGE 1", "STAGE 2", "STAGE 3", "LIMITS"):
        assert word in section, word
    assert section.count("INFERRED") >= 4      # origin, summation order, strict <, more than nb_points with self
    kernel = open(os.path.join(ROOT, "dh3d_amd", "csrc", "prepare.hip")).read()
    assert kernel.count("INFERRED") >= 4
    makefile = open(os.path.join(ROOT, "dh3d_amd", "csrc", "Makefile")).read()
    exact = [ln for ln in makefile.splitlines() if ln.startswith("EXACT :=")][0]
    assert "prepare.o" in exact                # the -ffp-contract=off group


def _call(lib, B=2, Nraw=1000, targetnum=256, raw=256, num_raw=256, voxel=0.2, radius=1.0, nb=4, sortby=1, points=256,
          num_valid=256, counts=256, centroid=256, ws=256, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dh3d_prepare_clouds_workspace(B, Nraw, targetnum) or (1 << 40)
    return lib.dh3d_prepare_clouds(B, Nraw, targetnum, raw, num_raw, voxel, radius, nb, sortby, points, num_valid, counts,
                                   centroid, ws, ws_bytes, None)


def test_bad_arguments_are_status_1():
    from dh3d_amd import _lib
    lib = _lib.lib()
    # (256: a non-null, 16-byte-aligned fake pointer -- every check below fails before a launch)
    for kw in (dict(B=0), dict(B=-1), dict(Nraw=0), dict(Nraw=-7), dict(targetnum=0), dict(targetnum=-1), dict(raw=None),
               dict(num_raw=None), dict(points=None), dict(num_valid=None), dict(counts=None), dict(centroid=None),
               dict(ws=None), dict(voxel=-0.2), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(radius=-1.0),
               dict(radius=float("nan")), dict(radius=float("inf")), dict(nb=-1), dict(ws_bytes=0), dict(ws=264),
               dict(ws_bytes=lib.dh3d_prepare_clouds_workspace(2, 1000, 256) - 1)):
        assert _call(lib, **kw) == 1, kw


def test_oversize_shapes_are_status_2():
    from dh3d_amd import _lib, pm
    lib = _lib.lib()
    assert pm.PREPARE_MAX_N == 131072 and pm.PREPARE_MAX_TARGET == 1 << 20
    for kw in (dict(Nraw=131073), dict(Nraw=1 << 20), dict(targetnum=(1 << 20) + 1), dict(B=65536)):
        assert _call(lib, **kw) == 2, kw
        shape = dict(dict(B=2, Nraw=1000, targetnum=256), **kw)
        assert lib.dh3d_prepare_clouds_workspace(shape["B"], shape["Nraw"], shape["targetnum"]) == 0
    assert lib.dh3d_prepare_clouds_workspace(1, 131072, 1 << 20) > 0
    for bad in ((0, 10, 10), (1, 0, 10), (1, 10, 0), (-1, 10, 10)):
        assert lib.dh3d_prepare_clouds_workspace(*bad) == 0


def test_workspace_grows_monotonically():
    from dh3d_amd import _lib
    f = _lib.lib().dh3d_prepare_clouds_workspace
    sizes = (1, 2, 63, 64, 65, 1000, 1024, 1025, 4096, 9000, 16384, 16385, 32768, 60300, 65536, 100000, 131072)
    for B in (1, 2, 8, 32):
        row = [f(B, n, 8192) for n in sizes]
        assert all(v > 0 and v % 16 == 0 for v in row) and row == sorted(row), (B, row)
    for n in (1000, 65536):
        col = [f(B, n, 8192) for B in (1, 2, 3, 8, 32, 100)]
        assert col == sorted(col) and len(set(col)) == len(col), (n, col)
    assert f(1, 1000, 64) <= f(1, 1000, 65536)
    # every point has room: two table slots, its list links, both intermediate clouds
    assert f(1, 131072, 8192) >= 131072 * (2 * 8 + 2 * 12)


def test_python_entry_point_refusals():
    from dh3d_amd import pm, utils
    raw, num = torch.zeros(2, 50, 3), torch.full((2,), 50, dtype=torch.int32)
    # what the op itself refuses comes before the device check, so a CPU run tells the two kinds of refusal apart
    with pytest.raises(NotImplementedError, match="get_fixednum_pcd"):
        utils.prepare_clouds(raw, num, 64, randsample=True)
    with pytest.raises(ValueError, match="targetnum"):
        utils.prepare_clouds(raw, num, 0)
    with pytest.raises(ValueError, match=r"\(batch_size,nraw,3\)"):
        utils.prepare_clouds(raw[0], num, 64)
    with pytest.raises(ValueError, match=r"\(batch_size,nraw,3\)"):
        utils.prepare_clouds(torch.zeros(2, 50, 4), num, 64)
    with pytest.raises(ValueError, match="num_raw"):
        utils.prepare_clouds(raw, num[:1], 64)
    with pytest.raises(ValueError, match="num_raw"):
        utils.prepare_clouds(raw, num.reshape(2, 1), 64)
    with pytest.raises(ValueError, match="beyond the kernels"):
        utils.prepare_clouds(torch.zeros(1, 131073, 3), num[:1], 64)
    with pytest.raises(ValueError, match="voxel_size"):
        utils.prepare_clouds(raw, num, 64, voxel_size=0.0)
    with pytest.raises(ValueError, match="radius"):
        utils.prepare_clouds(raw, num, 64, radius=-1.0)
    with pytest.raises(ValueError, match="nb_points"):
        utils.prepare_clouds(raw, num, 64, nb_points=-1)
    with pytest.raises(ValueError, match="float32"):
        utils.prepare_clouds(raw.double(), num, 64)
    with pytest.raises(ValueError, match="int32"):
        utils.prepare_clouds(raw, num.long(), 64)
    with pytest.raises(ValueError, match="GPU"):
        utils.prepare_clouds(raw, num, 64)
    with pytest.raises(ValueError, match="GPU"):
        pm.prepare_clouds(raw, num, 64, voxel_size=None, radius=None)
    assert "prepare_clouds" in utils.get_fixednum_pcd.__doc__          # the host function points to the device one
    assert "permutation" in utils.prepare_clouds.__doc__               # the kept points are not shuffled: said so
