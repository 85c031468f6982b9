"""CPU: the training-batch entry points (include/dh3d_hip.h "Training batches", csrc/pairs.hip) are declared, bound and
exported; every refusal is a status code before anything touches the GPU; the Python module refuses what the kernels do
not take before it looks at where the tensors live."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dh3d_resample_clouds_ws_bytes", "dh3d_resample_clouds", "dh3d_augment_clouds", "dh3d_pair_rotate",
               "dh3d_sample_pair_nodes")
P = 256  # a non-null, 16-byte-aligned fake pointer: every check below fails before a launch


def test_symbols_declared_bound_and_exported():
    from dh3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(handle, name), name
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION   # additions only
    section = header[header.index("Training batches"):header.index("int dh3d_sample_pair_nodes")]
    for word in ("RANDOMNESS", "splitmix64", "1 resample keys", "10 first pick", "Box-Muller", "DEVICE pointer", "FIRST position",
                 "lowest j", "rounded ONCE", "graph-capturable"):
        assert word in section, word
    makefile = open(os.path.join(ROOT, "dh3d_amd", "csrc", "Makefile")).read()
    exact = [ln for ln in makefile.splitlines() if ln.startswith("EXACT :=")][0]
    assert "pairs.o" in exact                  # the -ffp-contract=off group: picks and neighbours depend on d2's roundings


def test_workspace_sizes():
    from dh3d_amd import _lib
    f = _lib.lib().dh3d_resample_clouds_ws_bytes
    assert f(1, 131072, 1 << 20) > 0
    for bad in ((0, 10, 10), (1, 0, 10), (1, 10, 0), (-1, 10, 10), (1, 131073, 10), (1, 10, (1 << 20) + 1), (65536, 10, 10)):
        assert f(*bad) == 0, bad
    sizes = [f(4, n, 8192) for n in (1, 1024, 1025, 4096, 9000, 65536, 131072)]
    assert all(v > 0 and v % 16 == 0 for v in sizes) and sizes == sorted(sizes)
    # a threshold key per cloud (8 bytes, the segment padded to 16) and a prefix per chunk of 1024 source rows (4 bytes, padded
    # likewise); targetnum takes no room.  Exact, as tests/test_workspace_layout.py pins the other ops' layouts.
    for shape, size in (((3, 5000, 64), 32 + 64), ((1, 1, 1), 16 + 16), ((2, 131072, 1 << 20), 16 + 1024), ((5, 1025, 8192), 48 + 48)):
        assert f(*shape) == size, shape


def _resample(lib, B=2, Nsrc=1000, T=256, points=P, num=P, seed=P, out=P, orig=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.dh3d_resample_clouds_ws_bytes(B, Nsrc, T) or (1 << 40)
    return lib.dh3d_resample_clouds(B, Nsrc, T, points, num, seed, out, orig, ws, ws_bytes, None)


def _augment(lib, B=2, N=100, points=P, mask=31, sigma=0.05, clip=0.1, lo=0.8, hi=1.25, asig=0.06, aclip=0.18, shift_range=0.1,
             seed=P, out=P, rot1d=P, scale=P, rot_small=P, shift=P):
    return lib.dh3d_augment_clouds(B, N, points, mask, sigma, clip, lo, hi, asig, aclip, shift_range, seed, out, rot1d, scale,
                                   rot_small, shift, None)


def _rotate(lib, B=2, N=100, pc2=P, maxv=3.0, seed=P, out=P, R=P):
    return lib.dh3d_pair_rotate(B, N, pc2, maxv, seed, out, R, None)


def _nodes(lib, B=2, N=1000, M=64, pc1=P, pc2=P, seed=P, anc=P, pos=P):
    return lib.dh3d_sample_pair_nodes(B, N, M, pc1, pc2, seed, anc, pos, None)


def test_bad_arguments_are_status_1():
    from dh3d_amd import _lib
    lib = _lib.lib()
    small = lib.dh3d_resample_clouds_ws_bytes(2, 1000, 256) - 1
    for kw in (dict(B=0), dict(Nsrc=0), dict(T=0), dict(T=-3), dict(points=None), dict(num=None), dict(seed=None), dict(out=None),
               dict(orig=None), dict(ws=None), dict(ws=264), dict(ws_bytes=0), dict(ws_bytes=small)):
        assert _resample(lib, **kw) == 1, kw
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=0), dict(N=0), dict(points=None), dict(seed=None), dict(out=None), dict(rot1d=None), dict(scale=None),
               dict(rot_small=None), dict(shift=None), dict(mask=32), dict(mask=1 << 31), dict(sigma=-1.0), dict(sigma=nan),
               dict(clip=0.0), dict(clip=inf), dict(lo=0.0), dict(lo=2.0), dict(hi=inf), dict(asig=-0.1), dict(aclip=nan),
               dict(shift_range=-0.1)):
        assert _augment(lib, **kw) == 1, kw
    for kw in (dict(B=0), dict(N=-1), dict(pc2=None), dict(seed=None), dict(out=None), dict(R=None), dict(maxv=-1.0),
               dict(maxv=inf)):
        assert _rotate(lib, **kw) == 1, kw
    for kw in (dict(B=0), dict(N=0), dict(pc1=None), dict(pc2=None), dict(seed=None), dict(anc=None), dict(pos=None)):
        assert _nodes(lib, **kw) == 1, kw


def test_unsupported_shapes_are_status_2():
    from dh3d_amd import _lib
    lib = _lib.lib()
    for kw in (dict(Nsrc=131073), dict(T=(1 << 20) + 1), dict(B=65536)):
        assert _resample(lib, **kw) == 2, kw
    for kw in (dict(N=16385), dict(N=1000, M=501), dict(N=1001, M=501), dict(M=0), dict(M=-1), dict(N=1, M=1), dict(B=65536)):
        assert _nodes(lib, **kw) == 2, kw
    assert _augment(lib, B=65536) == 2 and _rotate(lib, B=65536) == 2


def test_python_entry_point_refusals():
    from dh3d_amd import pairs
    pts, num = torch.zeros(2, 50, 3), torch.full((2,), 50, dtype=torch.int32)
    with pytest.raises(ValueError, match="unknown augmentation"):
        pairs.augment_clouds(pts, ("Jitter", "Flip"))
    with pytest.raises(ValueError, match="unknown augmentation"):
        pairs.make_local_pairs(pts, num, 32, 8, aug=("jitter",))
    with pytest.raises(ValueError, match="unknown augmentation"):
        pairs.make_global_batch(pts, num, 32, aug=("Rotate",))
    assert pairs.aug_mask(pairs.AUGMENTATIONS) == 31 and pairs.aug_mask(None) == 0 and pairs.aug_mask(("Shift", "Jitter")) == 18
    with pytest.raises(ValueError, match="targetnum"):
        pairs.resample_clouds(pts, num, 0)
    with pytest.raises(ValueError, match="beyond the kernels"):
        pairs.resample_clouds(torch.zeros(1, 131073, 3), num[:1], 64)
    with pytest.raises(ValueError, match=r"\(batch_size,npoints,3\)"):
        pairs.resample_clouds(pts[0], num, 64)
    with pytest.raises(ValueError, match="sample_nodes"):
        pairs.sample_pair_nodes(pts, pts, 26)
    with pytest.raises(ValueError, match="sample_nodes"):
        pairs.sample_pair_nodes(pts, pts, 0)
    with pytest.raises(ValueError, match="beyond the kernel"):
        pairs.sample_pair_nodes(torch.zeros(1, 16385, 3), torch.zeros(1, 16385, 3), 4)
    with pytest.raises(ValueError, match="float32"):
        pairs.augment_clouds(pts.double(), ("Jitter",))
    with pytest.raises(ValueError, match="seed"):
        pairs.seed_tensor(torch.zeros(2, dtype=torch.int64), "cpu")
    with pytest.raises(ValueError, match="GPU"):
        pairs.seed_tensor(torch.zeros(1, dtype=torch.int64), "cpu")
    for call in (lambda: pairs.resample_clouds(pts, num, 64), lambda: pairs.augment_clouds(pts, ("Jitter",)),
                 lambda: pairs.sample_pair_nodes(pts, pts, 8), lambda: pairs.rotate_pairs(pts),
                 lambda: pairs.make_local_pairs(pts, num, 32, 8), lambda: pairs.make_global_batch(pts, num, 32)):
        with pytest.raises(ValueError, match="GPU"):
            call()
    assert "prepare_clouds(sortby_dis=True)" in pairs.make_global_batch.__doc__
    assert "loadPC" in pairs.resample_clouds.__doc__
