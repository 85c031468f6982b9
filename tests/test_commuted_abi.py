"""CPU: the C entry points of the commuted training walks (csrc/interp_train.hip, csrc/netvlad_train.hip and the
training forward of the attention head, dense_x6.hip) refuse unsupported shapes (status 2) and missing pointers or
empty sizes (status 1) before anything is launched.  No call here reaches a kernel: every one is rejected by its
argument checks."""
import ctypes

import pytest

# argument kinds: P required pointer, o optional pointer (order / mask / stream), e epilogue (may be NULL),
# H channel width (Hd or c), r row_major flag, B n m sizes
SPECS = {
    "dh3d_interp_bn_colstats": "PHrPPoBnmoPo",
    "dh3d_interp_bn_bwd_sums": "PHrPPoBnmoPPPPPPPo",
    "dh3d_interp_bn_bwd_apply": "PHrPPoBnmoPPPPPPPo",
    "dh3d_three_interpolate_bwd_sorted": "BnHmPPPoPo",
    "dh3d_interp_scatter_scaled": "PPPPoBnmoPo",
    "dh3d_netvlad_commuted_fwd_stats": "PPPPoBnmoPPPo",
    "dh3d_netvlad_commuted_fwd_assign": "PPPPPPPoBnmoPPPo",
    "dh3d_netvlad_commuted_bwd_sums": "PPPPPPPPPPoBnmoPPPPo",
    "dh3d_netvlad_commuted_bwd_apply": "PPPPPPPPPoBnmoPPo",
    "dh3d_interp_head_sorted_fwd_dev": "PHrPPoBnmePPPo",
}
GOOD = {"H": 256, "r": 0, "B": 2, "n": 300, "m": 40}
FAKE = 16   # a non-null address that is never dereferenced: the checks return first


def _args(spec, **over):
    vals = dict(GOOD, **over)
    out = []
    for i, k in enumerate(spec):
        if k in "Po":
            out.append(ctypes.c_void_p(0 if over.get("null") == i else FAKE))
        elif k == "e":
            out.append(None)
        else:
            out.append(vals[k])
    return out


@pytest.fixture(scope="module")
def lib():
    from dh3d_amd import _lib
    return _lib.lib()


def _call(lib, name, **over):
    return getattr(lib, name)(*_args(SPECS[name], **over))


@pytest.mark.parametrize("name", sorted(SPECS))
def test_unsupported_shapes_are_status_2(lib, name):
    assert _call(lib, name, m=1025) == 2, "m > 1024"
    if name.startswith("dh3d_interp_bn_"):
        for Hd in (0, 128, 300, 1280):
            assert _call(lib, name, H=Hd) == 2, Hd
            assert _call(lib, name, H=Hd, r=1) == 2, Hd
    if name == "dh3d_interp_head_sorted_fwd_dev":
        for Hd in (128, 300, 1280):
            assert _call(lib, name, H=Hd) == 2, Hd
    if name == "dh3d_three_interpolate_bwd_sorted":
        for c in (64, 128, 255, 257, 512):
            assert _call(lib, name, H=c) == 2, c


@pytest.mark.parametrize("name", sorted(SPECS))
def test_missing_pointers_and_empty_sizes_are_status_1(lib, name):
    spec = SPECS[name]
    stream = len(spec) - 1
    for i, k in enumerate(spec):
        if k == "P":
            assert _call(lib, name, null=i) == 1, "argument %d NULL" % i
    for k in "Bnm":
        for v in (0, -1):
            assert _call(lib, name, **{k: v}) == 1, (k, v)
    assert stream == spec.rindex("o")   # (the stream is the last argument and may be NULL)
