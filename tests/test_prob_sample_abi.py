"""CPU: the weighted-sampling entry points (include/dh3d_hip.h "Weighted sampling", csrc/prob_sample.hip) are declared, bound
and exported; bad arguments give status codes before anything touches the GPU; the op is part of the drop-in surface and
refuses what the reference's op refuses."""
import ctypes
import os
import re

import pytest
import torch

NEW_SYMBOLS = ("dh3d_prob_sample", "dh3d_prob_sample_seeded")
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
    for word in ("Weighted sampling", "CUMULATIVE SUMS", "SEARCH", "stream 16"):
        assert word in header


def test_bad_arguments_are_status_codes():
    from dh3d_amd import _lib
    lib = _lib.lib()
    z, p = None, 256  # (a non-null fake pointer: every check below fails before a launch)

    def plain(b=2, n=100, m=10, w=p, r=p, temp=p, out=p):
        return lib.dh3d_prob_sample(b, n, m, w, r, temp, out, None)

    def seeded(b=2, n=100, m=10, w=p, count=p, seed=p, temp=p, out=p):
        return lib.dh3d_prob_sample_seeded(b, n, m, w, count, seed, temp, out, None)

    for f in (plain, seeded):
        for kw in (dict(b=0), dict(n=0), dict(m=0), dict(b=-1), dict(n=-5), dict(m=-2), dict(w=z), dict(temp=z), dict(out=z)):
            assert f(**kw) == 1, (f.__name__, kw)
        for kw in (dict(b=65536), dict(n=(1 << 20) + 1), dict(m=(1 << 20) + 1)):
            assert f(**kw) == 2, (f.__name__, kw)
    assert plain(r=z) == 1 and seeded(seed=z) == 1
    assert seeded(count=z, b=65536) == 2      # a NULL count is no error: the shape check is reached


def test_ops_surface_and_refusals():
    from dh3d_amd import ops, pm, utils
    assert "prob_sample" in ops.__all__
    w, r = torch.ones(2, 50), torch.zeros(2, 7)
    # the operator's own refusals come before the device check, so a CPU run tells them from the CPU-tensor refusal
    with pytest.raises(ValueError, match=r"ProbSample expects \(batch_size,num_choices\) inp shape"):
        ops.prob_sample(w[0], r)
    with pytest.raises(ValueError, match=r"ProbSample expects \(batch_size,num_points\) inpr shape"):
        ops.prob_sample(w, r[0])
    with pytest.raises(ValueError, match=r"ProbSample expects \(batch_size,num_points\) inpr shape"):
        ops.prob_sample(w, r[:1])
    with pytest.raises(ValueError, match="GPU"):
        ops.prob_sample(w, r)
    with pytest.raises(ValueError, match="GPU"):
        pm.prob_sample(w, r)
    with pytest.raises(ValueError, match="GPU"):
        utils.sample_by_weight(w, 4)
    with pytest.raises(ValueError, match="num_choices"):
        utils.sample_by_weight(w[0], 4)
