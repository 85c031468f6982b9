"""CPU: dh3d_match_descriptors2 is declared, bound and exported, refuses bad arguments with status codes before any launch,
and the Python entry points check their options.  The entry takes no workspace: there is no size query to disagree with."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _match2(lib, a=256, ac=256, b=256, bc=256, P=2, Ma=512, Mb=512, D=128, ratio2=0.81, mutual=1, nn1=256, d1=256, nn2=256,
            d2=256, rev=256, rd=256, m=256, nk=256, sa=132, sb=132):
    return lib.dh3d_match_descriptors2(a, sa, ac, b, sb, bc, P, Ma, Mb, D, ratio2, mutual, nn1, d1, nn2, d2, rev, rd, m, nk, None)


def test_entry_is_declared_bound_and_exported():
    import ctypes
    from dh3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    assert re.search(r"\bint\s+dh3d_match_descriptors2\s*\(", header) and "dh3d_match_descriptors2" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dh3d_match_descriptors2")
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION                            # an addition only
    said = header[header.index("The two nearest positives of every anchor"):header.index("int dh3d_match_descriptors2")]
    assert "No workspace" in said and "dh3d_match_descriptors2_workspace_bytes" not in header
    assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), "dh3d_match_descriptors2_workspace_bytes")


def test_status_codes():
    from dh3d_amd import _lib
    lib = _lib.lib()
    z = None  # (256: a non-null fake pointer; every check below fails before a launch)
    for kw in (dict(a=z), dict(ac=z), dict(b=z), dict(bc=z), dict(nn1=z), dict(d1=z), dict(nn2=z), dict(d2=z), dict(m=z),
               dict(nk=z), dict(P=0), dict(Ma=0), dict(Mb=0), dict(D=0), dict(sa=64), dict(sb=100),
               dict(rev=z), dict(rd=z),                         # only one of the reverse outputs
               dict(rev=z, rd=z, mutual=1),                     # the mutual check without them
               dict(ratio2=1.5), dict(ratio2=float("nan"))):
        assert _match2(lib, **kw) == 1, kw
    for kw in (dict(D=130), dict(D=258, sa=300, sb=300), dict(D=260, sa=300, sb=300), dict(Ma=4097), dict(Mb=4097),
               dict(P=65536)):
        assert _match2(lib, **kw) == 2, kw
    # an invalid argument is reported ahead of an unsupported shape, as dh3d_match_descriptors does
    assert _match2(lib, a=z, Ma=4097) == 1


def test_python_entry_points_check_their_options():
    import torch
    from dh3d_amd import registration as reg
    cpu = torch.zeros(1, 8, 132)
    cnt = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError):
        reg.match_descriptors2(cpu[:, :, 3:131], cnt, cpu[:, :, 3:131], cnt)  # CPU tensors: no fallback
    with pytest.raises(ValueError):
        reg.register(cpu, cnt, cpu, cnt, match={})
    for bad in ({"ratio": 0.9, "k": 3}, "mutual", 0.9, [("ratio", 0.9)]):
        with pytest.raises(ValueError):
            reg._match_options(bad)
    assert reg._match_options(None) is None and reg._match_options({}) == {}
    assert reg._match_options({"ratio": 0.9, "mutual": True}) == {"ratio": 0.9, "mutual": True}
