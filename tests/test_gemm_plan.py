"""CPU: dh3d_gemm_plan (host only) is the one dispatch decision of csrc/gemm.hip -- the kernel, the reduction chunks and
the steps per chunk that gemm_launch takes -- and dh3d_gemm_is_split, by which callers choose the zero arena, answers over
the same function exactly what it answered before the two were gathered (tests/golden/gemm_is_split_sweep.json, recorded
from the library of the commit before)."""
import ctypes
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MN = (4, 32, 36, 64, 68, 128, 132, 260, 1024)
KS = (4, 32, 33, 36, 256, 512, 516, 1000, 2048, 4128)
BATCH = (1, 3, 16)
STAGE = {"rows1": 1, "rows2": 1, "rows3": 1, "rows4": 1, "shortk": 1, "f32_narrow": 16, "f32_wide": 16, "x6_narrow": 32,
         "x6_wide": 16}


def _grid():
    for ta in (0, 1):
        for M in MN:
            for N in MN:
                for K in KS:
                    for batch in BATCH:
                        yield ta, M, N, K, batch


def test_symbol_declared_bound_and_exported():
    from dh3d_amd import _lib, pm
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    assert re.search(r"\bint\s+dh3d_gemm_plan\s*\(", header) and "dh3d_gemm_plan" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dh3d_gemm_plan")
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION                            # an addition only
    said = header[header.index("int dh3d_gemm_is_split"):header.index("int dh3d_gemm_plan")]
    assert "Host only; looks at the shape alone" in said
    for code, name in pm.GEMM_KERNELS.items():                                               # the ids are the header's
        macro = "DH3D_GEMM_" + name.upper()
        if not name.startswith("rows") or name in ("rows1", "rows4"):
            assert re.search(r"#define\s+%s\s+%d\b" % (macro, code), header), macro
    assert sorted(pm.GEMM_KERNELS) == list(range(1, 10)) and set(pm.GEMM_KERNELS.values()) == set(STAGE)


def test_is_split_is_what_it_was_before_the_plan():
    from dh3d_amd import _lib
    lib = _lib.lib()
    pinned = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_is_split_sweep.json")))["is_split"]
    grid = list(_grid())
    assert len(pinned) == len(grid) == 4860 and set(pinned) == {0, 1}
    got = [lib.dh3d_gemm_is_split(ta, M, N, K, batch) for ta, M, N, K, batch in grid]
    moved = [g for g, a, b in zip(grid, got, pinned) if a != b]
    assert not moved, "%d shapes changed their answer, the first (ta, M, N, K, batch) = %s" % (len(moved), moved[0])
    # batch <= 0 reads as 1, as before
    assert all(lib.dh3d_gemm_is_split(ta, M, N, K, 0) == lib.dh3d_gemm_is_split(ta, M, N, K, 1)
               for ta, M, N, K, batch in grid if batch == 1)


def test_plan_sweep_chunks_bias_and_stage():
    """(i) chunks > 1 implies is_split; (ii) a bias implies one chunk; (iii) kchunk is a multiple of the stage depth and
    chunks * kchunk >= K > (chunks - 1) * kchunk -- on every shape of the grid the entry points serve, which is every shape
    but nn with K = 33 (K % 4) and tn with a bias (no such entry point): those are 0."""
    from dh3d_amd import _lib, pm
    lib = _lib.lib()
    seen = set()
    for ta, M, N, K, batch in _grid():
        split = lib.dh3d_gemm_is_split(ta, M, N, K, batch)
        for bias in (False, True):
            p = pm.gemm_plan(ta, M, N, K, batch, bias)
            at = (ta, M, N, K, batch, bias)
            if (ta and bias) or (not ta and K % 4):
                assert p is None, at
                continue
            kernel, chunks, kchunk, stage = p
            seen.add(kernel)
            assert chunks >= 1 and (chunks == 1 or split == 1), at                                   # (i)
            assert not bias or chunks == 1, at                                                       # (ii)
            assert stage == STAGE[kernel] and kchunk % stage == 0, at                                # (iii)
            assert chunks * kchunk >= K > (chunks - 1) * kchunk, at
            # the kernel is the one its conditions name
            if batch == 1 and not ta and M <= 32 and K <= 512:
                assert kernel == "rows%d" % ((M + 7) // 8) and chunks == 1 and kchunk == K, at
            elif batch == 1 and ta and K <= 32:
                assert kernel == "shortk" and chunks == 1 and kchunk == K, at
            else:
                x6 = K % 32 == 0 and M * N * K * batch >= 1 << 26
                assert kernel == ("x6_" if x6 else "f32_") + ("narrow" if N <= 64 else "wide"), at
                if x6:
                    assert kchunk % 32 == 0, at
    assert seen == set(STAGE) - {"rows2", "rows3"}                # (the grid's M <= 32 are 4 and 32)
    assert [pm.gemm_plan(0, M, 64, 64)[0] for M in (1, 8, 9, 16, 17, 24, 25, 32, 33)] == [
        "rows1", "rows1", "rows2", "rows2", "rows3", "rows3", "rows4", "rows4", "f32_narrow"]


def test_plan_refuses_what_the_entry_points_refuse():
    from dh3d_amd import pm
    plan = pm.gemm_plan
    assert plan(0, 64, 64, 64) and plan(1, 64, 64, 64)
    for bad in ((0, 0, 64, 64), (0, 64, 0, 64), (0, 64, 64, 0), (1, -4, 64, 64), (0, 64, 64, 64, 0), (0, 64, 64, 64, -1)):
        assert plan(*bad) is None, bad
    assert plan(0, 64, 64, 66) is None and plan(0, 64, 66, 64) is None and plan(0, 66, 64, 64) is not None   # nn: K, N % 4
    assert plan(1, 66, 64, 64) is None and plan(1, 64, 66, 64) is None and plan(1, 64, 64, 66) is not None   # tn: M, N % 4
    assert plan(1, 64, 64, 64, 1, True) is None                                                              # tn has no bias
    # chunks * batch beyond the grid's z limit
    assert plan(1, 4, 4, 64, 65535) == ("f32_narrow", 1, 64, 16) and plan(1, 4, 4, 64, 65536) is None
    # NULL outputs are allowed
    from dh3d_amd import _lib
    assert _lib.lib().dh3d_gemm_plan(0, 8, 8, 8, 1, 0, None, None, None) == 1
