"""CPU: the C-ABI library loads, exports every symbol include/dh3d_hip.h declares, and rejects bad
arguments before touching the GPU (no compute calls here)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dh3d_[a-z0-9_]+)\s*\(", src)))


def test_header_and_binding_table_agree():
    from dh3d_amd import _lib
    assert sorted(_lib.EXPORTED_SYMBOLS) == declared_symbols()


def test_library_exports_every_declared_symbol():
    from dh3d_amd import _lib
    assert os.path.isfile(_lib.LIB_PATH), "build with `make -C dh3d_amd/csrc` or __graft_entry__.build()"
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(handle, name), name
    lib = _lib.lib()
    assert lib.dh3d_version() >= 100
    assert lib.dh3d_arch() == b"gfx950"
    assert lib.dh3d_status_string(0) == b"ok"


def test_invalid_arguments_are_status_codes_not_crashes():
    from dh3d_amd import _lib
    lib = _lib.lib()
    z = ctypes.c_void_p(0)
    assert lib.dh3d_knn_bruteforce(z, 1, 3, 8, 4, z, z, z) == 1          # null pointers
    one = ctypes.c_void_p(16)
    assert lib.dh3d_knn_bruteforce(one, 1, 17, 8, 4, one, one, z) == 2     # Dp > 16: beyond the staging tile
    assert lib.dh3d_knn_bruteforce(one, 1, 3, 8, 0, one, one, z) == 1      # K <= 0
    assert lib.dh3d_farthest_point_sample(1, 20000, 8, one, z, one, z) == 2  # N > 16384
    assert lib.dh3d_farthest_point_sample(1, 64, 0, one, z, one, z) == 1     # npoint <= 0 (tf_sampling.cpp:100)
    assert lib.dh3d_flex_conv_pm_fwd(one, one, one, one, 1, 64, 8, 48, 64, None, one, z) == 2
    assert lib.dh3d_knn_bruteforce_xyz(one, 65536, 8, 4, one, one, z) == 2   # B > 65535: a cloud is a grid row
    assert lib.dh3d_knn_sorted(one, one, 65536, 8, 4, one, one, z) == 2
    assert lib.dh3d_netvlad_workspace_bytes(4, 1024, 128, 64) == 0
    assert lib.dh3d_netvlad_workspace_bytes(4, 1024, 256, 64) > 0


def test_fps_sorted_fits_is_the_launchers_lds_budget():
    """dh3d_fps_sorted_fits (host only): the shapes the sorted FPS launcher takes, from the same LDS byte count it checks
    (1104 + 4m + 12N bytes, + 4(N+1) + 2((N+1) & ~1) + 24 ceil(m/64) for the ordered output, against 159 KB)."""
    from dh3d_amd import pm
    fits = pm.fps_sorted_fits
    # the shipped levels: 8 x 8192 / 8 and 32 x 4096 / 8 on the ordered kernel, cfg 5's 16384 / 8 on the cloud
    assert fits(8192, 1024, ordered=True) and fits(4096, 512, ordered=True)
    assert fits(16384, 2048, with_cloud=True) and not fits(16384, 2048)
    # the ordered output at N = 8192: m <= 3257 (dilate 2, m = 4096, needs 166484 B)
    assert fits(8192, 3257, ordered=True) and not fits(8192, 3258, ordered=True)
    assert not fits(8192, 4096, ordered=True) and fits(8192, 4096)
    assert fits(8009, 4004, ordered=True) and not fits(8010, 4005, ordered=True)
    assert not fits(8193, 16, ordered=True)  # the ordered kernel's N limit, whatever m
    # the coordinate table at N = 12288: m <= 3564; beyond it (or N > 12288) only with the cloud
    assert fits(12288, 3564) and not fits(12288, 3565)
    assert not fits(12288, 4096) and fits(12288, 4096, with_cloud=True)
    assert not fits(12289, 16) and fits(12289, 16, with_cloud=True) and not fits(16385, 16, with_cloud=True)
    assert not fits(0, 16) and not fits(4096, 0)
    # monotone in m: once a shape does not fit, no larger sample fits
    for N in (4096, 6000, 8009, 8192, 11551, 12288, 16384):
        for ordered, cloud in ((True, False), (False, False), (False, True)):
            row = [fits(N, m, ordered=ordered, with_cloud=cloud) for m in range(1, N + 1, 7)]
            assert row == sorted(row, reverse=True), (N, ordered, cloud)


def test_knn_grid_plan_is_the_launchers_choice():
    """dh3d_knn_grid_plan (host only): the launch dh3d_knn_grid makes, by G = B * ceil(N / 64) query groups -- the pruned
    scan for crowded clouds inside knn_grid_kernel<4, 4> up to G = 1280, <4, 2> up to 4096, a second gated launch
    beyond -- and the grid drop D (one bit less per halving of N below 4096 points, down to 2^-6)."""
    from dh3d_amd import pm
    plan = pm.knn_grid_plan
    assert plan(6, 8192, 8) == (4, 0) and plan(20, 4096, 8) == (4, 0)         # G 768, 1280
    assert plan(21, 3904, 8) == (2, 0) and plan(32, 4096, 8) == (2, 0)        # G 1281, 2048 (the shipped global batch)
    assert plan(64, 4096, 1) == (2, 0) and plan(241, 1088, 8) == (0, 2)       # G 4096, 4097
    assert plan(300, 1000, 3) == (0, 2) and plan(1, 16384, 8) == (4, 0)
    assert [plan(1, n, 8)[1] for n in (3073, 3072, 1536, 1537, 768, 384, 96, 48, 1)] == [0, 1, 2, 1, 3, 4, 6, 6, 6]
    assert plan(1, 16385, 8) is None and plan(1, 4096, 9) is None and plan(1, 4096, 0) is None
    assert plan(0, 4096, 8) is None and plan(65536, 64, 8) is None and plan(65535, 64, 8) == (0, 6)
    # monotone in G: more query groups never go back to a plan with more waves per group
    for N in (64, 1000, 3904, 4031, 4096, 8000, 16384):
        codes = [plan(B, N, 8)[0] for B in range(1, 300)]
        assert codes == sorted(codes, reverse=True), N


def test_knn_sorted_plan_is_the_launchers_choice():
    """dh3d_knn_sorted_plan (host only): the kernel dh3d_knn_sorted launches, (S, KMAX) -- S waves per 64-query group by
    G = B * ceil(N / 64) (8 up to 256, 4 up to 1280, 2 up to 4096) on knn_split_kernel<KMAX, S>, S = 0 the one-wave
    knn_sorted_kernel<KMAX> beyond and for every K > 16.  tests/test_knn_plan.py sweeps it."""
    from dh3d_amd import _lib, pm
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    assert re.search(r"\bint\s+dh3d_knn_sorted_plan\s*\(", header) and "dh3d_knn_sorted_plan" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dh3d_knn_sorted_plan")
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION                             # an addition only
    plan = pm.knn_sorted_plan
    assert plan(8, 8192, 8) == (4, 8) and plan(32, 4096, 8) == (2, 8)          # the shipped batches: G 1024, 2048
    assert plan(4, 4096, 12) == (8, 16) and plan(257, 50, 12) == (4, 16)       # G 256, 257
    assert plan(20, 4096, 4) == (4, 4) and plan(21, 3904, 4) == (2, 4)         # G 1280, 1281
    assert plan(64, 4096, 16) == (2, 16) and plan(241, 1088, 16) == (0, 16)    # G 4096, 4097
    assert plan(1, 64, 3) == (8, 8)                                            # K <= 4 at S = 8: <8, 8> is what exists
    assert plan(1, 64, 17) == (0, 32) and plan(1, 64, 33) == (0, 64) and plan(300, 1000, 64) == (0, 64)
    assert plan(1, 64, 65) is None and plan(65536, 64, 8) is None and plan(0, 64, 8) is None and plan(1, 0, 8) is None
    assert plan(65535, 64, 8) == (0, 8)


def test_knn_bruteforce_plan_is_the_launchers_choice():
    """dh3d_knn_bruteforce_plan (host only): the kernel dh3d_knn_bruteforce / _xyz run -- ("small", CPL, Q) a wave per query
    up to 2048 points, ("lane", KMAX) a lane per query beyond, ("anydp", KMAX) for Dp != 3.  tests/test_knn_plan.py sweeps it."""
    from dh3d_amd import _lib, pm
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    assert re.search(r"\bint\s+dh3d_knn_bruteforce_plan\s*\(", header) and "dh3d_knn_bruteforce_plan" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dh3d_knn_bruteforce_plan")
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION                             # an addition only
    plan = pm.knn_plan
    assert plan(8, 1024, 8) == ("small", 16, 2) and plan(32, 512, 8) == ("small", 8, 2)       # the model's sampled sets
    assert plan(33, 512, 8) == ("small", 8, 4) and plan(9, 2048, 12) == ("small", 32, 4)
    assert plan(1, 513, 8) == ("small", 16, 2) and plan(1, 1025, 8) == ("small", 32, 2)
    assert plan(1, 2049, 4) == ("lane", 4) and plan(8, 8192, 8) == ("lane", 8) and plan(1, 3000, 33) == ("lane", 64)
    assert plan(2, 300, 8, Dp=1) == ("anydp", 8) and plan(2, 300, 9, Dp=16) == ("anydp", 16)
    assert plan(2, 300, 17, Dp=2) == ("anydp", 64)
    assert plan(1, 64, 65) is None and plan(65536, 64, 8) is None and plan(1, 64, 8, Dp=17) is None
    assert plan(0, 64, 8) is None and plan(1, 64, 8, Dp=0) is None


def test_flex_conv_fwd_plan_is_the_dispatchers_choice():
    """dh3d_flex_conv_fwd_plan (host only): the forward dh3d_flex_conv_fwd_ws runs for a shape -- 3 the bf16x6 kernel, 1 the
    fused f32-MFMA kernel, 2 flex_S + GEMM, 0 not served, which is exactly where the workspace query returns 0."""
    from dh3d_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    assert re.search(r"\bint\s+dh3d_flex_conv_fwd_plan\s*\(", header) and "dh3d_flex_conv_fwd_plan" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dh3d_flex_conv_fwd_plan")
    assert lib.dh3d_abi_version() == 4 == _lib.ABI_VERSION                                   # an addition only
    said = header[header.index("size_t dh3d_flex_conv_fwd_workspace_bytes"):header.index("int dh3d_flex_conv_fwd_plan")]
    assert "Host only; looks at the shape alone" in said
    plan, ws = lib.dh3d_flex_conv_fwd_plan, lib.dh3d_flex_conv_fwd_workspace_bytes
    pairs = [(32, 64), (32, 128), (64, 64), (64, 128), (64, 256), (128, 128), (128, 256)]
    seen = set()
    for B in (-1, 0, 1, 3):
        for N in (0, 1, 2, 257):
            for K in (0, 1, 5, 8, 12):
                for Dp in (1, 2, 3, 4):
                    for Din, Dout in pairs + [(4, 4), (36, 100), (48, 96), (64, 32), (128, 64), (3, 7), (33, 64), (32, 66)]:
                        r = plan(B, N, K, Dp, Din, Dout)
                        assert r in (0, 1, 2, 3) and (r == 0) == (ws(B, N, K, Dp, Din, Dout) == 0), (B, N, K, Dp, Din, Dout)
                        if B <= 0 or N <= 1 or K <= 0 or Dp != 3 or Din % 4 or Dout % 4:
                            assert r == 0, (B, N, K, Dp, Din, Dout)
                        elif (Din, Dout) in pairs:
                            assert r == (3 if K == 8 and Dout == 64 else 1), (K, Din, Dout)
                        else:
                            assert r == 2, (K, Din, Dout)
                        seen.add(r)
    assert seen == {0, 1, 2, 3}
    assert [plan(2, 300, 8, 3, di, do) for di, do in pairs] == [3, 1, 3, 1, 1, 1, 1]          # the table's seven pairs
    assert plan(2, 300, 8, 3, 32, 64) == 3 and plan(2, 300, 5, 3, 32, 64) == 1                # K != 8: x6 -> the f32 kernel
    assert plan(2, 300, 12, 3, 64, 64) == 1 and plan(2, 300, 8, 3, 48, 96) == 2
    assert plan(2, 300, 8, 2, 32, 64) == 0 and plan(4, 1, 1, 3, 32, 64) == 0                  # Dp = 2; N = 1
    assert plan(1 << 14, 1 << 16, 8, 3, 64, 64) == 0 and plan(1 << 13, 1 << 14, 8, 3, 4, 4) == 0   # beyond 32-bit indices


def test_gemm_plan_is_the_launchers_choice():
    """dh3d_gemm_plan (host only): the kernel of csrc/gemm.hip and the cut of the reduction that the GEMM entry points take
    for a shape -- ids 1 .. 4 gemm_rows_kernel<RB>, 5 gemm_shortk_kernel, 6 / 7 gemm_f32_kernel narrow / wide, 8 / 9
    gemm_x6_kernel narrow / wide, 0 a shape they refuse.  tests/test_gemm_plan.py sweeps it."""
    from dh3d_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    assert re.search(r"\bint\s+dh3d_gemm_plan\s*\(", header) and "dh3d_gemm_plan" in _lib.EXPORTED_SYMBOLS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "dh3d_gemm_plan")
    assert lib.dh3d_abi_version() == 4 == _lib.ABI_VERSION                                   # an addition only

    def plan(ta, M, N, K, batch=1, bias=0):
        c, kc, st = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
        r = lib.dh3d_gemm_plan(ta, M, N, K, batch, bias, ctypes.byref(c), ctypes.byref(kc), ctypes.byref(st))
        return r, c.value, kc.value, st.value

    assert plan(0, 22, 256, 256) == (3, 1, 256, 1) and plan(1, 256, 256, 22) == (5, 1, 22, 1)     # the [clouds, 256] layers
    assert plan(0, 33, 68, 36) == (7, 1, 48, 16) and plan(1, 68, 60, 33) == (6, 1, 48, 16)
    assert plan(1, 132, 68, 70) == (7, 2, 48, 16) and plan(0, 129, 132, 1000) == (7, 4, 256, 16)
    assert plan(0, 256, 128, 2048) == (9, 8, 256, 16) and plan(0, 256, 128, 2048, 1, 1) == (9, 1, 2048, 16)
    assert plan(0, 512, 64, 2048) == (8, 8, 256, 32) and plan(1, 132, 132, 4128) == (9, 65, 64, 16)
    assert plan(0, 130, 68, 512, 16) == (9, 2, 256, 16) and plan(1, 64, 132, 1024, 8) == (9, 16, 64, 16)
    assert plan(0, 64, 64, 66) == (0, 0, 0, 0) and plan(1, 66, 64, 64) == (0, 0, 0, 0) and plan(1, 64, 64, 64, 1, 1)[0] == 0
    for ta, M, N, K, b in ((0, 256, 128, 2048, 1), (1, 132, 68, 70, 1), (0, 129, 132, 1000, 1)):
        assert lib.dh3d_gemm_is_split(ta, M, N, K, b) == 1                                  # chunks > 1 implies is_split


def test_library_was_built_from_this_tree():
    """The loaded library carries the hash of the sources it was compiled from (csrc/Makefile SRC_HASH -> dh3d_source_hash):
    a stale .so that travelled with the tree (built artefacts are git-ignored, not gpurun-ignored) fails here."""
    from dh3d_amd import _lib
    lib = _lib.lib()
    assert lib.dh3d_source_hash().decode() == _lib.tree_source_hash()


def test_python_ops_refuse_cpu_tensors():
    import pytest
    import torch
    from dh3d_amd import ops
    with pytest.raises(ValueError):
        ops.knn_bruteforce(torch.zeros(1, 3, 8), 4)  # CPU tensor: no fallback
    with pytest.raises(ValueError):
        ops.farthest_point_sample(4, torch.zeros(1, 8, 3))


def test_oracle_is_not_imported_by_the_product():
    pkg = os.path.join(ROOT, "dh3d_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            txt = open(os.path.join(pkg, fn)).read()
            assert "oracle" not in re.sub(r'""".*?"""', "", txt, flags=re.S), fn


def _code_only(path):
    """Source text without docstrings and comments."""
    import io
    import tokenize
    out = []
    for tok in tokenize.generate_tokens(io.StringIO(open(path).read()).readline):
        if tok.type == tokenize.COMMENT:
            continue
        if tok.type == tokenize.STRING and tok.string.lstrip("rbuRBU").startswith(('"""', "'''")):
            continue
        out.append(tok.string)
    return " ".join(out)


def test_training_module_has_no_tensor_op_restatement():
    """dh3d_amd/training.py runs the step on HIP kernels only: no tensor-op GEMM / activation / softmax path selectable at
    run time (the plain-torch restatement the HIP step is compared with lives in tests/torch_reference.py), and nothing in
    the package imports that test module."""
    import ast
    path = os.path.join(ROOT, "dh3d_amd", "training.py")
    tree = ast.parse(open(path).read())
    banned_attrs = {"matmul", "mm", "bmm", "addmm", "einsum", "softmax", "sigmoid", "relu", "linear", "batch_norm"}
    for node in ast.walk(tree):
        assert not (isinstance(node, ast.BinOp) and isinstance(node.op, ast.MatMult)), "matrix product at line %d" % node.lineno
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in ("torch", "F"):
            assert node.attr not in banned_attrs, "%s.%s at line %d" % (node.value.id, node.attr, node.lineno)
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            names = [a.name for a in node.names] + [getattr(node, "module", "") or ""]
            assert not any("functional" in n for n in names), "torch.nn.functional imported at line %d" % node.lineno
        if isinstance(node, ast.arg):
            assert node.arg != "impl", "an implementation switch at line %d" % node.lineno
    pkg = os.path.join(ROOT, "dh3d_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            assert "torch_reference" not in _code_only(os.path.join(pkg, fn)), fn
