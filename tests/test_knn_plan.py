"""CPU: dh3d_knn_sorted_plan and dh3d_knn_bruteforce_plan (host only) are the launch decisions of csrc/knn.hip's
knn_sorted_launch and knn_launch -- the launchers run the functions the queries report -- swept here over every threshold
and every refusal; and tests/knn_regime_cases.py, the table of tests/test_knn_regimes_gpu.py, is filed under the plans the
launchers make, reaches every plan there is, and has the cloud kinds each regime needs."""
import ctypes
import os
import re

import knn_regime_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTH_EDGES = ((4, 4), (5, 8), (8, 8), (9, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64))  # (K, list width)


def test_plan_queries_are_declared_and_additions_only():
    from dh3d_amd import _lib
    header = open(os.path.join(ROOT, "include", "dh3d_hip.h")).read()
    for name in ("dh3d_knn_sorted_plan", "dh3d_knn_bruteforce_plan"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header) and name in _lib.EXPORTED_SYMBOLS
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.lib().dh3d_abi_version() == 4 == _lib.ABI_VERSION


def test_sorted_plan_threshold_sweep():
    """S by G = B * ceil(N / 64): 8 | 4 at 256 | 257, 4 | 2 at 1280 | 1281, 2 | 0 at 4096 | 4097 -- each edge reached by
    more than one (B, N) -- and KMAX at every width edge in every S; K > 16 ignores S; the refusals."""
    from dh3d_amd import pm
    plan = pm.knn_sorted_plan
    edges = {256: 8, 257: 4, 1280: 4, 1281: 2, 4096: 2, 4097: 0}
    shapes = {256: ((4, 4096), (256, 64), (16, 1000), (256, 1)), 257: ((257, 50), (257, 64), (1, 16385)),
              1280: ((20, 4096), (80, 1000), (1280, 7)), 1281: ((21, 3904), (1281, 64), (427, 129)),
              4096: ((64, 4096), (4096, 64), (256, 1024)), 4097: ((241, 1088), (4097, 1), (17, 15400))}
    for G, S in edges.items():
        for B, N in shapes[G]:
            assert B * ((N + 63) // 64) == G
            for K, km in WIDTH_EDGES:
                want = (0, km) if K > 16 else (S, 8 if (S == 8 and km == 4) else km)
                assert plan(B, N, K) == want, (B, N, K)
    assert plan(16, 1000, 1) == (8, 8) and plan(17, 1000, 1) == (4, 4)   # K <= 4 at S = 8: <8, 8> is the instantiated one
    # N enters through ceil(N / 64) alone
    assert plan(4, 4033, 8) == plan(4, 4096, 8) == (8, 8) and plan(4, 4097, 8) == (4, 8)
    # monotone in G: more query groups never go back to more waves per group
    for N in (1, 50, 64, 65, 1000, 4031, 4096, 16384):
        for K in (3, 8, 16):
            row = [plan(B, N, K)[0] for B in range(1, 300)]
            assert row == sorted(row, reverse=True), (N, K)
    # refusals: exactly dh3d_knn_sorted's
    for B, N, K in ((0, 64, 8), (-1, 64, 8), (1, 0, 8), (1, 64, 0), (1, 64, -3), (1, 64, 65), (65536, 64, 8)):
        assert plan(B, N, K) is None, (B, N, K)
    assert plan(65535, 64, 64) == (0, 64) and plan(65535, 1, 1) == (0, 4) and plan(1, 1, 1) == (8, 8)
    assert plan(1, 1 << 24, 8) == (0, 8) and plan(65535, 1 << 24, 8) == (0, 8)   # (G beyond 2^31: counted in 64 bits)


def test_bruteforce_plan_threshold_sweep():
    """CPL by N at 512 | 513 and 1024 | 1025, the family at 2048 | 2049, Q at B * N = 16384 | the next reachable value, the
    list width at every edge for the lane-per-query and the any-Dp kernel; the refusals."""
    from dh3d_amd import pm
    plan = pm.knn_plan
    for N, cpl in ((1, 8), (512, 8), (513, 16), (1024, 16), (1025, 32), (2048, 32)):
        for K in (1, 8, 12, 64):   # K plays no part up to 2048 points
            assert plan(1, N, K) == ("small", cpl, 2), (N, K)
    for K, km in WIDTH_EDGES:
        assert plan(1, 2049, K) == ("lane", km) and plan(40, 16384, K) == ("lane", km), K
        assert plan(1, 1 << 20, K) == ("lane", km), K
    for K in range(1, 65):
        assert plan(3, 3000, K)[1] >= K and plan(3, 300, K, Dp=5)[1] >= K   # the list holds K
    # Q: B * N <= 16384 -> 2, else 4 (16385 is reachable as 1 x 16385 only beyond 2048 points: the nearest values below)
    for B, N, q in ((32, 512, 2), (33, 512, 4), (16384, 1, 2), (16385, 1, 4), (16, 1024, 2), (17, 1024, 4), (8, 2048, 2),
                    (9, 2048, 4), (1, 2048, 2), (32, 513, 4), (31, 513, 2), (5, 3277, None), (8, 2047, 2), (65535, 1, 4),
                    (65535, 2048, 4)):
        p = plan(B, N, 8)
        assert (p[0] == "lane" and q is None) or (p[0] == "small" and p[2] == q), (B, N, p)
    # any Dp but 3: the any-Dp kernel whatever N and B, widths 8 | 16 | 64
    for Dp in (1, 2, 4, 16):
        for K, km in ((1, 8), (8, 8), (9, 16), (16, 16), (17, 64), (32, 64), (33, 64), (64, 64)):
            for N in (1, 300, 2049, 20000):
                assert plan(2, N, K, Dp=Dp) == ("anydp", km), (Dp, K, N)
    # refusals: exactly dh3d_knn_bruteforce's
    for B, N, K, Dp in ((0, 64, 8, 3), (1, 0, 8, 3), (1, 64, 0, 3), (1, 64, 65, 3), (65536, 64, 8, 3), (1, 64, 8, 0),
                        (1, 64, 8, 17), (1, 64, 8, -1), (1, 64, 65, 2), (65536, 64, 8, 2), (-5, 64, 8, 3)):
        assert plan(B, N, K, Dp=Dp) is None, (B, N, K, Dp)
    assert plan(65535, 64, 64) == ("small", 8, 4) and plan(1, 64, 64, Dp=16) == ("anydp", 64)
    # the raw encoding, as the header documents it: family * 65536 + a * 256 + b
    from dh3d_amd import _lib
    lib = _lib.lib()
    assert lib.dh3d_knn_bruteforce_plan(33, 3, 512, 8) == 65536 + 8 * 256 + 4
    assert lib.dh3d_knn_bruteforce_plan(1, 3, 3000, 17) == 2 * 65536 + 32
    assert lib.dh3d_knn_bruteforce_plan(1, 1, 300, 9) == 3 * 65536 + 16
    assert lib.dh3d_knn_sorted_plan(21, 3904, 12) == 2 * 256 + 16 and lib.dh3d_knn_sorted_plan(1, 64, 65) == -1


def test_every_case_is_filed_under_the_launchers_plan():
    from dh3d_amd import pm
    for name, c in C.SORTED_CASES.items():
        assert c.Dp == 3 and pm.knn_sorted_plan(len(c.kinds), c.N, c.K) == c.plan, name
    for name, c in C.BRUTE_CASES.items():
        assert pm.knn_plan(len(c.kinds), c.N, c.K, c.Dp) == c.plan, name


def _reachable_plans():
    """every code the planners return over a sweep that crosses all their thresholds"""
    from dh3d_amd import pm
    Ks = [k for k, _ in WIDTH_EDGES] + [1]
    srt = {pm.knn_sorted_plan(B, N, K) for B in (1, 4, 5, 20, 21, 64, 65, 300) for N in (1, 64, 1000, 4096, 16384) for K in Ks}
    brute = {pm.knn_plan(B, N, K, Dp) for B in (1, 9, 17, 33) for N in (1, 512, 513, 1024, 1025, 2048, 2049, 9000)
             for K in Ks for Dp in (1, 3)}
    return srt, brute


def test_table_reaches_every_plan():
    """The codes the planners can return, enumerated by a sweep, are the ones the case module lists, and the table has a
    case under each."""
    srt, brute = _reachable_plans()
    assert srt == C.SORTED_PLANS and brute == C.BRUTE_PLANS
    assert {c.plan for c in C.SORTED_CASES.values()} == C.SORTED_PLANS
    assert {c.plan for c in C.BRUTE_CASES.values()} == C.BRUTE_PLANS


def test_table_sits_on_the_edges_and_shapes_the_regimes_need():
    G = {C.groups(c) for c in C.SORTED_CASES.values()}
    assert {256, 257, 1280, 1281, 4096, 4097} <= G
    for g in (256, 257, 1280, 1281, 4096, 4097):   # each edge under two list widths
        assert len({c.plan[1] for c in C.SORTED_CASES.values() if C.groups(c) == g}) >= 2, g
    one_wave = [c for c in C.SORTED_CASES.values() if c.plan[0] == 0]
    assert any(((c.N + 63) // 64) % 4 for c in one_wave if c.K <= 16)          # waves without a group at S = 0
    assert any(c.N % 64 for c in C.SORTED_CASES.values())
    for S in (8, 4, 2, 0):                                                      # padding in every regime
        assert any(c.K > c.N for c in C.SORTED_CASES.values() if c.plan[0] == S), S
    for K in (17, 32, 33, 64):                                                  # K > 16 on either side of every G threshold
        gs = [C.groups(c) for c in C.SORTED_CASES.values() if c.K == K]
        assert min(gs) <= 256 and max(gs) > 4096, K
    small = [c for c in C.BRUTE_CASES.values() if c.plan[0] == "small"]
    assert {(c.plan[1], c.plan[2], c.K) for c in small} == {(cpl, q, K) for cpl in (8, 16, 32) for q in (2, 4) for K in (8, 12)}
    # Q = 4: a workgroup is 4 waves x 4 queries; N % 16 = r queries in the last one, (r - 1) % 4 + 1 in its last live wave
    live = {(c.N % 16 - 1) % 4 + 1 for c in small if c.plan[2] == 4 and c.N % 16}
    assert {1, 2, 3} <= live
    assert any(c.plan[2] == 4 and 0 < c.N % 16 <= 12 for c in small)            # and a wave with none
    lane = [c for c in C.BRUTE_CASES.values() if c.plan[0] == "lane"]
    assert {(c.N, c.K) for c in lane} >= {(N, K) for N in (2049, 3000) for K in (3, 4, 5, 8, 9, 16, 17, 32, 33, 64)}
    assert any(c.Dp == 1 for c in C.BRUTE_CASES.values())


def test_cloud_mix_per_regime():
    """Every sorted-scan plan has a crowded and a tie cloud among its cases; every brute-force family has a tie cloud."""
    for plan in C.SORTED_PLANS:
        classes = {C.kind_class(k) for c in C.SORTED_CASES.values() if c.plan == plan for k in c.kinds}
        assert {"crowded", "tie"} <= classes, plan
    for family in ("small", "lane", "anydp"):
        classes = {C.kind_class(k) for c in C.BRUTE_CASES.values() if c.plan[0] == family for k in c.kinds}
        assert "tie" in classes, family
    both = [c for c in C.SORTED_CASES.values() if set(c.kinds) == {"one_point", "scene_duplicates"}]
    assert any(c.N == 4096 and c.K == 16 for c in both)                          # the tie-order case
    for c in list(C.SORTED_CASES.values()) + list(C.BRUTE_CASES.values()):
        assert len(C.sampled_clouds(c)) in (1, 2) and max(C.sampled_clouds(c)) < len(c.kinds)


def test_batches_are_deterministic_and_shared():
    c = C.SORTED_CASES["pad_300x5_k8"]
    a = C.batch(c)
    assert a.shape == (300, 5, 3) and a.dtype.name == "float32" and not a.flags.writeable
    assert C.batch(C.SORTED_CASES["pad_300x5_k16"]) is a                          # same kinds and N: one array
    C._batch_cached.cache_clear()
    assert (C.batch(c) == a).all()
