"""Cases of tests/test_knn_regimes_gpu.py: the brute-force kNN (dh3d_knn_bruteforce / _xyz, csrc/knn.hip knn_launch) and
the pruned scan (dh3d_knn_sorted, knn_sorted_launch) in every launch regime.  No GPU here; tests/test_knn_plan.py pins the
table against the two host-only plan queries and checks what it covers.

A case gives B (the number of per-cloud kinds), N, K, the kinds and the PLAN it expects, as pm.knn_sorted_plan /
pm.knn_plan report it: the GPU test asserts the plan before it compares anything, so a moved threshold cannot quietly take
a case out of the regime it was written for.  Shapes are the smallest that reach a regime.

Sorted scan, plan (S, KMAX): G = B * ceil(N / 64) query groups give S = 8 (G <= 256), 4 (<= 1280), 2 (<= 4096) waves per
group on knn_split_kernel<KMAX, S>, or S = 0, the one-wave knn_sorted_kernel<KMAX> (beyond, and for every K > 16).
Brute force, plan ("small", CPL, Q) | ("lane", KMAX) | ("anydp", KMAX): a wave per query up to N = 2048 (CPL 8 / 16 / 32
by N <= 512 / 1024, Q = 2 queries per wave while B * N <= 16384, else 4), a lane per query beyond, the any-Dp kernel for
Dp != 3.

Cloud kinds are test_ops_gpu._knn_clouds' and the grid regime test's (_cloud): CROWDED ones (scene, clusters: long
candidate streams, most groups pruned) and TIE ones (lattice, duplicates, scene_duplicates, one_point: equal distances, the
reference's (id mod C_THREADS, id div C_THREADS) order decides; one_point: nothing can be pruned)."""
import collections
import functools
import zlib

import numpy as np

from test_knn_grid_regimes_gpu import _cloud, _cyc

CROWDED_KINDS = ("scene", "clusters")
TIE_KINDS = ("lattice", "duplicates", "one_point")

Case = collections.namedtuple("Case", "N K kinds plan Dp")
MIX = ("scene", "uniform", "lattice", "clusters", "duplicates", "one_point")


def _width(K):
    return 4 if K <= 4 else 8 if K <= 8 else 16 if K <= 16 else 32 if K <= 32 else 64


def _sorted_case(B, N, K, S, kinds=MIX):
    km = _width(K)
    if S and K > 16:
        S = 0
    if S == 8 and km == 4:
        km = 8  # (knn_split_kernel<4, 8> does not exist: K <= 4 runs <8, 8>)
    return Case(N, K, _cyc(B, *kinds), (S, km), 3)


def _sorted_cases():
    out = {}
    # many small ragged clouds (16 groups a cloud, the last of 40 points), every regime and both sides of each threshold
    for B, S in ((16, 8), (17, 4), (80, 4), (81, 2), (257, 0)):
        for K in (3, 8, 16):
            out["ragged_%dx1000_k%d" % (B, K)] = _sorted_case(B, 1000, K, S)
    # 63 groups a cloud: the four-wave workgroups of the one-wave kernel end on a wave without a group
    for B, S in ((5, 4), (21, 2), (66, 0)):
        for K in (3, 8, 16):
            out["odd_%dx4031_k%d" % (B, K)] = _sorted_case(B, 4031, K, S)
    # fewer points than K = 8 / 16: ids -1 and FLT_MAX behind the fifth neighbour, in every regime
    for B, S in ((4, 8), (300, 4), (1300, 2), (4100, 0)):
        for K in (3, 8, 16):
            out["pad_%dx5_k%d" % (B, K)] = _sorted_case(B, 5, K, S, ("scene", "lattice", "one_point", "uniform"))
    # the thresholds' edges, G = 256 | 257, 1280 | 1281 (61 groups a cloud), 4096 | 4097 (17 groups a cloud)
    for B, N, S in ((4, 4096, 8), (257, 50, 4), (20, 4096, 4), (21, 3904, 2), (64, 4096, 2), (241, 1088, 0)):
        for K in (5, 12):
            out["edge_%dx%d_k%d" % (B, N, K)] = _sorted_case(B, N, K, S)
    # K > 16: the one-wave kernel whatever G (32 groups: the eight-wave range; 4112 groups: beyond every threshold)
    for B, kinds in ((2, ("scene", "lattice")), (257, MIX)):
        for K in (17, 32, 33, 64):
            out["wide_%dx1000_k%d" % (B, K)] = _sorted_case(B, 1000, K, 8 if B == 2 else 0, kinds)
    # nothing to prune, only the tie order decides
    out["ties_2x4096_k16"] = _sorted_case(2, 4096, 16, 8, ("one_point", "scene_duplicates"))
    return out


def _small_case(B, N, K, kinds=("uniform", "lattice", "duplicates", "one_point")):
    return Case(N, K, _cyc(B, *kinds), ("small", 8 if N <= 512 else 16 if N <= 1024 else 32, 2 if B * N <= 16384 else 4), 3)


def _brute_cases():
    out = {}
    # knn_small_kernel<CPL>: both sides of N = 512 | 513, 1024 | 1025 and of B * N = 16384 (Q 2 | 4); K = 8 takes the
    # screened path (one_point and duplicate-heavy queries fall back from it), K = 12 knn_small_select_all.
    # Ragged Q = 4 shapes (a workgroup = 4 waves x 4 queries): 515 = 32 x 16 + 3, the last wave with a query has 3 and
    # three waves have none; 1001 = 62 x 16 + 9: 1 and one dead wave; 2042 = 127 x 16 + 10: 2 and one dead wave;
    # 2047 = 127 x 16 + 15: 3 in the last wave.
    shapes = ((2, 512), (32, 512), (33, 512), (32, 515), (2, 513), (16, 1024), (17, 1024), (17, 1001), (2, 1025),
              (8, 2048), (9, 2048), (9, 2047), (9, 2042))
    for B, N in shapes:
        for K in (8, 12):
            out["small_%dx%d_k%d" % (B, N, K)] = _small_case(B, N, K)
    # knn_kernel<KMAX>: 2049 = 8 x 256 + 1 = 2 x 1024 + 1 (one query in the last workgroup, one candidate in the last
    # staged chunk) and 3000, on both sides of every list width
    for N in (2049, 3000):
        for K in (3, 4, 5, 8, 9, 16, 17, 32, 33, 64):
            out["lane_4x%d_k%d" % (N, K)] = Case(N, K, ("uniform", "lattice", "duplicates", "scene"), ("lane", _width(K)), 3)
    # knn_anydp_kernel<8 | 16 | 64> at Dp = 1: the x coordinates of the clouds (a lattice's are 32 values: ties everywhere)
    for K in (8, 9, 17):
        out["anydp_2x300_k%d" % K] = Case(300, K, ("lattice", "uniform"), ("anydp", 8 if K <= 8 else 16 if K <= 16 else 64), 1)
    return out


SORTED_CASES = _sorted_cases()
BRUTE_CASES = _brute_cases()

# every code the planners can return
SORTED_PLANS = {(S, km) for S in (4, 2) for km in (4, 8, 16)} | {(8, 8), (8, 16)} | {(0, km) for km in (4, 8, 16, 32, 64)}
BRUTE_PLANS = ({("small", cpl, q) for cpl in (8, 16, 32) for q in (2, 4)} | {("lane", km) for km in (4, 8, 16, 32, 64)}
               | {("anydp", km) for km in (8, 16, 64)})


def groups(c):
    """G = B * ceil(N / 64), the query groups knn_sorted_launch counts"""
    return len(c.kinds) * ((c.N + 63) // 64)


@functools.lru_cache(maxsize=8)
def _batch_cached(kinds, N):
    rng = np.random.default_rng(zlib.crc32(repr((kinds, N)).encode()))
    made = {}
    out = np.empty((len(kinds), N, 3), np.float32)
    for b, k in enumerate(kinds):
        # a batch of thousands of clouds repeats each kind's first 16 draws: the regimes differ by the launch, not the data
        slot = (k, (b // len(set(kinds))) % 16)
        if slot not in made:
            made[slot] = _cloud(k, N, rng)
        out[b] = made[slot]
    out.setflags(write=False)
    return out


def batch(c):
    """the case's clouds [B, N, 3] float32 (read-only; cases that share kinds and N share the array)"""
    return _batch_cached(c.kinds, c.N)


def kind_class(k):
    return "tie" if k in TIE_KINDS or k == "scene_duplicates" else "crowded" if k in CROWDED_KINDS else "plain"


def sampled_clouds(c):
    """the clouds the CPU references look at: the first tie cloud, the first crowded one, else the first other -- two at most"""
    first = {}
    for b, k in enumerate(c.kinds):
        first.setdefault(kind_class(k), b)
    return sorted([first[cls] for cls in ("tie", "crowded", "plain") if cls in first][:2])
