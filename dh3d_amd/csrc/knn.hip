// Brute-force exact kNN for gfx950 -- replaces KnnBruteforceFunctor<GPUDevice,float,int>
// (user_ops/kernels/knn_bruteforce_kernel_gpu.cu.cc:36-134,163-228).
//
// The reference sorts all N (distance, id) pairs per query with cub::BlockRadixSort and keeps K.
// Here one lane owns one query and streams every candidate of its cloud from LDS (all 64 lanes read the
// same 16 bytes -> broadcast ds_read_b128).  Per 8 candidates the hot loop is 12 packed-f32 VALU ops
// (v_pk_add/mul/fma: two candidates per instruction) + a min tree + ONE branch: a candidate is screened
// on its squared distance against a conservative bound derived from the lane's current K-th entry.
// Survivors are not inserted on the spot -- with 64 independent queries per wave "some lane has a
// survivor" is true far more often than "this lane has one", and a divergent K-deep insertion per hit
// dominated the first version (profiles/r01_a).  They are appended to a per-lane LDS queue (3 VALU) and
// the whole wave drains its queues only when one of them is half full: then the IEEE sqrt, the tie key
// and the register insertion run back to back for every queued entry.
//
// Bit-exactness (compiled with -ffp-contract=off; every rounding below is explicit):
//   distance  d = sqrt( fma(dz,dz, fma(dy,dy, dx*dx)) ), dx = c.x - q.x   (gpu.cu.cc:102-107 with
//             nvcc's default fma contraction of `sum += val*val`)
//   order     ascending (d, tb), tb(x) = (x % C_THREADS)*C_VPT + x / C_THREADS  -- the rank of
//             point x in CUB's blocked arrangement, which the stable radix sort preserves among
//             equal keys (gpu.cu.cc:98-123); (C_THREADS, C_VPT) from the N ladder (:181-216).
//   The list is kept as 64-bit keys (bits(d) << 32 | tb): d >= 0, so unsigned order == (d, tb) order.
#include <float.h>
#include <limits.h>

#include <type_traits>

#include "cell_walk.h"
#include "common.h"
#include "group_box.h"
#include "keys.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

constexpr int kQueriesPerBlock = 256;
constexpr int kChunk = 1024;   // candidates staged per LDS round: 256 groups of 4 x 12 floats = 12 KiB
constexpr int kQueue = 16;     // per-lane survivor queue depth (drained when any lane holds > 8)

struct KnnLadder {
  int log2ct;  // log2(C_THREADS)
  int ctmask;  // C_THREADS-1
  int cv;      // C_VPT
};

static KnnLadder knn_ladder(int N) {
  int t, v;
  if (N <= 32) { t = 32; v = 1; }
  else if (N <= 64) { t = 64; v = 1; }
  else if (N <= 128) { t = 128; v = 1; }
  else if (N <= 256) { t = 128; v = 2; }
  else if (N <= 512) { t = 128; v = 4; }
  else if (N <= 1024) { t = 256; v = 4; }
  else if (N <= 2048) { t = 256; v = 8; }
  else if (N <= 4096) { t = 512; v = 8; }
  else if (N <= 8192) { t = 1024; v = 8; }
  else { t = 1024; v = (N + 1023) / 1024; }  // superset: upstream stops at 8192
  KnnLadder l;
  l.ctmask = t - 1;
  l.cv = v;
  l.log2ct = 0;
  while ((1 << l.log2ct) < t) ++l.log2ct;
  return l;
}

// the set bit of m (!= 0) nearest to position gl (0..63), wave-uniform: candidate groups are visited outwards from the
// queries' own group -- Morton neighbours are mostly spatial neighbours, and a K-list fed nearest-first takes ~K
// insertions where one fed in index order takes ~K ln(n/K)
__device__ __forceinline__ int knn_pick_near(unsigned long long m, int gl) {
  const unsigned long long up = m >> gl, dn = m & ((1ull << gl) - 1);
  const int da = up ? __builtin_ctzll(up) : 128;
  const int db = dn ? gl - (63 - __builtin_clzll(dn)) : 128;
  return da <= db ? gl + da : gl - db;
}

template <int KMAX>
struct KnnState {
  u64 keys[KMAX];
  float bound;  // s > bound  =>  sqrt(s) > current K-th distance
};

constexpr u64 kKnnNoKey = ~0ull;  // an unfilled slot: above every real key
template <int KMAX>
__device__ __forceinline__ void knn_list_clear(KnnState<KMAX> &st) {  // (the bound stays)
#pragma unroll
  for (int i = 0; i < KMAX; ++i) st.keys[i] = kKnnNoKey;
}
// An empty list that takes everything.  knn_kernel and knn_sorted_kernel keep these two lines written out on purpose: with
// the call in their place the compiler allocated both kernels differently (knn_sorted_kernel<32>: 203 -> 170 VGPRs, the
// insertion's compares chained through vcc) and knn_sorted at K = 32, 8 x 8192, measured 0.606 -> 0.720 ms.
template <int KMAX>
__device__ __forceinline__ void knn_list_reset(KnnState<KMAX> &st) {
  knn_list_clear(st);
  st.bound = INFINITY;
}

// The screening bound that a list entry's distance gives, from the high word of its key: the (1 + 2^-20)-inflated square
// of the distance -- a relative 2^-20 in s is 2^-21 in d, more than 3 ulp, so any s above it has sqrt(s) > d strictly.
// An unfilled slot (or a NaN distance) gives none: false, and `out` is left as it is.
__device__ __forceinline__ bool knn_inflated_sq(const unsigned key_hi, float &out) {
  if (key_hi > 0x7f800000u) return false;
  const float d = __uint_as_float(key_hi);
  out = __fmul_rn(__fmul_rn(d, d), 1.000001f);
  return true;
}

// One slot of the output.  Fewer than K points: the reference pads with id -1 / FLT_MAX (:110-111); otherwise the id is
// the CUB rank tb turned back into the point's index (tb = (x % C_THREADS) * C_VPT + x / C_THREADS).
__device__ __forceinline__ void knn_emit(const u64 key, const KnnLadder &lad, int32_t *nn, float *dist) {
  if (key == kKnnNoKey) {
    *nn = -1;
    *dist = FLT_MAX;
  } else {
    const unsigned tb = (unsigned)key;
    *nn = (int)(((tb % (unsigned)lad.cv) << lad.log2ct) + tb / (unsigned)lad.cv);
    *dist = __uint_as_float((unsigned)(key >> 32));
  }
}
// the first K entries of a lane's list
template <int KMAX>
__device__ __forceinline__ void knn_emit_list(const KnnState<KMAX> &st, int K, const KnnLadder &lad, int32_t *o_nn,
                                              float *o_d) {
#pragma unroll
  for (int i = 0; i < KMAX; ++i)
    if (i < K) knn_emit(st.keys[i], lad, o_nn + i, o_d + i);
}

// KEEP_MIN: the bound may already be tighter than this list's own K-th entry (knn_split_kernel)
template <int KMAX, bool KEEP_MIN = false>
__device__ __forceinline__ void knn_insert_key(KnnState<KMAX> &st, const u64 key) {
  if (key < st.keys[KMAX - 1]) {
    if constexpr (KMAX <= 16) {
      // the list is sorted and keys are unique: entry i becomes its left neighbour where the key goes in further
      // left, the key where it goes in exactly here.  KMAX - 1 independent compares and two selects per entry --
      // no dependent chain (a bubble pass is one compare + four selects per step, each waiting for the last)
      bool lt[KMAX];
#pragma unroll
      for (int i = 0; i < KMAX - 1; ++i) lt[i] = key < st.keys[i];
      lt[KMAX - 1] = true;
#pragma unroll
      for (int i = KMAX - 1; i > 0; --i) {
        const u64 in = lt[i - 1] ? st.keys[i - 1] : key;
        st.keys[i] = lt[i] ? in : st.keys[i];
      }
      st.keys[0] = lt[0] ? key : st.keys[0];
    } else {
      st.keys[KMAX - 1] = key;
#pragma unroll
      for (int i = KMAX - 1; i > 0; --i) {
        const u64 a = st.keys[i - 1], b = st.keys[i];
        const bool lt = b < a;
        st.keys[i - 1] = lt ? b : a;
        st.keys[i] = lt ? a : b;
      }
    }
    float nb;
    if (knn_inflated_sq((unsigned)(st.keys[KMAX - 1] >> 32), nb)) st.bound = KEEP_MIN ? fminf(st.bound, nb) : nb;
  }
}
template <int KMAX, bool KEEP_MIN = false>
__device__ __forceinline__ void knn_offer(KnnState<KMAX> &st, float s, int x, const KnnLadder &lad) {
  if (s <= st.bound) {
    const float d = sqrtf(s);  // IEEE-rounded (llvm.sqrt.f32 under -fhip-fp32-correctly-rounded-divide-sqrt)
    const unsigned tb = (unsigned)((x & lad.ctmask) * lad.cv + (x >> lad.log2ct));
    knn_insert_key<KMAX, KEEP_MIN>(st, ((u64)__float_as_uint(d) << 32) | tb);
  }
}


// Squared distances (reference rounding order) of 8 consecutive candidates of the pair-SoA LDS image.
__device__ __forceinline__ void knn_dist8(const float *g0, const f32x2 qx2, const f32x2 qy2, const f32x2 qz2,
                                          f32x2 (&s)[4]) {
  const f32x4 a0 = *reinterpret_cast<const f32x4 *>(g0), a1 = *reinterpret_cast<const f32x4 *>(g0 + 4),
              a2 = *reinterpret_cast<const f32x4 *>(g0 + 8), b0 = *reinterpret_cast<const f32x4 *>(g0 + 12),
              b1 = *reinterpret_cast<const f32x4 *>(g0 + 16), b2 = *reinterpret_cast<const f32x4 *>(g0 + 20);
  {
    const f32x2 dx = f32x2{a0[0], a0[1]} - qx2, dy = f32x2{a0[2], a0[3]} - qy2, dz = f32x2{a1[0], a1[1]} - qz2;
    s[0] = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
  }
  {
    const f32x2 dx = f32x2{a1[2], a1[3]} - qx2, dy = f32x2{a2[0], a2[1]} - qy2, dz = f32x2{a2[2], a2[3]} - qz2;
    s[1] = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
  }
  {
    const f32x2 dx = f32x2{b0[0], b0[1]} - qx2, dy = f32x2{b0[2], b0[3]} - qy2, dz = f32x2{b1[0], b1[1]} - qz2;
    s[2] = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
  }
  {
    const f32x2 dx = f32x2{b1[2], b1[3]} - qx2, dy = f32x2{b2[0], b2[1]} - qy2, dz = f32x2{b2[2], b2[3]} - qz2;
    s[3] = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
  }
}
__device__ __forceinline__ float knn_min8(const f32x2 (&s)[4]) {
  return fminf(fminf(fminf(s[0][0], s[0][1]), fminf(s[1][0], s[1][1])),
               fminf(fminf(s[2][0], s[2][1]), fminf(s[3][0], s[3][1])));
}

// The screen-and-queue step of the lane-per-query kernels, over the 32 candidates whose pair-SoA image starts at img:
// candidates first .. first + 31 of the caller's numbering, real below `end` (padding is +inf).  24 broadcast LDS reads + 48 packed ops with nothing between them that
// depends on the lane's list, so they pipeline; ONE wave-uniform test decides whether anybody needs the slow path (a
// per-8 branch serialised every step behind its own LDS latency: 650-800 cycles/step measured with one wave per SIMD).
// A survivor (s <= bound) is appended to the lane's queue as (bits(s), id_of(its number)): slot cnt of the
// lane is q[cnt * qstride + col].  drain() -- the caller's: it empties every lane's queue into the lists and zeroes cnt, and
// may tighten bound -- runs for the whole wave as soon as one queue could not take another eight.
template <class IdOf, class Drain>
__device__ __forceinline__ void knn_screen32(const float *img, uint2 *q, const int qstride, const int col, const bool valid,
                                             const int first, const int end,
                                             const f32x2 qx2, const f32x2 qy2, const f32x2 qz2, const float &bound, int &cnt,
                                             IdOf id_of, Drain drain) {
  f32x2 s[4][4];
  float mn[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    knn_dist8(img + 2 * u * 12, qx2, qy2, qz2, s[u]);
    mn[u] = knn_min8(s[u]);
  }
  const float m = fminf(fminf(mn[0], mn[1]), fminf(mn[2], mn[3]));
  if (__any(valid && m <= bound)) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (valid && mn[u] <= bound) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const float sv = s[u][t >> 1][t & 1];
          if (sv <= bound && first + 8 * u + t < end) {
            q[cnt * qstride + col] = make_uint2(__float_as_uint(sv), (unsigned)id_of(first + 8 * u + t));
            ++cnt;
          }
        }
      }
      if (__any(cnt > kQueue - 8)) drain();  // wave-uniform
    }
  }
}

// The queue drain of the group-scanning kernels (slot i of a lane is q[i * 64 + lane]): ONE copy of the (long)
// insertion per drain site, the next slot requested from LDS while this one is inserted.  Unrolled over the 16 slots
// knn_sorted_kernel was > 100 KB of code (the drain is inlined at every site of the scan); the instruction cache coped with
// that in the shipped build (0.2 % misses, profiles/r03_d_pmc_knn.txt) but not in the probe build, and nothing is gained
// by the unrolling.
template <int KMAX, bool KEEP_MIN>
__device__ __forceinline__ void knn_drain_queue(KnnState<KMAX> &st, int &cnt, const uint2 *q, const int lane,
                                                const KnnLadder &lad) {
  const int deepest = -wave_min_i32(-cnt);
  uint2 nxt = q[lane];
#pragma unroll 1
  for (int i = 0; i < deepest; ++i) {  // wave-uniform trip count
    const uint2 e = nxt;
    if (i + 1 < deepest) nxt = q[(i + 1) * 64 + lane];
    if (i < cnt) knn_offer<KMAX, KEEP_MIN>(st, __uint_as_float(e.x), (int)e.y, lad);
  }
  cnt = 0;
}

// the lanes' records of a 64-record group (one each; padding is +inf) -> the wave's pair-SoA image and id strip
__device__ __forceinline__ void knn_stage_group(float *my_c, int *my_id, const int lane, const float4 cr) {
  my_c[cand4_slot(lane, 0)] = cr.x;
  my_c[cand4_slot(lane, 1)] = cr.y;
  my_c[cand4_slot(lane, 2)] = cr.z;
  my_id[lane] = __float_as_int(cr.w);
  __builtin_amdgcn_wave_barrier();
}
// One group of the sorted cloud (clen real records) through the screen: staged, then 32 candidates per step.
template <class Drain>
__device__ __forceinline__ void knn_scan_group(float *my_c, int *my_id, uint2 *my_q, const int lane, const float4 cr,
                                               const int clen, const bool valid, const f32x2 qx2, const f32x2 qy2,
                                               const f32x2 qz2, const float &bound, int &cnt, Drain drain) {
  knn_stage_group(my_c, my_id, lane, cr);
  for (int j = 0; j < clen; j += 32)
    knn_screen32(my_c + (j >> 2) * 12, my_q, 64, lane, valid, j, clen, qx2, qy2, qz2, bound, cnt,
                 [my_id](int i) { return my_id[i]; }, drain);
  __builtin_amdgcn_wave_barrier();
}

// The visit loop of a chunk walk: the candidate groups of `mask` (bit l = the group whose box lane l holds: clo, chi, and
// bd = its gap to the query group's box), nearest to position gl first; the next group's records are prefetched while
// this one is scanned.  group_of(l) names the group, load_group(g) fetches the lanes' records of it, scan_group(g, records)
// evaluates it (and may tighten bound and wave_bound = the loosest bound of the wave's valid lanes).
template <class GroupOf, class LoadGroup, class ScanGroup>
__device__ __forceinline__ void knn_visit_groups(unsigned long long mask, const int gl, const float bd, const float4 &clo,
                                                 const float4 &chi, const float4 &qr, const bool valid, const float &bound,
                                                 const float &wave_bound, GroupOf group_of, LoadGroup load_group,
                                                 ScanGroup scan_group) {
  if (!mask) return;
  int l = knn_pick_near(mask, gl);
  mask &= ~(1ull << l);
  float4 nxt = load_group(group_of(l));
  while (true) {
    const int lcur = l;
    const float4 cr = nxt;
    const bool more = mask != 0;
    if (more) {
      l = knn_pick_near(mask, gl);
      mask &= ~(1ull << l);
      nxt = load_group(group_of(l));
    }
    const float bdl = wave_bcast_f32(bd, lcur);
    if (bdl <= wave_bound) {  // the bound may have tightened since the ballot
      // box against box says "some query of the wave MIGHT reach the group" with the union of the 64 queries and
      // the loosest of their bounds; the same test per query (point to box, own bound) is ~20 instructions
      // against the ~450 of scanning the group, and decides most of the overlapping (tier 0) groups of a query
      // group whose own box is large (Morton order jumps across the cloud inside it)
      const float lx = wave_bcast_f32(clo.x, lcur), ly = wave_bcast_f32(clo.y, lcur), lz = wave_bcast_f32(clo.z, lcur);
      const float hx = wave_bcast_f32(chi.x, lcur), hy = wave_bcast_f32(chi.y, lcur), hz = wave_bcast_f32(chi.z, lcur);
      const float pd = point_box_gap2(lx, ly, lz, hx, hy, hz, qr.x, qr.y, qr.z);
      if (__any(valid && pd <= bound)) scan_group(group_of(lcur), cr);
    }
    if (!more) break;
  }
}

// XYZ_LAYOUT: false = positions [B,3,N] (op layout), true = xyz [B,N,3].
template <int KMAX, bool XYZ_LAYOUT>
__global__ __launch_bounds__(kQueriesPerBlock) void knn_kernel(const float *__restrict__ pos, int N,
                                                              int K, KnnLadder lad,
                                                              int32_t *__restrict__ nn,
                                                              float *__restrict__ dist) {
  __shared__ __attribute__((aligned(16))) float s_c[kChunk * 3];
  __shared__ uint2 s_q[kQueue * kQueriesPerBlock];
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const int y = blockIdx.x * kQueriesPerBlock + tid;
  const float *pc = pos + (size_t)b * 3 * N;

  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (y < N) {
    if (XYZ_LAYOUT) { qx = pc[(size_t)y * 3]; qy = pc[(size_t)y * 3 + 1]; qz = pc[(size_t)y * 3 + 2]; }
    else { qx = pc[y]; qy = pc[(size_t)N + y]; qz = pc[(size_t)2 * N + y]; }
  }
  const f32x2 qx2 = {qx, qx}, qy2 = {qy, qy}, qz2 = {qz, qz};

  KnnState<KMAX> st;
#pragma unroll
  for (int i = 0; i < KMAX; ++i) st.keys[i] = kKnnNoKey;  // (written out, not knn_list_reset: see there)
  st.bound = INFINITY;
  int cnt = 0;
  auto drain = [&]() {  // every lane's queue, as deep as the deepest
    for (int i = 0; i < kQueue; ++i) {
      if (!__any(i < cnt)) break;
      if (i < cnt) {
        const uint2 e = s_q[i * kQueriesPerBlock + tid];
        knn_offer<KMAX>(st, __uint_as_float(e.x), (int)e.y, lad);
      }
    }
    cnt = 0;
  };

  for (int base = 0; base < N; base += kChunk) {
    const int len = min(kChunk, N - base);
    const int len8 = (len + 31) & ~31;  // padded (+inf) to the 32-candidate step of the scan loop
    __syncthreads();
    if (XYZ_LAYOUT) {
      for (int e = tid; e < len8 * 3; e += kQueriesPerBlock) {
        const int c = e / 3, comp = e - c * 3;
        s_c[cand4_slot(c, comp)] = c < len ? pc[(size_t)base * 3 + e] : INFINITY;
      }
    } else {
      for (int e = tid; e < len8 * 3; e += kQueriesPerBlock) {
        const int comp = e / len8, c = e - comp * len8;
        s_c[cand4_slot(c, comp)] = c < len ? pc[(size_t)comp * N + base + c] : INFINITY;
      }
    }
    __syncthreads();
    const int len32 = (len8 + 31) & ~31;  // the image is padded with +inf up to a multiple of 32
    for (int j = 0; j < len32; j += 32)
      knn_screen32(s_c + (j >> 2) * 12, s_q, kQueriesPerBlock, tid, y < N, base + j, N, qx2, qy2, qz2, st.bound, cnt,
                   [](int x) { return x; }, drain);
  }
  for (int i = 0; i < kQueue; ++i) {  // final drain
    if (i < cnt) {
      const uint2 e = s_q[i * kQueriesPerBlock + tid];
      knn_offer<KMAX>(st, __uint_as_float(e.x), (int)e.y, lad);
    }
  }

  if (y < N) knn_emit_list(st, K, lad, nn + ((size_t)b * N + y) * K, dist + ((size_t)b * N + y) * K);
}

// ------------------------------------------------------------------------------------------------
// kNN on a spatially ordered cloud (spatial.hip).  Still exhaustive in effect -- every candidate is either
// evaluated or PROVEN unable to enter any list of the wave -- but most of the N^2 work disappears:
// a wave owns one group of 64 Morton-consecutive queries and walks the candidate groups nearest-first
// (g, g+1, g-1, g+2, ...).  A candidate group is skipped when the squared distance between the two
// bounding boxes exceeds every lane's current screening bound (which already over-estimates the K-th
// distance): a skipped candidate would also have failed the per-candidate screen (group_box.h).  Evaluated groups go through
// exactly the same screen / queue / 64-bit-key insertion as knn_kernel, so ids and distances are
// bit-identical to it (tests).  Waves are independent: no block-level barrier.
constexpr int kSortedWaves = 4;

template <int KMAX>
__global__ __launch_bounds__(64 * kSortedWaves) void knn_sorted_kernel(const float4 *__restrict__ sorted,
                                                                    const float *__restrict__ gbox, int N,
                                                                    int K, KnnLadder lad,
                                                                    int32_t *__restrict__ nn,
                                                                    float *__restrict__ dist, const int *__restrict__ gate) {
  if (gate && !gate[(size_t)blockIdx.y * kCellInts + kCellFlag]) return;  // (dh3d_knn_grid: only the clouds the cell lists left)
  __shared__ __attribute__((aligned(16))) float s_c[kSortedWaves][64 * 3];  // pair-SoA image per wave
  __shared__ uint2 s_q[kSortedWaves][kQueue * 64];
  __shared__ int s_id[kSortedWaves][64];  // original ids of the staged candidates
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int NG = (N + 63) / 64;
  const int g = blockIdx.x * kSortedWaves + wave;
  if (g >= NG) return;  // whole wave
  const float4 *sc = sorted + (size_t)b * N;
  const float4 *gb = reinterpret_cast<const float4 *>(gbox) + (size_t)b * NG * 2;  // [lo.xyz,_ | hi.xyz,_]
  float *my_c = s_c[wave];
  uint2 *my_q = s_q[wave];
  int *my_id = s_id[wave];

  const int qi = g * 64 + lane;
  const bool valid = qi < N;
  const float4 pad = make_float4(INFINITY, INFINITY, INFINITY, __int_as_float(-1));
  float4 qr = valid ? sc[qi] : pad;
  const f32x2 qx2 = {qr.x, qr.x}, qy2 = {qr.y, qr.y}, qz2 = {qr.z, qr.z};
  const float4 qlo = gb[g * 2], qhi = gb[g * 2 + 1];

  KnnState<KMAX> st;
#pragma unroll
  for (int i = 0; i < KMAX; ++i) st.keys[i] = kKnnNoKey;  // (written out, not knn_list_reset: see there)
  st.bound = INFINITY;
  int cnt = 0;
  float wave_bound = INFINITY;  // max over the wave's valid lanes of st.bound (refreshed after each drain)

  auto drain = [&]() {
    knn_drain_queue<KMAX, false>(st, cnt, my_q, lane, lad);
    wave_bound = wave_max_f32(valid ? st.bound : 0.f);
  };
  // evaluate the 64 candidates of group gcc (records already in `cr`, one per lane)
  auto scan_group = [&](int gcc, const float4 cr) {
    knn_scan_group(my_c, my_id, my_q, lane, cr, min(64, N - gcc * 64), valid, qx2, qy2, qz2, st.bound, cnt, drain);
  };
  auto load_group = [&](int gcc) { const int ci = gcc * 64 + lane; return ci < N ? sc[ci] : pad; };

  // own group first: it fills every list and gives the first finite bounds
  scan_group(g, qr);
  if (__any(cnt > 0)) drain();

  // other groups: lane <-> candidate group box test (64 groups per round), overlapping boxes (distance 0)
  // first, then whatever still lies within the (tightened) bound; next group's records are prefetched.
  const int cg = g >> 6, NC = (NG + 63) >> 6;
  for (int tier = 0; tier < 2; ++tier) {
    for (int k = 0; k < 2 * NC; ++k) {  // chunks of 64 groups outwards from the own one: cg, cg+1, cg-1, cg+2, ...
      const int ci = cg + ((k & 1) ? (k + 1) / 2 : -(k / 2));
      if (ci < 0 || ci >= NC) continue;
      const int c0 = ci * 64, gl = min(max(g - c0, 0), 63);
      const int gi = c0 + lane;
      const bool other = gi < NG && gi != g;
      float bd = INFINITY;
      float4 clo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), chi = clo;
      if (other) {
        clo = gb[gi * 2];
        chi = gb[gi * 2 + 1];
        bd = group_box_gap2(clo, chi, qlo, qhi);
      }
      const unsigned long long mask =
          tier == 0 ? __ballot(other && bd == 0.f) : __ballot(other && bd > 0.f && bd <= wave_bound);
      knn_visit_groups(mask, gl, bd, clo, chi, qr, valid, st.bound, wave_bound, [c0](int l) { return c0 + l; }, load_group,
                       scan_group);
    }
  }
  if (__any(cnt > 0)) drain();

  if (valid) {
    const size_t y = (size_t)b * N + __float_as_int(qr.w);  // original index of this query
    knn_emit_list(st, K, lad, nn + y * K, dist + y * K);
  }
}

// ------------------------------------------------------------------------------------------------
// The same search with S waves per query group.  knn_sorted_kernel has one wave per 64 queries: at the model's sizes
// that is ONE wave per SIMD on the whole chip, each a dependent instruction stream (a wave issues ~1 instruction per
// 4.6 cycles), and the kernel ends with its slowest group.  Here the S waves of a workgroup hold the same 64 queries and
// split the CANDIDATE groups (group gi belongs to wave gi % S), each with its own K-lists; the lists are merged through
// LDS at the end.  A wave alone would prune with the K-th entry of a list that saw 1/S of the candidates; instead every
// wave publishes, per query, the distance of its ceil(K/S)-th entry: S lists hold at least K candidates within the
// largest of those S distances, so max_w d_w bounds the true K-th distance -- as does any single wave's own K-th
// distance; the screen uses the smallest of all of these.  Published values are only ever replaced by smaller ones, so a stale read is still valid
// (no barrier).  Every candidate is evaluated by exactly one wave with the same arithmetic, keys are unique: the merged
// list is the list of the one-wave kernel, bit for bit.
// The body is a device function over a raw LDS block (knn_split_lds_bytes<S>()): knn_split_kernel gives it a block of its
// own, knn_grid_kernel ALIASES it with its candidate lists and serves a crowded cloud in the same launch (round 6: the
// pruned scan as a second launch behind the cell lists was a 4.8 us no-op on every uniform cloud, and vice versa).
// The contract with those callers: the body is entered by whole groups of S waves (wave0 = the group's first), and a group
// may share its workgroup with another group or with idle waves (knn_grid_kernel<4, 2>: two groups of two).  Its
// __syncthreads() are the WORKGROUP's, so the number it executes must not depend on data -- 2 + 2 log2(S), whatever the
// cloud -- and it must not return early: every wave of a group that enters runs to the end.
template <int S>
__host__ __device__ constexpr int knn_split_lds_bytes() {
  return S * (64 * 3 * 4 + kQueue * 64 * 8 + 64 * 4 + 64 * 4 + 64 * 4);
}
template <int KMAX, int S>
__device__ __forceinline__ void knn_split_body(const float4 *__restrict__ sorted, const float *__restrict__ gbox, int N, int K,
                                               const KnnLadder lad, int32_t *__restrict__ nn, float *__restrict__ dist,
                                               const int b, const int g, unsigned char *lds, const int wave0 = 0) {
  static_assert(KMAX * 64 * sizeof(u64) <= kQueue * 64 * sizeof(uint2), "a K-list fits its wave's survivor queue");
  uint2 (*s_q)[kQueue * 64] = reinterpret_cast<uint2 (*)[kQueue * 64]>(lds);                     // [S] survivor queues
  float (*s_c)[64 * 3] = reinterpret_cast<float (*)[64 * 3]>(lds + S * kQueue * 64 * 8);         // [S] pair-SoA image per wave
  int (*s_id)[64] = reinterpret_cast<int (*)[64]>(lds + S * (kQueue * 64 * 8 + 64 * 3 * 4));     // [S]
  float (*s_share)[64] = reinterpret_cast<float (*)[64]>(lds + S * (kQueue * 64 * 8 + 64 * 3 * 4 + 64 * 4));  // per wave, per query:
                                                                 // inflated square of the distance of its R-th entry
  float (*s_kth)[64] = reinterpret_cast<float (*)[64]>(lds + S * (kQueue * 64 * 8 + 64 * 3 * 4 + 64 * 8));    // ... and of its K-th
                                                                 // entry (its own screening bound)
  constexpr int R = (KMAX + S - 1) / S - 1;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6) - wave0);   // (wave0: the first of this group's S waves)
  const int NG = (N + 63) / 64;
  const float4 *sc = sorted + (size_t)b * N;
  const float4 *gb = reinterpret_cast<const float4 *>(gbox) + (size_t)b * NG * 2;  // [lo.xyz,_ | hi.xyz,_]
  float *my_c = s_c[wave];
  uint2 *my_q = s_q[wave];
  int *my_id = s_id[wave];

  const int qi = g * 64 + lane;
  const bool valid = qi < N;
  const float4 pad = make_float4(INFINITY, INFINITY, INFINITY, __int_as_float(-1));
  const float4 qr = valid ? sc[qi] : pad;
  const f32x2 qx2 = {qr.x, qr.x}, qy2 = {qr.y, qr.y}, qz2 = {qr.z, qr.z};
  const float4 qlo = gb[g * 2], qhi = gb[g * 2 + 1];

  KnnState<KMAX> st;
  knn_list_reset(st);
  int cnt = 0;
  float wave_bound = INFINITY;
  s_share[wave][lane] = INFINITY;
  s_kth[wave][lane] = INFINITY;
  __syncthreads();

  // everyone's progress -> my screen: the true K-th distance is at most any wave's own K-th, and at most the largest
  // of the S R-th distances
  auto adopt = [&](float mx) {
    float mk = st.bound;
#pragma unroll
    for (int w = 1; w < S; ++w) {
      mx = fmaxf(mx, s_share[(wave + w) % S][lane]);
      mk = fminf(mk, s_kth[(wave + w) % S][lane]);
    }
    st.bound = fminf(mk, mx);
    wave_bound = wave_max_f32(valid ? st.bound : 0.f);
  };

  auto drain = [&]() {
    knn_drain_queue<KMAX, true>(st, cnt, my_q, lane, lad);
    // publish my R-th distance, take the largest of everyone's
    float mx = INFINITY;
    knn_inflated_sq((unsigned)(st.keys[R] >> 32), mx);
    s_share[wave][lane] = mx;
    float kth;
    if (knn_inflated_sq((unsigned)(st.keys[KMAX - 1] >> 32), kth)) s_kth[wave][lane] = kth;
    adopt(mx);
  };
  auto scan_group = [&](int gcc, const float4 cr) {
    knn_scan_group(my_c, my_id, my_q, lane, cr, min(64, N - gcc * 64), valid, qx2, qy2, qz2, st.bound, cnt, drain);
  };
  auto load_group = [&](int gcc) { const int ci = gcc * 64 + lane; return ci < N ? sc[ci] : pad; };

  // lane <-> a candidate group this wave OWNS: the j-th is group j * S + wave.  Box against box in the lanes, 64 owned
  // groups per round; their boxes are requested before the own group is scanned and stay in registers for both tiers.
  const int NO = (NG - wave + S - 1) / S, NCH = (NO + 63) >> 6;  // owned groups, chunks of 64 of them
  const int jg = g / S, cj = min(jg >> 6, max(NCH - 1, 0));      // where the own group sits among them
  bool other = false;
  float bd = INFINITY;
  float4 clo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), chi = clo;
  auto fetch_boxes = [&](int ci) {
    const int j = ci * 64 + lane, gi = j * S + wave;
    other = j < NO && gi != g;
    if (other) {
      clo = gb[gi * 2];
      chi = gb[gi * 2 + 1];
    }
  };
  auto test_boxes = [&]() {
    bd = INFINITY;
    if (other) bd = group_box_gap2(clo, chi, qlo, qhi);
  };
  if (NCH == 1) fetch_boxes(0);

  {
    // The queries' own group goes first, its blocks of 8 candidates dealt round-robin to the S waves: every wave enters
    // the other groups with a list of its own and -- after the one barrier -- a bound all 64 candidates contributed
    // to.  (With the group scanned by its owner alone the other waves met their first group with no bound at all and
    // queued every candidate of it.)
    knn_stage_group(my_c, my_id, lane, qr);
    const int clen = min(64, N - g * 64);
    for (int blk = wave; blk * 8 < clen; blk += S) {
      f32x2 sq[4];
      knn_dist8(my_c + 2 * blk * 12, qx2, qy2, qz2, sq);
      if (valid) {
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const float sv = sq[t >> 1][t & 1];
          if (sv <= st.bound && blk * 8 + t < clen) {
            my_q[cnt * 64 + lane] = make_uint2(__float_as_uint(sv), (unsigned)my_id[blk * 8 + t]);
            ++cnt;
          }
        }
      }
      if (__any(cnt > 0)) drain();
    }
    __builtin_amdgcn_wave_barrier();
    __syncthreads();
    adopt(s_share[wave][lane]);
  }
  for (int tier = 0; tier < 2; ++tier) {
    for (int k = 0; k < 2 * NCH; ++k) {  // chunks of 64 owned groups outwards from the own one: cj, cj+1, cj-1, ...
      const int ci = cj + ((k & 1) ? (k + 1) / 2 : -(k / 2));
      if (ci < 0 || ci >= NCH) continue;
      if (NCH > 1) fetch_boxes(ci);  // one chunk (N <= 64*64*S points): fetched once, before the own group
      if (NCH > 1 || tier == 0) test_boxes();
      const int gl = min(max(jg - ci * 64, 0), 63);
      if (tier == 1) adopt(s_share[wave][lane]);  // the others have worked since the last look
      const unsigned long long mask =
          tier == 0 ? __ballot(other && bd == 0.f) : __ballot(other && bd > 0.f && bd <= wave_bound);
      knn_visit_groups(mask, gl, bd, clo, chi, qr, valid, st.bound, wave_bound,
                       [ci, wave](int l) { return (ci * 64 + l) * S + wave; }, load_group, scan_group);
    }
  }
  if (__any(cnt > 0)) drain();

  // merge the S lists (tree: w <- w + step), keys are unique so plain insertion
  for (int step = S / 2; step >= 1; step >>= 1) {
    __syncthreads();  // the queues of the waves about to publish are drained
    if (wave >= step && wave < 2 * step) {
#pragma unroll
      for (int i = 0; i < KMAX; ++i)
        my_q[i * 64 + lane] = make_uint2((unsigned)st.keys[i], (unsigned)(st.keys[i] >> 32));
    }
    __syncthreads();
    if (wave < step) {
      const uint2 *oq = s_q[wave + step];
#pragma unroll
      for (int i = 0; i < KMAX; ++i) {
        const uint2 e = oq[i * 64 + lane];
        const u64 key = ((u64)e.y << 32) | e.x;
        if (key < st.keys[KMAX - 1]) {
          st.keys[KMAX - 1] = key;
#pragma unroll
          for (int t = KMAX - 1; t > 0; --t) {
            const u64 a = st.keys[t - 1], c = st.keys[t];
            const bool lt = c < a;
            st.keys[t - 1] = lt ? c : a;
            st.keys[t] = lt ? a : c;
          }
        }
      }
    }
  }

  if (wave == 0 && valid) {
    const size_t y = (size_t)b * N + __float_as_int(qr.w);  // original index of this query
    knn_emit_list(st, K, lad, nn + y * K, dist + y * K);
  }
}


template <int KMAX, int S>
__global__ __launch_bounds__(64 * S) void knn_split_kernel(const float4 *__restrict__ sorted,
                                                         const float *__restrict__ gbox, int N, int K,
                                                         KnnLadder lad, int32_t *__restrict__ nn,
                                                         float *__restrict__ dist, const int *__restrict__ gate) {
  if (gate && !gate[(size_t)blockIdx.y * kCellInts + kCellFlag]) return;  // (only the clouds the cell lists left)
  __shared__ __attribute__((aligned(16))) unsigned char s_lds[knn_split_lds_bytes<S>()];
  // (the group is rotated by the cloud: see knn_grid_kernel)
  const unsigned ng = (unsigned)((N + 63) / 64);
  knn_split_body<KMAX, S>(sorted, gbox, N, K, lad, nn, dist, blockIdx.y, (int)((blockIdx.x + 37u * blockIdx.y) % ng), s_lds);
}

// ------------------------------------------------------------------------------------------------
// Small clouds (N <= 2048: the N/8 sampled sets of the model).  The lane-per-query kernels above leave most of the
// chip idle there (B*N/64 waves, each a long dependent scan).  Here a WAVE owns a query: every lane holds
// CPL = N/64 candidates in registers (loaded once, reused for Q queries) and evaluates their squared distances s.
// The K nearest are the K smallest keys (bits(sqrt s) << 32 | tb); keys are unique (tb is).  Same keys, same order,
// same outputs as knn_kernel.
//
// K <= 8 -- the screened path.  Only candidates that can reach the K-list get a square root and a key:
//   U     = the largest of the eight minima of s over the lane groups 8g..8g+7 (all slots of a lane): eight disjoint
//           groups each hold a candidate with s <= U, so at least 8 >= K candidates do and the K-th nearest has
//           d_K <= sqrt(U) (sqrtf is correctly rounded, hence monotone).  A group without a valid candidate
//           (N < 57 or so) makes U = +inf, which screens nothing out.
//   keep  s <= U * 1.000001f.  The knn_inflated_sq margin: a relative 2^-20 in s is 2^-21 in d, more than 3 ulp, so
//           any s above the inflated bound has sqrt(s) > sqrt(U) >= d_K strictly and loses to K candidates whatever
//           its tb.  Two candidates with s1 < s2 but one rounded distance both stay, and tb orders them as the
//           reference does.  U = 0 (8 copies of the query) keeps exactly the copies.
//   Slots past N carry NaN coordinates: their s is a NaN, which no v_min picks and no `<=` admits, +inf bound or not.
//   The survivors are compacted to one per lane through a 64-entry LDS strip per wave (position = v_mbcnt of the
//   slot's ballot + a scalar running count), each lane takes ONE sqrtf and builds one key, and K rounds of the
//   two-step unsigned wave minimum pick the list; the winner retires its key.
//   Counted on uniform cubes (a numpy restatement, tests/test_knn_small_screen_gpu.py): 20-22 survivors per query on
//   average at N = 512, 1024 and 2048, the most over the test clouds 64; a larger sample at N = 2048 has 0.3 % of the
//   queries above 64.
// Otherwise -- K > 8, more than 64 survivors (lattices, duplicate-heavy clouds), or fewer than K survivors in a cloud of
// K or more (NaN distances) -- the wave takes knn_small_select_all for this query: every candidate's key, as before
// the screen.  The choice is wave-uniform and made per query.

// Every candidate's key; each lane caches its two smallest admissible keys (m1 < m2): a round is two wave minima and a
// pop in the winning lane, the per-lane scan over all CPL keys is redone only when some lane has used up both.
// s[] is overwritten with the distance bits.
template <int CPL>
__device__ __forceinline__ void knn_small_select_all(float (&s)[CPL], int N, int K, const KnnLadder &lad, int lane,
                                                     unsigned &my_hi, unsigned &my_lo) {
  // (the rank codes are rebuilt from an opaque copy of the lane id at every scan: as loop invariants of the query loop
  // they would be hoisted into CPL registers held across the screened path too)
  int ln = lane;
  asm volatile("" : "+v"(ln));
  unsigned kd[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) kd[c] = ln + 64 * c < N ? __float_as_uint(sqrtf(s[c])) : 0xFFFFFFFFu;
  u64 need = 0;  // smallest key still admissible
  u64 m1 = ~0ull, m2 = ~0ull;
  bool more = false;  // this lane may hold admissible keys beyond m2
  auto rescan = [&]() {
    m1 = ~0ull; m2 = ~0ull;
    int cnt = 0;
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int j = ln + 64 * c;
      const unsigned tb = j < N ? (unsigned)((j & lad.ctmask) * lad.cv + (j >> lad.log2ct)) : 0xFFFFFFFFu;
      const u64 key = ((u64)kd[c] << 32) | tb;
      const bool ok = key >= need && key != ~0ull;
      const bool c1 = ok && key < m1, c2 = ok && key < m2;
      m2 = c1 ? m1 : (c2 ? key : m2);
      m1 = c1 ? key : m1;
      cnt += ok ? 1 : 0;
    }
    more = cnt > 2;
  };
  rescan();
  for (int r = 0; r < K; ++r) {
    const unsigned hi = wave_min_u32((unsigned)(m1 >> 32));
    const unsigned lo = wave_min_u32((unsigned)(m1 >> 32) == hi ? (unsigned)m1 : 0xFFFFFFFFu);
    if (lane == r) { my_hi = hi; my_lo = lo; }
    const u64 sel = ((u64)hi << 32) | lo;
    if (sel == ~0ull) break;  // fewer than K points: the remaining slots keep the pad value
    need = sel + 1;
    const bool won = m1 == sel;
    const bool dry = won && m2 == ~0ull && more;  // both cached keys used, more behind them
    m1 = won ? m2 : m1;
    m2 = won ? ~0ull : m2;
    if (__ballot(dry) != 0ull) rescan();  // wave-uniform
  }
}

template <int CPL, bool XYZ>
__global__ __launch_bounds__(256) void knn_small_kernel(const float *__restrict__ pos, int N, int K, KnnLadder lad,
                                                       int32_t *__restrict__ nn, float *__restrict__ dist, int Q) {
  // Q: queries per wave (the candidates are loaded once per wave): 4, or 2 when that still leaves few waves per SIMD --
  // a query is K dependent rounds of two DPP reductions, the kernel is as long as one wave's queries
  __shared__ uint2 s_strip[4][64];  // per wave: (bits(s), id) of the survivors, 2 KiB a workgroup
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int q0 = (blockIdx.x * 4 + wave) * Q;
  if (q0 >= N) return;
  const float *base = pos + (size_t)b * N * 3;
  float cx[CPL], cy[CPL], cz[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    const int j = lane + 64 * c, jj = j < N ? j : 0;
    const float x = XYZ ? base[(size_t)jj * 3] : base[jj];
    cx[c] = j < N ? x : __builtin_nanf("");  // (one NaN coordinate makes the slot's s a NaN)
    cy[c] = XYZ ? base[(size_t)jj * 3 + 1] : base[(size_t)N + jj];
    cz[c] = XYZ ? base[(size_t)jj * 3 + 2] : base[(size_t)2 * N + jj];
  }
  uint2 *strip = s_strip[wave];
#pragma unroll 1
  for (int qi = 0; qi < Q; ++qi) {
    const int q = q0 + qi;
    if (q >= N) break;
    const float qx = XYZ ? base[(size_t)q * 3] : base[q];
    const float qy = XYZ ? base[(size_t)q * 3 + 1] : base[(size_t)N + q];
    const float qz = XYZ ? base[(size_t)q * 3 + 2] : base[(size_t)2 * N + q];
    float s[CPL];
    float smin = __builtin_inff();
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      // same roundings as knn_offer / the reference: sqrt(fma(dz,dz,fma(dy,dy,dx*dx))), :102-107
      const float dx = qx - cx[c], dy = qy - cy[c], dz = qz - cz[c];
      s[c] = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
      smin = fminf(smin, s[c]);  // (minnum: the NaN of an invalid slot is dropped)
    }
    unsigned my_hi = 0xFFFFFFFFu, my_lo = 0xFFFFFFFFu;  // lane r keeps result r
    bool screened = K <= 8;  // wave-uniform throughout
    int cnt = 0;
    if (screened) {
      const float ub = __fmul_rn(wave_max_of_min8_f32(smin), 1.000001f);
      // (an opaque copy of the lane id: the ids lane + 64 c are query-loop invariants, and hoisted they hold CPL registers)
      int ln = lane;
      asm volatile("" : "+v"(ln));
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const bool in = s[c] <= ub;
        const u64 mk = __ballot(in);
        const int at0 = cnt;
        cnt += __popcll(mk);  // scalar; once past 64 it stays there and nothing more is written: the strip holds 64
        if (in && cnt <= 64) {
          const unsigned at = __builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
          (strip + at0)[at] = make_uint2(__float_as_uint(s[c]), (unsigned)(ln + 64 * c));
        }
      }
      screened = cnt <= 64 && (cnt >= K || cnt >= N);  // (only NaN distances can leave fewer than K of N >= K)
    }
    if (screened) {
      // the strip is wave-private and LDS operations of a wave complete in order: the fences only pin the compiler
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const uint2 e = strip[lane];  // (lanes >= cnt read a stale entry and drop it)
      const float d = sqrtf(__uint_as_float(e.x));
      const int j = (int)e.y;
      unsigned khi = lane < cnt ? __float_as_uint(d) : 0xFFFFFFFFu;
      unsigned klo = lane < cnt ? (unsigned)((j & lad.ctmask) * lad.cv + (j >> lad.log2ct)) : 0xFFFFFFFFu;
      for (int r = 0; r < K; ++r) {
        const unsigned hi = wave_min_u32(khi);
        const unsigned lo = wave_min_u32(khi == hi ? klo : 0xFFFFFFFFu);
        if (lane == r) { my_hi = hi; my_lo = lo; }
        if ((hi & lo) == 0xFFFFFFFFu) break;  // fewer than K points: the remaining slots keep the pad value
        const bool won = khi == hi && klo == lo;
        khi = won ? 0xFFFFFFFFu : khi;
        klo = won ? 0xFFFFFFFFu : klo;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (the next query's writes stay behind this read)
    } else {
      knn_small_select_all<CPL>(s, N, K, lad, lane, my_hi, my_lo);
    }
    if (lane < K) {
      const size_t o = ((size_t)b * N + q) * K + lane;
      knn_emit(((u64)my_hi << 32) | my_lo, lad, nn + o, dist + o);
    }
  }
}

// What every kNN entry of this file takes beyond positive sizes: the K-lists hold 64 keys, a cloud is a grid row.
constexpr int kKnnMaxK = 64, kKnnMaxB = 65535;

// The K-list width (KMAX) of the lane-per-query kernels: knn_kernel here, knn_sorted_kernel below.
static int knn_list_width(int K) { return K <= 4 ? 4 : K <= 8 ? 8 : K <= 16 ? 16 : K <= 32 ? 32 : 64; }

// The launch plan of dh3d_knn_bruteforce (Dp = 3) and dh3d_knn_bruteforce_xyz -- the one place knn_launch's thresholds
// live (knn_launch runs it, dh3d_knn_bruteforce_plan reports it).
//   cpl > 0: knn_small_kernel<cpl> (a wave per query, 64 * cpl >= N candidates in registers), q queries per wave;
//   cpl = 0: knn_kernel<kmax> (a lane per query).
struct KnnPlan {
  int cpl, q, kmax;
};
static KnnPlan knn_plan(int B, int N, int K) {
  KnnPlan p{0, 0, 0};
  if (N <= 2048) {
    p.cpl = N <= 512 ? 8 : N <= 1024 ? 16 : 32;
    p.q = (long long)B * N <= 16384 ? 2 : 4;  // <= 4 waves per SIMD with two queries per wave
    return p;
  }
  p.kmax = knn_list_width(K);
  return p;
}

// The K-list width of knn_anydp_kernel (Dp != 3, up to the 16 coordinates its staging tile holds).
constexpr int kAnyDpMax = 16;
static int knn_anydp_width(int K) { return K <= 8 ? 8 : K <= 16 ? 16 : 64; }

template <bool XYZ>
int knn_launch(const float *pos, int B, int N, int K, int32_t *nn, float *dist, hipStream_t s) {
  const KnnLadder lad = knn_ladder(N);
  const KnnPlan p = knn_plan(B, N, K);
  if (p.cpl > 0) {  // wave-per-query kernel
    dim3 sgrid(dh3d_cdiv(N, 4 * p.q), B), sblock(256);
#define DH3D_SMALL_CASE(CPL)                                                                                     \
  if (p.cpl == CPL) {                                                                                            \
    hipLaunchKernelGGL((knn_small_kernel<CPL, XYZ>), sgrid, sblock, 0, s, pos, N, K, lad, nn, dist, p.q);        \
    return dh3d_launch_status();                                                                                 \
  }
    DH3D_SMALL_CASE(8) DH3D_SMALL_CASE(16) DH3D_SMALL_CASE(32)
#undef DH3D_SMALL_CASE
    return DH3D_ERR_UNSUPPORTED;  // (a plan without a kernel)
  }
  dim3 grid(dh3d_cdiv(N, kQueriesPerBlock), B), block(kQueriesPerBlock);
#define DH3D_LANE_CASE(KM)                                                                                       \
  if (p.kmax == KM) {                                                                                            \
    hipLaunchKernelGGL((knn_kernel<KM, XYZ>), grid, block, 0, s, pos, N, K, lad, nn, dist);                      \
    return dh3d_launch_status();                                                                                 \
  }
  DH3D_LANE_CASE(4) DH3D_LANE_CASE(8) DH3D_LANE_CASE(16) DH3D_LANE_CASE(32) DH3D_LANE_CASE(64)
#undef DH3D_LANE_CASE
  return DH3D_ERR_UNSUPPORTED;
}

// Any position dimension (the reference loops over Dp, knn_bruteforce_kernel_gpu.cu.cc:98-107; DH3D itself only ever
// passes xyz).  The coverage path: lane = query, candidates staged 256 at a time through LDS ([Dp][256], Dp <= 16), the
// same roundings -- sum = fma(val, val, sum) in dimension order from 0, IEEE sqrt -- and the same (distance, CUB rank)
// order, kept as a sorted list of 64-bit keys per lane (insertion; in scratch for large K).  Unfilled slots (N < K):
// id -1, distance FLT_MAX (:110-111).
template <int KMAX>
__global__ __launch_bounds__(256) void knn_anydp_kernel(const float *__restrict__ pos, int Dp, int N, int K, KnnLadder lad,
                                                        int32_t *__restrict__ nn, float *__restrict__ dist) {
  __shared__ float s_c[16][256];
  const int b = blockIdx.y, y = blockIdx.x * 256 + threadIdx.x;
  const float *pc = pos + (size_t)b * Dp * N;
  float q[16];
#pragma unroll
  for (int dp = 0; dp < 16; ++dp) q[dp] = (dp < Dp && y < N) ? pc[(size_t)dp * N + y] : 0.f;
  u64 keys[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i) keys[i] = kKnnNoKey;
  for (int x0 = 0; x0 < N; x0 += 256) {
    __syncthreads();
    for (int dp = 0; dp < Dp; ++dp) s_c[dp][threadIdx.x] = x0 + (int)threadIdx.x < N ? pc[(size_t)dp * N + x0 + threadIdx.x] : 0.f;
    __syncthreads();
    const int cnt = min(256, N - x0);
    for (int j = 0; j < cnt; ++j) {
      float sum = 0.f;
      for (int dp = 0; dp < Dp; ++dp) {
        const float val = s_c[dp][j] - q[dp];
        sum = __builtin_fmaf(val, val, sum);
      }
      const float d = sqrtf(sum);
      const int x = x0 + j;
      const unsigned tb = (unsigned)((x & lad.ctmask) * lad.cv + (x >> lad.log2ct));
      const u64 key = ((u64)__float_as_uint(d) << 32) | tb;
      if (key < keys[K - 1]) {
        int i = K - 1;
        while (i > 0 && keys[i - 1] > key) { keys[i] = keys[i - 1]; --i; }
        keys[i] = key;
      }
    }
  }
  if (y >= N) return;
  int32_t *o_nn = nn + ((size_t)b * N + y) * K;
  float *o_d = dist + ((size_t)b * N + y) * K;
  for (int i = 0; i < K; ++i) knn_emit(keys[i], lad, o_nn + i, o_d + i);
}

}  // namespace

DH3D_API int dh3d_knn_bruteforce(const float *positions, int B, int Dp, int N, int K, int32_t *nn,
                                 float *dist, void *stream) {
  DH3D_REQUIRE(positions && nn && dist && B > 0 && N > 0 && K > 0 && Dp > 0);
  DH3D_SUPPORTED(K <= kKnnMaxK && B <= kKnnMaxB);
  if (Dp == 3) return knn_launch<false>(positions, B, N, K, nn, dist, (hipStream_t)stream);
  DH3D_SUPPORTED(Dp <= kAnyDpMax);  // (any Dp upstream; the staging tile here holds 16 coordinates)
  const KnnLadder lad = knn_ladder(N);
  dim3 grid(dh3d_cdiv(N, 256), B), block(256);
  hipStream_t s = (hipStream_t)stream;
  const int km = knn_anydp_width(K);
#define DH3D_ANYDP_CASE(KM)                                                                                      \
  if (km == KM) {                                                                                                \
    hipLaunchKernelGGL(knn_anydp_kernel<KM>, grid, block, 0, s, positions, Dp, N, K, lad, nn, dist);             \
    return dh3d_launch_status();                                                                                 \
  }
  DH3D_ANYDP_CASE(8) DH3D_ANYDP_CASE(16) DH3D_ANYDP_CASE(64)
#undef DH3D_ANYDP_CASE
  return DH3D_ERR_UNSUPPORTED;  // (a width without a kernel)
}

DH3D_API int dh3d_knn_bruteforce_xyz(const float *xyz, int B, int N, int K, int32_t *nn, float *dist,
                                     void *stream) {
  DH3D_REQUIRE(xyz && nn && dist && B > 0 && N > 0 && K > 0);
  DH3D_SUPPORTED(K <= kKnnMaxK && B <= kKnnMaxB);
  return knn_launch<true>(xyz, B, N, K, nn, dist, (hipStream_t)stream);
}

// The kernel dh3d_knn_bruteforce runs for [B, Dp, N] positions and K neighbours (dh3d_knn_bruteforce_xyz: Dp = 3), from
// the launchers' own functions; host only.  family * 65536 + a * 256 + b, or -1 where the entry refuses the shape:
//   family 1, a = CPL (8 / 16 / 32), b = Q (2 / 4): knn_small_kernel<CPL>, Q queries per wave   (Dp = 3, N <= 2048)
//   family 2, a = 0, b = KMAX (4 .. 64):            knn_kernel<KMAX>                            (Dp = 3, N > 2048)
//   family 3, a = 0, b = KMAX (8 / 16 / 64):        knn_anydp_kernel<KMAX>                      (Dp != 3, Dp <= 16)
DH3D_API int dh3d_knn_bruteforce_plan(int B, int Dp, int N, int K) {
  if (!(B > 0 && N > 0 && K > 0 && Dp > 0) || !(K <= kKnnMaxK && B <= kKnnMaxB)) return -1;
  if (Dp != 3) return Dp <= kAnyDpMax ? 3 * 65536 + knn_anydp_width(K) : -1;
  const KnnPlan p = knn_plan(B, N, K);
  return p.cpl > 0 ? 1 * 65536 + p.cpl * 256 + p.q : 2 * 65536 + p.kmax;
}

// The launch plan of dh3d_knn_sorted (and of dh3d_knn_grid's gated second launch) -- the one place knn_sorted_launch's
// thresholds live (knn_sorted_launch runs it, dh3d_knn_sorted_plan reports it).
//   s: waves per query group, knn_split_kernel<kmax, s>; 0 = the one-wave kernel, knn_sorted_kernel<kmax>.
struct KnnSortedPlan {
  int s, kmax;
};
static KnnSortedPlan knn_sorted_plan(int B, int N, int K) {
  // waves per query group: as many as keep the chip at <= ~4 waves per SIMD, where the search turns from latency- to
  // issue-bound (MI355X: 8x8192 0.194 -> 0.109 ms at 4; 32x4096 0.178 -> 0.147 at 2)
  const long long groups = (long long)((N + 63) / 64) * B;
  KnnSortedPlan p{groups <= 256 ? 8 : groups <= 1280 ? 4 : groups <= 4096 ? 2 : 0, knn_list_width(K)};
  if (p.kmax > 16) p.s = 0;                 // the split kernels keep lists of up to 16
  if (p.s == 8 && p.kmax == 4) p.kmax = 8;  // (no <4, 8> instantiation: K <= 4 runs the width-8 kernel there)
  return p;
}

static int knn_sorted_launch(const float *sorted, const float *gbox, int B, int N, int K, int32_t *nn, float *dist,
                             const int *gate, void *stream) {
  DH3D_REQUIRE(sorted && gbox && nn && dist && B > 0 && N > 0 && K > 0);
  DH3D_SUPPORTED(K <= kKnnMaxK && B <= kKnnMaxB);
  const KnnLadder lad = knn_ladder(N);
  const int NG = (N + 63) / 64;
  dim3 grid(dh3d_cdiv(NG, kSortedWaves), B), block(64 * kSortedWaves);
  hipStream_t s = (hipStream_t)stream;
  const float4 *so = reinterpret_cast<const float4 *>(sorted);
  const KnnSortedPlan p = knn_sorted_plan(B, N, K);
  if (p.s > 0) {
    dim3 sgrid(NG, B);
#define DH3D_SPLIT_CASE(KM, SS)                                                                               \
  if (p.kmax == KM && p.s == SS) {                                                                           \
    hipLaunchKernelGGL((knn_split_kernel<KM, SS>), sgrid, dim3(64 * SS), 0, s, so, gbox, N, K, lad, nn, dist, gate); \
    return dh3d_launch_status();                                                                             \
  }
    DH3D_SPLIT_CASE(4, 2) DH3D_SPLIT_CASE(4, 4)
    DH3D_SPLIT_CASE(8, 2) DH3D_SPLIT_CASE(8, 4) DH3D_SPLIT_CASE(8, 8)
    DH3D_SPLIT_CASE(16, 2) DH3D_SPLIT_CASE(16, 4) DH3D_SPLIT_CASE(16, 8)
#undef DH3D_SPLIT_CASE
    return DH3D_ERR_UNSUPPORTED;  // (a plan without a kernel)
  }
#define DH3D_SORTED_CASE(KM)                                                                                  \
  if (p.kmax == KM) {                                                                                        \
    hipLaunchKernelGGL((knn_sorted_kernel<KM>), grid, block, 0, s, so, gbox, N, K, lad, nn, dist, gate);      \
    return dh3d_launch_status();                                                                             \
  }
  DH3D_SORTED_CASE(4) DH3D_SORTED_CASE(8) DH3D_SORTED_CASE(16) DH3D_SORTED_CASE(32) DH3D_SORTED_CASE(64)
#undef DH3D_SORTED_CASE
  return DH3D_ERR_UNSUPPORTED;
}

DH3D_API int dh3d_knn_sorted(const float *sorted, const float *gbox, int B, int N, int K, int32_t *nn,
                             float *dist, void *stream) {
  return knn_sorted_launch(sorted, gbox, B, N, K, nn, dist, nullptr, stream);
}

// The kernel dh3d_knn_sorted launches for (B, N, K), from the launcher's own function; host only.  S * 256 + KMAX, or -1
// where dh3d_knn_sorted refuses the shape.  S = 8 / 4 / 2: knn_split_kernel<KMAX, S>, S waves per 64-query group
// (KMAX 4 / 8 / 16; 8 / 16 at S = 8); S = 0: knn_sorted_kernel<KMAX>, one wave per group (KMAX 4 .. 64).
DH3D_API int dh3d_knn_sorted_plan(int B, int N, int K) {
  if (!(B > 0 && N > 0 && K > 0) || !(K <= kKnnMaxK && B <= kKnnMaxB)) return -1;
  const KnnSortedPlan p = knn_sorted_plan(B, N, K);
  return p.s * 256 + p.kmax;
}

// ------------------------------------------------------------------------------------------------ cell-list kNN
// The same operator on the grid spatial_sort_kernel lays over a cloud's bounding box (the top 12 bits of the sort key,
// dealt to the axes by extent: 16 x 16 x 16 on a cube, 32 x 32 x 4 on a street scene -- every grid cell is ONE contiguous
// range of the sorted records, cells[] holds the ranges).  Where the pruned scan above shares a candidate stream between 64 queries -- the union of their search balls,
// ~1800 candidates per query at 8 x 8192 -- this one gives every query its own cells.  L lanes per query, two passes:
//   (0) the 27 cells around the query's cell;
//   (1) every other cell of the BOX the ball of the K-th distance seen so far meets (its own radius per axis), skipping a
//       cell whose box lies beyond that distance.
// Each pass pools the surviving cells' records per query in LDS, the query's lanes then take the pooled candidates L apart
// into their own sorted K-lists, and the lists are merged with log2(L) bitonic exchange steps.  Exact after pass 1: the K
// nearest neighbours all lie within the K-th distance seen after pass 0, i.e. inside the box, and a skipped cell provably
// holds nothing closer (conservative box distance, ties included).  What the box pass cannot serve (no K-th distance after
// 27 cells nor within the +-2 block, a box of more than kGridBoxCells cells, a pass-1 pool past kGridCap) restarts over the sort's 64-point group boxes; clouds
// whose points crowd into few cells (the sort's verdict, cells[kCellFlag]) are left to the pruned scan (dh3d_knn_grid).
// Same distances (reference rounding order, IEEE sqrt) and the same 64-bit (distance, CUB rank) order as every other
// kernel of this file: ids and distance bits are identical.
constexpr int kGridCap = 256;    // pooled candidates per query and pass (knn_grid_kernel)
// A query's row of the pool in LDS, in 16-bit entries: kGridCap and one dword more.  At 128 dwords the rows of the eight
// queries that share a 32-lane half start on one bank, and every drain access (slot i of each) is an 8-way conflict; at 129
// consecutive queries sit on consecutive banks.
constexpr int kGridRow = kGridCap + 2;
// Pass 0's screened drain takes pools up to this size: the query's 512-byte row then holds 80 record indices (bytes 0..159,
// replaced by the 16-bit ids as they are read) and behind them the 80 squared distances (bytes 160..479).  A multiple of
// 4 x 4 lanes: a padded trip stays inside the row.  (Pools of a uniform 8192-point cube: 48 on average, 77 at most.)
constexpr int kGridScreenCap = 80;
static_assert(kGridScreenCap % 16 == 0 && kGridScreenCap * 6 <= kGridCap * 2, "the screened drain's row");
// Pass 1 serves a query whose box -- the cells the ball of its K-th distance meets, clipped to the grid -- has at most
// this many cells (the 5 x 128 columns of the first versions); a wider ball goes to the group-box restart.  It also
// bounds the operands of knn_small_div below.
constexpr int kGridBoxCells = 640;

// What a lane that looks at a cell of ANOTHER query's box needs of that query (pass 1 deals the cells of a wave's sixteen
// queries over all its lanes): two 16-byte LDS reads.
struct alignas(16) KnnBoxRec {
  float4 qb;  // the query's x y z, its bound
  int4 box;   // x: the query's cell, a byte per axis; y, z: its box as offsets from that cell, a byte per axis: -lo, hi
              // (lo <= 0 <= hi); w: the query's first place in the wave's list of cells
};
__device__ __forceinline__ int knn_pack3(int x, int y, int z) { return x | (y << 8) | (z << 16); }
__device__ __forceinline__ int knn_byte(int v, int a) { return (v >> (8 * a)) & 0xFF; }

// t / d for 0 <= t < kGridBoxCells, 1 <= d <= kGridBoxCells without an integer division: m = 2^20 / d rounded up by at
// most 2.125 (v_rcp_f32 is within one ulp: 2^20 / d is off by less than 1 / 8, the conversion truncates, + 2), so
// d * m = 2^20 + e with 0 < e <= 2.125 d, and t * m >> 20 == t / d as long as t * e < 2^20.
static_assert(2.125 * kGridBoxCells * kGridBoxCells < (1 << 20), "knn_small_div");
__device__ __forceinline__ int knn_small_div(int t, int d) {
  const unsigned m = (unsigned)(1048576.f * __builtin_amdgcn_rcpf((float)d)) + 2u;
  return (int)(((unsigned)t * m) >> 20);
}

// The cells of the box [lo, hi] (offsets from the query's cell, lo <= 0 <= hi on every axis) that pass 0 has not served:
// the box without its inner block [max(lo, -1), min(hi, 1)]^3, as three groups of slabs that are walked one after the other,
//   z: the whole x y extent at the z offsets outside the inner block,   bx * by * oz cells, x fastest, then y;
//   y: the whole x extent, the inner z, the y offsets outside,          bx * iz * oy,       x fastest, then z;
//   x: the inner y and z, the x offsets outside,                        iy * iz * ox,       y fastest, then z.
// An offset outside counts up from lo to the inner block and goes on behind it.  Returns the number of cells and, for
// 0 <= t < that <= kGridBoxCells, the offsets of cell t: one definition for the count a query publishes and the place a
// lane decodes.  (Scalars, selected by value: a select between members of a struct or an array becomes an indexed load,
// and the aggregate goes to scratch memory.)
__device__ __forceinline__ int knn_box_shell(int lo0, int lo1, int lo2, int hi0, int hi1, int hi2, int t, int &dx, int &dy, int &dz) {
  const int in00 = max(lo0, -1), in01 = max(lo1, -1), in02 = max(lo2, -1);  // the inner block's first offsets
  const int in10 = min(hi0, 1), in11 = min(hi1, 1), in12 = min(hi2, 1);     // and its last
  const int b0 = hi0 - lo0 + 1, b1 = hi1 - lo1 + 1, b2 = hi2 - lo2 + 1;
  const int i0 = in10 - in00 + 1, i1 = in11 - in01 + 1, i2 = in12 - in02 + 1;
  const int nz = b0 * b1 * (b2 - i2), ny = b0 * i2 * (b1 - i1), nx = i1 * i2 * (b0 - i0);
  const int g = t < nz ? 0 : t < nz + ny ? 1 : 2;  // the group; its slabs lie along axis 2 - g
  t -= g == 0 ? 0 : g == 1 ? nz : nz + ny;
  const int d1 = g == 2 ? i1 : b0, d2 = g == 0 ? b1 : i2;
  const int u = knn_small_div(t, d1), f = t - u * d1;
  const int k = knn_small_div(u, d2), s = u - k * d2;
  const int slo = g == 0 ? lo2 : g == 1 ? lo1 : lo0;
  const int sin0 = g == 0 ? in02 : g == 1 ? in01 : in00;
  const int sin1 = g == 0 ? in12 : g == 1 ? in11 : in10;
  const int v = k < sin0 - slo ? slo + k : sin1 + 1 + (k - (sin0 - slo));
  dx = g == 2 ? v : lo0 + f;
  dy = g == 2 ? in01 + f : g == 1 ? v : lo1 + s;
  dz = g == 0 ? v : in02 + s;
  return nz + ny + nx;
}

__device__ __forceinline__ unsigned knn_spread4(unsigned v) {  // 4 bits -> every third bit (the sort's spread6 >> 6)
  return (v & 1u) | ((v & 2u) << 2) | ((v & 4u) << 4) | ((v & 8u) << 6);
}
__device__ __forceinline__ void knn_cswap(u64 &a, u64 &b) {
  const bool lt = b < a;
  const u64 lo = lt ? b : a, hi = lt ? a : b;
  a = lo; b = hi;
}
// the L lanes of a query end up with the same list: the 8 smallest keys of all their lists.  log2(L) exchange steps on
// the DPP crossbar (no LDS round trip): partner = lane ^ 1, lane ^ 2 (quad permutes), then (L = 8) 7 - lane within the
// eight (row_half_mirror: every lane meets one of the other quad, whose four lanes already agree).
template <int CTRL>
__device__ __forceinline__ u64 knn_dpp_u64(u64 v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)v, CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, true);
  return ((u64)(unsigned)hi << 32) | (unsigned)lo;
}
template <int CTRL>
__device__ __forceinline__ int knn_dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ void knn_merge_step(KnnState<8> &st) {
  u64 c[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const u64 mine = st.keys[i], theirs = knn_dpp_u64<CTRL>(st.keys[7 - i]);
    c[i] = mine < theirs ? mine : theirs;  // ascending list against the partner's descending one: the 8 smallest, bitonic
  }
  knn_cswap(c[0], c[4]); knn_cswap(c[1], c[5]); knn_cswap(c[2], c[6]); knn_cswap(c[3], c[7]);
  knn_cswap(c[0], c[2]); knn_cswap(c[1], c[3]); knn_cswap(c[4], c[6]); knn_cswap(c[5], c[7]);
  knn_cswap(c[0], c[1]); knn_cswap(c[2], c[3]); knn_cswap(c[4], c[5]); knn_cswap(c[6], c[7]);
#pragma unroll
  for (int i = 0; i < 8; ++i) st.keys[i] = c[i];
}
__device__ __forceinline__ void knn_bound_of_list(KnnState<8> &st) {
  knn_inflated_sq((unsigned)(st.keys[7] >> 32), st.bound);
}
template <int L>
__device__ __forceinline__ void knn_merge_sublanes(KnnState<8> &st) {
  if (L >= 2) knn_merge_step<0xB1>(st);   // quad_perm [1,0,3,2]
  if (L >= 4) knn_merge_step<0x4E>(st);   // quad_perm [2,3,0,1]
  if (L >= 8) knn_merge_step<0x141>(st);  // row_half_mirror
  knn_bound_of_list(st);
}
// The merge of a query whose lanes 1..L-1 started a pass with empty lists (keep_one_copy) and took nothing in it: lane 0's
// list IS the merged one (its own insertions included), so the others copy it -- 16 permutes instead of two exchange
// steps.  The same lists and the same bound as knn_merge_sublanes.  The choice is the wave's: one lane that took an entry
// sends all of it through the merge.
template <int L>
__device__ __forceinline__ void knn_merge_after_sparse_pass(KnnState<8> &st, int sub) {
  if (L != 4 || __any(sub != 0 && st.keys[0] != kKnnNoKey)) {
    knn_merge_sublanes<L>(st);
    return;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) st.keys[i] = knn_dpp_u64<0x00>(st.keys[i]);  // quad_perm [0,0,0,0]
  knn_bound_of_list(st);
}

// L = lanes per query (2, 4 or 8): fewer lanes = longer private candidate streams, but an insertion round serves 64 / L
// queries and the merge has log2(L) steps.
// SF > 0 (L = 4: a workgroup is 64 queries, as in the pruned scan): a cloud the sort flagged as crowded is served HERE by
// the pruned scan with SF waves per query group (knn_split_body on the same LDS block) -- one launch for both kinds of
// cloud; SF = 0: such clouds are left to a second launch (dh3d_knn_grid).
template <int L, int SF>
__global__ __launch_bounds__(256) void knn_grid_kernel(const float4 *__restrict__ sorted, const float *__restrict__ gbox,
                                                      const int *__restrict__ cells, int N, int K, int D, KnnLadder lad,
                                                      int32_t *__restrict__ nn, float *__restrict__ dist) {
  constexpr int QB = 256 / L;  // queries per workgroup
  static_assert(SF == 0 || (L == 4 && SF <= 4), "the merged scan: 64 queries per workgroup, at most four waves");
  constexpr int QW = 64 / L;   // queries per wave
  constexpr int kGridRecAt = 3 * 64 * 4 + QB * kGridRow * 2 + QB * 4;  // the deposit tables, the pool rows, their counts
  constexpr int kGridLds = kGridRecAt + QB * (int)sizeof(KnnBoxRec);   // and pass 1's per-query records
  static_assert(kGridRecAt % 16 == 0 && (L != 4 || kGridLds <= 40 * 1024), "16-byte records; four workgroups per CU");
  constexpr int kSplitLds = SF == 2 ? 2 * knn_split_lds_bytes<2>() : SF > 0 ? knn_split_lds_bytes<(SF > 0 ? SF : 1)>() : 0;
  __shared__ __attribute__((aligned(16))) unsigned char s_raw[kGridLds > kSplitLds ? kGridLds : kSplitLds];
  const int b = blockIdx.y, lane = threadIdx.x & 63, sub = lane & (L - 1);
  if (cells[(size_t)b * kCellInts + kCellFlag]) {  // dense cells: the pruned scan takes this cloud
    if constexpr (SF > 0) {
      // (the group a workgroup serves is rotated by the cloud: workgroups x, x + 256, ... share a CU, and with clouds of one
      //  kind in a batch -- the same street, the same sensor -- the same x is the same kind of region in all of them: the
      //  slow far-field groups of every cloud would meet on the same CUs)
      const int ngq = (N + 63) / 64;
      if constexpr (SF == 2) {
        // TWO query groups per workgroup, two waves each (half the workgroups of a crowded cloud leave at once): a CU then
        // carries eight groups instead of four, and the launch ends with its most loaded CU
        const int half = (int)(threadIdx.x >> 7), pairs = (ngq + 1) / 2;
        if ((int)blockIdx.x >= pairs) return;
        const int g0 = (int)blockIdx.x + half * pairs;
        if (g0 >= ngq) return;
        knn_split_body<8, 2>(sorted, gbox, N, K, lad, nn, dist, b, (int)(((unsigned)g0 + 37u * (unsigned)b) % (unsigned)ngq),
                             s_raw + half * knn_split_lds_bytes<2>(), half * 2);
      } else if (threadIdx.x < 64 * SF) {
        knn_split_body<8, (SF > 0 ? SF : 1)>(sorted, gbox, N, K, lad, nn, dist, b, (int)((blockIdx.x + 37u * (unsigned)b) % (unsigned)ngq), s_raw);
      }
    }
    return;
  }
  // (the cell lists too: a query group's work depends on where it sits in the Morton order -- the cloud's border, the big
  //  jumps of the curve -- which is the same place in every cloud of a batch: rotated by the cloud like the scan's)
  const int qi = (int)((blockIdx.x + 37u * (unsigned)b) % gridDim.x) * QB + threadIdx.x / L;
  const bool valid = qi < N;
  const float4 *sc = sorted + (size_t)b * N;
  const CellGrid g = cell_grid(cells, b);
  const int *ct = g.ct;
  // (copies: indexed by a per-thread axis below, which on the struct's members would put them in scratch memory)
  const float lo[3] = {g.lo[0], g.lo[1], g.lo[2]}, scl[3] = {g.scl[0], g.scl[1], g.scl[2]};
  const int nb[3] = {g.nb[0], g.nb[1], g.nb[2]};
  const float4 qr = sc[valid ? qi : N - 1];
  const float q[3] = {qr.x, qr.y, qr.z};
  // The grid: the sort dealt the cell code's 12 bits to the axes by extent (spatial.hip: `sched`, step 0 = the top bit;
  // a cube: z y x z y x ... = 16 x 16 x 16).  D = low bits of the code left out: a coarser grid whose cells are still
  // contiguous ranges of the order -- 2^D consecutive cells of the table.
  int nc[3], drop[3];  // bits per axis of the coarser grid | of the D steps left out
  sched_bits(g.sched, nc, kGridSteps - D);
#pragma unroll
  for (int a = 0; a < 3; ++a) drop[a] = nb[a] - nc[a];
  const int span = 1 << D;
  int cq[3], gmax[3];
  float w[3], eps[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    // (= grid_cell(g, a, q[a]) >> drop[a]: q is a point of the cloud, so the product is finite and below the float clamp)
    cq[a] = min((4 << nb[a]) - 1, max(0, (int)((q[a] - lo[a]) * scl[a]))) >> (2 + drop[a]);
    gmax[a] = ((1 << nb[a]) >> drop[a]) - 1;
    w[a] = (float)(4 << drop[a]) / scl[a];  // cell width
    eps[a] = 2.5e-6f * ((float)(4 << nb[a]) / scl[a]);  // a point may sit outside its cell's nominal interval by a few ulps of the extent
  }
  // the table index of cell (ax, ay, az): every axis' cell number with its bits at their places in the code (per
  // workgroup, in LDS: 64 entries per axis)
  unsigned (*s_ctab)[64] = reinterpret_cast<unsigned (*)[64]>(s_raw);   // [3][64]
  cell_deposit_tables(g.sched, nc[0], nc[1], nc[2], kGridSteps - D, s_ctab);
  auto tab_code = [&](int ax, int ay, int az) { return s_ctab[0][ax & 63] | s_ctab[1][ay & 63] | s_ctab[2][az & 63]; };
  KnnState<8> st;
  knn_list_reset(st);
  if (!valid) st.bound = -1.f;  // (takes nothing)

  // conservative squared distance from the query to cells cq[a] + o along one axis (0 inside the cell's own slab)
  // (cell_d2: from coordinate qa of any query of the cloud to cell c of axis a)
  auto cell_d2 = [&](int a, float qa, int c) __attribute__((always_inline)) {
    const float l = lo[a] + (float)c * w[a];
    const float d = fmaxf(fmaxf(fmaxf(l - qa, qa - (l + w[a])), 0.f) - eps[a], 0.f);
    return d * d;
  };
  auto axis_d2 = [&](int a, int o) __attribute__((always_inline)) { return cell_d2(a, q[a], cq[a] + o); };
  // the 3 x 3 x 3 block of pass 0: everything that depends on the x offset alone is computed once (three slabs: distance,
  // cell bits, inside the grid or not); a lane then walks (dy, dz) columns and, per column, the three x offsets with constants
  float d2x[3];
  unsigned bitx[3];
  bool okx[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int ax = cq[0] + t - 1;
    okx[t] = (unsigned)ax <= (unsigned)gmax[0];
    d2x[t] = okx[t] ? axis_d2(0, t - 1) : INFINITY;
    bitx[t] = s_ctab[0][ax & 63];
  }
  // is the K-th distance strictly inside the block of radius R around the query's cell?  (faces on the grid's border
  // have nothing behind them)
  auto inside = [&](int R) {
    float G = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (cq[a] - R > 0) G = fminf(G, (q[a] - (lo[a] + (float)(cq[a] - R) * w[a])) - eps[a]);
      if (cq[a] + R < gmax[a]) G = fminf(G, ((lo[a] + (float)(cq[a] + R + 1) * w[a]) - q[a]) - eps[a]);
    }
    if (G == INFINITY) return true;
    G = fmaxf(G, 0.f);
    return st.bound < G * G * 0.99999f;  // bound = the (1 + 2^-20)-inflated square of the K-th distance, inf while the list is short
  };

  // Cells hold 0..~8 points: walking them cell by cell leaves most lanes of the wave idle in every iteration (and the
  // ~45-instruction insertion runs for the whole wave whenever one lane inserts).  So a pass first POOLS: every lane
  // appends the record indices of its surviving cells to its query's list in LDS (one LDS atomic per cell for the
  // place), then the query's lanes take the pooled candidates L apart, four per lane in flight -- every lane busy in
  // every iteration, ~5x fewer iterations of the candidate loop.  The result does not depend on who scans what (keys
  // are unique, the merge sorts).  A list that is full (dense clusters) sends the rest of the cell down the direct path.
  // After a merge all L lanes hold the SAME list: before they scan on, all but one empty theirs (the bound stays), or the
  // next merge would count every entry L times
  auto keep_one_copy = [&]() {
    if (sub != 0) knn_list_clear(st);
  };
  unsigned short (*s_list)[kGridRow] = reinterpret_cast<unsigned short (*)[kGridRow]>(s_raw + 3 * 64 * 4);   // [QB][kGridRow]
  int *s_cnt = reinterpret_cast<int *>(s_raw + 3 * 64 * 4 + QB * kGridRow * 2);                                // [QB]
  const int qs = threadIdx.x / L;
  auto direct = [&](int j) {
    const float4 r = sc[j];
    const float dx = r.x - q[0], dy = r.y - q[1], dz = r.z - q[2];
    knn_offer<8, false>(st, fmaf(dz, dz, fmaf(dy, dy, dx * dx)), __float_as_int(r.w), lad);
  };
  auto enqueue = [&](int beg, int end) {
    const int len = end - beg;
    if (len <= 0) return;
    const int off = atomicAdd(&s_cnt[qs], len);
    const int fit = min(len, kGridCap - off);
    for (int k = 0; k < fit; ++k) s_list[qs][off + k] = (unsigned short)(beg + k);
    for (int k = max(fit, 0); k < len; ++k) direct(beg + k);
  };
  // (wave_lds_sync below: a row is wave-private and a wave's LDS operations complete in order: it pins the compiler)
  // Pass 0's pool is ~48 candidates of which 8 are wanted, the list is empty and the bound infinite: offered one by one,
  // every slot pays the square root, the rank code and the insertion (some lane of the wave always inserts).  So the pool
  // is SCREENED first, on squared distances alone (the rule written out above knn_small_kernel):
  //   sweep 1  every lane walks its share (records L apart, four loads in flight), keeps its two smallest s, m1 <= m2
  //            (v_min semantics: a NaN never enters them), and leaves (s, 16-bit id) in the row -- the id over the record
  //            index it has just read, s behind the indices;
  //   U        = the largest m2 of the query's L lanes (two quad permutes): every lane saw two candidates, so at least
  //            2 L >= 8 >= K candidates have s <= U and the K-th distance is at most sqrt(U).  thr = U * (1 + 2^-20):
  //            anything above it has a strictly larger rounded distance than K others, whatever its rank code; equal
  //            rounded distances from different s both stay and the rank orders them; U = 0 keeps exactly the copies.
  //            A lane with fewer than two finite s (NaN coordinates) makes U = thr = +inf: everything is ranked, as before;
  //   sweep 2  the survivors (s <= thr) are compacted IN PLACE, sixteen slots of the row per trip: a lane's place is the
  //            query's count so far + a prefix over the quad (DPP, no atomic), which never passes the slots already read;
  //   ranking  the query's lanes take the compacted survivors L apart -- ~13 of 48, ~3.6 insertion rounds per lane
  //            instead of ~12.5 -- through the one knn_offer below.
  // The choice is the WAVE's (16 queries), so that no wave runs both drains: it screens when every pool of its queries fits
  // the row (T <= kGridScreenCap: nothing went down direct() then) and some pool is past two trips of the old drain
  // (T > 32: below that the two sweeps cost what the insertions they save do).  A pool below 2 L in such a wave has a lane
  // with fewer than two candidates: U = +inf, everything is ranked.  Any other wave -- a dense cell, an overflow, a coarse
  // grid with short pools -- drains as before, below.  Returns the number of candidates the old drain has left to do.
  auto drain_screened = [&]() __attribute__((always_inline)) {
    const int T = s_cnt[qs];
    if constexpr (L != 4) return min(T, kGridCap);
    const bool screen = !__any(T > kGridScreenCap) && __any(T > 32);
    const int ns = screen ? T : 0;
    unsigned short *row = s_list[qs];
    float *s2v = reinterpret_cast<float *>(row + kGridScreenCap);
    float m1 = INFINITY, m2 = INFINITY;
#pragma unroll 1
    for (int k0 = 0; k0 < ns; k0 += 4 * L) {
      float4 r[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) r[u] = sc[row[min(k0 + sub + u * L, ns - 1)]];
      wave_lds_sync();  // (a padded slot reads the last index: before its owner replaces it)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = k0 + sub + u * L;
        const float dx = r[u].x - q[0], dy = r[u].y - q[1], dz = r[u].z - q[2];
        const float s = i < ns ? fmaf(dz, dz, fmaf(dy, dy, dx * dx)) : __builtin_nanf("");  // the reference's rounding order
        m2 = s < m1 ? m1 : fminf(m2, s);
        m1 = fminf(m1, s);
        s2v[i] = s;
        row[i] = (unsigned short)__float_as_int(r[u].w);  // (ids are below 16384)
      }
    }
    float U = m2;
    U = fmaxf(U, __int_as_float(knn_dpp_i32<0xB1>(__float_as_int(U))));  // quad_perm [1,0,3,2]
    U = fmaxf(U, __int_as_float(knn_dpp_i32<0x4E>(__float_as_int(U))));  // quad_perm [2,3,0,1]
    const float thr = __fmul_rn(U, 1.000001f);
    wave_lds_sync();
    int c = 0;  // survivors of the query so far
#pragma unroll 1
    for (int k0 = 0; k0 < ns; k0 += 4 * L) {
      float s[4];
      unsigned short id[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        s[u] = s2v[k0 + sub + u * L];
        id[u] = row[k0 + sub + u * L];
      }
      wave_lds_sync();  // (all sixteen slots are read before one of them is written)
      int n = 0, at[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        at[u] = n;
        n += s[u] <= thr ? 1 : 0;  // (the NaN of a padded slot stays out)
      }
      // inclusive prefix over the quad (the permutes are taken by all four lanes, then selected: not under a branch)
      const int n1 = knn_dpp_i32<0x90>(n);  // quad_perm [0,0,1,2]
      int p = n + (sub >= 1 ? n1 : 0);
      const int p2 = knn_dpp_i32<0x40>(p);  // quad_perm [0,0,0,1]
      p += sub >= 2 ? p2 : 0;
      const int first = c + p - n;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (s[u] <= thr) {
          s2v[first + at[u]] = s[u];
          row[first + at[u]] = id[u];
        }
      c += knn_dpp_i32<0xFF>(p);  // quad_perm [3,3,3,3]
      wave_lds_sync();
    }
    // one entry ahead of the insertion; lanes past the end drop out (an entry read past c is stale and never offered)
    float s_n = s2v[sub];
    int id_n = row[sub];
#pragma unroll 1
    for (int j = sub; j < c; j += L) {
      const float s = s_n;
      const int id = id_n;
      const int jn = min(j + L, kGridScreenCap - 1);
      s_n = s2v[jn];
      id_n = row[jn];
      knn_offer<8, false>(st, s, id, lad);
    }
    return screen ? 0 : min(T, kGridCap);
  };
  auto drain = [&](auto screen) __attribute__((always_inline)) {
    wave_lds_sync();
    int total;
    if constexpr (decltype(screen)::value) total = drain_screened();
    else total = min(s_cnt[qs], kGridCap);
#pragma unroll 1
    for (int base = sub; base < total; base += 4 * L) {
      float4 r[4];
      bool ok[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = base + u * L;
        ok[u] = i < total;
        r[u] = sc[s_list[qs][min(i, total - 1)]];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float dx = r[u].x - q[0], dy = r[u].y - q[1], dz = r[u].z - q[2];
        const float s2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));  // the reference's rounding order
        knn_offer<8, false>(st, ok[u] ? s2 : __builtin_nanf(""), __float_as_int(r[u].w), lad);
      }
    }
    wave_lds_sync();
  };
  // One column (dy, dz in -1..1) of the inner block, its three cells: their ranges in flight together (no load under the
  // per-cell branches), then the box tests and the pooling.
  auto column = [&](int dy, int dz) __attribute__((always_inline)) {
    const int ay = cq[1] + dy, az = cq[2] + dz;
    if ((unsigned)ay > (unsigned)gmax[1] || (unsigned)az > (unsigned)gmax[2]) return;
    const float d2yz = axis_d2(1, dy) + axis_d2(2, dz);
    const unsigned bityz = tab_code(0, ay, az);
    int beg[3], end[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      beg[t] = ct[bityz | bitx[t]];
      end[t] = ct[(bityz | bitx[t]) + span];
    }
    // (nearly) every cell is taken -- they reserve their places in the query's list together (one LDS atomic, not one per
    // cell); cells hold 0..~8 records: the first four places are written without a loop
    int len[3], tot = 0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      len[t] = okx[t] && !((d2yz + d2x[t]) * 0.99999f > st.bound) ? end[t] - beg[t] : 0;
      tot += len[t];
    }
    if (tot == 0) return;
    int off = atomicAdd(&s_cnt[qs], tot);
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int fit = min(len[t], kGridCap - off);  // (a full list sends the rest of the cell down the direct path)
      unsigned short *dst = &s_list[qs][off];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < fit) dst[k] = (unsigned short)(beg[t] + k);
      for (int k = 4; k < fit; ++k) dst[k] = (unsigned short)(beg[t] + k);
      for (int k = max(fit, 0); k < len[t]; ++k) direct(beg[t] + k);
      off += len[t];
    }
  };
  auto begin_pass = [&]() __attribute__((always_inline)) {
    if (sub == 0) s_cnt[qs] = 0;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  };
  // The columns are dealt DENSELY: walking all 25 of the +-2 block with the other pass's columns skipped cost the wave the
  // full body in nearly every iteration (some lane always had a live column) -- clock stamps: the first pass's 27 cells took
  // as long as the second's 98, and the two together two thirds of the kernel.
  // pass 0: the nine inner columns at dx in -1..1
  begin_pass();
  if constexpr (L == 4) {
    // nine columns over four lanes are 4 + 4 + 1: a third trip through the whole column body for one lane in four.  The
    // ninth column (dy = dz = +1) goes cell by cell to lanes 0..2 instead; its ranges are asked for here, ahead of the two
    // trips, and pooled behind them
    const int ay = cq[1] + 1, az = cq[2] + 1;
    const bool mine = sub < 3 && (unsigned)ay <= (unsigned)gmax[1] && (unsigned)az <= (unsigned)gmax[2];
    const bool okc = sub == 0 ? okx[0] : sub == 1 ? okx[1] : okx[2];
    const float d2c = (sub == 0 ? d2x[0] : sub == 1 ? d2x[1] : d2x[2]) + axis_d2(1, 1) + axis_d2(2, 1);
    const unsigned code = tab_code(0, ay, az) | (sub == 0 ? bitx[0] : sub == 1 ? bitx[1] : bitx[2]);
    const int beg9 = ct[mine ? code : 0], end9 = ct[mine ? code + span : 0];
#pragma unroll 1
    for (int ci = sub; ci < 8; ci += L) column(ci % 3 - 1, ci / 3 - 1);
    if (mine && okc && !(d2c * 0.99999f > st.bound)) enqueue(beg9, end9);
  } else {
#pragma unroll 1
    for (int ci = sub; ci < 9; ci += L) column(ci % 3 - 1, ci / 3 - 1);
  }
  drain(std::true_type{});
  knn_merge_sublanes<L>(st);
  // pass 1: every other cell the ball of the merged bound meets.  The K nearest neighbours all lie within the K-th distance
  // seen so far, so the cells to look at are a BOX with its own radius per axis -- two cells each way in a uniform cloud
  // (the 5 x 5 x 5 block of the first versions of this kernel), one cell in x / y and four thin layers in z on the ground
  // plane of a street scene whose bounding box is a tenth as high as wide.  Exact after this pass: nothing outside the box
  // is within the bound.  (The fixed block + shell-by-shell widening of the first version took 5.9 ms instead of 30 us
  // on such a scene, tools/knn_scene_bench.py.)
  // The cells of the box that pass 0 has not seen (knn_box_shell) are few: on a uniform 8192-point cube 86 % of the
  // queries have none and a wave of sixteen has ~22 together, where walking the box column by column looked ~260 ranges up
  // in ~3 trips through a heavy body (profiles/knn_grid_box.txt).  So the wave lists them: every query publishes its count
  // and a record of what a test of one of its cells needs, a prefix over the sixteen counts places the queries, and lane j
  // takes cell j of the list WHOEVER'S it is -- finds the query among the prefixes, decodes the cell's offsets, tests it
  // against that query's bound, looks its range up and reserves its places in that query's pool row.  The rows stay
  // wave-private.  A row that is full cannot send the rest of a cell down direct() here (the lane's list is another
  // query's): the count goes past kGridCap all the same, which marks the query for the restart below, as do a box of more
  // than kGridBoxCells cells (nothing is enumerated for it) and, unless it ends inside the +-2 block, no K-th distance
  // yet (fewer than K points in the 27 cells: the +-2 block is enumerated, every cell passes the test).
  bool exact = false, wide = false;
  int blo[3] = {0, 0, 0}, bhi[3] = {0, 0, 0};  // (an idle lane: the box of one cell, nothing outside its inner block)
  if (valid && st.bound < INFINITY) {
    const float r = sqrtf(st.bound) * 1.0001f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float inv = scl[a] / (float)(4 << drop[a]);  // cells per unit length
      blo[a] = min(0, max(0, (int)floorf((q[a] - r - eps[a] - lo[a]) * inv)) - cq[a]);
      bhi[a] = max(0, min(gmax[a], (int)floorf((q[a] + r + eps[a] - lo[a]) * inv)) - cq[a]);
    }
    wide = (bhi[0] - blo[0] + 1) * (bhi[1] - blo[1] + 1) * (bhi[2] - blo[2] + 1) > kGridBoxCells;
    exact = !wide;
  } else if (valid) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      blo[a] = max(-2, -cq[a]);
      bhi[a] = min(2, gmax[a] - cq[a]);
    }
  }
  int ncell, unused[3];
  ncell = knn_box_shell(blo[0], blo[1], blo[2], bhi[0], bhi[1], bhi[2], 0, unused[0], unused[1], unused[2]);
  if (wide) ncell = 0;
  int last = ncell;  // inclusive prefix over the wave's queries (the L lanes of a query agree)
#pragma unroll
  for (int off = L; off < 64; off <<= 1) {
    const int o = __shfl_up(last, off, 64);
    if (lane >= off) last += o;
  }
  const int wave_cells = __builtin_amdgcn_readlane(last, 63);
  bool full = false;
  if (wave_cells > 0) {
    KnnBoxRec *s_rec = reinterpret_cast<KnnBoxRec *>(s_raw + kGridRecAt);  // [QB]
    const int q0 = qs & ~(QW - 1);  // the wave's first query
    if (sub == 0) {
      s_cnt[qs] = 0;
      s_rec[qs].qb = make_float4(q[0], q[1], q[2], st.bound);
      s_rec[qs].box = make_int4(knn_pack3(cq[0], cq[1], cq[2]), knn_pack3(-blo[0], -blo[1], -blo[2]),
                                knn_pack3(bhi[0], bhi[1], bhi[2]), last - ncell);
    }
    wave_lds_sync();
    bool pooled = false;
#pragma unroll 1
    for (int base = 0; base < wave_cells; base += 64) {
      const int j = base + lane;
      if (j >= wave_cells) continue;
      int f = 0;  // the last query of the wave that starts at or before j: the one with a cell there
#pragma unroll
      for (int step = QW / 2; step > 0; step >>= 1)
        if (s_rec[q0 + f + step].box.w <= j) f += step;
      const float4 fq = s_rec[q0 + f].qb;
      const int4 fb = s_rec[q0 + f].box;
      int fd[3], fc[3];
      knn_box_shell(-knn_byte(fb.y, 0), -knn_byte(fb.y, 1), -knn_byte(fb.y, 2), knn_byte(fb.z, 0), knn_byte(fb.z, 1),
                    knn_byte(fb.z, 2), j - fb.w, fd[0], fd[1], fd[2]);
#pragma unroll
      for (int a = 0; a < 3; ++a) fc[a] = knn_byte(fb.x, a) + fd[a];
      const unsigned code = tab_code(fc[0], fc[1], fc[2]);
      const int beg = ct[code], len = ct[code + span] - beg;  // (asked for ahead of the test)
      const float d2 = (cell_d2(1, fq.y, fc[1]) + cell_d2(2, fq.z, fc[2])) + cell_d2(0, fq.x, fc[0]);
      if (d2 * 0.99999f > fq.w || len <= 0) continue;
      pooled = true;
      const int off = atomicAdd(&s_cnt[q0 + f], len);
      const int fit = min(len, kGridCap - off);
      for (int k = 0; k < fit; ++k) s_list[q0 + f][off + k] = (unsigned short)(beg + k);
    }
    // (a wave that pooled nothing -- 94 % of them at 16384 points -- keeps the lists of pass 0's merge as they are)
    if (__any(pooled)) {
      keep_one_copy();
      drain(std::false_type{});
      knn_merge_after_sparse_pass<L>(st, sub);  // (0.03 insertions per query in this pass on a uniform cloud)
      full = s_cnt[qs] > kGridCap;
    }
  }
  // What is left -- sparse corners, outliers, clusters that put everything into a few cells -- restarts against the bound
  // it has, over the 64-point groups of the Morton order whose box the search ball meets (the sort's group boxes): exact
  // (the list is emptied first, every point within the bound is offered again, nothing twice) and bounded: N / 64 box
  // tests per query dealt over its lanes.
  const bool done = !valid || (!full && !wide && (exact || inside(2)));
  if (__any(!done)) {
    if (done) {
      keep_one_copy();
    } else {
      knn_list_clear(st);  // (the bound stays: it is the K-th distance of a superset of nothing less)
      const int NG = (N + 63) >> 6;
      const float4 *gb = reinterpret_cast<const float4 *>(gbox) + (size_t)b * NG * 2;  // (group_box.h)
#pragma unroll 1
      for (int g = sub; g < NG; g += L) {
        const float4 lo4 = gb[2 * g], hi4 = gb[2 * g + 1];
        if (point_box_gap2(lo4, hi4, q[0], q[1], q[2]) > st.bound) continue;
        const int j1 = min(N, g * 64 + 64);
#pragma unroll 1
        for (int j = g * 64; j < j1; j += 8) {  // eight records in flight
          float4 r8[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) r8[u] = sc[min(j + u, j1 - 1)];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const float dx = r8[u].x - q[0], dy = r8[u].y - q[1], dz = r8[u].z - q[2];
            const float s2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            knn_offer<8, false>(st, j + u < j1 ? s2 : __builtin_nanf(""), __float_as_int(r8[u].w), lad);
          }
        }
      }
    }
    knn_merge_sublanes<L>(st);
  }
  if (valid) {
    const int y = __float_as_int(qr.w);  // the query's original index
#pragma unroll
    for (int e = 0; e < 8 / L; ++e) {
      const int slot = e * L + sub;
      if (slot >= K) break;
      u64 key = st.keys[0];
#pragma unroll
      for (int i = 1; i < 8; ++i) key = slot == i ? st.keys[i] : key;
      const size_t o = ((size_t)b * N + y) * K + slot;
      knn_emit(key, lad, nn + o, dist + o);
    }
  }
}

constexpr int kGridLanes = 4;  // per query

// The launch plan of dh3d_knn_grid -- the one place its thresholds live (dh3d_knn_grid, dh3d_knn_grid_plan).
//   sf: how a crowded cloud is served.  4 / 2 = the pruned scan inside knn_grid_kernel<4, sf> (one launch); 0 =
//       knn_grid_kernel<kGridLanes, 0> for the uniform clouds, then knn_sorted_launch gated on the crowded flag.
//   drop: D, the grid bits dropped for small sets (2^D consecutive cells of the table searched as one).
struct KnnGridPlan {
  int sf, drop;
};
static KnnGridPlan knn_grid_plan(int B, int N) {
  KnnGridPlan p{0, 0};
  // one to two points per cell: all 4096 cells down to 4096 points (measured: 32 x 4096 77 us against 83 with half the
  // cells), one bit of the cell code less for every halving below that
  while (p.drop < 6 && ((long long)N << p.drop) <= 3072) ++p.drop;
  // The clouds whose points crowd into few cells (the sort's verdict, cells[kCellFlag]) go to the pruned scan -- in the SAME
  // launch (four waves per query group = the cell lists' 256-thread workgroup) up to 4096 query groups, as a second launch
  // (whose workgroups leave at once for the other clouds) for the one-wave scan beyond that.
  // (four waves per query group up to 1280 groups, as the scan on its own; beyond that two groups per workgroup with two
  // waves each -- ONE two-wave group per 256-thread workgroup left half its waves unused while it held its LDS: 139.8 us;
  // 32 x 4096 demo clouds: 97.7 us against 117.9)
  const long long groups = (long long)((N + 63) / 64) * B;
  if (kGridLanes == 4 && groups <= 4096) p.sf = groups > 1280 ? 2 : 4;
  return p;
}

DH3D_API int dh3d_knn_grid_plan(int B, int N, int K) {
  if (B <= 0 || N <= 0 || K <= 0 || K > 8 || N > 16384 || B > 65535) return -1;
  const KnnGridPlan p = knn_grid_plan(B, N);
  return p.sf + 16 * p.drop;
}

DH3D_API int dh3d_knn_grid(const float *sorted, const float *gbox, const int32_t *cells, int B, int N, int K, int32_t *nn,
                           float *dist, void *stream) {
  DH3D_REQUIRE(sorted && gbox && cells && nn && dist && B > 0 && N > 0 && K > 0);
  DH3D_SUPPORTED(K <= 8 && N <= 16384 && B <= 65535);
  const KnnLadder lad = knn_ladder(N);
  constexpr int kLanes = kGridLanes;
  const KnnGridPlan plan = knn_grid_plan(B, N);
  const int D = plan.drop;
  const dim3 grid(dh3d_cdiv(N, 256 / kLanes), B);
  const float4 *so = reinterpret_cast<const float4 *>(sorted);
  if (plan.sf == 2) {
    hipLaunchKernelGGL((knn_grid_kernel<4, 2>), grid, dim3(256), 0, (hipStream_t)stream, so, gbox, cells, N, K, D, lad, nn, dist);
    return dh3d_launch_status();
  }
  if (plan.sf == 4) {
    hipLaunchKernelGGL((knn_grid_kernel<4, 4>), grid, dim3(256), 0, (hipStream_t)stream, so, gbox, cells, N, K, D, lad, nn, dist);
    return dh3d_launch_status();
  }
  hipLaunchKernelGGL((knn_grid_kernel<kLanes, 0>), grid, dim3(256), 0, (hipStream_t)stream, so, gbox, cells, N, K, D, lad, nn, dist);
  if (dh3d_launch_status() != DH3D_OK) return DH3D_ERR_LAUNCH;
  return knn_sorted_launch(sorted, gbox, B, N, K, nn, dist, cells, stream);
}
