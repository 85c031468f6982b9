// KnnPoint / SelectionSort (tf_ops/grouping: tf_grouping.py:37-47,63-88, tf_grouping_g.cu:134-177) for gfx950.
// The reference tiles both clouds into a [b,m,n] matrix of squared distances and runs, one thread per row, a partial
// selection sort: for s = 0 .. k-1 find the FIRST position t >= s holding the smallest value (strict <) and swap
// positions s and t of the value row and of the id row.  The whole row is the op's result, and its tie order is the swap
// walk's own (a swapped-out entry re-enters further up), not "lowest id first".
//
// What makes a parallel kernel exact (tests/test_knn_point_reference.py proves it on tie-heavy rows): the walk only ever
// moves the positions of
//   C = {0 .. k-1}  U  {the min(k, n-k) smallest by (value, position) among the positions >= k},
// and the k-step walk on C taken in position order, written back to the positions of C, is the whole row.  So every
// kernel here has two stages: (1) scan the row once and keep a (value, position) k-list over the positions >= k -- keys
// are 64-bit (ordered value bits << 32 | position), all distinct, so the list does not depend on the order the scan meets
// them in; (2) replay the walk on the at most 2k candidates.
//
//   knn3_fused_kernel   c = 3, k <= 64.  A workgroup of 4 waves serves 16 queries (4 per wave); the dataset streams
//                       through LDS in tiles of 1024 points, lane = candidate.  Per query the k-list is one key per lane,
//                       kept sorted across the wave; a candidate below the list's k-th key goes to a 64-slot buffer in LDS
//                       that is folded into the list by a wave-wide bitonic sort + merge when it fills.  No [m,n]
//                       intermediate ever exists.
//   topk_row_kernel     one workgroup per row, any value source: a row of a distance matrix (dh3d_select_top_k) or the
//                       distances of one query for any c, computed on the fly (the generic path of dh3d_knn_point).  The
//                       k-list is built in LDS by threshold + append + bitonic compaction.  k <= 1024.
//   walk_row_kernel     dh3d_select_top_k beyond that (up to k = n): the reference's walk on the output row itself, the
//                       argmin of each step spread over the workgroup.
// Rounding of the distance: every difference and every square rounded to f32 on its own, the squares added left to right
// over c (this file is built with -ffp-contract=off).  NaN / infinite inputs are outside the contract.
#include "common.h"
#include "keys.h"
#include "block_ops.h"

namespace {

typedef unsigned long long u64;
constexpr u64 kNoKey = ~0ull;  // above every key: the value field of a key never holds 0xFFFFFFFF (a NaN pattern)

constexpr int kFusedMaxK = 64;   // one list entry per lane
constexpr int kFusedQ = 4;       // queries per wave
constexpr int kFusedWaves = 4;   // waves per workgroup
constexpr int kFusedTile = 1024; // dataset points per LDS tile (12 KiB)
constexpr int kRowMaxK = 1024;   // topk_row_kernel: k-list + walk arrays in LDS
constexpr int kRowThreads = 256;

__device__ __forceinline__ u64 wave_min64(u64 v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = key_min(v, __shfl_xor(v, off, 64));
  return v;
}

__device__ __forceinline__ float sq3(float qx, float qy, float qz, float x, float y, float z) {
  const float dx = x - qx, dy = y - qy, dz = z - qz;
  return (dx * dx + dy * dy) + dz * dz;
}

// ------------------------------------------------------------------------------------------------ fused, c = 3
// Keys here are (f32 bits << 32 | position): a squared distance is never negative, so its bits order as the value does.
__global__ __launch_bounds__(64 * kFusedWaves) void knn3_fused_kernel(const float *__restrict__ xyz1,
                                                                      const float *__restrict__ xyz2, int n, int m, int k,
                                                                      int tiles, float *__restrict__ val,
                                                                      int32_t *__restrict__ idx) {
  __shared__ float s_c[3 * kFusedTile];                        // x[tile] | y[tile] | z[tile]
  __shared__ u64 s_buf[kFusedWaves][kFusedQ][64];
  const int bid = dh3d_xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int b = bid / tiles, tile = bid - b * tiles;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const float *pc = xyz1 + (size_t)b * n * 3;
  const int j0 = tile * (kFusedWaves * kFusedQ) + wave * kFusedQ;
  const int kk = min(k, n - k);                                // entries of the k-list over the positions >= k

  float qx[kFusedQ], qy[kFusedQ], qz[kFusedQ];
  u64 list[kFusedQ], tau[kFusedQ];
  int cnt[kFusedQ];
#pragma unroll
  for (int q = 0; q < kFusedQ; ++q) {
    const size_t qrow = (size_t)b * m + min(j0 + q, m - 1);    // (a padding query repeats the last one; it writes nothing)
    qx[q] = xyz2[qrow * 3], qy[q] = xyz2[qrow * 3 + 1], qz[q] = xyz2[qrow * 3 + 2];
    list[q] = kNoKey, tau[q] = kNoKey, cnt[q] = 0;
  }
  // fold a query's buffer into its list: sort the buffer, reverse it against the list (the elementwise minimum is a
  // bitonic sequence holding the 64 smallest of both), merge; the threshold is the list's kk-th key
  auto flush = [&](int q) {
    wave_lds_sync();
    u64 bv = lane < cnt[q] ? s_buf[wave][q][lane] : kNoKey;
    wave_lds_sync();
    list[q] = wave_fold(list[q], bv, lane);
    tau[q] = __shfl(list[q], kk - 1, 64);
    cnt[q] = 0;
  };

  for (int base = 0; base < n; base += kFusedTile) {
    const int len = min(kFusedTile, n - base);
    __syncthreads();
    for (int e = threadIdx.x; e < len * 3; e += 64 * kFusedWaves) {
      const int c = e / 3;
      s_c[(e - c * 3) * kFusedTile + c] = pc[(size_t)base * 3 + e];
    }
    __syncthreads();
    if (kk > 0 && base + len > k) {                            // (uniform: the tile holds positions >= k)
      for (int jj = 0; jj < len; jj += 64) {
        const int t = jj + lane, i = base + t;
        const bool live = t < len && i >= k;
        const float x = s_c[min(t, len - 1)], y = s_c[kFusedTile + min(t, len - 1)], z = s_c[2 * kFusedTile + min(t, len - 1)];
#pragma unroll
        for (int q = 0; q < kFusedQ; ++q) {
          const u64 key = ((u64)__float_as_uint(sq3(qx[q], qy[q], qz[q], x, y, z)) << 32) | (unsigned)i;
          const bool acc = live && key < tau[q];
          const u64 mask = __ballot(acc);
          if (mask) {                                          // wave-uniform
            const int pcnt = __popcll(mask);
            if (cnt[q] + pcnt > 64) flush(q);                  // (what the new threshold would now refuse is still correct to keep)
            if (acc) s_buf[wave][q][cnt[q] + __popcll(mask & ((1ull << lane) - 1ull))] = key;
            cnt[q] += pcnt;
          }
        }
      }
    }
  }

  // ---- stage 2: the walk on positions 0 .. k-1 and the list's kk entries in position order: T = k + kk <= 128 keys, two
  // per lane (w0: walk position lane, w1: walk position 64 + lane)
  const int T = k + kk;
#pragma unroll
  for (int q = 0; q < kFusedQ; ++q) {
    if (kk > 0) flush(q);
    const int j = j0 + q;
    if (j >= m) continue;                                      // (uniform)
    // the list by position: swap the halves of each key, sort, swap back
    u64 tl = lane < kk ? (list[q] << 32) | (list[q] >> 32) : kNoKey;
    tl = wave_sort(tl, lane);
    tl = (tl << 32) | (tl >> 32);
    u64 *w = s_buf[wave][q];                                   // (64 slots: walk positions k .. T-1 pass through LDS)
    wave_lds_sync();
    if (lane < kk) w[lane] = tl;
    wave_lds_sync();
    u64 w0 = kNoKey, w1 = kNoKey;
    if (lane < k) {
      w0 = ((u64)__float_as_uint(sq3(qx[q], qy[q], qz[q], pc[lane * 3], pc[lane * 3 + 1], pc[lane * 3 + 2])) << 32) | (unsigned)lane;
    } else if (lane < T) {
      w0 = w[lane - k];
    }
    if (64 + lane < T) w1 = w[64 + lane - k];
    for (int s = 0; s < k; ++s) {
      // the first walk position t >= s with the smallest value: the minimum of (value bits, t)
      u64 c0 = lane >= s && lane < T ? (w0 & 0xFFFFFFFF00000000ull) | (unsigned)lane : kNoKey;
      const u64 c1 = 64 + lane < T ? (w1 & 0xFFFFFFFF00000000ull) | (unsigned)(64 + lane) : kNoKey;
      const int t = (int)(unsigned)wave_min64(key_min(c0, c1));
      if (t != s) {                                            // (uniform) swap walk positions s (< 64) and t
        const u64 vs = __shfl(w0, s, 64);
        const u64 vt = t < 64 ? __shfl(w0, t, 64) : __shfl(w1, t - 64, 64);
        if (lane == s) w0 = vt;
        if (t < 64) { if (lane == t) w0 = vs; }
        else if (lane == t - 64) w1 = vs;
      }
    }
    if (lane < k) {
      const size_t o = ((size_t)b * m + j) * k + lane;
      val[o] = __uint_as_float((unsigned)(w0 >> 32));
      idx[o] = (int32_t)(unsigned)w0;
    }
  }
}

// ------------------------------------------------------------------------------------------------ one workgroup per row
struct DistRow {  // a row of a [rows, n] matrix
  const float *row;
  __device__ __forceinline__ float value(int p) const { return row[p]; }
};
struct XyzRow {  // the distances of one query to a cloud of n points of c components
  const float *cloud, *query;
  int c;
  __device__ __forceinline__ float value(int p) const {
    const float *x = cloud + (size_t)p * c;
    float s = 0.f;
    for (int cc = 0; cc < c; ++cc) {
      const float d = x[cc] - query[cc];
      s = cc == 0 ? d * d : s + d * d;
    }
    return s;
  }
};

// FULL: write the whole row (values + ids, dh3d_select_top_k); otherwise its first k columns (val, idx of dh3d_knn_point).
// Dynamic LDS: u64 key[P] | unsigned wk[T] | int wi[T], T = k + kk, P a power of two >= max(2 kk, 512).
template <class SRC, bool FULL>
__device__ __forceinline__ void topk_row(const SRC &src, int n, int k, int P, float *__restrict__ out,
                                         int32_t *__restrict__ outi) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  __shared__ int s_cnt;
  const int kk = min(k, n - k), T = k + kk, tid = threadIdx.x;
  u64 *s_key = reinterpret_cast<u64 *>(s_dyn);
  unsigned *s_wk = reinterpret_cast<unsigned *>(s_key + P);
  int *s_wi = reinterpret_cast<int *>(s_wk + T);

  if (kk > 0) {
    // ---- stage 1: the kk smallest keys over the positions >= k.  Keys below the threshold are appended; when another
    // round might overflow the array it is sorted and cut back to kk, whose last key is the new threshold.
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    u64 tau = kNoKey;
    auto compact = [&](int have) {
      for (int i = have + tid; i < kk; i += kRowThreads) s_key[i] = kNoKey;  // (a cut before kk keys have arrived)
      block_sort<kRowThreads>(s_key, max(have, kk));
      tau = s_key[kk - 1];
      if (tid == 0) s_cnt = kk;
      __syncthreads();
    };
    for (int base = k; base < n; base += kRowThreads) {
      const int have = s_cnt;                                  // (uniform: read after a barrier, written before one)
      __syncthreads();
      if (have + kRowThreads > P) compact(have);
      const int p = base + tid;
      if (p < n) {
        const u64 key = ((u64)f32_order_bits_nz(src.value(p)) << 32) | (unsigned)p;
        if (key < tau) s_key[atomicAdd(&s_cnt, 1)] = key;
      }
      __syncthreads();
    }
    const int have = s_cnt;
    __syncthreads();
    compact(have);
    // ---- the kk chosen in position order
    for (int i = tid; i < kk; i += kRowThreads) {
      const u64 v = s_key[i];
      s_key[i] = (v << 32) | (v >> 32);
    }
    block_sort<kRowThreads>(s_key, kk);
  }
  // ---- stage 2: the walk on C, by the first wave; walk position t < k is row position t, k + i the i-th chosen
  for (int t = tid; t < T; t += kRowThreads) {
    if (t < k) {
      s_wk[t] = f32_order_bits_nz(src.value(t)), s_wi[t] = t;
    } else {
      const u64 v = s_key[t - k];
      s_wk[t] = (unsigned)v, s_wi[t] = (int)(v >> 32);
    }
  }
  __syncthreads();
  if (tid < 64) {
    for (int s = 0; s < k; ++s) {
      u64 best = kNoKey;
      for (int t = s + tid; t < T; t += 64) best = key_min(best, ((u64)s_wk[t] << 32) | (unsigned)t);
      const int t = (int)(unsigned)wave_min64(best);
      if (t != s && tid == 0) {
        const unsigned a = s_wk[s];
        const int ai = s_wi[s];
        s_wk[s] = s_wk[t], s_wi[s] = s_wi[t];
        s_wk[t] = a, s_wi[t] = ai;
      }
      wave_lds_sync();
    }
  }
  __syncthreads();
  if (FULL) {
    // the row as it was from position k on, then the positions of C from the walk (a barrier orders the two stores of
    // a patched position)
    for (int p = k + tid; p < n; p += kRowThreads) out[p] = src.value(p), outi[p] = p;
    __threadfence_block();
    __syncthreads();
    for (int t = tid; t < T; t += kRowThreads) {
      const int p = t < k ? t : (int)(s_key[t - k] >> 32);
      out[p] = src.value(s_wi[t]), outi[p] = s_wi[t];
    }
  } else {
    for (int t = tid; t < k; t += kRowThreads) out[t] = src.value(s_wi[t]), outi[t] = s_wi[t];
  }
}

__global__ __launch_bounds__(kRowThreads) void select_row_kernel(const float *__restrict__ dist, int n, int k, int P,
                                                                 int32_t *__restrict__ outi, float *__restrict__ out) {
  const size_t r = (size_t)blockIdx.x * (size_t)n;             // 64-bit: b m n can pass 2^31
  topk_row<DistRow, true>(DistRow{dist + r}, n, k, P, out + r, outi + r);
}

__global__ __launch_bounds__(kRowThreads) void knn_row_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2,
                                                              int n, int m, int c, int k, int P, float *__restrict__ val,
                                                              int32_t *__restrict__ idx) {
  const size_t r = blockIdx.x, b = r / (size_t)m;
  topk_row<XyzRow, false>(XyzRow{xyz1 + b * (size_t)n * c, xyz2 + r * (size_t)c, c}, n, k, P, val + r * (size_t)k,
                          idx + r * (size_t)k);
}

// k > kRowMaxK: the reference's walk on the output row itself, each step's argmin by the whole workgroup.
__global__ __launch_bounds__(kRowThreads) void walk_row_kernel(const float *__restrict__ dist, int n, int k,
                                                               int32_t *__restrict__ outi, float *__restrict__ out) {
  __shared__ u64 s_red[kRowThreads / 64];
  const size_t r = (size_t)blockIdx.x * (size_t)n;
  const float *src = dist + r;
  float *o = out + r;
  int32_t *oi = outi + r;
  const int tid = threadIdx.x;
  for (int p = tid; p < n; p += kRowThreads) o[p] = src[p], oi[p] = p;
  __threadfence_block();
  __syncthreads();
  for (int s = 0; s < k; ++s) {
    u64 best = kNoKey;
    for (int t = s + tid; t < n; t += kRowThreads) best = key_min(best, ((u64)f32_order_bits_nz(o[t]) << 32) | (unsigned)t);
    best = wave_min64(best);
    if ((tid & 63) == 0) s_red[tid >> 6] = best;
    __syncthreads();
    const int t = (int)(unsigned)key_min(key_min(s_red[0], s_red[1]), key_min(s_red[2], s_red[3]));
    if (t != s && tid == 0) {
      const float a = o[s];
      const int32_t ai = oi[s];
      o[s] = o[t], oi[s] = oi[t];
      o[t] = a, oi[t] = ai;
    }
    __threadfence_block();
    __syncthreads();
  }
}

// P and the dynamic LDS of topk_row for (n, k)
int row_pow2(int n, int k) {
  const int kk = k < n - k ? k : n - k;
  int P = 512;
  while (P < 2 * kk) P <<= 1;
  return P;
}
size_t row_lds(int n, int k, int P) {
  const int kk = k < n - k ? k : n - k;
  return (size_t)P * 8 + (size_t)(k + kk) * 8;
}

}  // namespace

DH3D_API int dh3d_knn_point_plan(int n, int m, int c, int k) {
  if (n <= 0 || m <= 0 || c <= 0 || k <= 0 || k > n) return -1;
  if (c == 3 && k <= kFusedMaxK) return 1;
  return k <= kRowMaxK ? 0 : -1;
}

DH3D_API int dh3d_knn_point(int b, int n, int m, int c, int k, const float *xyz1, const float *xyz2, float *val,
                            int32_t *idx, void *stream) {
  DH3D_REQUIRE(xyz1 && xyz2 && val && idx && b > 0 && n > 0 && m > 0 && c > 0 && k > 0 && k <= n);
  const int plan = dh3d_knn_point_plan(n, m, c, k);
  DH3D_SUPPORTED(plan >= 0);
  hipStream_t s = (hipStream_t)stream;
  if (plan == 1) {
    const int tiles = dh3d_cdiv(m, kFusedWaves * kFusedQ);
    DH3D_SUPPORTED((long long)b * tiles <= 0x7FFFFFFFll);
    hipLaunchKernelGGL(knn3_fused_kernel, dim3(b * tiles), dim3(64 * kFusedWaves), 0, s, xyz1, xyz2, n, m, k, tiles, val, idx);
  } else {
    DH3D_SUPPORTED((long long)b * m <= 0x7FFFFFFFll);
    const int P = row_pow2(n, k);
    hipLaunchKernelGGL(knn_row_kernel, dim3(b * m), dim3(kRowThreads), row_lds(n, k, P), s, xyz1, xyz2, n, m, c, k, P, val,
                       idx);
  }
  return dh3d_launch_status();
}

DH3D_API int dh3d_select_top_k(int b, int n, int m, int k, const float *dist, int32_t *outi, float *out, void *stream) {
  DH3D_REQUIRE(dist && outi && out && b > 0 && n > 0 && m > 0 && k > 0 && k <= n);
  DH3D_SUPPORTED((long long)b * m <= 0x7FFFFFFFll);
  hipStream_t s = (hipStream_t)stream;
  if (k <= kRowMaxK) {
    const int P = row_pow2(n, k);
    hipLaunchKernelGGL(select_row_kernel, dim3(b * m), dim3(kRowThreads), row_lds(n, k, P), s, dist, n, k, P, outi, out);
  } else {
    hipLaunchKernelGGL(walk_row_kernel, dim3(b * m), dim3(kRowThreads), 0, s, dist, n, k, outi, out);
  }
  return dh3d_launch_status();
}
