// PointNet++ grouping / interpolation operators for gfx950.
//   group_point(+grad)        replaces tf_ops/grouping/tf_grouping_g.cu:94-132 (one CUDA block per
//                             cloud, serial over channels) with a flat, channel-coalesced gather.
//   three_nn                  replaces the host loop tf_ops/interpolation/tf_interpolate.cpp:60-103
//                             (the reference has no GPU kernel: every call crossed PCIe twice).  Four kernels, one
//                             result: plain (any order), both sets in Morton order (every candidate visited), the
//                             same pruned by the candidates' 64-sample group boxes, and -- dh3d_three_nn_cells, what
//                             the model's levels take -- the candidates of a query group read off the sampled set's
//                             cell table (three_nn_pruned_kernel_cells).
//   three_interpolate(+grad)  replaces tf_interpolate.cpp:107-153.
//   three_interpolate_idw     fuses the weight computation of core/backbones.py:92-95.
// Arithmetic that decides integer outputs (three_nn) is written with explicit, unfused roundings.
#include <limits.h>

#include "cell_grid.h"
#include "common.h"
#include "group_box.h"
#include "interp_walk.h"
#include "keys.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;

// ------------------------------------------------------------------ group_point
__global__ __launch_bounds__(kBlock) void group_point_fwd_kernel(
    long long rows, int n, int c, int rows_per_cloud, const float *__restrict__ points,
    const int32_t *__restrict__ idx, float *__restrict__ out) {
  const long long total = rows * c;
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total;
       e += (long long)gridDim.x * kBlock) {
    const long long row = e / c;
    const int l = (int)(e - row * c);
    const long long bi = row / rows_per_cloud;
    const int ii = idx[row];
    out[e] = points[(bi * n + ii) * c + l];
  }
}

// c % 4 == 0: one 16-byte element per lane (the model's gathers: 64 / 128 channels)
__global__ __launch_bounds__(kBlock) void group_point_fwd4_kernel(
    long long rows, int n, int c4, int rows_per_cloud, const float4 *__restrict__ points,
    const int32_t *__restrict__ idx, float4 *__restrict__ out) {
  const long long total = rows * c4;
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total;
       e += (long long)gridDim.x * kBlock) {
    const long long row = e / c4;
    const int l = (int)(e - row * c4);
    const long long bi = row / rows_per_cloud;
    out[e] = points[(bi * n + idx[row]) * c4 + l];
  }
}

__global__ __launch_bounds__(kBlock) void group_point_bwd_kernel(
    long long rows, int n, int c, int rows_per_cloud, const float *__restrict__ grad_out,
    const int32_t *__restrict__ idx, float *__restrict__ grad_points) {
  const long long total = rows * c;
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total;
       e += (long long)gridDim.x * kBlock) {
    const long long row = e / c;
    const int l = (int)(e - row * c);
    const long long bi = row / rows_per_cloud;
    const int ii = idx[row];
    atomicAdd(&grad_points[(bi * n + ii) * c + l], grad_out[e]);
  }
}

// ------------------------------------------------------------------ three_nn
constexpr int kNNChunk = 1024;
typedef float f32x2 __attribute__((ext_vector_type(2)));

// lane = query (64 per workgroup); the four waves split the candidates (32-candidate steps, interleaved) so a
// query group keeps 4 waves per SIMD busy instead of one long scan, and their four 3-deep lists are merged
// through LDS on (distance, index) -- the reference's strict '<' in index order = smallest index among equals.
// 8 candidates per packed-f32 sub-step (unfused mul/add, the reference's roundings); the 3-deep insertion only
// runs when one of them beats the lane's current third-best.
__global__ __launch_bounds__(kBlock) void three_nn_kernel(int n, int m, const float *__restrict__ xyz1,
                                                         const float *__restrict__ xyz2,
                                                         float *__restrict__ dist,
                                                         int32_t *__restrict__ idx) {
  __shared__ __attribute__((aligned(16))) float s_c[kNNChunk * 3];
  __shared__ float s_md[3][3][64];  // partial lists of waves 1..3: [wave-1][rank][query]
  __shared__ int s_mi[3][3][64];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  const float *q = xyz1 + ((size_t)b * n + j) * 3;
  const float *cand = xyz2 + (size_t)b * m * 3;
  float x1 = 0.f, y1 = 0.f, z1 = 0.f;
  if (j < n) { x1 = q[0]; y1 = q[1]; z1 = q[2]; }
  const f32x2 qx = {x1, x1}, qy = {y1, y1}, qz = {z1, z1};
  // double 1e40 of the reference: any finite float compares below it, +inf does not.
  float best1 = INFINITY, best2 = INFINITY, best3 = INFINITY;
  int bi1 = 0, bi2 = 0, bi3 = 0;
  for (int base = 0; base < m; base += kNNChunk) {
    const int len = min(kNNChunk, m - base);
    const int len8 = (len + 31) & ~31;  // padded (+inf) to the 32-candidate step
    const int len32 = len8;
    __syncthreads();
    for (int e = threadIdx.x; e < len8 * 3; e += kBlock) {
      const int c = e / 3, comp = e - c * 3;
      s_c[cand4_slot(c, comp)] = c < len ? cand[(size_t)base * 3 + e] : INFINITY;  // padding: d = inf, never < best
    }
    __syncthreads();
    // 32 candidates per iteration with one wave-uniform test, so the LDS reads and packed ops pipeline
    for (int k = 32 * wave; k < len32; k += 32 * (kBlock / 64)) {
      f32x2 d[4][4];
      float mn[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float *g0 = s_c + ((k >> 2) + 2 * u) * 12;
        const f32x4 a0 = *reinterpret_cast<const f32x4 *>(g0), a1 = *reinterpret_cast<const f32x4 *>(g0 + 4),
                    a2 = *reinterpret_cast<const f32x4 *>(g0 + 8), b0 = *reinterpret_cast<const f32x4 *>(g0 + 12),
                    b1 = *reinterpret_cast<const f32x4 *>(g0 + 16), b2 = *reinterpret_cast<const f32x4 *>(g0 + 20);
        {
          const f32x2 dx = f32x2{a0[0], a0[1]} - qx, dy = f32x2{a0[2], a0[3]} - qy, dz = f32x2{a1[0], a1[1]} - qz;
          d[u][0] = (dx * dx + dy * dy) + dz * dz;
        }
        {
          const f32x2 dx = f32x2{a1[2], a1[3]} - qx, dy = f32x2{a2[0], a2[1]} - qy, dz = f32x2{a2[2], a2[3]} - qz;
          d[u][1] = (dx * dx + dy * dy) + dz * dz;
        }
        {
          const f32x2 dx = f32x2{b0[0], b0[1]} - qx, dy = f32x2{b0[2], b0[3]} - qy, dz = f32x2{b1[0], b1[1]} - qz;
          d[u][2] = (dx * dx + dy * dy) + dz * dz;
        }
        {
          const f32x2 dx = f32x2{b1[2], b1[3]} - qx, dy = f32x2{b2[0], b2[1]} - qy, dz = f32x2{b2[2], b2[3]} - qz;
          d[u][3] = (dx * dx + dy * dy) + dz * dz;
        }
        mn[u] = fminf(fminf(fminf(d[u][0][0], d[u][0][1]), fminf(d[u][1][0], d[u][1][1])),
                      fminf(fminf(d[u][2][0], d[u][2][1]), fminf(d[u][3][0], d[u][3][1])));
      }
      const float m = fminf(fminf(mn[0], mn[1]), fminf(mn[2], mn[3]));
      if (__any(j < n && m < best3)) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (j < n && mn[u] < best3) {
#pragma unroll
            for (int t = 0; t < 8; ++t) {  // in index order: strict '<' keeps the first of equal distances
              const float dv = d[u][t >> 1][t & 1];
              const int kk = base + k + 8 * u + t;
              if (dv < best1) {
                best3 = best2; bi3 = bi2; best2 = best1; bi2 = bi1; best1 = dv; bi1 = kk;
              } else if (dv < best2) {
                best3 = best2; bi3 = bi2; best2 = dv; bi2 = kk;
              } else if (dv < best3) {
                best3 = dv; bi3 = kk;
              }
            }
          }
        }
      }
    }
  }
  if (wave > 0) {
    s_md[wave - 1][0][lane] = best1; s_md[wave - 1][1][lane] = best2; s_md[wave - 1][2][lane] = best3;
    s_mi[wave - 1][0][lane] = bi1; s_mi[wave - 1][1][lane] = bi2; s_mi[wave - 1][2][lane] = bi3;
  }
  __syncthreads();
  if (wave == 0 && j < n) {
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const float dv = s_md[w][t][lane];
        const int kk = s_mi[w][t][lane];
        if (dv < best1 || (dv == best1 && kk < bi1)) {
          best3 = best2; bi3 = bi2; best2 = best1; bi2 = bi1; best1 = dv; bi1 = kk;
        } else if (dv < best2 || (dv == best2 && kk < bi2)) {
          best3 = best2; bi3 = bi2; best2 = dv; bi2 = kk;
        } else if (dv < best3 || (dv == best3 && kk < bi3)) {
          best3 = dv; bi3 = kk;
        }
      }
    const size_t o = ((size_t)b * n + j) * 3;
    dist[o] = best1; dist[o + 1] = best2; dist[o + 2] = best3;
    idx[o] = bi1; idx[o + 1] = bi2; idx[o + 2] = bi3;
  }
}

// ------------------------------------------------------------------ three_nn on ordered clouds
// Same outputs as three_nn_kernel from the Morton-ordered records of both sets (spatial.hip: float4 (x, y, z,
// bits(original index))).  What the brute-force kernel spends its time on is not the 8 flop per pair but the 3-deep
// insertion: with queries and candidates in arbitrary order SOME lane of the wave improves its list in nearly every
// 8-candidate sub-step (P ~ 64 * 8 * 3/k until k > 1536), so the branch is taken all the way through.  Here a wave
// holds 64 CONSECUTIVE queries of the Morton order (a compact region) and starts its candidate scan at the position
// of the sampled set's own Morton order that corresponds to that region (farthest-point samples spread evenly over
// the cloud, so rank-proportional is close), wrapping around: the lists are nearly final after the first 128
// candidates and the rest of the scan is the bare distance test.  Every candidate is still visited -- no pruning
// structure, nothing to get wrong -- and equal distances resolve to the smallest candidate index explicitly, so ids
// and distances are bit-identical to three_nn_kernel whatever the visiting order (tf_interpolate.cpp:66-96).
// The 3-deep list as 64-bit keys (bits(d) << 32 | index), ascending: one insertion is three compares + selects, no branch.
__device__ __forceinline__ void nn3_insert(unsigned long long x, unsigned long long &k1, unsigned long long &k2,
                                           unsigned long long &k3) {
  const bool l1 = x < k1, l2 = x < k2, l3 = x < k3;
  k3 = l2 ? k2 : (l3 ? x : k3);
  k2 = l1 ? k1 : (l2 ? x : k2);
  k1 = l1 ? x : k1;
}
// The lists of waves 1..3 merged into wave 0's through s_mk (a workgroup barrier inside: every wave calls).
__device__ __forceinline__ void nn3_merge_waves(unsigned long long (*s_mk)[3][64], int wave, int lane, unsigned long long &k1,
                                                unsigned long long &k2, unsigned long long &k3) {
  if (wave > 0) { s_mk[wave - 1][0][lane] = k1; s_mk[wave - 1][1][lane] = k2; s_mk[wave - 1][2][lane] = k3; }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
      for (int t = 0; t < 3; ++t) nn3_insert(s_mk[w][t][lane], k1, k2, k3);
  }
}
// a query's three distances and ids, row = its place in the original order
__device__ __forceinline__ void nn3_write(float *dist, int32_t *idx, size_t row, unsigned long long k1, unsigned long long k2,
                                          unsigned long long k3) {
  const size_t o = row * 3;
  dist[o] = __uint_as_float((unsigned)(k1 >> 32)); dist[o + 1] = __uint_as_float((unsigned)(k2 >> 32));
  dist[o + 2] = __uint_as_float((unsigned)(k3 >> 32));
  idx[o] = (int)(unsigned)k1; idx[o + 1] = (int)(unsigned)k2; idx[o + 2] = (int)(unsigned)k3;
}

__global__ __launch_bounds__(kBlock) void three_nn_sorted_kernel(int n, int m, const float4 *__restrict__ qs,
                                                                const float4 *__restrict__ cs,
                                                                float *__restrict__ dist, int32_t *__restrict__ idx) {
  __shared__ __attribute__((aligned(16))) float s_c[kNNChunk * 3];
  __shared__ int s_k[kNNChunk];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  const bool valid = j < n;
  const float4 q = qs[(size_t)b * n + (valid ? j : blockIdx.x * 64)];
  const float4 *cand = cs + (size_t)b * m;
  const f32x2 qx = {q.x, q.x}, qy = {q.y, q.y}, qz = {q.z, q.z};
  // The 3-deep list as 64-bit keys (bits(d) << 32 | index): d >= 0, so unsigned order is (distance, index) -- the
  // smallest index among equal distances, i.e. the reference's strict '<' in index order -- and an insertion is three
  // compares + selects with no branch (the branchy form was ~5x the cost of the distance arithmetic per visit).
  // Start: (+inf, 0), the reference's 1e40 / index 0.
  const unsigned long long kInf = (unsigned long long)__float_as_uint(INFINITY) << 32;
  unsigned long long k1 = kInf, k2 = kInf, k3 = kInf;
  // rank-proportional start, 64 candidates before the centre of this query group's image, aligned to the 32-step
  const int nchunks = (m + kNNChunk - 1) / kNNChunk;
  long long c0 = ((long long)blockIdx.x * 64 + 32) * m / n - 64;
  c0 = c0 < 0 ? 0 : c0;
  const int chunk0 = (int)(c0 / kNNChunk);
  for (int ci = 0; ci < nchunks; ++ci) {
    const int base = ((chunk0 + ci) % nchunks) * kNNChunk;
    const int len = min(kNNChunk, m - base);
    const int len32 = (len + 31) & ~31;  // padded (+inf) to the 32-candidate step
    int k0 = ci == 0 ? ((int)(c0 - base) & ~31) : 0;
    k0 = k0 < len32 ? k0 : 0;
    __syncthreads();
    for (int e = threadIdx.x; e < len32; e += kBlock) {
      float4 r = make_float4(INFINITY, INFINITY, INFINITY, __int_as_float(INT_MAX));  // padding: d = inf, never taken
      if (e < len) r = cand[base + e];
      s_c[cand4_slot(e, 0)] = r.x; s_c[cand4_slot(e, 1)] = r.y; s_c[cand4_slot(e, 2)] = r.z;
      s_k[e] = __float_as_int(r.w);
    }
    __syncthreads();
    for (int kr = 32 * wave; kr < len32; kr += 32 * (kBlock / 64)) {
      int k = k0 + kr;
      k = k >= len32 ? k - len32 : k;  // wrap around inside the chunk
      f32x2 d[4][4];
      float mn[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float *g0 = s_c + ((k >> 2) + 2 * u) * 12;
        const f32x4 a0 = *reinterpret_cast<const f32x4 *>(g0), a1 = *reinterpret_cast<const f32x4 *>(g0 + 4),
                    a2 = *reinterpret_cast<const f32x4 *>(g0 + 8), b0 = *reinterpret_cast<const f32x4 *>(g0 + 12),
                    b1 = *reinterpret_cast<const f32x4 *>(g0 + 16), b2 = *reinterpret_cast<const f32x4 *>(g0 + 20);
        {
          const f32x2 dx = f32x2{a0[0], a0[1]} - qx, dy = f32x2{a0[2], a0[3]} - qy, dz = f32x2{a1[0], a1[1]} - qz;
          d[u][0] = (dx * dx + dy * dy) + dz * dz;
        }
        {
          const f32x2 dx = f32x2{a1[2], a1[3]} - qx, dy = f32x2{a2[0], a2[1]} - qy, dz = f32x2{a2[2], a2[3]} - qz;
          d[u][1] = (dx * dx + dy * dy) + dz * dz;
        }
        {
          const f32x2 dx = f32x2{b0[0], b0[1]} - qx, dy = f32x2{b0[2], b0[3]} - qy, dz = f32x2{b1[0], b1[1]} - qz;
          d[u][2] = (dx * dx + dy * dy) + dz * dz;
        }
        {
          const f32x2 dx = f32x2{b1[2], b1[3]} - qx, dy = f32x2{b2[0], b2[1]} - qy, dz = f32x2{b2[2], b2[3]} - qz;
          d[u][3] = (dx * dx + dy * dy) + dz * dz;
        }
        mn[u] = fminf(fminf(fminf(d[u][0][0], d[u][0][1]), fminf(d[u][1][0], d[u][1][1])),
                      fminf(fminf(d[u][2][0], d[u][2][1]), fminf(d[u][3][0], d[u][3][1])));
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        // '<=': an equal distance with a smaller index must still be seen
        if (__any(valid && mn[u] <= __uint_as_float((unsigned)(k3 >> 32)))) {
#pragma unroll
          for (int t = 0; t < 8; ++t) {
            nn3_insert(((unsigned long long)__float_as_uint(d[u][t >> 1][t & 1]) << 32) | (unsigned)s_k[k + 8 * u + t], k1, k2, k3);
          }
        }
      }
    }
  }
  __shared__ unsigned long long s_mk[3][3][64];  // partial lists of waves 1..3
  nn3_merge_waves(s_mk, wave, lane, k1, k2, k3);
  if (wave == 0 && valid) nn3_write(dist, idx, (size_t)b * n + __float_as_int(q.w), k1, k2, k3);
}

// U 8-candidate sub-steps of the LDS image (cand4_slot coordinates in s_c, original indices in s_k) from candidate k on
// (k % 8 == 0) against the lane's query: packed f32 with the reference's unfused roundings; a sub-step reaches the 3-deep
// list -- 64-bit keys (bits(d) << 32 | index), see three_nn_sorted_kernel -- only when one of its distances passes some
// lane's screen kb.  All U sub-steps' LDS reads are issued before the first is used.
template <int U>
__device__ __forceinline__ void nn3_scan(const float *s_c, const int *s_k, int k, bool valid, f32x2 qx, f32x2 qy, f32x2 qz,
                                         unsigned long long &k1, unsigned long long &k2, unsigned long long &k3,
                                         float &kb) {
  f32x2 d[U][4];
  float mn[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float *g0 = s_c + ((k >> 2) + 2 * u) * 12;
    const f32x4 a0 = *reinterpret_cast<const f32x4 *>(g0), a1 = *reinterpret_cast<const f32x4 *>(g0 + 4),
                a2 = *reinterpret_cast<const f32x4 *>(g0 + 8), b0 = *reinterpret_cast<const f32x4 *>(g0 + 12),
                b1 = *reinterpret_cast<const f32x4 *>(g0 + 16), b2 = *reinterpret_cast<const f32x4 *>(g0 + 20);
    {
      const f32x2 dx = f32x2{a0[0], a0[1]} - qx, dy = f32x2{a0[2], a0[3]} - qy, dz = f32x2{a1[0], a1[1]} - qz;
      d[u][0] = (dx * dx + dy * dy) + dz * dz;
    }
    {
      const f32x2 dx = f32x2{a1[2], a1[3]} - qx, dy = f32x2{a2[0], a2[1]} - qy, dz = f32x2{a2[2], a2[3]} - qz;
      d[u][1] = (dx * dx + dy * dy) + dz * dz;
    }
    {
      const f32x2 dx = f32x2{b0[0], b0[1]} - qx, dy = f32x2{b0[2], b0[3]} - qy, dz = f32x2{b1[0], b1[1]} - qz;
      d[u][2] = (dx * dx + dy * dy) + dz * dz;
    }
    {
      const f32x2 dx = f32x2{b1[2], b1[3]} - qx, dy = f32x2{b2[0], b2[1]} - qy, dz = f32x2{b2[2], b2[3]} - qz;
      d[u][3] = (dx * dx + dy * dy) + dz * dz;
    }
    mn[u] = fminf(fminf(fminf(d[u][0][0], d[u][0][1]), fminf(d[u][1][0], d[u][1][1])),
                  fminf(fminf(d[u][2][0], d[u][2][1]), fminf(d[u][3][0], d[u][3][1])));
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    // '<=': an equal distance with a smaller index must still be seen
    if (__any(valid && mn[u] <= kb)) {
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        nn3_insert(((unsigned long long)__float_as_uint(d[u][t >> 1][t & 1]) << 32) | (unsigned)s_k[k + 8 * u + t], k1, k2, k3);
      }
      kb = fminf(kb, __uint_as_float((unsigned)(k3 >> 32)));
    }
  }
}

// The same search with the candidates pruned by their group boxes (m <= kNNChunk: the whole sampled set in LDS -- every
// DH3D level).  three_nn_sorted_kernel evaluates every candidate for every query: 2.5 k VALU instructions per wave, the
// kernel is VALU-issue bound (profiles/r03_d_pmc_three_nn.txt: 37 us for 8 x 8192 against 8 x 1024).  Here
//   A. every wave scans ONE 32-candidate step around the rank-proportional start (128 candidates per query group):
//      every lane gets a 3-deep list; the waves share, per query, the smallest of their third distances -- each is an
//      upper bound of the query's true third distance;
//   B. lane = candidate group (64 Morton-consecutive samples, box from dh3d_spatial_sort): the groups whose box lies
//      within the loosest bound of the query group's box are dealt round-robin to the waves; before a group is scanned
//      the same test per QUERY (point to box, own bound); steps of phase A are not scanned again.
// Skipping is exact (group_box.h), and '<=' keeps a candidate at exactly the third distance (a smaller index must still
// be seen).  Same lists, same merge as above.
__global__ __launch_bounds__(kBlock) void three_nn_pruned_kernel(int n, int m, const float4 *__restrict__ qs,
                                                                const float *__restrict__ qbox,
                                                                const float4 *__restrict__ cs,
                                                                const float *__restrict__ cbox,
                                                                float *__restrict__ dist, int32_t *__restrict__ idx) {
  __shared__ __attribute__((aligned(16))) float s_c[kNNChunk * 3];
  __shared__ int s_k[kNNChunk];
  __shared__ float s_b[4][64];
  __shared__ unsigned long long s_mk[3][3][64];  // partial lists of waves 1..3
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // (the query group is rotated by the cloud: workgroups x, x + 256, ... share a CU -- the same group of every second cloud
  //  -- and clouds of one kind have the same kind of region at the same place of their order: round 6, csrc/knn.hip)
  const int bx = (int)((blockIdx.x + 37u * (unsigned)b) % gridDim.x);
  const int j = bx * 64 + lane;
  const bool valid = j < n;
  const float4 q = qs[(size_t)b * n + (valid ? j : bx * 64)];
  const float4 *cand = cs + (size_t)b * m;
  const f32x2 qx = {q.x, q.x}, qy = {q.y, q.y}, qz = {q.z, q.z};
  const int len32 = (m + 31) & ~31, nsteps = len32 >> 5;
  for (int e = threadIdx.x; e < len32; e += kBlock) {
    float4 r = make_float4(INFINITY, INFINITY, INFINITY, __int_as_float(INT_MAX));  // padding: d = inf, never taken
    if (e < m) r = cand[e];
    s_c[cand4_slot(e, 0)] = r.x; s_c[cand4_slot(e, 1)] = r.y; s_c[cand4_slot(e, 2)] = r.z;
    s_k[e] = __float_as_int(r.w);
  }
  // boxes: the query group's, and (lane = candidate group) the candidates'
  const int NGq = (n + 63) / 64, MG = (m + 63) / 64;
  const float *qb = qbox + ((size_t)b * NGq + bx) * 8;
  const float qlx = qb[0], qly = qb[1], qlz = qb[2], qhx = qb[4], qhy = qb[5], qhz = qb[6];
  float clx = INFINITY, cly = INFINITY, clz = INFINITY, chx = -INFINITY, chy = -INFINITY, chz = -INFINITY, bd = INFINITY;
  if (lane < MG) {
    const float *cb = cbox + ((size_t)b * MG + lane) * 8;
    clx = cb[0]; cly = cb[1]; clz = cb[2]; chx = cb[4]; chy = cb[5]; chz = cb[6];
    bd = group_box_gap2(clx, cly, clz, chx, chy, chz, qlx, qly, qlz, qhx, qhy, qhz);
  }
  const unsigned long long kInf = (unsigned long long)__float_as_uint(INFINITY) << 32;
  unsigned long long k1 = kInf, k2 = kInf, k3 = kInf;
  float kb = INFINITY;  // the screen: min(own third distance, the shared bound)
  __syncthreads();

  auto scan_step = [&](int step) __attribute__((always_inline)) {
    nn3_scan<4>(s_c, s_k, step << 5, valid, qx, qy, qz, k1, k2, k3, kb);  // a 32-candidate step
  };

  // A. one step per wave around the rank-proportional start
  long long c0 = ((long long)bx * 64 + 32) * m / n - 64;
  c0 = c0 < 0 ? 0 : c0;
  const int s0 = (int)(c0 >> 5);
  unsigned long long done = 0ull;  // steps of phase A (all four waves')
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int st = (s0 + w) % nsteps;
    if (!((done >> st) & 1ull)) {
      done |= 1ull << st;
      if (w == wave) scan_step(st);
    }
  }
  s_b[wave][lane] = __uint_as_float((unsigned)(k3 >> 32));
  __syncthreads();
  kb = fminf(fminf(s_b[0][lane], s_b[1][lane]), fminf(s_b[2][lane], s_b[3][lane]));
  const float wb = wave_max_f32(valid ? kb : 0.f);

  // B. the candidate groups that can still matter, dealt to the waves
  unsigned long long mask = __ballot(lane < MG && bd <= wb);
  int mine = 0;
  while (mask != 0ull) {
    const int g = __builtin_ctzll(mask);
    mask &= mask - 1;
    // the group's two 32-candidate steps are dealt to the waves ONE BY ONE (round 6: whole groups left a wave up to two steps
    // behind its neighbours, and the workgroup ends with its slowest wave)
    const bool own0 = (mine & 3) == wave, own1 = ((mine + 1) & 3) == wave;
    mine += 2;
    if (!own0 && !own1) continue;
    const float lx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(clx), g)),
                ly = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cly), g)),
                lz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(clz), g)),
                hx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(chx), g)),
                hy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(chy), g)),
                hz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(chz), g));
    if (!__any(valid && point_box_gap2(lx, ly, lz, hx, hy, hz, q.x, q.y, q.z) <= kb)) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int st = 2 * g + h;
      if ((h == 0 ? own0 : own1) && st < nsteps && !((done >> st) & 1ull)) scan_step(st);
    }
  }

  nn3_merge_waves(s_mk, wave, lane, k1, k2, k3);
  if (wave == 0 && valid) nn3_write(dist, idx, (size_t)b * n + __float_as_int(q.w), k1, k2, k3);
}

// The pruned search with the candidates chosen through the sampled set's CELL TABLE (cells2 of dh3d_three_nn_cells: the
// table dh3d_fps_sorted_ordered writes on the cloud's grid, or dh3d_spatial_sort_cells of the sampled set on its own).
// The boxes above prune by 64-sample Morton groups, 16 boxes of ~0.4 of the cloud each: a query group stages all m
// records and scans about half of them.  Here the workgroup stages only the samples of the cells it can reach:
//   1. the grid is coarsened by dropping the schedule's last D steps (nn3_cell_drop), so a coarse cell is ONE range
//      ct[c << D] .. ct[(c + 1) << D] of the order; round 1 takes the coarse cells of the query group's box +- 1 (a lane
//      per cell: it requests the cell's first kNNDirect records at once and a prefix sum over the cells places them in
//      the cand4_slot image; the rest of a fuller cell follows by a search over the prefix; +inf pads the list to the
//      8-candidate sub-step), the sub-steps are dealt to the four waves one by one and merged;
//   2. every query has a third distance r now.  If the coarse cells of its [q - r, q + r] lie inside round 1's for every
//      query, the lists are final; otherwise the samples of the ADDITIONAL cells of the union are appended and scanned
//      (an unbounded r -- fewer than three candidates so far -- takes every cell: the whole set, what the boxes cost at
//      worst).  (Per query, not the group's box widened by its largest r: the query with the largest r is seldom the one
//      next to the edge of round 1's cells.)
// Exactness.  grid_cell (cell_grid.h) is the sort's own expression on the table's own origin and scales, and monotone in x
// IN FLOAT ARITHMETIC: a sample with s.x >= t lies in a cell >= grid_cell(t), whatever was rounded.  A sample that belongs
// to a query's list has d <= the query's third distance <= r^2, so |s.x - q.x| <= r (1 + 4 * 2^-24) on every axis:
// s.x >= q.x - r' for the inflated r' = r (1 + 1e-5), and the margin subtracted on top covers the two roundings of
// (q.x - r') - margin.  The samples are inside the grid they were binned on, so the clamps only ever act on the query side
// (a table of the sampled set's own grid: queries outside it reach its border cells).  Lists only improve in round 2, so
// round 1's r stays valid.
// The schedule steps dropped: a coarse cell should hold about two samples (512 coarse cells from 768 samples on: 2 x 2 x 2
// cells of a cube's grid; 256 below), so that a query group looks up a few dozen ranges and a third distance seldom
// exceeds the one coarse cell of margin.  (8 x 8192 vs 1024 / 32 x 4096 vs 512, uniform: D = 3 everywhere 16.5 / 28.2 us,
// D = 4 everywhere 17.3 / 26.7 us, this rule 16.3 / 27.0 us -- profiles/three_nn_cells.txt.)
constexpr int nn3_cell_drop(int m) { return m < 768 ? 4 : 3; }
constexpr int kNNCoarse = kGridCells >> 3;                // coarse cells of the grid at most
constexpr int kNNDirect = 8;                        // records a cell's own lane copies (Poisson(2): 2e-4 hold more)
constexpr int kNNCellCap = kNNChunk + 16;           // both rounds are padded to the sub-step: at most m + 14 slots

template <int D>  // the schedule steps dropped: 2^D table cells are one coarse cell
__global__ __launch_bounds__(kBlock) void three_nn_pruned_kernel_cells(int n, int m, const float4 *__restrict__ qs,
                                                                      const float *__restrict__ qbox,
                                                                      const float4 *__restrict__ cs,
                                                                      const int *__restrict__ cells,
                                                                      float *__restrict__ dist, int32_t *__restrict__ idx) {
  __shared__ __attribute__((aligned(16))) float s_c[kNNCellCap * 3];
  __shared__ int s_k[kNNCellCap];
  __shared__ int s_ro[kNNCoarse], s_rb[kNNCoarse];  // per cell of the box: records up to and with it | first record - its slot
  __shared__ int s_wt[2][4];                        // the waves' record counts of one 256-cell pass (two passes alternate)
  __shared__ float s_b[64];                         // round 1's third distance per query
  __shared__ int s_box2[7];                         // round 2's coarse box (lo, hi) and whether there is a round 2
  __shared__ unsigned long long s_mk[3][3][64];     // partial lists of waves 1..3
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int bx = (int)((blockIdx.x + 37u * (unsigned)b) % gridDim.x);  // (rotated by the cloud: three_nn_pruned_kernel)
  const int j = bx * 64 + lane;
  const bool valid = j < n;
  const float4 q = qs[(size_t)b * n + (valid ? j : bx * 64)];
  const float4 *cand = cs + (size_t)b * m;
  const f32x2 qx = {q.x, q.x}, qy = {q.y, q.y}, qz = {q.z, q.z};

  // ---- the grid (the table's header) and the query group's box on it
  const CellGrid g = cell_grid(cells, b);
  const int *ct = g.ct;
  int nc[3];  // the coarse grid's bits per axis
  sched_bits(g.sched, nc, kGridSteps - D);
  const float *qb = qbox + ((size_t)b * ((n + 63) / 64) + bx) * 8;
  const float ql[3] = {qb[0], qb[1], qb[2]}, qh[3] = {qb[4], qb[5], qb[6]};
  int lo1[3], hi1[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int sh = g.nb[a] - nc[a];
    lo1[a] = max((grid_cell(g, a, ql[a]) >> sh) - 1, 0);
    hi1[a] = min((grid_cell(g, a, qh[a]) >> sh) + 1, (1 << nc[a]) - 1);
  }

  // The samples of the coarse cells [lo, hi] (outer: without round 1's) appended to the LDS image from slot `at` on, padded
  // to the sub-step.  Returns the slots taken.  (t < 512 and c <= 64: the float quotient is off by < 1e-4, (t + 0.5) / c is
  // never within 0.5 / 64 of an integer.)
  auto put = [&](int e, float4 rec) __attribute__((always_inline)) {
    s_c[cand4_slot(e, 0)] = rec.x; s_c[cand4_slot(e, 1)] = rec.y; s_c[cand4_slot(e, 2)] = rec.z;
    s_k[e] = __float_as_int(rec.w);
  };
  auto small_div = [](int t, int c) { return (int)(((float)t + 0.5f) * (1.0f / (float)c)); };
  auto stage = [&](const int (&lo)[3], const int (&hi)[3], bool outer, int at) __attribute__((always_inline)) {
    const int c0 = hi[0] - lo[0] + 1, c1 = hi[1] - lo[1] + 1, total = c0 * c1 * (hi[2] - lo[2] + 1);
    int run = 0;
    bool big = false;  // a cell with more than kNNDirect samples
    for (int t0 = 0, pass = 0; t0 < total; t0 += kBlock, pass ^= 1) {
      const int t = t0 + (int)threadIdx.x;
      int beg = 0, len = 0;
      if (t < total) {
        const int tq = small_div(t, c0), iz = lo[2] + small_div(tq, c1);
        const int ix = lo[0] + t - tq * c0, iy = lo[1] + tq - (iz - lo[2]) * c1;
        const bool inner = ix >= lo1[0] && ix <= hi1[0] && iy >= lo1[1] && iy <= hi1[1] && iz >= lo1[2] && iz <= hi1[2];
        if (!(outer && inner)) {
          const unsigned code = cell_code<D>(g.sched, nc, ix, iy, iz);
          beg = min(max(ct[code << D], 0), m);
          len = min(max(ct[(code + 1) << D], beg), m) - beg;
        }
      }
      // a cell's first kNNDirect records are its own lane's, requested now: their way runs under the prefix sum
      float4 rec[kNNDirect];
#pragma unroll
      for (int i = 0; i < kNNDirect; ++i)
        if (i < len) rec[i] = cand[beg + i];
      int inc = len;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
      }
      if (lane == 63) s_wt[pass][wave] = inc;
      big |= __syncthreads_or(len > kNNDirect) != 0;
      int base = run;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int v = s_wt[pass][w];
        base += w < wave ? v : 0;
        run += v;
      }
      const int first = base + inc - len;
#pragma unroll
      for (int i = 0; i < kNNDirect; ++i)
        if (i < len && at + first + i < kNNCellCap) put(at + first + i, rec[i]);
      if (t < total) { s_ro[t] = first + len; s_rb[t] = beg - first; }
    }
    // (A table of this set never fills more than kNNCellCap slots; the cap keeps any other table inside the image.)
    const int cnt = min(run, kNNCellCap - at), pad = min((cnt + 7) & ~7, kNNCellCap - at);
    if ((int)threadIdx.x < pad - cnt)  // padding: d = inf, never taken
      put(at + cnt + (int)threadIdx.x, make_float4(INFINITY, INFINITY, INFINITY, __int_as_float(INT_MAX)));
    if (big) {  // (workgroup-uniform) fuller cells: a lane per record, the first cell whose inclusive count exceeds its rank
      __syncthreads();
      int top = 1;
      while (2 * top <= total) top *= 2;
      for (int r = threadIdx.x; r < cnt; r += kBlock) {
        int o = 0;
        for (int step = top; step > 0; step >>= 1)
          if (o + step <= total && s_ro[o + step - 1] <= r) o += step;
        if (r - (o > 0 ? s_ro[o - 1] : 0) >= kNNDirect) put(at + r, cand[s_rb[o] + r]);
      }
    }
    __syncthreads();
    return pad;
  };

  const unsigned long long kInf = (unsigned long long)__float_as_uint(INFINITY) << 32;
  unsigned long long k1 = kInf, k2 = kInf, k3 = kInf;
  float kb = INFINITY;  // the screen: the lane's third distance so far
  const size_t row = (size_t)b * n + __float_as_int(q.w);

  // ---- round 1.  (The sub-steps are dealt from a wave that turns with the query group: the waves of the workgroups of a CU
  // that share a SIMD do not all get the odd sub-step.)
  const int w0 = (wave - bx) & 3;
  const int pad1 = stage(lo1, hi1, false, 0);
  for (int k = 8 * w0; k < pad1; k += 32) nn3_scan<1>(s_c, s_k, k, valid, qx, qy, qz, k1, k2, k3, kb);
  nn3_merge_waves(s_mk, wave, lane, k1, k2, k3);
  if (wave == 0) {
    const float d3 = __uint_as_float((unsigned)(k3 >> 32));
    s_b[lane] = d3;
    // ---- the cells the lists can still reach: every query's own box [q - r, q + r], r = its third distance
    const float r = sqrtf(d3) * 1.00001f;
    const float qc[3] = {q.x, q.y, q.z};
    int lo2[3], hi2[3];
    bool out = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int sh = g.nb[a] - nc[a];
      // (1e-18: a difference whose square underflows counts as distance zero)
      const float marg = r * 1e-5f + fabsf(qc[a]) * 1e-6f + 1e-18f;
      lo2[a] = valid ? grid_cell(g, a, (qc[a] - r) - marg) >> sh : lo1[a];
      hi2[a] = valid ? grid_cell(g, a, (qc[a] + r) + marg) >> sh : hi1[a];
      out = out || lo2[a] < lo1[a] || hi2[a] > hi1[a];
    }
    const bool more = __any(out);
    if (more) {  // (wave-uniform) round 2's box: the union of the queries' and round 1's
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo2[a] = wave_min_i32(min(lo2[a], lo1[a]));
        hi2[a] = -wave_min_i32(-max(hi2[a], hi1[a]));
      }
    }
    if (lane == 0) {
      s_box2[0] = lo2[0]; s_box2[1] = lo2[1]; s_box2[2] = lo2[2];
      s_box2[3] = hi2[0]; s_box2[4] = hi2[1]; s_box2[5] = hi2[2];
      s_box2[6] = (int)more;
    }
  }
  __syncthreads();
  if (!s_box2[6]) {  // (workgroup-uniform)
    if (wave == 0 && valid) nn3_write(dist, idx, row, k1, k2, k3);
    return;
  }

  // ---- round 2: the additional cells.  Wave 0 keeps the merged lists, the others start empty behind the same screen.
  const int lo2[3] = {s_box2[0], s_box2[1], s_box2[2]}, hi2[3] = {s_box2[3], s_box2[4], s_box2[5]};
  const int pad2 = stage(lo2, hi2, true, pad1);
  if (wave > 0) k1 = k2 = k3 = kInf;
  kb = s_b[lane];
  for (int k = pad1 + 8 * w0; k < pad1 + pad2; k += 32) nn3_scan<1>(s_c, s_k, k, valid, qx, qy, qz, k1, k2, k3, kb);
  nn3_merge_waves(s_mk, wave, lane, k1, k2, k3);
  if (wave == 0 && valid) nn3_write(dist, idx, row, k1, k2, k3);
}

// ------------------------------------------------------------------ three_interpolate
// IDW: weights derived from squared distances (core/backbones.py:92-95); else read from `weight`.
template <bool IDW, int VEC>
__global__ __launch_bounds__(kBlock) void three_interp_fwd_kernel(
    long long rows, int n, int m, int c, const float *__restrict__ points,
    const int32_t *__restrict__ idx, const float *__restrict__ wd, float *__restrict__ out) {
  const int cv = c / VEC;
  const long long total = rows * cv;
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total;
       e += (long long)gridDim.x * kBlock) {
    const long long row = e / cv;
    const int l = (int)(e - row * cv) * VEC;
    const long long bi = row / n;
    const int i1 = idx[row * 3], i2 = idx[row * 3 + 1], i3 = idx[row * 3 + 2];
    float w1 = wd[row * 3], w2 = wd[row * 3 + 1], w3 = wd[row * 3 + 2];
    if (IDW) dh3d_walk::idw3(w1, w2, w3, w1, w2, w3);
    const float *p1 = points + (bi * m + i1) * c + l;
    const float *p2 = points + (bi * m + i2) * c + l;
    const float *p3 = points + (bi * m + i3) * c + l;
    float *o = out + row * c + l;
    if (VEC == 4) {
      const float4 a = *reinterpret_cast<const float4 *>(p1);
      const float4 bq = *reinterpret_cast<const float4 *>(p2);
      const float4 cq = *reinterpret_cast<const float4 *>(p3);
      *reinterpret_cast<float4 *>(o) = dh3d_walk::mix3(a, bq, cq, w1, w2, w3);
    } else {
      o[0] = dh3d_walk::mix3(p1[0], p2[0], p3[0], w1, w2, w3);
    }
  }
}

__global__ __launch_bounds__(kBlock) void three_interp_bwd_kernel(
    long long rows, int n, int m, int c, const float *__restrict__ grad_out,
    const int32_t *__restrict__ idx, const float *__restrict__ weight,
    float *__restrict__ grad_points) {
  const long long total = rows * c;
  for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < total;
       e += (long long)gridDim.x * kBlock) {
    const long long row = e / c;
    const int l = (int)(e - row * c);
    const long long bi = row / n;
    const float g = grad_out[e];
#pragma unroll
    for (int t = 0; t < 3; ++t)
      atomicAdd(&grad_points[(bi * m + idx[row * 3 + t]) * c + l], g * weight[row * 3 + t]);
  }
}

inline int flat_grid(long long total) {
  long long g = (total + kBlock - 1) / kBlock;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace

DH3D_API int dh3d_group_point_fwd(int b, int n, int c, int m, int nsample, const float *points,
                                  const int32_t *idx, float *out, void *stream) {
  DH3D_REQUIRE(points && idx && out && b > 0 && n > 0 && c > 0 && m > 0 && nsample > 0);
  const long long rows = (long long)b * m * nsample;
  if (c % 4 == 0)
    hipLaunchKernelGGL(group_point_fwd4_kernel, dim3(flat_grid(rows * (c / 4))), dim3(kBlock), 0, (hipStream_t)stream,
                       rows, n, c / 4, m * nsample, reinterpret_cast<const float4 *>(points), idx,
                       reinterpret_cast<float4 *>(out));
  else
    hipLaunchKernelGGL(group_point_fwd_kernel, dim3(flat_grid(rows * c)), dim3(kBlock), 0,
                       (hipStream_t)stream, rows, n, c, m * nsample, points, idx, out);
  return dh3d_launch_status();
}

DH3D_API int dh3d_group_point_bwd(int b, int n, int c, int m, int nsample, const float *grad_out,
                                  const int32_t *idx, float *grad_points, void *stream) {
  DH3D_REQUIRE(grad_out && idx && grad_points && b > 0 && n > 0 && c > 0 && m > 0 && nsample > 0);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(grad_points, 0, sizeof(float) * (size_t)b * n * c, s) != hipSuccess)
    return DH3D_ERR_LAUNCH;
  const long long rows = (long long)b * m * nsample;
  hipLaunchKernelGGL(group_point_bwd_kernel, dim3(flat_grid(rows * c)), dim3(kBlock), 0, s, rows, n, c,
                     m * nsample, grad_out, idx, grad_points);
  return dh3d_launch_status();
}

DH3D_API int dh3d_three_nn(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist,
                           int32_t *idx, void *stream) {
  DH3D_REQUIRE(xyz1 && xyz2 && dist && idx && b > 0 && n > 0 && m > 0);
  DH3D_SUPPORTED(b <= 65535);
  hipLaunchKernelGGL(three_nn_kernel, dim3(dh3d_cdiv(n, 64), b), dim3(kBlock), 0,
                     (hipStream_t)stream, n, m, xyz1, xyz2, dist, idx);
  return dh3d_launch_status();
}

DH3D_API int dh3d_three_nn_sorted(int b, int n, int m, const float *sorted1, const float *gbox1,
                                  const float *sorted2, const float *gbox2, float *dist, int32_t *idx,
                                  void *stream) {
  DH3D_REQUIRE(sorted1 && sorted2 && dist && idx && b > 0 && n > 0 && m > 0);
  DH3D_SUPPORTED(b <= 65535);
  if (m <= kNNChunk && m >= 128 && gbox1 && gbox2) {  // the sampled set fits LDS: candidate groups pruned by their boxes
    hipLaunchKernelGGL(three_nn_pruned_kernel, dim3(dh3d_cdiv(n, 64), b), dim3(kBlock), 0, (hipStream_t)stream, n, m,
                       reinterpret_cast<const float4 *>(sorted1), gbox1, reinterpret_cast<const float4 *>(sorted2), gbox2,
                       dist, idx);
    return dh3d_launch_status();
  }
  hipLaunchKernelGGL(three_nn_sorted_kernel, dim3(dh3d_cdiv(n, 64), b), dim3(kBlock), 0, (hipStream_t)stream, n, m,
                     reinterpret_cast<const float4 *>(sorted1), reinterpret_cast<const float4 *>(sorted2), dist, idx);
  return dh3d_launch_status();
}

DH3D_API int dh3d_three_nn_cells(int b, int n, int m, const float *sorted1, const float *gbox1, const float *sorted2,
                                 const float *gbox2, const int32_t *cells2, float *dist, int32_t *idx, void *stream) {
  DH3D_REQUIRE(sorted1 && sorted2 && dist && idx && b > 0 && n > 0 && m > 0);
  DH3D_SUPPORTED(b <= 65535);
  if (cells2 && gbox1 && m <= kNNChunk && m >= 128 && n <= 16384) {  // candidates through the sampled set's cell table
    const dim3 grid(dh3d_cdiv(n, 64), b);
    const float4 *s1 = reinterpret_cast<const float4 *>(sorted1), *s2 = reinterpret_cast<const float4 *>(sorted2);
    if (nn3_cell_drop(m) == 4)
      hipLaunchKernelGGL(three_nn_pruned_kernel_cells<4>, grid, dim3(kBlock), 0, (hipStream_t)stream, n, m, s1, gbox1, s2,
                         cells2, dist, idx);
    else
      hipLaunchKernelGGL(three_nn_pruned_kernel_cells<3>, grid, dim3(kBlock), 0, (hipStream_t)stream, n, m, s1, gbox1, s2,
                         cells2, dist, idx);
    return dh3d_launch_status();
  }
  return dh3d_three_nn_sorted(b, n, m, sorted1, gbox1, sorted2, gbox2, dist, idx, stream);
}

DH3D_API int dh3d_three_interpolate_fwd(int b, int m, int c, int n, const float *points,
                                        const int32_t *idx, const float *weight, float *out,
                                        void *stream) {
  DH3D_REQUIRE(points && idx && weight && out && b > 0 && m > 0 && c > 0 && n > 0);
  const long long rows = (long long)b * n;
  hipStream_t s = (hipStream_t)stream;
  if (c % 4 == 0)
    hipLaunchKernelGGL((three_interp_fwd_kernel<false, 4>), dim3(flat_grid(rows * (c / 4))), dim3(kBlock),
                       0, s, rows, n, m, c, points, idx, weight, out);
  else
    hipLaunchKernelGGL((three_interp_fwd_kernel<false, 1>), dim3(flat_grid(rows * c)), dim3(kBlock), 0, s,
                       rows, n, m, c, points, idx, weight, out);
  return dh3d_launch_status();
}

DH3D_API int dh3d_three_interpolate_idw_fwd(int b, int m, int c, int n, const float *points,
                                            const int32_t *idx, const float *dist, float *out,
                                            void *stream) {
  DH3D_REQUIRE(points && idx && dist && out && b > 0 && m > 0 && c > 0 && n > 0);
  const long long rows = (long long)b * n;
  hipStream_t s = (hipStream_t)stream;
  if (c % 4 == 0)
    hipLaunchKernelGGL((three_interp_fwd_kernel<true, 4>), dim3(flat_grid(rows * (c / 4))), dim3(kBlock), 0, s,
                       rows, n, m, c, points, idx, dist, out);
  else
    hipLaunchKernelGGL((three_interp_fwd_kernel<true, 1>), dim3(flat_grid(rows * c)), dim3(kBlock), 0, s,
                       rows, n, m, c, points, idx, dist, out);
  return dh3d_launch_status();
}

DH3D_API int dh3d_three_interpolate_bwd(int b, int n, int c, int m, const float *grad_out,
                                        const int32_t *idx, const float *weight, float *grad_points,
                                        void *stream) {
  DH3D_REQUIRE(grad_out && idx && weight && grad_points && b > 0 && m > 0 && c > 0 && n > 0);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(grad_points, 0, sizeof(float) * (size_t)b * m * c, s) != hipSuccess)
    return DH3D_ERR_LAUNCH;
  const long long rows = (long long)b * n;
  hipLaunchKernelGGL(three_interp_bwd_kernel, dim3(flat_grid(rows * c)), dim3(kBlock), 0, s, rows, n, m, c,
                     grad_out, idx, weight, grad_points);
  return dh3d_launch_status();
}
