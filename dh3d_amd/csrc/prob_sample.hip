// ProbSample (tf_ops/sampling: tf_sampling.py:15-26, tf_sampling.cpp:65-92, tf_sampling_g.cu:7-104) for gfx950, and its
// seeded form: m indices a row, drawn with probability proportional to a row of n weights.  The op has no CPU twin
// upstream; the contract is the reference kernels' own arithmetic, restated here (all values f32, every operation rounded
// on its own -- csrc/Makefile EXACT, no contraction) and in tests/prob_sample_reference.py.
//
// CUMULATIVE SUMS of a row w[0 .. n-1] (cumsumKernel, tf_sampling_g.cu:7-88), in chunks of 8192 entries (:14-15), the
// running sum R and its compensation C starting at 0 (:13):
//   a chunk of L entries has G = ceil(L / 4) quads (:16-17).  A full quad (a, b, c, d) (:19-32):
//       l0 = a    l1 = b + a    t = d + c    l2 = c + l1    l3 = t + l1    s[g] = l3
//   the partial last quad of 1 .. 3 entries (:33-42): v = 0, then v += x in order; l_i the running v, s[g] the last v.
//   The tree over s[0 .. G-1], in place:
//       up-sweep (:45-55)    for u = 0, 1, .. while 2^(u+1) <= G, for k < floor(G / 2^(u+1)):
//                                s[(2k+2) 2^u - 1] += s[(2k+1) 2^u - 1]
//       down-sweep (:56-66)  from the last such u down to 0, for k < floor((G - 2^u) / 2^(u+1)):
//                                s[(2k+3) 2^u - 1] += s[(2k+2) 2^u - 1]
//   after which s[g] is the inclusive sum of the quads 0 .. g.  For the quads g >= 1: l_i += s[g-1] (:68-76).
//   cum = l_i + R (:78-80).  Then t = s[G-1] + C, R' = R + t, C = t - (R' - R), R = R' (:81-84).
// The sums are NOT a sequential prefix sum (most entries differ from one in the last bit) and they are not monotone: the
// last entry of quad g is l3 + s[g-1] while the first of quad g+1 is a + s[g], and s[g] reaches the same quads through
// another tree, so cum may step down by an ulp between two quads on non-negative weights.
//
// SEARCH, one per draw (binarysearchKernel, :90-104): P = the smallest power of two >= n, q = r_in * cum[n-1] (one
// multiply), r = n-1; for k = P, P/2, .. 1: if r >= k and cum[r-k] >= q then r -= k.  A fixed halving walk that never
// assumes order: on a non-monotone row it is not a searchsorted.  A draw of 0 walks down to index 0 whatever its weight.
//
//   prob_cumsum_kernel  grid b, 1024 threads, the chunk loop serial as upstream.  A thread keeps its two quads of a chunk
//                       in registers (upstream: two LDS arrays and a barrier per tree level, 23 a chunk).  Lane = quad: the
//                       64 quads of a wave are one aligned segment of s, so the levels u <= 5 of both sweeps stay inside a
//                       wave (a lane shift by 2^u); the levels u >= 6 touch only the last quad of every segment, 32 values
//                       that go through LDS once and that every wave walks for itself.  Two barriers a chunk.  Every
//                       addition has the operands stated above -- only who performs it differs: a down-sweep step whose
//                       left operand is the last quad of the previous segment takes it from those 32 (final by then).
//   prob_search_kernel  a thread a draw, the walk's 1 + log2(n) reads dependent on one another.  n <= 8192 (one chunk): grid
//                       (ceil(m / 1024), b), the row's sums copied from temp to LDS (32 KiB) once per workgroup, four draws a
//                       thread -- the chain then costs LDS latencies.  Longer rows: grid (ceil(m / 256), b), the sums read
//                       from temp in global memory; the first levels of every walk of a row touch the same few entries.
//                       (Measured at n = 8192 only; the rule is "one chunk", not a tuned threshold.)
// The seeded form draws r_in on the device (include/dh3d_hip.h "Training batches", stream 16) and takes a count per row.
#include "common.h"
#include "keys.h"

namespace {

typedef unsigned long long u64;

constexpr int kScanThreads = 1024;
constexpr int kChunk = 8192;                      // tf_sampling_g.cu:8,14  BlockSize * 4
constexpr int kQuads = kChunk / 4;
constexpr int kQuadsPer = kQuads / kScanThreads;  // quads of a chunk a thread holds
constexpr int kWaves = kScanThreads / 64;
constexpr int kSegs = kQuads / 64;                // segments of 64 quads: one per wave and p
constexpr int kSearchThreads = 256;
constexpr int kStagedDraws = 4;                   // draws a thread when the row is staged in LDS
constexpr int kMaxBatch = 65535;                  // grid.y
constexpr int kMaxN = 1 << 20, kMaxM = 1 << 20;
constexpr unsigned kDrawStream = 16;              // include/dh3d_hip.h lists the streams

__device__ __forceinline__ int row_count(const int32_t *count, int b, int n) { return count ? clamp_count(count[b], n) : n; }

// does quad index i (or, one level up, segment index i) receive an addition at level u of the up- / down-sweep?  The
// reference's loop bounds (k < floor(G / 2^(u+1)), k < floor((G - 2^u) / 2^(u+1))) are "the receiving index is < G".
__device__ __forceinline__ bool up_target(int i, int u) { return ((i + 1) & ((2 << u) - 1)) == 0; }
__device__ __forceinline__ bool down_target(int i, int u) { return ((i + 1) & ((2 << u) - 1)) == (1 << u) && i + 1 >= (3 << u); }

__global__ __launch_bounds__(kScanThreads) void prob_cumsum_kernel(int n, const float *__restrict__ inp,
                                                                   const int32_t *__restrict__ count,
                                                                   float *__restrict__ temp) {
  __shared__ float s_top[kSegs];  // s[64 j + 63]: the last quad of segment j
  __shared__ float s_last;        // s[G-1] after the tree
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = row_count(count, b, n);
  const float *w = inp + (size_t)b * n;
  float *cum = temp + (size_t)b * n;
  float run = 0.f, comp = 0.f;
  for (int j = 0; j < nb; j += kChunk) {
    const int L = min(nb - j, kChunk), G = (L + 3) >> 2;
    float l[kQuadsPer][4], v[kQuadsPer];
#pragma unroll
    for (int p = 0; p < kQuadsPer; ++p) {
      const int g = tid + p * kScanThreads, k = 4 * g;
      v[p] = 0.f;
      if (k + 3 < L) {
        const float a = w[j + k], bb = w[j + k + 1], c = w[j + k + 2], d = w[j + k + 3];
        const float l1 = bb + a, t = d + c;
        l[p][0] = a, l[p][1] = l1, l[p][2] = c + l1, l[p][3] = t + l1;
        v[p] = l[p][3];
      } else if (k < L) {
        float x = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          if (k + i < L) x += w[j + k + i];
          l[p][i] = x;
        }
        l[p][3] = x;
        v[p] = x;
      }
      // up-sweep, u = 0 .. 5: inside the segment
#pragma unroll
      for (int u = 0; u < 6; ++u) {
        const float o = __shfl_up(v[p], 1 << u, 64);
        if (up_target(lane, u) && g < G) v[p] += o;
      }
      if (lane == 63) s_top[wave + p * kWaves] = v[p];
    }
    __syncthreads();
    // both sweeps at u = 6 .. 10 on the 32 segment ends, a copy in every wave (lanes 0 .. 31)
    float t = lane < kSegs ? s_top[lane] : 0.f;
    const bool whole = lane < kSegs && 64 * lane + 63 < G;  // the segment's last quad exists
#pragma unroll
    for (int u = 0; u < 5; ++u) {
      const float o = __shfl_up(t, 1 << u, 64);
      if (whole && up_target(lane, u)) t += o;
    }
#pragma unroll
    for (int u = 4; u >= 0; --u) {
      const float o = __shfl_up(t, 1 << u, 64);
      if (whole && down_target(lane, u)) t += o;
    }
#pragma unroll
    for (int p = 0; p < kQuadsPer; ++p) {
      const int seg = wave + p * kWaves, g = tid + p * kScanThreads, k = 4 * g;
      const float own = __shfl(t, seg, 64), prev = __shfl(t, seg > 0 ? seg - 1 : 0, 64);  // s[64 seg + 63], s[64 seg - 1]
      if (lane == 63 && g < G) v[p] = own;
      // down-sweep, u = 5 .. 0
#pragma unroll
      for (int u = 5; u >= 0; --u) {
        const float o = __shfl_up(v[p], 1 << u, 64);
        if (g < G && ((lane + 1) & ((2 << u) - 1)) == (1 << u)) {
          if (lane + 1 == (1 << u)) {
            if (seg > 0) v[p] += prev;  // (2k+2) 2^u - 1 is the previous segment's end
          } else {
            v[p] += o;
          }
        }
      }
      float before = __shfl_up(v[p], 1, 64);  // s[g-1]
      if (lane == 0) before = prev;
      if (k < L) {
        if (g > 0) {
#pragma unroll
          for (int i = 0; i < 4; ++i) l[p][i] += before;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (k + i < L) cum[j + k + i] = l[p][i] + run;
      }
      if (g == G - 1) s_last = v[p];
    }
    __syncthreads();
    const float tt = s_last + comp;
    const float r2 = run + tt;
    comp = tt - (r2 - run);
    run = r2;
  }
  for (int i = nb + tid; i < n; i += kScanThreads) cum[i] = 0.f;  // behind the row's count: no sums, but every element is written
}

// One draw on the sums of one row, in LDS or in global memory (the caller's pointer decides after inlining).
__device__ __forceinline__ int halving_walk(const float *cum, int nb, int base, float q) {
  int r = nb - 1;
  for (int k = base; k >= 1; k >>= 1)
    if (r >= k && cum[r - k] >= q) r -= k;
  return r;
}

// kStaged: the row fits one chunk and is copied to LDS first; a workgroup then serves kStagedDraws draws a thread.
template <bool kSeeded, bool kStaged>
__global__ __launch_bounds__(kSearchThreads) void prob_search_kernel(int n, int m, const float *__restrict__ temp,
                                                                     const float *__restrict__ inp_r,
                                                                     const int32_t *__restrict__ count,
                                                                     const u64 *__restrict__ seed, int32_t *__restrict__ out) {
  __shared__ float s_cum[kStaged ? kChunk : 1];
  constexpr int kPer = kStaged ? kStagedDraws : 1;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int nb = row_count(count, b, n);
  const float *cum = temp + (size_t)b * n;
  if (kStaged) {
    for (int i = tid; i < nb; i += kSearchThreads) s_cum[i] = cum[i];
    __syncthreads();
  }
  const float total = nb == 0 ? 0.f : (kStaged ? s_cum[nb - 1] : cum[nb - 1]);
  const bool none = kSeeded && !(total > 0.f);  // an empty row, or nothing to draw from
  const u64 h = kSeeded ? stream_h(*seed, kDrawStream, (unsigned)b) : 0ull;
  int base = 1;
  while (base < nb) base <<= 1;
#pragma unroll
  for (int d = 0; d < kPer; ++d) {
    const int j = (blockIdx.x * kPer + d) * kSearchThreads + tid;
    if (j >= m) break;
    const size_t at = (size_t)b * m + j;
    if (none) {
      out[at] = -1;
      continue;
    }
    const float r_in = kSeeded ? (float)((splitmix64(h + (u64)j) >> 40) + 1ull) * 0x1p-24f  // (0, 1], exact
                               : inp_r[at];
    const float q = r_in * total;
    out[at] = kStaged ? halving_walk(s_cum, nb, base, q) : halving_walk(cum, nb, base, q);
  }
}

template <bool kSeeded>
int launch_search(int b, int n, int m, const float *temp, const float *inp_r, const int32_t *count, const u64 *seed, int32_t *out,
                  hipStream_t stream) {
  if (n <= kChunk)
    hipLaunchKernelGGL((prob_search_kernel<kSeeded, true>), dim3(dh3d_cdiv(m, kStagedDraws * kSearchThreads), b),
                       dim3(kSearchThreads), 0, stream, n, m, temp, inp_r, count, seed, out);
  else
    hipLaunchKernelGGL((prob_search_kernel<kSeeded, false>), dim3(dh3d_cdiv(m, kSearchThreads), b), dim3(kSearchThreads), 0,
                       stream, n, m, temp, inp_r, count, seed, out);
  return dh3d_launch_status();
}

}  // namespace

DH3D_API int dh3d_prob_sample(int b, int n, int m, const float *inp_p, const float *inp_r, float *temp, int32_t *out,
                              void *stream) {
  DH3D_REQUIRE(b > 0 && n > 0 && m > 0);
  DH3D_REQUIRE(inp_p && inp_r && temp && out);
  DH3D_SUPPORTED(b <= kMaxBatch && n <= kMaxN && m <= kMaxM);
  hipLaunchKernelGGL(prob_cumsum_kernel, dim3(b), dim3(kScanThreads), 0, (hipStream_t)stream, n, inp_p, (const int32_t *)nullptr,
                     temp);
  if (dh3d_launch_status() != DH3D_OK) return DH3D_ERR_LAUNCH;
  return launch_search<false>(b, n, m, temp, inp_r, nullptr, nullptr, out, (hipStream_t)stream);
}

DH3D_API int dh3d_prob_sample_seeded(int b, int n, int m, const float *inp_p, const int32_t *count,
                                     const unsigned long long *seed, float *temp, int32_t *out, void *stream) {
  DH3D_REQUIRE(b > 0 && n > 0 && m > 0);
  DH3D_REQUIRE(inp_p && seed && temp && out);
  DH3D_SUPPORTED(b <= kMaxBatch && n <= kMaxN && m <= kMaxM);
  hipLaunchKernelGGL(prob_cumsum_kernel, dim3(b), dim3(kScanThreads), 0, (hipStream_t)stream, n, inp_p, count, temp);
  if (dh3d_launch_status() != DH3D_OK) return DH3D_ERR_LAUNCH;
  return launch_search<true>(b, n, m, temp, nullptr, count, seed, out, (hipStream_t)stream);
}
