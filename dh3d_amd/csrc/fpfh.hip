// FPFH descriptors (Fast Point Feature Histograms, Rusu et al. 2009) of P clouds from given normals and neighbour lists for
// gfx950 (include/dh3d_hip.h dh3d_spfh_counts / dh3d_fpfh state the rule: 3 x 11 bins, weights 1 / d^2, float64 on the exact
// float32 inputs).  No search here: the ids come from the exact kNN, the normals from dh3d_estimate_normals or the caller.
//   spfh_counts_kernel<G>  lane = one neighbour of one point; G = 4 / 8 / 16 / 32 / 64 lanes per point (the power of two
//                   that holds K), 256 / G points per workgroup.  One gather instruction fetches the rows of a point's
//                   whole list (two 12-byte reads per lane: x_j, n_j; all four rows of a pair are requested before any
//                   test on them, one round trip behind the id); the pair features stay in registers; the three bins
//                   of a usable pair are three LDS counter increments (no per-lane histogram, no dynamic register index).
//                   Then the workgroup packs its counters into 36-byte rows and stores them as dwords, coalesced.
//   fpfh_kernel     28 output points per workgroup.  Phase A, lane = (point, neighbour): the near test, w = 1 / d2 and
//                   100 / m_j (one byte of the neighbour's count row) into LDS.  Phase B, lane = (point, one of the 9 dwords
//                   of a count row): K independent 4-byte gathers of that dword (the 9 lanes of a point read one 36-byte
//                   row), four float64 sums per lane in list order.  Phase C, four lanes per point: the three block sums in
//                   ascending order from LDS and their scales, and 100 / m_i.  Phase D, lane = one output column: the scaled
//                   sum plus the point's own SPFH, one rounding to float32, coalesced stores.
// What bounds them is measured in DESIGN.md section 7: mostly VALU issue (the rule's float64 arithmetic), with the gathers
// only partly hidden under it.
// One launch each on the caller's stream, no workspace, no atomics on global memory: graph-capturable.
// Compiled without contraction (csrc/Makefile EXACT): the rule rounds every operation on its own.
#include <math.h>

#include "common.h"
#include "keys.h"

namespace {

constexpr int kMaxPoints = 131072;
constexpr int kMaxClouds = 65535;
constexpr int kMaxK = 64;
constexpr int kThreads = 256;
constexpr int kRow = 36;         // bytes of a count row = floats of an output row
constexpr int kRowWords = 9;
constexpr int kBins = 11;
constexpr int kPts2 = 28;        // output points per workgroup of fpfh_kernel: 28 * 9 = 252 lanes in phase B

struct __attribute__((packed, aligned(4))) Row3 {  // three floats at any element stride: one 12-byte read
  float x, y, z;
};

struct D3 {
  double a, b, c;
};

__device__ __forceinline__ D3 load3(const float *base, long long row, long long stride) {
  const Row3 r = *reinterpret_cast<const Row3 *>(base + row * stride);
  return D3{(double)r.x, (double)r.y, (double)r.z};
}
__device__ __forceinline__ double dot3(const D3 &u, const D3 &v) { return (u.a * v.a + u.b * v.b) + u.c * v.c; }
__device__ __forceinline__ D3 cross3(const D3 &u, const D3 &v) {
  return D3{u.b * v.c - u.c * v.b, u.c * v.a - u.a * v.c, u.a * v.b - u.b * v.a};
}
__device__ __forceinline__ int bin11(double s) {
  const double f = floor(s);
  return f < 0.0 ? 0 : (f > 10.0 ? 10 : (int)f);
}

// d = x_j - x_i and its squared length; the pair is near iff the return value is true
__device__ __forceinline__ bool near_pair(const float *base, long long stride, int i, int j, int n, bool has_r, double r2, D3 *d,
                                          double *d2) {
  if (j < 0 || j >= n || j == i) return false;
  const D3 xi = load3(base, i, stride), xj = load3(base, j, stride);
  *d = D3{xj.a - xi.a, xj.b - xi.b, xj.c - xi.c};
  *d2 = dot3(*d, *d);
  return *d2 > 0.0 && (!has_r || *d2 <= r2);
}

template <int G>
__global__ __launch_bounds__(kThreads) void spfh_counts_kernel(const float *__restrict__ xyz, long long xs,
                                                               const float *__restrict__ nrm, long long ns, int N,
                                                               const int32_t *__restrict__ count,
                                                               const int32_t *__restrict__ nbr, int K, int has_r, double r2,
                                                               uint32_t *__restrict__ counts) {
  constexpr int kPts = kThreads / G;
  __shared__ uint32_t s_hist[kPts * kRow];  // per point: 33 bin counters, m, two unused
  const int p = blockIdx.y, tid = threadIdx.x;
  const int g = tid / G, k = tid % G;
  const int i0 = blockIdx.x * kPts, i = i0 + g;
  for (int t = tid; t < kPts * kRow; t += kThreads) s_hist[t] = 0u;
  __syncthreads();
  const int n = count ? clamp_count(count[p], N) : N;
  if (i < n && k < K) {
    const float *base = xyz + (long long)p * N * xs;
    const float *nbase = nrm + (long long)p * N * ns;
    const int j = nbr[((long long)p * N + i) * K + k];
    if (j >= 0 && j < n && j != i) {
      // the four rows of a pair are fetched together, before any test on them: one memory round trip behind the id
      const D3 xi = load3(base, i, xs), xj = load3(base, j, xs), ni = load3(nbase, i, ns), nj = load3(nbase, j, ns);
      const D3 d = D3{xj.a - xi.a, xj.b - xi.b, xj.c - xi.c};
      const double d2 = dot3(d, d);
      const int near = (int)(d2 > 0.0) & (int)(!has_r || d2 <= r2);
      if (near & (int)(dot3(ni, ni) > 0.0) & (int)(dot3(nj, nj) > 0.0)) {  // (no short circuit: nothing is fetched late)
        const double len = sqrt(d2);
        const double a1 = dot3(ni, d) / len, a2 = dot3(nj, d) / len;
        const bool swap = fabs(a1) < fabs(a2);
        const D3 n1 = swap ? nj : ni, n2 = swap ? ni : nj;
        const D3 dd = swap ? D3{-d.a, -d.b, -d.c} : d;
        const double f3 = swap ? -a2 : a1;
        D3 v = cross3(dd, n1);
        const double vn = sqrt(dot3(v, v));
        if (vn > 0.0) {
          v = D3{v.a / vn, v.b / vn, v.c / vn};
          const D3 w = cross3(n1, v);
          const double f2 = dot3(v, n2);
          const double f1 = atan2(dot3(w, n2), dot3(n1, n2));
          const double s1 = (f1 + M_PI) * (11.0 / (2.0 * M_PI)), s2 = (f2 + 1.0) * 5.5, s3 = (f3 + 1.0) * 5.5;
          uint32_t *h = s_hist + g * kRow;
          atomicAdd(h + bin11(s1), 1u);  // LDS counters
          atomicAdd(h + kBins + bin11(s2), 1u);
          atomicAdd(h + 2 * kBins + bin11(s3), 1u);
          atomicAdd(h + 3 * kBins, 1u);
        }
      }
    }
  }
  __syncthreads();
  for (int t = tid; t < kPts * kRowWords; t += kThreads) {
    const int pt = t / kRowWords, q = t % kRowWords;
    if (i0 + pt < N) {
      const uint32_t *h = s_hist + pt * kRow + q * 4;  // every counter is at most K <= 64: one byte each
      counts[((long long)p * N + i0 + pt) * kRowWords + q] = h[0] | (h[1] << 8) | (h[2] << 16) | (h[3] << 24);
    }
  }
}

__global__ __launch_bounds__(kThreads) void fpfh_kernel(const float *__restrict__ xyz, long long xs, int N,
                                                        const int32_t *__restrict__ count, const int32_t *__restrict__ nbr,
                                                        int K, const uint32_t *__restrict__ counts,
                                                        const int32_t *__restrict__ ids, int M, int has_r, double r2,
                                                        float *__restrict__ out) {
  extern __shared__ double s_dyn[];
  double *s_w = s_dyn;                                     // [kPts2 * K]  1 / d2 of a near pair, else 0
  double *s_s = s_w + kPts2 * K;                           // [kPts2 * K]  100 / m_j, 0 when m_j = 0 or the pair is not near
  double *s_acc = s_s + kPts2 * K;                         // [kPts2 * 36]
  double *s_f = s_acc + kPts2 * kRow;                      // [kPts2 * 4]  scale_0..2 and 100 / m_i of an output point
  int *s_j = reinterpret_cast<int *>(s_f + kPts2 * 4);     // [kPts2 * K]  the row to read (0 for a pair that is not near)
  int *s_i = s_j + kPts2 * K;                              // [kPts2]      the point of an output row, -1: a zero row
  const int p = blockIdx.y, tid = threadIdx.x, r0 = blockIdx.x * kPts2;
  const int n = count ? clamp_count(count[p], N) : N;
  const uint32_t *crow = counts + (long long)p * N * kRowWords;
  const uint8_t *cbyte = reinterpret_cast<const uint8_t *>(crow);
  if (tid < kPts2) {
    int i = -1;
    if (r0 + tid < M) {
      i = ids ? ids[(long long)p * M + r0 + tid] : r0 + tid;
      if (i < 0 || i >= n) i = -1;
    }
    s_i[tid] = i;
  }
  __syncthreads();
  const float *base = xyz + (long long)p * N * xs;
  for (int t = tid; t < kPts2 * K; t += kThreads) {
    const int pt = t / K, k = t - pt * K, i = s_i[pt];
    int row = 0;
    double w = 0.0, s = 0.0;
    if (i >= 0) {
      const int j = nbr[((long long)p * N + i) * K + k];
      D3 d;
      double d2;
      if (near_pair(base, xs, i, j, n, has_r != 0, r2, &d, &d2)) {
        const int mj = cbyte[(long long)j * kRow + 3 * kBins];
        row = j;
        w = 1.0 / d2;
        s = mj ? 100.0 / (double)mj : 0.0;
      }
    }
    s_j[t] = row; s_w[t] = w; s_s[t] = s;
  }
  __syncthreads();
  if (tid < kPts2 * kRowWords) {
    const int pt = tid / kRowWords, q = tid - pt * kRowWords;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (s_i[pt] >= 0) {  // (n > 0 here, so row 0 of a pair that is not near can be read; its terms are w * (c * 0) = 0)
#pragma unroll 4
      for (int k = 0; k < K; ++k) {
        const uint32_t c = crow[(long long)s_j[pt * K + k] * kRowWords + q];
        const double w = s_w[pt * K + k], s = s_s[pt * K + k];
        a0 = a0 + w * ((double)(c & 255u) * s);
        a1 = a1 + w * ((double)((c >> 8) & 255u) * s);
        a2 = a2 + w * ((double)((c >> 16) & 255u) * s);
        a3 = a3 + w * ((double)(c >> 24) * s);
      }
    }
    double *a = s_acc + pt * kRow + q * 4;
    a[0] = a0; a[1] = a1; a[2] = a2; a[3] = a3;
  }
  __syncthreads();
  if (tid < kPts2 * 4) {  // per point: the three block scales and 100 / m_i, once instead of once per column
    const int pt = tid >> 2, t = tid & 3, i = s_i[pt];
    double f = 0.0;
    if (i >= 0) {
      if (t < 3) {
        const double *a = s_acc + pt * kRow + t * kBins;
        double S = 0.0;
#pragma unroll
        for (int e = 0; e < kBins; ++e) S = S + a[e];
        f = S > 0.0 ? 100.0 / S : 0.0;
      } else {
        const int mi = cbyte[(long long)i * kRow + 3 * kBins];
        f = mi ? 100.0 / (double)mi : 0.0;
      }
    }
    s_f[tid] = f;
  }
  __syncthreads();
  for (int t = tid; t < kPts2 * kRow; t += kThreads) {
    const int pt = t / kRow, c = t - pt * kRow;
    if (r0 + pt >= M) break;
    const int i = s_i[pt];
    float o = 0.f;
    if (i >= 0 && c < 3 * kBins) {
      const double own = (double)cbyte[(long long)i * kRow + c] * s_f[pt * 4 + 3];
      o = (float)(s_acc[pt * kRow + c] * s_f[pt * 4 + c / kBins] + own);
    }
    out[((long long)p * M + r0 + pt) * kRow + c] = o;
  }
}

size_t fpfh_lds_bytes(int K) { return (size_t)kPts2 * K * 20 + (size_t)kPts2 * (kRow + 4) * 8 + (size_t)kPts2 * 4; }

}  // namespace

DH3D_API int dh3d_spfh_counts(const float *xyz, long long xyz_stride, const float *normals, long long normals_stride,
                              const int32_t *count, const int32_t *nbr, int P, int N, int K, double max_dist, uint8_t *counts,
                              void *stream) {
  DH3D_REQUIRE(xyz && normals && nbr && counts && ((uintptr_t)counts & 3) == 0);
  DH3D_REQUIRE(P > 0 && N > 0 && K >= 1 && K <= kMaxK && xyz_stride >= 3 && normals_stride >= 3);
  DH3D_SUPPORTED(P <= kMaxClouds && N <= kMaxPoints);
  const int has_r = max_dist > 0.0;
  const double r2 = has_r ? max_dist * max_dist : 0.0;
  uint32_t *out = reinterpret_cast<uint32_t *>(counts);
#define DH3D_SPFH_LAUNCH(G)                                                                                                   \
  hipLaunchKernelGGL(spfh_counts_kernel<G>, dim3(dh3d_cdiv(N, kThreads / G), P), dim3(kThreads), 0, (hipStream_t)stream, xyz, \
                     xyz_stride, normals, normals_stride, N, count, nbr, K, has_r, r2, out)
  if (K <= 4) DH3D_SPFH_LAUNCH(4);
  else if (K <= 8) DH3D_SPFH_LAUNCH(8);
  else if (K <= 16) DH3D_SPFH_LAUNCH(16);
  else if (K <= 32) DH3D_SPFH_LAUNCH(32);
  else DH3D_SPFH_LAUNCH(64);
#undef DH3D_SPFH_LAUNCH
  return dh3d_launch_status();
}

DH3D_API int dh3d_fpfh(const float *xyz, long long xyz_stride, const int32_t *count, const int32_t *nbr, const uint8_t *counts,
                       const int32_t *ids, int P, int N, int K, int M, double max_dist, float *fpfh, void *stream) {
  DH3D_REQUIRE(xyz && nbr && counts && fpfh && ((uintptr_t)counts & 3) == 0);
  DH3D_REQUIRE(P > 0 && N > 0 && M > 0 && K >= 1 && K <= kMaxK && xyz_stride >= 3 && (ids || M == N));
  DH3D_SUPPORTED(P <= kMaxClouds && N <= kMaxPoints && M <= kMaxPoints);
  const int has_r = max_dist > 0.0;
  const double r2 = has_r ? max_dist * max_dist : 0.0;
  hipLaunchKernelGGL(fpfh_kernel, dim3(dh3d_cdiv(M, kPts2), P), dim3(kThreads), fpfh_lds_bytes(K), (hipStream_t)stream, xyz,
                     xyz_stride, N, count, nbr, K, reinterpret_cast<const uint32_t *>(counts), ids, M, has_r, r2, fpfh);
  return dh3d_launch_status();
}
