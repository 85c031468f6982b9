// Surface normals of P clouds from given neighbour lists for gfx950 (include/dh3d_hip.h dh3d_estimate_normals states the
// rule; external/findPointNormals.m of the reference's evaluation is the anchor): per point the float64 covariance of its
// usable neighbours, the eigenvector of the smallest eigenvalue by cyclic Jacobi (rigid_fit.h smallest_eigenvector_3), the
// flip towards the viewpoint, one rounding to float32.  No search here: the ids come from the exact kNN.
//   normals_kernel  lane = point, 256 per workgroup.  Two walks over the K ids of the lane's row (the mean, then the six
//                   centred sums), each neighbour row gathered as one 12-byte read; the covariance and the Jacobi stay in
//                   registers (no dynamic index).  The lanes of a wave read unrelated rows: the kernel is bound by those
//                   gathers (2 K per point), not by its ~200 float64 operations of the solve.
// One launch on the caller's stream, no workspace, no atomics: graph-capturable.
// Compiled without contraction (csrc/Makefile EXACT): the rule rounds every operation on its own.
#include <math.h>

#include "common.h"
#include "keys.h"
#include "rigid_fit.h"

namespace {

constexpr int kMaxPoints = 131072;
constexpr int kMaxClouds = 65535;
constexpr int kMaxK = 64;
constexpr int kThreads = 256;

struct __attribute__((packed, aligned(4))) Row3 {  // three floats at any element stride: one 12-byte read
  float x, y, z;
};

__global__ __launch_bounds__(kThreads) void normals_kernel(const float *__restrict__ xyz, long long stride, int N,
                                                           const int32_t *__restrict__ count,
                                                           const int32_t *__restrict__ nbr, int K, double v0, double v1,
                                                           double v2, float *__restrict__ normals,
                                                           float *__restrict__ curvature) {
  const int p = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= N) return;
  const int n = count ? clamp_count(count[p], N) : N;
  const float *base = xyz + (long long)p * N * stride;
  const int32_t *row = nbr + ((long long)p * N + i) * K;
  float o0 = 0.f, o1 = 0.f, o2 = 0.f, oc = 0.f;
  if (i < n) {
    int m = 0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < K; ++k) {
      const int id = row[k];
      if (id >= 0 && id < n) {
        const Row3 r = *reinterpret_cast<const Row3 *>(base + (long long)id * stride);
        s0 += (double)r.x; s1 += (double)r.y; s2 += (double)r.z;
        ++m;
      }
    }
    if (m >= 3) {
      const double dm = (double)m, c0 = s0 / dm, c1 = s1 / dm, c2 = s2 / dm;
      double C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // c00 c01 c02 c11 c12 c22
      for (int k = 0; k < K; ++k) {
        const int id = row[k];
        if (id >= 0 && id < n) {
          const Row3 r = *reinterpret_cast<const Row3 *>(base + (long long)id * stride);
          const double d0 = (double)r.x - c0, d1 = (double)r.y - c1, d2 = (double)r.z - c2;
          C[0] += d0 * d0; C[1] += d0 * d1; C[2] += d0 * d2;
          C[3] += d1 * d1; C[4] += d1 * d2; C[5] += d2 * d2;
        }
      }
#pragma unroll
      for (int e = 0; e < 6; ++e) C[e] = C[e] / dm;
      double lam[3], nv[3];
      const double low = smallest_eigenvector_3(C, lam, nv);
      const double sum = (lam[0] + lam[1]) + lam[2];
      if (sum > 0.0) {  // (not for 0, not for NaN)
        const Row3 x = *reinterpret_cast<const Row3 *>(base + (long long)i * stride);
        const double s = ((v0 - (double)x.x) * nv[0] + (v1 - (double)x.y) * nv[1]) + (v2 - (double)x.z) * nv[2];
        const bool flip = s < 0.0;
        o0 = (float)(flip ? -nv[0] : nv[0]);
        o1 = (float)(flip ? -nv[1] : nv[1]);
        o2 = (float)(flip ? -nv[2] : nv[2]);
        oc = (float)(low / sum);
      }
    }
  }
  float *dst = normals + ((long long)p * N + i) * 3;
  dst[0] = o0; dst[1] = o1; dst[2] = o2;
  curvature[(long long)p * N + i] = oc;
}

}  // namespace

DH3D_API int dh3d_estimate_normals(const float *xyz, long long xyz_stride, const int32_t *count, const int32_t *nbr, int P, int N,
                                   int K, const double *viewpoint, float *normals, float *curvature, void *stream) {
  DH3D_REQUIRE(xyz && nbr && viewpoint && normals && curvature);
  DH3D_REQUIRE(P > 0 && N > 0 && K > 0 && xyz_stride >= 3);
  DH3D_SUPPORTED(P <= kMaxClouds && N <= kMaxPoints && K <= kMaxK);
  hipLaunchKernelGGL(normals_kernel, dim3(dh3d_cdiv(N, kThreads), P), dim3(kThreads), 0, (hipStream_t)stream, xyz, xyz_stride,
                     N, count, nbr, K, viewpoint[0], viewpoint[1], viewpoint[2], normals, curvature);
  return dh3d_launch_status();
}
