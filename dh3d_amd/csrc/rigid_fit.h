// The float64 rigid fit of estimateRigidTransform.m that csrc/registration.hip (RANSAC trial models and the refit) and
// csrc/icp.hip (the fit of every ICP iteration) share: one copy, one set of roundings.  Both files are built without
// contraction (csrc/Makefile EXACT).  block_rigid_fit_256 is the fit of a workgroup over many pairs: RANSAC's refit on the
// inliers and the fit of a point-to-point ICP iteration.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

// B += A^T A for one centred pair (X anchor, Y positive): A = [0, (Y-X)^T; X-Y, crossTimesMatrix(Y+X)]
// (estimateRigidTransform.m); B holds the upper triangle b00 b01 b02 b03 b11 b12 b13 b22 b23 b33
__device__ __forceinline__ void accumulate_b(double *B, double x0, double x1, double x2, double y0, double y1, double y2) {
  const double d0 = x0 - y0, d1 = x1 - y1, d2 = x2 - y2;
  const double s0 = y0 + x0, s1 = y1 + x1, s2 = y2 + x2;
  // columns of A
  const double c0[4] = {0.0, d0, d1, d2};
  const double c1[4] = {-d0, 0.0, s2, -s1};
  const double c2[4] = {-d1, -s2, 0.0, s0};
  const double c3[4] = {-d2, s1, -s0, 0.0};
  const double *cols[4] = {c0, c1, c2, c3};
  int e = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = r; c < 4; ++c) {
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) v = v + cols[r][q] * cols[c][q];
      B[e++] += v;
    }
  }
}

// R (row-major 3x3) from the unit eigenvector of B's smallest eigenvalue (cyclic Jacobi, float64), quat2rot.m
__device__ void rotation_from_b(const double *Bu, double *R) {
  double a[4][4], v[4][4];
  int e = 0;
  for (int r = 0; r < 4; ++r)
    for (int c = r; c < 4; ++c) a[r][c] = a[c][r] = Bu[e++];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) v[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; ++sweep) {  // (converges in 5-6 sweeps)
    double off = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = r + 1; c < 4; ++c) off += a[r][c] * a[r][c];
    if (!(off > 0.0)) break;  // (also stops on NaN)
#pragma unroll
    for (int pp = 0; pp < 3; ++pp) {
#pragma unroll
      for (int qq = pp + 1; qq < 4; ++qq) {
        const double apq = a[pp][qq];
        if (fabs(apq) <= 1e-18 * (fabs(a[pp][pp]) + fabs(a[qq][qq]))) {  // negligible: drop it
          a[pp][qq] = a[qq][pp] = 0.0;
          continue;
        }
        // the rotation that zeroes a[pp][qq], in the rounding-friendly form of Numerical Recipes' jacobi (tau = s / (1 + c))
        const double theta = (a[qq][qq] - a[pp][pp]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
        a[pp][pp] -= t * apq;
        a[qq][qq] += t * apq;
        a[pp][qq] = a[qq][pp] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (k != pp && k != qq) {
            const double g = a[k][pp], h = a[k][qq];
            a[k][pp] = a[pp][k] = g - s * (h + g * tau);
            a[k][qq] = a[qq][k] = h + s * (g - h * tau);
          }
          const double g = v[k][pp], h = v[k][qq];
          v[k][pp] = g - s * (h + g * tau);
          v[k][qq] = h + s * (g - h * tau);
        }
      }
    }
  }
  double lam = a[0][0], q0 = v[0][0], q1 = v[1][0], q2 = v[2][0], q3 = v[3][0];  // (the first smallest; no dynamic index)
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    if (a[k][k] < lam) {
      lam = a[k][k];
      q0 = v[0][k]; q1 = v[1][k]; q2 = v[2][k]; q3 = v[3][k];
    }
  }
  R[0] = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3;
  R[1] = 2.0 * (q1 * q2 - q0 * q3);
  R[2] = 2.0 * (q1 * q3 + q0 * q2);
  R[3] = 2.0 * (q1 * q2 + q0 * q3);
  R[4] = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3;
  R[5] = 2.0 * (q2 * q3 - q0 * q1);
  R[6] = 2.0 * (q1 * q3 - q0 * q2);
  R[7] = 2.0 * (q2 * q3 + q0 * q1);
  R[8] = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
}

// The 3x3 twin of rotation_from_b's loop, for csrc/normals.hip: cyclic Jacobi on the symmetric C (upper triangle c00 c01 c02
// c11 c12 c22), the same rotation formulas and the same drop rule.  lam = the diagonal after the sweeps, in its places; n = the
// column of the accumulated rotations at the first smallest diagonal entry (unit up to the rotations' roundings); returns
// that entry.  Registers only: every index is a constant after unrolling.
__device__ __forceinline__ double smallest_eigenvector_3(const double *Cu, double *lam, double *n) {
  double a[3][3], v[3][3];
  int e = 0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = r; c < 3; ++c) a[r][c] = a[c][r] = Cu[e++];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; ++sweep) {  // (converges in 4-5 sweeps)
    const double off = (a[0][1] * a[0][1] + a[0][2] * a[0][2]) + a[1][2] * a[1][2];
    if (!(off > 0.0)) break;  // (also stops on NaN)
#pragma unroll
    for (int pp = 0; pp < 2; ++pp) {
#pragma unroll
      for (int qq = pp + 1; qq < 3; ++qq) {
        const double apq = a[pp][qq];
        if (fabs(apq) <= 1e-18 * (fabs(a[pp][pp]) + fabs(a[qq][qq]))) {  // negligible: drop it
          a[pp][qq] = a[qq][pp] = 0.0;
          continue;
        }
        const double theta = (a[qq][qq] - a[pp][pp]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
        a[pp][pp] -= t * apq;
        a[qq][qq] += t * apq;
        a[pp][qq] = a[qq][pp] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (k != pp && k != qq) {
            const double g = a[k][pp], h = a[k][qq];
            a[k][pp] = a[pp][k] = g - s * (h + g * tau);
            a[k][qq] = a[qq][k] = h + s * (g - h * tau);
          }
          const double g = v[k][pp], h = v[k][qq];
          v[k][pp] = g - s * (h + g * tau);
          v[k][qq] = h + s * (g - h * tau);
        }
      }
    }
  }
  lam[0] = a[0][0]; lam[1] = a[1][1]; lam[2] = a[2][2];
  double low = a[0][0];
  n[0] = v[0][0]; n[1] = v[1][0]; n[2] = v[2][0];
#pragma unroll
  for (int k = 1; k < 3; ++k) {
    if (lam[k] < low) {
      low = lam[k];
      n[0] = v[0][k]; n[1] = v[1][k]; n[2] = v[2][k];
    }
  }
  return low;
}

// The three eigenvalues of the symmetric C (upper triangle as above) in descending order l[0] >= l[1] >= l[2], for
// csrc/iss.hip: smallest_eigenvector_3's solve with the vector dropped (the compiler removes the rotations' products).
__device__ __forceinline__ void eigenvalues_3_descending(const double *Cu, double *l) {
  double d[3], n[3];
  smallest_eigenvector_3(Cu, d, n);
  double a = d[0], b = d[1], c = d[2], t;
  if (a < b) { t = a; a = b; b = t; }
  if (b < c) { t = b; b = c; c = t; }
  if (a < b) { t = a; a = b; b = t; }
  l[0] = a; l[1] = b; l[2] = c;
}

// t = xc - R yc
__device__ __forceinline__ void translation(const double *R, const double *xc, const double *yc, double *t) {
  for (int r = 0; r < 3; ++r) t[r] = xc[r] - (R[3 * r] * yc[0] + R[3 * r + 1] * yc[1] + R[3 * r + 2] * yc[2]);
}

// The least-squares fit of a 256-lane workgroup over the pairs of `slots` slots: pair(j, x, y) fills slot j's anchor x[3]
// and positive y[3] and returns true, or returns false for a slot without a pair.  Float64 sums, each lane over its slots
// j = lane, lane + 256, ... in order, then block_sums_256's fixed tree: the count and the centroids, then B over the centred
// pairs; lane 0 solves and writes the 3 x 4 rt.  Returns the number of pairs to every lane; fewer than 3 leave rt as it
// was (workgroup-uniform).  s_red: 40 doubles.
template <typename Pair>
__device__ __forceinline__ int block_rigid_fit_256(int slots, Pair pair, double *s_red, double *rt) {
  float x[3], y[3];
  double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // the count, the anchors, the positives
  for (int j = threadIdx.x; j < slots; j += 256) {
    if (pair(j, x, y)) {
      s[0] += 1.0;
      s[1] += x[0]; s[2] += x[1]; s[3] += x[2];
      s[4] += y[0]; s[5] += y[1]; s[6] += y[2];
    }
  }
  block_sums_256<7>(s, s_red);
  const int n = (int)s[0];
  if (n < 3) return n;
  const double xc[3] = {s[1] / (double)n, s[2] / (double)n, s[3] / (double)n};
  const double yc[3] = {s[4] / (double)n, s[5] / (double)n, s[6] / (double)n};
  double B[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = threadIdx.x; j < slots; j += 256) {
    if (pair(j, x, y)) accumulate_b(B, x[0] - xc[0], x[1] - xc[1], x[2] - xc[2], y[0] - yc[0], y[1] - yc[1], y[2] - yc[2]);
  }
  block_sums_256<10>(B, s_red);
  if (threadIdx.x == 0) {
    double Rf[9], tf[3];
    rotation_from_b(B, Rf);
    translation(Rf, xc, yc, tf);
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) rt[4 * r + k] = Rf[3 * r + k];
      rt[4 * r + 3] = tf[r];
    }
  }
  return n;
}

// The weighted fit of a 256-lane workgroup over `slots` pairs (the fit of every graduated non-convexity iteration,
// include/dh3d_hip.h dh3d_gnc_rigid): pair(j, X, Y) fills slot j's anchor X[3] and positive Y[3] in float64 and returns the
// pair's weight w.  W = sum w, cx = (sum w X) / W, cy = (sum w Y) / W, B = sum of w * (the pair's accumulate_b term on
// (X - cx, Y - cy)), R = rotation_from_b(B), t = cx - R cy.  Each lane sums its slots j = lane, lane + 256, ... in order,
// then block_sums_256's fixed tree; pair is called twice per slot (nothing is kept between the two passes).  Lane 0 solves
// and leaves R (row-major, 9) and t (3) in s_pose; every lane may read them on return (a barrier stands before it).
// s_red: 40 doubles, s_pose: 12 doubles; both may be used again right away.
template <typename Pair>
__device__ __forceinline__ void block_weighted_rigid_fit_256(int slots, Pair pair, double *s_red, double *s_pose) {
  double X[3], Y[3];
  double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // W, the weighted anchors, the weighted positives
  for (int j = threadIdx.x; j < slots; j += 256) {
    const double w = pair(j, X, Y);
    s[0] += w;
    s[1] += w * X[0]; s[2] += w * X[1]; s[3] += w * X[2];
    s[4] += w * Y[0]; s[5] += w * Y[1]; s[6] += w * Y[2];
  }
  block_sums_256<7>(s, s_red);
  const double cx[3] = {s[1] / s[0], s[2] / s[0], s[3] / s[0]};
  const double cy[3] = {s[4] / s[0], s[5] / s[0], s[6] / s[0]};
  double B[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = threadIdx.x; j < slots; j += 256) {
    const double w = pair(j, X, Y);
    double T[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    accumulate_b(T, X[0] - cx[0], X[1] - cx[1], X[2] - cx[2], Y[0] - cy[0], Y[1] - cy[1], Y[2] - cy[2]);
#pragma unroll
    for (int e = 0; e < 10; ++e) B[e] += w * T[e];
  }
  block_sums_256<10>(B, s_red);
  if (threadIdx.x == 0) {
    double Rf[9], tf[3];
    rotation_from_b(B, Rf);
    translation(Rf, cx, cy, tf);
    for (int e = 0; e < 9; ++e) s_pose[e] = Rf[e];
    for (int e = 0; e < 3; ++e) s_pose[9 + e] = tf[e];
  }
  __syncthreads();
}

}  // namespace
