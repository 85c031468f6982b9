// Dense point-to-point ICP refinement of P registered cloud pairs for gfx950 (include/dh3d_hip.h dh3d_icp_refine states the
// rule): from the pose of dh3d_ransac_rigid, T times { nearest anchor of every moved positive point within max_dist,
// float64 estimateRigidTransform over those pairs }, then one last association that describes the returned pose.  Every
// launch follows the previous one on the caller's stream -- init, pack, sort, T x (associate, fit), associate, stats --
// no host sync, no allocation, no floating-point atomics: graph-capturable.
//   icp_scan_kernel   association, any shape: lane = positive point, 256 per workgroup; the anchor cloud passes through
//                     LDS in index order, 1024 points at a time, already widened to float64 (24 KiB; one conversion per
//                     staged coordinate, not one per lane and candidate), and is read as broadcasts.  Bound by the float64
//                     VALU: 3 subtractions, 3 products, 2 additions, a compare and two selects per (positive, anchor) --
//                     Na * Nb * 11 float64 operations and nothing to hide them behind.  Walking in index order with a
//                     strict < gives the lowest index at the smallest d2.
//   icp_grid_kernel   association for Na <= 16384 on the anchor's cell table (dh3d_spatial_sort_cells, built once per call:
//                     the anchor does not move).  Lane = positive point: every lane walks the cells that the box
//                     y' +- max_dist meets and the sorted records of each -- about 90 candidates in 8 cells on a street
//                     scene of 8192 points at 1 m, where the scan tests all Na.  Its float64 work is nothing; a step of
//                     the walk is one dependent read (a cell's range or a 16-byte record) and the loop control around it,
//                     and the lanes of a wave are at unrelated places of unrelated walks, so nearly every step of a wave
//                     runs both sides: what bounds the kernel is instructions issued per step times the steps of the
//                     slowest lane (8 waves per SIMD hide the reads).  Hence the cheap cell step: the cell's code comes
//                     from three per-axis deposit tables in LDS (768 bytes, built once per workgroup) and the box is
//                     walked with counters -- the first version divided t by the box's sides and deposited the twelve bits
//                     in a loop for every cell, ~400 instructions that almost every step of a wave paid for some lane.
//                     Candidates are compared by (d2, original index), so the order of the walk does not matter.  A box of
//                     more than 512 cells takes the 64-point groups of the order whose box the ball meets instead: the
//                     loop over the groups is wave-uniform, the records of a group are read as broadcasts.  The walk
//                     itself is cell_walk.h's cell_walk, shared with iss.hip; the float64 box and reach test are here.  The sort's
//                     crowded flag (cells[kCellFlag]) is NOT a reason to leave the cells: for one radius-bound neighbour a
//                     dense cell costs its points and no more, while 64 unrelated lanes meet nearly every group between
//                     them (sending crowded clouds to the groups measured 2.47 ms for 64 x 8192 x 8192 on the demo
//                     clouds, the scan 1.52).  The sort sees the rows below anchor_count only: cloud_pack_kernel
//                     (cloud_pack.h, shared with iss.hip) hands it row r % na in place of every row r >= na (such rows are
//                     never candidates: their index says so), so the grid of a cloud padded with rows of 100000.0 is the
//                     grid of its points, not of its padding.
// The fit and stats kernels, one 256-lane workgroup per cloud pair, share four helpers:
//   IcpClouds           the batch as one argument block: clouds, normals (null for a method without them), strides, counts,
//                       nn and the working pose.  icp_run fills it once; these kernels and icp_grid_kernel take it by value.
//   icp_for_pairs       the walk over the pairs (anchor[nn[j]], positive[j]) with nn[j] >= 0: lane j % 256 over ascending j.
//   block_sums_256<N>   (common.h) every sum of a kernel's pass in one reduction: a fixed tree behind two barriers.
//   icp_moved_centroid  the first pass of the plane and the generalized fit: count and centroid of the moved positives of
//                       the admitted pairs; icp_solve_compose is their last step (6 x 6 Cholesky in registers, the step
//                       composed with the pose; a refused pivot leaves the pose).
//   icp_fit_kernel          point-to-point: rigid_fit.h's block_rigid_fit_256 (ransac_kernel's refit) over the pairs -- 7 sums
//                           (count, centroids), 10 sums (B over the centred pairs), lane 0 solves.  n < 3 leaves the pose.
//                           80 VGPRs, 320 bytes of LDS.
//   icp_stats_kernel        num_corr, fitness, rmse (the sum in the fit's order) and the outputs of invalid pairs.  32 VGPRs.
//   icp_plane_fit_kernel    point-to-plane (dh3d_icp_refine_plane): the pairs whose anchor has a non-zero normal, 21 + 6 sums
//                           (H = sum a a^T, g = sum a r).  Fewer than 6 pairs leave the pose.  126 VGPRs, 864 bytes of LDS.
//   icp_plane_stats_kernel  num_plane and rmse_plane.  40 VGPRs.
//   icp_gicp_fit_kernel     generalized / plane-to-plane (dh3d_icp_refine_gicp): every pair of nn, weighted by
//                           M = (C_A + C_B)^-1 of the two normals' covariances (closed-form 3 x 3 inverse per pair), 21 + 6
//                           sums (H = sum J^T M J, g = sum J^T M d).  Fewer than 3 pairs leave the pose.  126 VGPRs, 864
//                           bytes of LDS.
//   icp_gicp_stats_kernel   num_planar and rmse_gicp.  60 VGPRs.
// None of them uses scratch.  Compiled without contraction (csrc/Makefile EXACT): the ids depend on every rounding of d2.
#include <math.h>

#include "cell_walk.h"
#include "cloud_pack.h"
#include "common.h"
#include "keys.h"
#include "rigid_fit.h"
#include "wave_ops.h"
#include "workspace.h"

namespace {

constexpr int kMaxPoints = 131072;  // Na, Nb
constexpr int kMaxPairs = 65535;
constexpr int kMaxIter = 256;
constexpr int kGridMaxNa = 16384;   // dh3d_spatial_sort_cells
constexpr int kThreads = 256;
constexpr int kChunk = 1024;        // anchors staged per step of the scan

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// y' = R y + t in the form of registration.hip's is_inlier
__device__ __forceinline__ void icp_move(const double *rt, float f0, float f1, float f2, double *m) {
  const double y0 = f0, y1 = f1, y2 = f2;
#pragma unroll
  for (int r = 0; r < 3; ++r) m[r] = ((rt[4 * r] * y0 + rt[4 * r + 1] * y1) + rt[4 * r + 2] * y2) + rt[4 * r + 3];
}

__device__ __forceinline__ double icp_d2(double x0, double x1, double x2, const double *m) {
  const double dx = x0 - m[0], dy = x1 - m[1], dz = x2 - m[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// A batch of P cloud pairs as the cell-list, fit and stats kernels take it (by value).  Strides are in elements; a count
// that is null means all rows; the normals of a method that has none are null.
struct IcpClouds {
  const float *anchor, *a_normals, *positive, *b_normals;
  long long a_stride, an_stride, b_stride, bn_stride;
  int Na, Nb;
  const int32_t *a_count, *b_count;
  int32_t *nn;   // [P, Nb] the anchor of every positive point, -1: none
  double *pose;  // [P, 12] the working pose (workspace)
};

// cloud pair p: its positive count and the first rows of its anchor, its positive and its ids
struct IcpRows {
  int nb;
  const float *a, *b;
  const int32_t *nn;
};
__device__ __forceinline__ IcpRows icp_rows(const IcpClouds &c, int p) {
  return {c.b_count ? clamp_count(c.b_count[p], c.Nb) : c.Nb, c.anchor + (long long)p * c.Na * c.a_stride,
          c.positive + (long long)p * c.Nb * c.b_stride, c.nn + (long long)p * c.Nb};
}
__device__ __forceinline__ const float *icp_anchor_normal(const IcpClouds &c, int p, int i) {
  return c.a_normals + ((long long)p * c.Na + i) * c.an_stride;
}
__device__ __forceinline__ const float *icp_positive_normal(const IcpClouds &c, int p, int j) {
  return c.b_normals + ((long long)p * c.Nb + j) * c.bn_stride;
}

// The pairs of cloud pair p, one 256-lane workgroup: body(i, j, x, y) for every j = lane, lane + 256, ... (ascending) with
// i = nn[j] >= 0, x the anchor's row i and y the positive's row j.  Every sum over the pairs is a lane's sum in this order.
template <typename Body>
__device__ __forceinline__ void icp_for_pairs(const IcpClouds &c, int p, Body body) {
  const IcpRows r = icp_rows(c, p);
  for (int j = threadIdx.x; j < r.nb; j += kThreads) {
    const int i = r.nn[j];
    if (i >= 0) body(i, j, r.a + (long long)i * c.a_stride, r.b + (long long)j * c.b_stride);
  }
}

// ---------------------------------------------------------------------------------------------------------------- init
// the working pose (workspace) and valid: a pair is valid when valid0 is not 0 and Rt0 is finite
__global__ __launch_bounds__(64) void icp_init_kernel(const double *__restrict__ Rt0, const int32_t *__restrict__ valid0, int P,
                                                      double *__restrict__ pose, int32_t *__restrict__ valid) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= P) return;
  double v[12];
  bool ok = valid0 == nullptr || valid0[p] != 0;
  for (int e = 0; e < 12; ++e) {
    v[e] = Rt0[(long long)p * 12 + e];
    ok = ok && isfinite(v[e]);
  }
  for (int e = 0; e < 12; ++e) pose[(long long)p * 12 + e] = ok ? v[e] : quiet_nan();
  valid[p] = ok ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------- scan
// (The one kernel that takes IcpClouds' fields one by one: with the block its loops compiled to the same instructions on
// other registers and ran 0.8 % slower, the same in two runs -- 1583 and 1586 against 1571 and 1573 us per iteration.)
__global__ __launch_bounds__(kThreads) void icp_scan_kernel(
    const float *__restrict__ anchor, long long a_stride, int Na, const int32_t *__restrict__ a_count,
    const float *__restrict__ positive, long long b_stride, int Nb, const int32_t *__restrict__ b_count,
    const double *__restrict__ pose, const int32_t *__restrict__ valid, double r2, int32_t *__restrict__ nn) {
  __shared__ __align__(16) double s_c[3 * kChunk];  // x[kChunk] | y[kChunk] | z[kChunk]
  const int p = blockIdx.y, j = blockIdx.x * kThreads + threadIdx.x;
  const int na = a_count ? clamp_count(a_count[p], Na) : Na, nb = b_count ? clamp_count(b_count[p], Nb) : Nb;
  int32_t *out = nn + (long long)p * Nb;
  if ((int)blockIdx.x * kThreads >= nb || na == 0 || !valid[p]) {  // (workgroup-uniform)
    if (j < Nb) out[j] = -1;
    return;
  }
  const bool live = j < nb;
  double m[3];
  const float *yr = positive + ((long long)p * Nb + (live ? j : 0)) * b_stride;
  icp_move(pose + (long long)p * 12, yr[0], yr[1], yr[2], m);
  const float *pa = anchor + (long long)p * Na * a_stride;
  double best = r2;  // strict: d2 == max_dist^2 is no neighbour
  int best_i = -1;
  for (int base = 0; base < na; base += kChunk) {
    const int len = min(kChunk, na - base);
    __syncthreads();  // the previous chunk has been read
    for (int c = threadIdx.x; c < len; c += kThreads) {
      const float *r = pa + (long long)(base + c) * a_stride;
      s_c[c] = r[0]; s_c[kChunk + c] = r[1]; s_c[2 * kChunk + c] = r[2];
    }
    __syncthreads();
#pragma unroll 4
    for (int c = 0; c < len; ++c) {
      const double d2 = icp_d2(s_c[c], s_c[kChunk + c], s_c[2 * kChunk + c], m);
      if (d2 < best) {  // index order and a strict <: the lowest index keeps a tie
        best = d2;
        best_i = base + c;
      }
    }
  }
  if (j < Nb) out[j] = live ? best_i : -1;
}

// ---------------------------------------------------------------------------------------------------------- cell lists
struct Best {
  double d2;
  int i;
};
// (d2, original index) ascending; the start value (max_dist^2, -1) refuses d2 == max_dist^2
__device__ __forceinline__ void icp_take(Best &b, const float4 rec, const double *m, int na) {
  const int k = __float_as_int(rec.w);  // (the plain original index: spatial.hip)
  const double d2 = icp_d2(rec.x, rec.y, rec.z, m);
  if (k < na && (d2 < b.d2 || (d2 == b.d2 && k < b.i))) {
    b.d2 = d2;
    b.i = k;
  }
}

__global__ __launch_bounds__(kThreads) void icp_grid_kernel(
    const float4 *__restrict__ sorted, const float *__restrict__ gbox, const int *__restrict__ cells, IcpClouds c,
    const int32_t *__restrict__ valid, double r2, double max_dist) {
  __shared__ unsigned s_dep[3][64];  // axis value -> its bits at their places in the cell's 12-bit code
  const int p = blockIdx.y, j = blockIdx.x * kThreads + threadIdx.x, Na = c.Na, Nb = c.Nb;
  const int na = c.a_count ? clamp_count(c.a_count[p], Na) : Na, nb = c.b_count ? clamp_count(c.b_count[p], Nb) : Nb;
  int32_t *out = c.nn + (long long)p * Nb;
  if ((int)blockIdx.x * kThreads >= nb || na == 0 || !valid[p]) {  // (workgroup-uniform)
    if (j < Nb) out[j] = -1;
    return;
  }
  const bool live = j < nb;
  const float *yr = c.positive + ((long long)p * Nb + (live ? j : 0)) * c.b_stride;
  const float y0 = yr[0], y1 = yr[1], y2 = yr[2];
  double m[3];
  icp_move(c.pose + (long long)p * 12, y0, y1, y2, m);
  const float4 *sc = sorted + (size_t)p * Na;
  const CellGrid g = cell_grid(cells, p);
  cell_deposit_tables(g, s_dep);
  // The cells that the box y' +- max_dist meets.  An anchor x that the float64 test accepts has dx * dx <= d2 < max_dist^2
  // up to three float64 roundings, so |x - y'| < max_dist (1 + 2^-50) on every axis.  The box edge y' -+ (max_dist + marg)
  // is formed in float64 (2 roundings of 2^-53) and rounded to float32 (2^-24 relative to |y'| + max_dist + marg at most);
  // marg = (max_dist + |y'|) * 1e-6 is 16 times that, so the float32 edge still lies outside x, which is a float32 itself.
  // The cell function is the sort's own and monotone in its argument (cell_grid.h grid_cell): cell(lower edge) <= cell(x)
  // <= cell(upper edge).
  CellBox box;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double marg = (max_dist + fabs(m[a])) * 1e-6;
    box.c0[a] = grid_cell(g, a, (float)((m[a] - max_dist) - marg));
    box.cn[a] = grid_cell(g, a, (float)((m[a] + max_dist) + marg)) - box.c0[a] + 1;
  }
  // The walk (cell_walk.h cell_walk).  A group of a wide box is walked when the ball can reach its box: the test is float64
  // on the exact box, and an accepted anchor lies in its group's box, so the box distance is at most its d2 (up to the
  // roundings that the 1e-9 margin covers).
  Best b{r2, -1};
  cell_walk(sc, gbox + (size_t)p * ((Na + 63) / 64) * 8, g.ct, Na, s_dep, box, live, [&](const float4 lo, const float4 hi) {
    const double dx = fmax(fmax((double)lo.x - m[0], m[0] - (double)hi.x), 0.0);
    const double dy = fmax(fmax((double)lo.y - m[1], m[1] - (double)hi.y), 0.0);
    const double dz = fmax(fmax((double)lo.z - m[2], m[2] - (double)hi.z), 0.0);
    return ((dx * dx + dy * dy) + dz * dz) * (1.0 - 1e-9) < r2;
  }, [&](int, const float4 rec) {
    icp_take(b, rec, m, na);
    return true;
  });
  if (j < Nb) out[j] = live ? b.i : -1;
}

// ----------------------------------------------------------------------------------------------------------------- fit
__global__ __launch_bounds__(kThreads) void icp_fit_kernel(IcpClouds c) {
  __shared__ double s_red[10 * (kThreads / 64)];
  const int p = blockIdx.x;
  const IcpRows r = icp_rows(c, p);
  block_rigid_fit_256(r.nb, [&](int j, float *x, float *y) {  // (the slots of icp_for_pairs)
    const int i = r.nn[j];
    if (i < 0) return false;
    const float *xa = r.a + (long long)i * c.a_stride, *yb = r.b + (long long)j * c.b_stride;
    x[0] = xa[0]; x[1] = xa[1]; x[2] = xa[2];
    y[0] = yb[0]; y[1] = yb[1]; y[2] = yb[2];
    return true;
  }, s_red, c.pose + (long long)p * 12);
}

// --------------------------------------------------------------------------------------------------------------- stats
__global__ __launch_bounds__(kThreads) void icp_stats_kernel(IcpClouds c, double *__restrict__ Rt, int32_t *__restrict__ num_corr,
                                                             double *__restrict__ fitness, double *__restrict__ rmse) {
  __shared__ double s_red[2 * (kThreads / 64)];
  const int p = blockIdx.x, tid = threadIdx.x;
  const double *rt = c.pose + (long long)p * 12;
  double s[2] = {0.0, 0.0};  // pairs, d2
  icp_for_pairs(c, p, [&](int, int, const float *x, const float *y) {
    double m[3];
    icp_move(rt, y[0], y[1], y[2], m);
    s[0] += 1.0;
    s[1] += icp_d2(x[0], x[1], x[2], m);
  });
  block_sums_256<2>(s, s_red);
  if (tid < 12) Rt[(long long)p * 12 + tid] = rt[tid];  // (NaN where the pair is not valid: icp_init_kernel)
  if (tid == 0) {
    const int n = (int)s[0], nb = icp_rows(c, p).nb;
    num_corr[p] = n;
    fitness[p] = (double)n / (double)(nb > 1 ? nb : 1);
    rmse[p] = n > 0 ? sqrt(s[1] / (double)n) : quiet_nan();
  }
}

// ----------------------------------------------------------------------------------------------------------- plane fit
// the pairs of the point-to-plane fit: nn[j] >= 0 and an anchor normal with n . n > 0
__device__ __forceinline__ bool icp_plane_pair(const float *nr, double *n) {
  n[0] = nr[0]; n[1] = nr[1]; n[2] = nr[2];
  return (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2] > 0.0;
}

// The end of F_plane and F_gicp, one lane: H s = g by Cholesky (H: the upper triangle, row by row; registers: every index is
// a constant after unrolling), then the step composed with the pose rt about the centroid c.  A refused pivot or a
// non-finite s leaves `out` as it was.
__device__ __forceinline__ void icp_solve_compose(const double *H, const double *g, const double *rt, const double *c,
                                                  double *out) {
  // Cholesky H = L L^T, row by row; L[k][j] lives at L[k * 6 + j]
  double L[36], big = 0.0;
  {
    int e = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      big = fmax(big, H[e]);
      e += 6 - r;
    }
  }
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int j = 0; j <= k; ++j) {
      double v = H[j * 6 - j * (j - 1) / 2 + (k - j)];  // H[j][k], j <= k
#pragma unroll
      for (int q = 0; q < j; ++q) v = v - L[k * 6 + q] * L[j * 6 + q];
      if (j < k) {
        L[k * 6 + j] = v / L[j * 6 + j];
      } else {
        ok = ok && isfinite(v) && v > 1e-12 * big;
        L[k * 6 + k] = sqrt(v);
      }
    }
  }
  if (!ok) return;  // a rank-deficient or non-finite system: the pose stays as it was
  double z[6], s[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    double v = g[k];
#pragma unroll
    for (int j = 0; j < k; ++j) v = v - L[k * 6 + j] * z[j];
    z[k] = v / L[k * 6 + k];
  }
#pragma unroll
  for (int k = 5; k >= 0; --k) {
    double v = z[k];
#pragma unroll
    for (int j = k + 1; j < 6; ++j) v = v - L[j * 6 + k] * s[j];
    s[k] = v / L[k * 6 + k];
  }
  // dR = I + (sin th / th) K + (2 sin^2(th / 2) / th^2) K^2, K = [w]x, K^2 = w w^T - (w . w) I
  const double w0 = s[0], w1 = s[1], w2 = s[2];
  const double tt = (w0 * w0 + w1 * w1) + w2 * w2, th = sqrt(tt);
  double dR[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  if (th > 0.0 && isfinite(th)) {
    const double hs = sin(th / 2.0), A = sin(th) / th, B = (2.0 * (hs * hs)) / (th * th);
    const double Km[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    const double w[3] = {w0, w1, w2};
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double k2 = r == k ? w[r] * w[k] - tt : w[r] * w[k];
        dR[3 * r + k] = (dR[3 * r + k] + A * Km[3 * r + k]) + B * k2;
      }
  }
  bool fin = true;
#pragma unroll
  for (int e = 0; e < 6; ++e) fin = fin && isfinite(s[e]);
  if (!fin) return;
  const double u[3] = {rt[3] - c[0], rt[7] - c[1], rt[11] - c[2]};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      out[4 * r + k] = (dR[3 * r] * rt[k] + dR[3 * r + 1] * rt[4 + k]) + dR[3 * r + 2] * rt[8 + k];
    out[4 * r + 3] = (((dR[3 * r] * u[0] + dR[3 * r + 1] * u[1]) + dR[3 * r + 2] * u[2]) + c[r]) + s[3 + r];
  }
}

// The first pass of F_plane and F_gicp: the count of the pairs that admit(i) takes and the centroid `cen` of their moved
// positives (one reduction).  False, to every lane, when they are fewer than `least`: the pose then stays as it was.
template <typename Admit>
__device__ __forceinline__ bool icp_moved_centroid(const IcpClouds &c, int p, const double *rt, Admit admit, int least,
                                                   double *s_red, double *cen) {
  double sm[4] = {0.0, 0.0, 0.0, 0.0};  // the count, then the moved points
  icp_for_pairs(c, p, [&](int i, int, const float *, const float *y) {
    if (!admit(i)) return;
    double m[3];
    icp_move(rt, y[0], y[1], y[2], m);
    sm[0] += 1.0;
    sm[1] += m[0]; sm[2] += m[1]; sm[3] += m[2];
  });
  block_sums_256<4>(sm, s_red);
  const int n = (int)sm[0];
  if (n < least) return false;  // (workgroup-uniform)
#pragma unroll
  for (int r = 0; r < 3; ++r) cen[r] = sm[1 + r] / (double)n;
  return true;
}

// r = n . (x - m)
__device__ __forceinline__ double icp_plane_residual(const float *x, const double *m, const double *n) {
  const double dx = (double)x[0] - m[0], dy = (double)x[1] - m[1], dz = (double)x[2] - m[2];
  return (dx * n[0] + dy * n[1]) + dz * n[2];
}

// One 256-lane workgroup per pair (include/dh3d_hip.h dh3d_icp_refine_plane F_plane): the centroid c of the moved positives
// of the pairs, then the 21 + 6 float64 sums of H = sum a a^T and g = sum a r over a = [(m - c) x n ; n], r = n . (x - m),
// reduced at once; lane 0 solves and composes (icp_solve_compose).  Fewer than 6 pairs or a refused pivot leave the pose.
__global__ __launch_bounds__(kThreads) void icp_plane_fit_kernel(IcpClouds c) {
  __shared__ double s_red[27 * (kThreads / 64)];
  const int p = blockIdx.x;
  double rt[12], cen[3], n[3];
#pragma unroll
  for (int e = 0; e < 12; ++e) rt[e] = c.pose[(long long)p * 12 + e];
  const auto planar = [&](int i) { return icp_plane_pair(icp_anchor_normal(c, p, i), n); };
  if (!icp_moved_centroid(c, p, rt, planar, 6, s_red, cen)) return;
  double S[27];  // H: the upper triangle, row by row; then g
#pragma unroll
  for (int e = 0; e < 27; ++e) S[e] = 0.0;
  icp_for_pairs(c, p, [&](int i, int, const float *x, const float *y) {
    if (!planar(i)) return;
    double m[3];
    icp_move(rt, y[0], y[1], y[2], m);
    const double q0 = m[0] - cen[0], q1 = m[1] - cen[1], q2 = m[2] - cen[2];
    const double a[6] = {q1 * n[2] - q2 * n[1], q2 * n[0] - q0 * n[2], q0 * n[1] - q1 * n[0], n[0], n[1], n[2]};
    const double res = icp_plane_residual(x, m, n);
    int e = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
      for (int k = r; k < 6; ++k) S[e++] += a[r] * a[k];
      S[21 + r] += a[r] * res;
    }
  });
  block_sums_256<27>(S, s_red);
  if (threadIdx.x == 0) icp_solve_compose(S, S + 21, rt, cen, c.pose + (long long)p * 12);
}

// num_plane and rmse_plane of the last association under the returned pose (the sums in the fit's order)
__global__ __launch_bounds__(kThreads) void icp_plane_stats_kernel(IcpClouds c, int32_t *__restrict__ num_plane,
                                                                   double *__restrict__ rmse_plane) {
  __shared__ double s_red[2 * (kThreads / 64)];
  const int p = blockIdx.x;
  const double *rt = c.pose + (long long)p * 12;
  double s[2] = {0.0, 0.0};  // pairs with a normal, r^2
  icp_for_pairs(c, p, [&](int i, int, const float *x, const float *y) {
    double n[3], m[3];
    if (!icp_plane_pair(icp_anchor_normal(c, p, i), n)) return;
    icp_move(rt, y[0], y[1], y[2], m);
    const double res = icp_plane_residual(x, m, n);
    s[0] += 1.0;
    s[1] += res * res;
  });
  block_sums_256<2>(s, s_red);
  if (threadIdx.x == 0) {
    const int npl = (int)s[0];
    num_plane[p] = npl;
    rmse_plane[p] = npl > 0 ? sqrt(s[1] / (double)npl) : quiet_nan();
  }
}

// ------------------------------------------------------------------------------------------------------------ gicp fit
// What a pair of the generalized fit carries (include/dh3d_hip.h dh3d_icp_refine_gicp F_gicp, steps 3 to 5): the weight matrix
// M = (C_A + C_B)^-1 as its six entries 00 01 02 11 12 22, and whether both normals are non-zero.
struct GicpPair {
  double M[6];
  bool planar;
};

// C = I - f v v^T as the entries 00 01 02 11 12 22, f = (1 - epsilon) / (v . v) or 0 for a zero v; returns v . v > 0
__device__ __forceinline__ bool gicp_cov(double v0, double v1, double v2, double one_m_eps, double *C) {
  const double s = (v0 * v0 + v1 * v1) + v2 * v2;
  const double f = s > 0.0 ? one_m_eps / s : 0.0;
  const double a0 = f * v0, a1 = f * v1, a2 = f * v2;
  C[0] = 1.0 - a0 * v0; C[1] = 0.0 - a0 * v1; C[2] = 0.0 - a0 * v2;
  C[3] = 1.0 - a1 * v1; C[4] = 0.0 - a1 * v2; C[5] = 1.0 - a2 * v2;
  return s > 0.0;
}

__device__ __forceinline__ GicpPair gicp_pair(const float *na, const float *kb, const double *rt, double one_m_eps) {
  double CA[6], CB[6], W[6], u[3];
  const double k0 = kb[0], k1 = kb[1], k2 = kb[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) u[r] = (rt[4 * r] * k0 + rt[4 * r + 1] * k1) + rt[4 * r + 2] * k2;
  const bool pa = gicp_cov(na[0], na[1], na[2], one_m_eps, CA);
  const bool pb = gicp_cov(u[0], u[1], u[2], one_m_eps, CB);
#pragma unroll
  for (int e = 0; e < 6; ++e) W[e] = CA[e] + CB[e];
  // W = [[0 1 2], [1 3 4], [2 4 5]]; M = adj(W) / det(W)
  const double c00 = W[3] * W[5] - W[4] * W[4], c01 = W[2] * W[4] - W[1] * W[5], c02 = W[1] * W[4] - W[2] * W[3];
  const double c11 = W[0] * W[5] - W[2] * W[2], c12 = W[1] * W[2] - W[0] * W[4], c22 = W[0] * W[3] - W[1] * W[1];
  const double det = (W[0] * c00 + W[1] * c01) + W[2] * c02;
  GicpPair g;
  g.M[0] = c00 / det; g.M[1] = c01 / det; g.M[2] = c02 / det;
  g.M[3] = c11 / det; g.M[4] = c12 / det; g.M[5] = c22 / det;
  g.planar = pa && pb;
  return g;
}

// One 256-lane workgroup per pair (include/dh3d_hip.h dh3d_icp_refine_gicp F_gicp): the centroid c of the moved positives of
// all pairs, then per pair the weight matrix M and the 21 + 6 float64 sums of H = sum J^T M J and g = sum J^T M d, reduced
// at once; lane 0 solves and composes as the plane fit does.  Fewer than 3 pairs or a refused pivot leave the pose.
__global__ __launch_bounds__(kThreads) void icp_gicp_fit_kernel(IcpClouds c, double one_m_eps) {
  __shared__ double s_red[27 * (kThreads / 64)];
  const int p = blockIdx.x;
  double rt[12], cen[3];
#pragma unroll
  for (int e = 0; e < 12; ++e) rt[e] = c.pose[(long long)p * 12 + e];
  if (!icp_moved_centroid(c, p, rt, [](int) { return true; }, 3, s_red, cen)) return;
  double S[27];  // H: the upper triangle, row by row; then g
#pragma unroll
  for (int e = 0; e < 27; ++e) S[e] = 0.0;
  icp_for_pairs(c, p, [&](int i, int j, const float *x, const float *y) {
    double m[3];
    icp_move(rt, y[0], y[1], y[2], m);
    const GicpPair w = gicp_pair(icp_anchor_normal(c, p, i), icp_positive_normal(c, p, j), rt, one_m_eps);
    const double *M = w.M;
    const double Mr[3][3] = {{M[0], M[1], M[2]}, {M[1], M[3], M[4]}, {M[2], M[4], M[5]}};
    const double q0 = m[0] - cen[0], q1 = m[1] - cen[1], q2 = m[2] - cen[2];
    const double d[3] = {(double)x[0] - m[0], (double)x[1] - m[1], (double)x[2] - m[2]};
    double b[6][3];  // b_v = M j_v
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      b[0][r] = Mr[r][2] * q1 - Mr[r][1] * q2;
      b[1][r] = Mr[r][0] * q2 - Mr[r][2] * q0;
      b[2][r] = Mr[r][1] * q0 - Mr[r][0] * q1;
      b[3][r] = Mr[r][0]; b[4][r] = Mr[r][1]; b[5][r] = Mr[r][2];
    }
    int e = 0;
#pragma unroll
    for (int u = 0; u < 6; ++u) {
#pragma unroll
      for (int v = u; v < 6; ++v) {  // j_u . b_v
        const double h = u == 0 ? q1 * b[v][2] - q2 * b[v][1] : u == 1 ? q2 * b[v][0] - q0 * b[v][2]
                       : u == 2 ? q0 * b[v][1] - q1 * b[v][0] : b[v][u - 3];
        S[e++] += h;
      }
      S[21 + u] += (b[u][0] * d[0] + b[u][1] * d[1]) + b[u][2] * d[2];
    }
  });
  block_sums_256<27>(S, s_red);
  if (threadIdx.x == 0) icp_solve_compose(S, S + 21, rt, cen, c.pose + (long long)p * 12);
}

// num_planar and rmse_gicp of the last association under the returned pose (the sums in the fit's order)
__global__ __launch_bounds__(kThreads) void icp_gicp_stats_kernel(IcpClouds c, double one_m_eps, int32_t *__restrict__ num_planar,
                                                                  double *__restrict__ rmse_gicp) {
  __shared__ double s_red[3 * (kThreads / 64)];
  const int p = blockIdx.x;
  double rt[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) rt[e] = c.pose[(long long)p * 12 + e];
  double s[3] = {0.0, 0.0, 0.0};  // pairs, planar pairs, d . (M d)
  icp_for_pairs(c, p, [&](int i, int j, const float *x, const float *y) {
    double m[3];
    icp_move(rt, y[0], y[1], y[2], m);
    const GicpPair w = gicp_pair(icp_anchor_normal(c, p, i), icp_positive_normal(c, p, j), rt, one_m_eps);
    const double *M = w.M;
    const double d0 = (double)x[0] - m[0], d1 = (double)x[1] - m[1], d2 = (double)x[2] - m[2];
    const double e0 = (M[0] * d0 + M[1] * d1) + M[2] * d2, e1 = (M[1] * d0 + M[3] * d1) + M[4] * d2;
    const double e2 = (M[2] * d0 + M[4] * d1) + M[5] * d2;
    s[0] += 1.0;
    s[1] += w.planar ? 1.0 : 0.0;
    s[2] += (d0 * e0 + d1 * e1) + d2 * e2;
  });
  block_sums_256<3>(s, s_red);
  if (threadIdx.x == 0) {
    const int n = (int)s[0];
    num_planar[p] = (int)s[1];
    rmse_gicp[p] = n > 0 ? sqrt(s[2] / (double)n) : quiet_nan();
  }
}

// ----------------------------------------------------------------------------------------------------------- workspace
struct IcpWs {
  double *pose;    // [P, 12] the working pose
  float4 *sorted;  // the anchor's spatial sort (Na <= 16384 only)
  float *gbox;
  int *cells;
  float *packed;   // [P, Na, 3] what the sort reads: the anchor without its stride and without the rows behind its count
  IcpWs(Carve &c, int P, int Na, int Nb) {
    const bool grid = Na <= kGridMaxNa;
    pose = c.take<double>((size_t)P * 12, 16);
    sorted = c.take<float4>(grid ? (size_t)P * Na : 0, 16);
    gbox = c.take<float>(grid ? (size_t)P * ((Na + 63) / 64) * 8 : 0, 16);
    cells = c.take<int>(grid ? (size_t)P * kCellInts : 0, 16);
    packed = c.take<float>(grid ? (size_t)P * Na * 3 : 0, 16);
  }
};

bool icp_served(int P, int Na, int Nb) {
  return P > 0 && Na > 0 && Nb > 0 && P <= kMaxPairs && Na <= kMaxPoints && Nb <= kMaxPoints;
}

}  // namespace

DH3D_API int dh3d_icp_plan(int Na, int Nb) {
  if (!icp_served(1, Na, Nb)) return -1;
  return Na <= kGridMaxNa ? 2 : 1;
}

DH3D_API size_t dh3d_icp_refine_ws_bytes(int P, int Na, int Nb) {
  return icp_served(P, Na, Nb) ? carve_bytes<IcpWs>(P, Na, Nb) : 0;
}

// What the three entries refuse alike; each adds its own normals, strides, outputs and epsilon ahead of this (all of them
// invalid-argument refusals, as the first three here, so the order between them decides nothing).
static int icp_check(const IcpClouds &c, const double *Rt0, int P, double max_dist, int iterations, int path, const double *Rt,
                     const int32_t *num_corr, const double *fitness, const double *rmse, const int32_t *valid,
                     const void *workspace, size_t workspace_bytes) {
  DH3D_REQUIRE(c.anchor && c.positive && Rt0 && Rt && c.nn && num_corr && fitness && rmse && valid);
  DH3D_REQUIRE(P > 0 && c.Na > 0 && c.Nb > 0 && c.a_stride >= 3 && c.b_stride >= 3);
  DH3D_REQUIRE(max_dist > 0.0 && isfinite(max_dist) && iterations >= 0 && path >= 0 && path <= 2);
  DH3D_SUPPORTED(icp_served(P, c.Na, c.Nb) && iterations <= kMaxIter);
  DH3D_SUPPORTED(path != 2 || c.Na <= kGridMaxNa);
  DH3D_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 &&
               workspace_bytes >= carve_bytes<IcpWs>(P, c.Na, c.Nb));
  return DH3D_OK;
}

// The launches of the three entries, after icp_check: without normals the point-to-point fit; with the anchor's alone the
// point-to-plane fit and its two outputs (num_plane, rmse_plane); with both clouds' the generalized fit at epsilon, the two
// outputs then being num_planar and rmse_gicp.
static int icp_run(IcpClouds c, double epsilon, const double *Rt0, const int32_t *valid0, int P, double max_dist, int iterations,
                   int path, double *Rt, int32_t *num_corr, double *fitness, double *rmse, int32_t *valid, int32_t *num_extra,
                   double *rmse_extra, void *workspace, void *stream) {
  Carve carve(workspace);
  const IcpWs ws(carve, P, c.Na, c.Nb);
  const bool grid = (path == 0 ? dh3d_icp_plan(c.Na, c.Nb) : path) == 2;
  hipStream_t s = (hipStream_t)stream;
  const double r2 = max_dist * max_dist, one_m_eps = 1.0 - epsilon;
  const dim3 fit(P), lanes(kThreads);
  c.pose = ws.pose;

  hipLaunchKernelGGL(icp_init_kernel, dim3(dh3d_cdiv(P, 64)), dim3(64), 0, s, Rt0, valid0, P, ws.pose, valid);
  if (grid) {
    hipLaunchKernelGGL(cloud_pack_kernel, dim3(dh3d_cdiv(c.Na, kPackThreads), P), dim3(kPackThreads), 0, s, c.anchor, c.a_stride,
                       c.Na, c.a_count, ws.packed);
    const int st = dh3d_spatial_sort_cells(ws.packed, P, c.Na, reinterpret_cast<float *>(ws.sorted), ws.gbox, ws.cells, stream);
    if (st != DH3D_OK) return st;
  }
  const dim3 agrid(dh3d_cdiv(c.Nb, kThreads), P);
  for (int it = 0; it <= iterations; ++it) {
    if (grid)
      hipLaunchKernelGGL(icp_grid_kernel, agrid, lanes, 0, s, ws.sorted, ws.gbox, ws.cells, c, valid, r2, max_dist);
    else
      hipLaunchKernelGGL(icp_scan_kernel, agrid, lanes, 0, s, c.anchor, c.a_stride, c.Na, c.a_count, c.positive, c.b_stride,
                         c.Nb, c.b_count, c.pose, valid, r2, c.nn);
    if (it == iterations) break;
    if (!c.a_normals)
      hipLaunchKernelGGL(icp_fit_kernel, fit, lanes, 0, s, c);
    else if (c.b_normals)
      hipLaunchKernelGGL(icp_gicp_fit_kernel, fit, lanes, 0, s, c, one_m_eps);
    else
      hipLaunchKernelGGL(icp_plane_fit_kernel, fit, lanes, 0, s, c);
  }
  hipLaunchKernelGGL(icp_stats_kernel, fit, lanes, 0, s, c, Rt, num_corr, fitness, rmse);
  if (c.b_normals)
    hipLaunchKernelGGL(icp_gicp_stats_kernel, fit, lanes, 0, s, c, one_m_eps, num_extra, rmse_extra);
  else if (c.a_normals)
    hipLaunchKernelGGL(icp_plane_stats_kernel, fit, lanes, 0, s, c, num_extra, rmse_extra);
  return dh3d_launch_status();
}

DH3D_API int dh3d_icp_refine(const float *anchor, long long anchor_stride, const int32_t *anchor_count, const float *positive,
                             long long positive_stride, const int32_t *positive_count, const double *Rt0,
                             const int32_t *valid0, int P, int Na, int Nb, double max_dist, int iterations, int path,
                             double *Rt, int32_t *nn, int32_t *num_corr, double *fitness, double *rmse, int32_t *valid,
                             void *workspace, size_t workspace_bytes, void *stream) {
  const IcpClouds c{anchor, nullptr, positive, nullptr, anchor_stride, 0, positive_stride, 0, Na, Nb, anchor_count,
                    positive_count, nn, nullptr};
  const int st = icp_check(c, Rt0, P, max_dist, iterations, path, Rt, num_corr, fitness, rmse, valid, workspace, workspace_bytes);
  if (st != DH3D_OK) return st;
  return icp_run(c, 0.0, Rt0, valid0, P, max_dist, iterations, path, Rt, num_corr, fitness, rmse, valid, nullptr, nullptr,
                 workspace, stream);
}

DH3D_API size_t dh3d_icp_refine_plane_ws_bytes(int P, int Na, int Nb) { return dh3d_icp_refine_ws_bytes(P, Na, Nb); }

DH3D_API int dh3d_icp_refine_plane(const float *anchor, long long anchor_stride, const int32_t *anchor_count,
                                   const float *anchor_normals, long long normals_stride, const float *positive,
                                   long long positive_stride, const int32_t *positive_count, const double *Rt0,
                                   const int32_t *valid0, int P, int Na, int Nb, double max_dist, int iterations, int path,
                                   double *Rt, int32_t *nn, int32_t *num_corr, double *fitness, double *rmse, int32_t *valid,
                                   int32_t *num_plane, double *rmse_plane, void *workspace, size_t workspace_bytes,
                                   void *stream) {
  const IcpClouds c{anchor, anchor_normals, positive, nullptr, anchor_stride, normals_stride, positive_stride, 0, Na, Nb,
                    anchor_count, positive_count, nn, nullptr};
  DH3D_REQUIRE(anchor_normals && normals_stride >= 3 && num_plane && rmse_plane);
  const int st = icp_check(c, Rt0, P, max_dist, iterations, path, Rt, num_corr, fitness, rmse, valid, workspace, workspace_bytes);
  if (st != DH3D_OK) return st;
  return icp_run(c, 0.0, Rt0, valid0, P, max_dist, iterations, path, Rt, num_corr, fitness, rmse, valid, num_plane, rmse_plane,
                 workspace, stream);
}

DH3D_API size_t dh3d_icp_refine_gicp_ws_bytes(int P, int Na, int Nb) { return dh3d_icp_refine_ws_bytes(P, Na, Nb); }

DH3D_API int dh3d_icp_refine_gicp(const float *anchor, long long anchor_stride, const int32_t *anchor_count,
                                  const float *anchor_normals, long long normals_stride, const float *positive_normals,
                                  long long positive_normals_stride, const float *positive, long long positive_stride,
                                  const int32_t *positive_count, const double *Rt0, const int32_t *valid0, int P, int Na, int Nb,
                                  double max_dist, int iterations, int path, double epsilon, double *Rt, int32_t *nn,
                                  int32_t *num_corr, double *fitness, double *rmse, int32_t *valid, int32_t *num_planar,
                                  double *rmse_gicp, void *workspace, size_t workspace_bytes, void *stream) {
  const IcpClouds c{anchor, anchor_normals, positive, positive_normals, anchor_stride, normals_stride, positive_stride,
                    positive_normals_stride, Na, Nb, anchor_count, positive_count, nn, nullptr};
  DH3D_REQUIRE(anchor_normals && positive_normals && normals_stride >= 3 && positive_normals_stride >= 3 && num_planar &&
               rmse_gicp);
  DH3D_REQUIRE(epsilon > 0.0 && epsilon <= 1.0);  // (NaN fails both)
  const int st = icp_check(c, Rt0, P, max_dist, iterations, path, Rt, num_corr, fitness, rmse, valid, workspace, workspace_bytes);
  if (st != DH3D_OK) return st;
  return icp_run(c, epsilon, Rt0, valid0, P, max_dist, iterations, path, Rt, num_corr, fitness, rmse, valid, num_planar,
                 rmse_gicp, workspace, stream);
}
