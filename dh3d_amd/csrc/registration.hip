// Keypoint matching and RANSAC rigid registration of cloud pairs for gfx950 (evaluate/local_eval/matlab_code:
// eval_align.m's pdist2(pos_desc, anc_desc, 'smallest', 1) followed by ransacfitRt.m / ransac.m / estimateRigidTransform.m,
// run there one pair at a time on the host).  Two launches per batch of P pairs, no atomics on global memory, no workspace,
// no host sync (graph-capturable):
//   match_kernel   one thread per anchor keypoint, 256 per block, (ceil(Ma / 256), P) blocks: the positives' descriptors
//                  pass through LDS 32 rows at a time and every thread keeps 32 running f32 sums of squared differences
//                  (d ascending, the same order for every pair: a pair's ids do not depend on the batch); the first
//                  smallest sum wins, ties to the lowest positive id;
//   ransac_kernel  one 256-lane workgroup per pair: the valid correspondences are compacted (anchor order kept) into LDS as
//                  f32 coordinates; every round each lane evaluates one trial k (splitmix64 sample, float64 3-point
//                  estimateRigidTransform with a cyclic Jacobi eigen-solve, float64 inlier count over all n matches); lane
//                  0 then replays ransac.m's serial stop rule over the round's 256 counts.  The winning trial's model is
//                  recomputed by every lane (same code, same bits), gives the inlier mask, and the inliers are refitted
//                  with float64 block sums in a fixed order.
// Compiled without contraction (csrc/Makefile EXACT): the ids and the inlier sets depend on every rounding.
#include "common.h"
#include "keys.h"
#include "rigid_fit.h"
#include "wave_ops.h"

namespace {

constexpr int kMatchThreads = 256;
constexpr int kMatchTile = 32;     // positive rows per LDS tile
constexpr int kMaxDim = 256;       // descriptor length limit (LDS tile: 32 x 256 f32 = 32 KB)
constexpr int kMaxKp = 4096;       // keypoints per cloud (pm.KEYPOINT_MAX)
constexpr int kRansacThreads = 256;
constexpr int kRansacWaves = kRansacThreads / 64;

__global__ __launch_bounds__(kMatchThreads) void match_kernel(const float *__restrict__ a, long long a_stride, int Ma,
                                                              const int32_t *__restrict__ a_count,
                                                              const float *__restrict__ b, long long b_stride, int Mb,
                                                              const int32_t *__restrict__ b_count, int D,
                                                              int32_t *__restrict__ match, float *__restrict__ dist) {
  __shared__ __align__(16) float s_b[kMatchTile * kMaxDim];
  const int p = blockIdx.y, i = blockIdx.x * kMatchThreads + threadIdx.x;
  const int na = clamp_count(a_count[p], Ma), nb = clamp_count(b_count[p], Mb);
  const bool live = i < na;
  const float *arow = a + ((long long)p * Ma + (live ? i : 0)) * a_stride;
  const float *bp = b + (long long)p * Mb * b_stride;
  float best = INFINITY;
  int best_j = -1;
  for (int j0 = 0; j0 < nb; j0 += kMatchTile) {
    const int rows = nb - j0 < kMatchTile ? nb - j0 : kMatchTile;
    __syncthreads();  // the previous tile has been read
    for (int e = threadIdx.x; e < rows * D; e += kMatchThreads) {
      const int r = e / D, c = e - r * D;
      s_b[r * D + c] = bp[(long long)(j0 + r) * b_stride + c];  // (rows may not be 16-byte aligned: column 3 of 132)
    }
    __syncthreads();
    if (!live) continue;
    float acc[kMatchTile];
#pragma unroll
    for (int r = 0; r < kMatchTile; ++r) acc[r] = 0.f;
    for (int c = 0; c < D; c += 4) {
      const float a0 = arow[c], a1 = arow[c + 1], a2 = arow[c + 2], a3 = arow[c + 3];
#pragma unroll
      for (int r = 0; r < kMatchTile; ++r) {
        const float4 v = *reinterpret_cast<const float4 *>(&s_b[r * D + c]);  // (D % 4 == 0: 16-byte aligned, broadcast)
        float d0 = a0 - v.x, d1 = a1 - v.y, d2 = a2 - v.z, d3 = a3 - v.w;
        float s = acc[r];
        s = s + d0 * d0;
        s = s + d1 * d1;
        s = s + d2 * d2;
        s = s + d3 * d3;
        acc[r] = s;
      }
    }
#pragma unroll
    for (int r = 0; r < kMatchTile; ++r) {
      if (r < rows && acc[r] < best) {  // strict: the lowest id keeps a tie
        best = acc[r];
        best_j = j0 + r;
      }
    }
  }
  if (i < Ma) {
    const long long o = (long long)p * Ma + i;
    match[o] = live ? best_j : -1;
    dist[o] = live && best_j >= 0 ? sqrtf(best) : INFINITY;
  }
}

// ---------------------------------------------------------------------------------------------------------- RANSAC

// three distinct ids in [0, n), n >= 4, of trial k (include/dh3d_hip.h dh3d_ransac_rigid)
__device__ __forceinline__ void sample3(unsigned long long seed_h, unsigned long long k, int n, int &i0, int &i1, int &i2) {
  const unsigned long long h = splitmix64(seed_h ^ k);
  const unsigned long long u0 = splitmix64(h), u1 = splitmix64(h + 1), u2 = splitmix64(h + 2);
  i0 = (int)(u0 % (unsigned long long)n);
  i1 = (int)(u1 % (unsigned long long)(n - 1));
  if (i1 >= i0) ++i1;
  i2 = (int)(u2 % (unsigned long long)(n - 2));
  const int lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
  if (i2 >= lo) ++i2;
  if (i2 >= hi) ++i2;
}

struct Corr {  // the compacted correspondences in LDS (f32, exact in f64)
  float *x0, *x1, *x2, *y0, *y1, *y2;
  int *id;
};

// the seven arrays of Ma rows each in the kernel's dynamic LDS (corr_lds_bytes)
__device__ __forceinline__ Corr corr_carve(float *s_dyn, int Ma) {
  Corr s;
  s.x0 = s_dyn;
  s.x1 = s.x0 + Ma;
  s.x2 = s.x1 + Ma;
  s.y0 = s.x2 + Ma;
  s.y1 = s.y0 + Ma;
  s.y2 = s.y1 + Ma;
  s.id = reinterpret_cast<int *>(s.y2 + Ma);
  return s;
}

// The staging that ransac_kernel and gnc_kernel share, by a 256-lane workgroup: pair p's valid correspondences (i < a_count,
// 0 <= match < Mb) compacted in anchor order into s, s.id their anchor rows; clears the pair's row of the inlier mask.
// Returns their number n to every lane, behind a barrier.  s_wave: kRansacWaves ints.
__device__ __forceinline__ int stage_corr(const Corr &s, int *s_wave, const float *__restrict__ axyz, long long a_stride, int Ma,
                                          const int32_t *__restrict__ a_count, const float *__restrict__ bxyz,
                                          long long b_stride, int Mb, const int32_t *__restrict__ match, int p,
                                          uint8_t *__restrict__ inliers) {
  const int tid = threadIdx.x, w = tid >> 6;
  const int na = clamp_count(a_count[p], Ma);
  int n = 0;
  for (int base = 0; base < Ma; base += kRansacThreads) {
    const int i = base + tid;
    int m = -1;
    if (i < Ma) {
      inliers[(long long)p * Ma + i] = 0;
      if (i < na) m = match[(long long)p * Ma + i];
    }
    const bool ok = m >= 0 && m < Mb;
    const unsigned long long bal = __ballot(ok);
    if ((tid & 63) == 0) s_wave[w] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
    for (int q = 0; q < kRansacWaves; ++q) {
      const int v = s_wave[q];
      off += q < w ? v : 0;
      tot += v;
    }
    if (ok) {
      const int slot = n + off + __popcll(bal & lanes_below());
      const float *xa = axyz + ((long long)p * Ma + i) * a_stride;
      const float *xb = bxyz + ((long long)p * Mb + m) * b_stride;
      s.x0[slot] = xa[0]; s.x1[slot] = xa[1]; s.x2[slot] = xa[2];
      s.y0[slot] = xb[0]; s.y1[slot] = xb[1]; s.y2[slot] = xb[2];
      s.id[slot] = i;
    }
    n += tot;
    __syncthreads();
  }
  return n;
}

// the model of the sample (j0, j1, j2): centroid = (sum in sample order) / 3, B over the centred points in sample order
__device__ void fit3(const Corr &s, int j0, int j1, int j2, double *R, double *t) {
  const int js[3] = {j0, j1, j2};
  double x[3][3], y[3][3], xc[3] = {0.0, 0.0, 0.0}, yc[3] = {0.0, 0.0, 0.0};
  for (int q = 0; q < 3; ++q) {
    const int j = js[q];
    x[q][0] = s.x0[j]; x[q][1] = s.x1[j]; x[q][2] = s.x2[j];
    y[q][0] = s.y0[j]; y[q][1] = s.y1[j]; y[q][2] = s.y2[j];
    for (int r = 0; r < 3; ++r) {
      xc[r] += x[q][r];
      yc[r] += y[q][r];
    }
  }
  for (int r = 0; r < 3; ++r) {
    xc[r] = xc[r] / 3.0;
    yc[r] = yc[r] / 3.0;
  }
  double B[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int q = 0; q < 3; ++q)
    accumulate_b(B, x[q][0] - xc[0], x[q][1] - xc[1], x[q][2] - xc[2], y[q][0] - yc[0], y[q][1] - yc[1], y[q][2] - yc[2]);
  rotation_from_b(B, R);
  translation(R, xc, yc, t);
}

// sqrt(|x - (R y + t)|^2) < thr (ransacfitRt.m euc3Ddist)
__device__ __forceinline__ bool is_inlier(const Corr &s, int j, const double *R, const double *t, double thr) {
  const double y0 = s.y0[j], y1 = s.y1[j], y2 = s.y2[j];
  const double e0 = (double)s.x0[j] - ((R[0] * y0 + R[1] * y1 + R[2] * y2) + t[0]);
  const double e1 = (double)s.x1[j] - ((R[3] * y0 + R[4] * y1 + R[5] * y2) + t[1]);
  const double e2 = (double)s.x2[j] - ((R[6] * y0 + R[7] * y1 + R[8] * y2) + t[2]);
  return sqrt(e0 * e0 + e1 * e1 + e2 * e2) < thr;
}

__global__ __launch_bounds__(kRansacThreads) void ransac_kernel(
    const float *__restrict__ axyz, long long a_stride, int Ma, const int32_t *__restrict__ a_count,
    const float *__restrict__ bxyz, long long b_stride, int Mb, const int32_t *__restrict__ match, double thr, double conf,
    int max_trials, unsigned long long seed, double *__restrict__ Rt, int32_t *__restrict__ valid,
    uint8_t *__restrict__ inliers, int32_t *__restrict__ num_inliers, int32_t *__restrict__ trials,
    int32_t *__restrict__ num_corr) {
  extern __shared__ float s_dyn[];
  __shared__ int s_wave[kRansacWaves];
  __shared__ int s_cnt[kRansacThreads];
  __shared__ int s_done, s_win, s_kstar;
  __shared__ double s_red[10 * kRansacWaves];  // block_rigid_fit_256
  const int p = blockIdx.x, tid = threadIdx.x;
  Corr s = corr_carve(s_dyn, Ma);

  // (1) compact the valid correspondences (i < a_count, 0 <= match < Mb) in anchor order; clear the mask row
  const int n = stage_corr(s, s_wave, axyz, a_stride, Ma, a_count, bxyz, b_stride, Mb, match, p, inliers);
  if (tid == 0 && num_corr) num_corr[p] = n;
  double *rt = Rt + (long long)p * 12;
  if (n < 3) {  // ransacfitRt.m: no model
    if (tid < 12) rt[tid] = __longlong_as_double(0x7ff8000000000000ll);
    if (tid == 0) {
      valid[p] = 0;
      num_inliers[p] = 0;
      trials[p] = 0;
    }
    return;
  }

  // (2) ransac.m's loop, 256 trials per round; lane 0 replays the serial stop rule over the round's counts
  int win = 0, kstar = -1;
  if (n > 3) {
    const unsigned long long seed_h = splitmix64(seed);
    const double log_fail = log(1.0 - conf);
    const double eps = 2.220446049250313e-16;
    int best = 0;     // (lane 0's state across rounds: ransac.m's bestscore and N)
    double N = 1.0;
    if (tid == 0) s_done = 0;
    for (int base = 0;; base += kRansacThreads) {
      const int k = base + tid;
      int c = -1;
      if (k <= max_trials) {
        int j0, j1, j2;
        sample3(seed_h, (unsigned long long)k, n, j0, j1, j2);
        double R[9], t[3];
        fit3(s, j0, j1, j2, R, t);
        c = 0;
        for (int j = 0; j < n; ++j) c += is_inlier(s, j, R, t, thr) ? 1 : 0;
      }
      s_cnt[tid] = c;
      __syncthreads();
      if (tid == 0) {
        for (int q = 0; q < kRansacThreads; ++q) {
          const int kk = base + q, ck = s_cnt[q];
          if (ck >= best) {  // ransac.m accepts on >=: the last trial with the best count wins
            best = ck;
            win = kk;
            const double frac = (double)best / (double)n;
            double pno = 1.0 - frac * frac * frac;
            pno = pno < eps ? eps : pno;
            pno = pno > 1.0 - eps ? 1.0 - eps : pno;
            N = log_fail / log(pno);
            N = N < 10.0 ? 10.0 : N;
          }
          if (N <= (double)(kk + 1) || kk + 1 > max_trials) {  // ransac.m: while N > trialcount ... > maxTrials
            s_done = 1;
            s_win = win;
            s_kstar = kk;
            break;
          }
        }
      }
      __syncthreads();
      if (s_done) break;
    }
    win = s_win;
    kstar = s_kstar;
  }

  // (3) the winning model (recomputed: the same bits as in its round), its inlier mask and count
  int j0 = 0, j1 = 1, j2 = 2;
  if (n > 3) sample3(splitmix64(seed), (unsigned long long)win, n, j0, j1, j2);
  double R[9], t[3];
  fit3(s, j0, j1, j2, R, t);
  int cnt = 0;
  for (int j = tid; j < n; j += kRansacThreads) {
    const bool in = n == 3 || is_inlier(s, j, R, t, thr);  // (n == 3: ransacfitRt.m takes all three)
    if (in) {
      inliers[(long long)p * Ma + s.id[j]] = 1;
      ++cnt;
    }
  }
  const int count = (int)block_sum_256<double>((double)cnt, s_red);
  if (tid == 0) {
    num_inliers[p] = count;
    trials[p] = n > 3 ? kstar + 1 : 0;
    valid[p] = count >= 3;
  }
  if (count < 3) {
    if (tid < 12) rt[tid] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }

  // (4) least-squares refit on the inliers (count of them: at least 3 here)
  block_rigid_fit_256(n, [&](int j, float *x, float *y) {
    if (n != 3 && !is_inlier(s, j, R, t, thr)) return false;
    x[0] = s.x0[j]; x[1] = s.x1[j]; x[2] = s.x2[j];
    y[0] = s.y0[j]; y[1] = s.y1[j]; y[2] = s.y2[j];
    return true;
  }, s_red, rt);
}

// ------------------------------------------------------------------------------------------------------------- GNC

constexpr int kGncMaxIter = 1024;

// The weights a fit uses are not stored: they are a function of the fit before it (R, t) and of that fit's mu, and both
// passes of block_weighted_rigid_fit_256 recompute them.  unit: the first fit, every w = 1.
struct GncWeights {
  double R[9], t[3], mu;
  bool unit;
};

// the centred pair j (X = x - xc, Y = y - yc) and its weight (mu / (|X - (R Y + t)|^2 + mu))^2
__device__ __forceinline__ double gnc_pair(const Corr &s, int j, const double *xc, const double *yc, const GncWeights &g,
                                           double *X, double *Y) {
  X[0] = (double)s.x0[j] - xc[0]; X[1] = (double)s.x1[j] - xc[1]; X[2] = (double)s.x2[j] - xc[2];
  Y[0] = (double)s.y0[j] - yc[0]; Y[1] = (double)s.y1[j] - yc[1]; Y[2] = (double)s.y2[j] - yc[2];
  if (g.unit) return 1.0;
  const double e0 = X[0] - ((g.R[0] * Y[0] + g.R[1] * Y[1] + g.R[2] * Y[2]) + g.t[0]);
  const double e1 = X[1] - ((g.R[3] * Y[0] + g.R[4] * Y[1] + g.R[5] * Y[2]) + g.t[1]);
  const double e2 = X[2] - ((g.R[6] * Y[0] + g.R[7] * Y[1] + g.R[8] * Y[2]) + g.t[2]);
  const double q = g.mu / ((e0 * e0 + e1 * e1 + e2 * e2) + g.mu);
  return q * q;
}

// One 256-lane workgroup per pair, the whole schedule in one launch (include/dh3d_hip.h dh3d_gnc_rigid states the rule):
// stage the correspondences as RANSAC does, centre them, then per fit two block reductions (the weighted centroids, then B)
// with lane 0's 4 x 4 Jacobi behind them.  Every decision of the loop is taken by every lane on the same float64 values.
__global__ __launch_bounds__(kRansacThreads) void gnc_kernel(
    const float *__restrict__ axyz, long long a_stride, int Ma, const int32_t *__restrict__ a_count,
    const float *__restrict__ bxyz, long long b_stride, int Mb, const int32_t *__restrict__ match, double thr, double division,
    int settle, int max_iter, double *__restrict__ Rt, double *__restrict__ weights, int32_t *__restrict__ valid,
    uint8_t *__restrict__ inliers, int32_t *__restrict__ num_inliers, int32_t *__restrict__ num_corr,
    int32_t *__restrict__ iterations) {
  extern __shared__ float s_dyn[];
  __shared__ int s_wave[kRansacWaves];
  __shared__ double s_red[10 * kRansacWaves];  // block_weighted_rigid_fit_256
  __shared__ double s_pose[12];
  const int p = blockIdx.x, tid = threadIdx.x;
  Corr s = corr_carve(s_dyn, Ma);
  for (int i = tid; i < Ma; i += kRansacThreads) weights[(long long)p * Ma + i] = 0.0;  // (rows that are no correspondence)
  const int n = stage_corr(s, s_wave, axyz, a_stride, Ma, a_count, bxyz, b_stride, Mb, match, p, inliers);
  double *rt = Rt + (long long)p * 12;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (n < 3) {  // no model
    if (tid < 12) rt[tid] = nan;
    if (tid == 0) {
      valid[p] = 0;
      num_inliers[p] = 0;
      num_corr[p] = n;
      iterations[p] = 0;
    }
    return;
  }

  // the centroids, and D2 = the largest squared norm of a centred point (a NaN term is skipped: v > D2 is false)
  double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = tid; j < n; j += kRansacThreads) {
    c[0] += s.x0[j]; c[1] += s.x1[j]; c[2] += s.x2[j];
    c[3] += s.y0[j]; c[4] += s.y1[j]; c[5] += s.y2[j];
  }
  block_sums_256<6>(c, s_red);
  const double xc[3] = {c[0] / (double)n, c[1] / (double)n, c[2] / (double)n};
  const double yc[3] = {c[3] / (double)n, c[4] / (double)n, c[5] / (double)n};
  GncWeights g;
  g.unit = true;
  g.mu = 0.0;
  for (int e = 0; e < 9; ++e) g.R[e] = 0.0;
  for (int e = 0; e < 3; ++e) g.t[e] = 0.0;
  double D2 = 0.0;
  for (int j = tid; j < n; j += kRansacThreads) {
    double X[3], Y[3];
    gnc_pair(s, j, xc, yc, g, X, Y);
    const double vx = X[0] * X[0] + X[1] * X[1] + X[2] * X[2], vy = Y[0] * Y[0] + Y[1] * Y[1] + Y[2] * Y[2];
    if (vx > D2) D2 = vx;
    if (vy > D2) D2 = vy;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(D2, off, 64);
    if (o > D2) D2 = o;
  }
  __syncthreads();  // (s_red: the centroid sums have been read)
  if ((tid & 63) == 0) s_red[tid >> 6] = D2;
  __syncthreads();
  for (int q = 0; q < kRansacWaves; ++q) D2 = s_red[q] > D2 ? s_red[q] : D2;  // (a maximum: the same bits in any order)

  const double d2 = thr * thr;
  double mu = D2 > d2 ? D2 : d2;
  double R[9], t[3];
  int k = 0, at = 0;
  for (;;) {
    block_weighted_rigid_fit_256(n, [&](int j, double *X, double *Y) { return gnc_pair(s, j, xc, yc, g, X, Y); }, s_red,
                                 s_pose);
    for (int e = 0; e < 9; ++e) R[e] = s_pose[e];
    for (int e = 0; e < 3; ++e) t[e] = s_pose[9 + e];
    ++k;
    if (mu == d2) ++at;
    if (at > settle || k >= max_iter) break;
    for (int e = 0; e < 9; ++e) g.R[e] = R[e];
    for (int e = 0; e < 3; ++e) g.t[e] = t[e];
    g.mu = mu;
    g.unit = false;
    mu = mu / division;
    mu = mu > d2 ? mu : d2;
  }

  // the pose in the clouds' own coordinates, the weights of the last fit, the inlier mask of the pose
  double tf[3];
  translation(R, xc, yc, tf);
  bool finite = true;
  for (int e = 0; e < 3; ++e) {
    tf[e] = tf[e] + t[e];
    finite = finite && isfinite(tf[e]);
  }
  for (int e = 0; e < 9; ++e) finite = finite && isfinite(R[e]);
  int cnt = 0;
  for (int j = tid; j < n; j += kRansacThreads) {
    double X[3], Y[3];
    weights[(long long)p * Ma + s.id[j]] = gnc_pair(s, j, xc, yc, g, X, Y);
    if (is_inlier(s, j, R, tf, thr)) {
      inliers[(long long)p * Ma + s.id[j]] = 1;
      ++cnt;
    }
  }
  const int count = (int)block_sum_256<double>((double)cnt, s_red);
  const bool ok = finite && count >= 3;
  if (tid == 0) {
    num_inliers[p] = count;
    num_corr[p] = n;
    iterations[p] = k;
    valid[p] = ok;
    for (int r = 0; r < 3; ++r) {
      for (int q = 0; q < 3; ++q) rt[4 * r + q] = ok ? R[3 * r + q] : nan;
      rt[4 * r + 3] = ok ? tf[r] : nan;
    }
  }
}

size_t corr_lds_bytes(int Ma) { return (size_t)Ma * (6 * sizeof(float) + sizeof(int)); }

}  // namespace

DH3D_API int dh3d_match_descriptors(const float *anchor_desc, long long anchor_stride, const int32_t *anchor_count,
                                    const float *positive_desc, long long positive_stride, const int32_t *positive_count,
                                    int P, int Ma, int Mb, int D, int32_t *match, float *dist, void *stream) {
  DH3D_REQUIRE(anchor_desc && anchor_count && positive_desc && positive_count && match && dist);
  DH3D_REQUIRE(P > 0 && Ma > 0 && Mb > 0 && D > 0 && anchor_stride >= D && positive_stride >= D);
  DH3D_SUPPORTED(D <= kMaxDim && D % 4 == 0 && Ma <= kMaxKp && Mb <= kMaxKp && P <= 65535);
  hipLaunchKernelGGL(match_kernel, dim3(dh3d_cdiv(Ma, kMatchThreads), P), dim3(kMatchThreads), 0, (hipStream_t)stream,
                     anchor_desc, anchor_stride, Ma, anchor_count, positive_desc, positive_stride, Mb, positive_count, D,
                     match, dist);
  return dh3d_launch_status();
}

DH3D_API int dh3d_ransac_rigid(const float *anchor_xyz, long long anchor_stride, const float *positive_xyz,
                               long long positive_stride, const int32_t *match, const int32_t *anchor_count, int P, int Ma,
                               int Mb, double threshold, double confidence, int max_trials, unsigned long long seed,
                               double *Rt, int32_t *valid, uint8_t *inliers, int32_t *num_inliers, int32_t *trials,
                               int32_t *num_corr, void *stream) {
  DH3D_REQUIRE(anchor_xyz && positive_xyz && match && anchor_count && Rt && valid && inliers && num_inliers && trials);
  DH3D_REQUIRE(P > 0 && Ma > 0 && Mb > 0 && anchor_stride >= 3 && positive_stride >= 3);
  DH3D_REQUIRE(threshold > 0.0 && confidence > 0.0 && confidence < 1.0 && max_trials >= 0);
  DH3D_SUPPORTED(Ma <= kMaxKp && Mb <= kMaxKp && P <= 65535 && max_trials < (1 << 30));
  // the dynamic-LDS cap for the largest staging (4096 correspondences: 112 KB) once per process, out of the steady state.
  // (Not DH3D_ALLOW_BIG_LDS: its 159 KB plus this kernel's 1 KB of static LDS is beyond the CU's 160 KB, and the refused
  // call would be reported as this launch's status.)
  static bool lds_cap_set = false;
  if (!lds_cap_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ransac_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)corr_lds_bytes(kMaxKp));
    lds_cap_set = true;
  }
  hipLaunchKernelGGL(ransac_kernel, dim3(P), dim3(kRansacThreads), corr_lds_bytes(Ma), (hipStream_t)stream, anchor_xyz,
                     anchor_stride, Ma, anchor_count, positive_xyz, positive_stride, Mb, match, threshold, confidence,
                     max_trials, seed, Rt, valid, inliers, num_inliers, trials, num_corr);
  return dh3d_launch_status();
}

DH3D_API int dh3d_gnc_rigid(const float *anchor_xyz, long long anchor_stride, const float *positive_xyz,
                            long long positive_stride, const int32_t *match, const int32_t *anchor_count, int P, int Ma, int Mb,
                            double threshold, double division, int settle, int max_iterations, double *Rt, double *weights,
                            int32_t *valid, uint8_t *inliers, int32_t *num_inliers, int32_t *num_corr, int32_t *iterations,
                            void *stream) {
  DH3D_REQUIRE(anchor_xyz && positive_xyz && match && anchor_count && Rt && weights && valid && inliers && num_inliers &&
               num_corr && iterations);
  DH3D_REQUIRE(P > 0 && Ma > 0 && Mb > 0 && anchor_stride >= 3 && positive_stride >= 3);
  DH3D_REQUIRE(threshold > 0.0 && division > 1.0 && settle >= 0 && max_iterations >= 1 && max_iterations <= kGncMaxIter);
  DH3D_SUPPORTED(Ma <= kMaxKp && Mb <= kMaxKp && P <= 65535);
  // the dynamic-LDS cap as dh3d_ransac_rigid sets it (and not DH3D_ALLOW_BIG_LDS, for the reason given there)
  static bool lds_cap_set = false;
  if (!lds_cap_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(gnc_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)corr_lds_bytes(kMaxKp));
    lds_cap_set = true;
  }
  hipLaunchKernelGGL(gnc_kernel, dim3(P), dim3(kRansacThreads), corr_lds_bytes(Ma), (hipStream_t)stream, anchor_xyz,
                     anchor_stride, Ma, anchor_count, positive_xyz, positive_stride, Mb, match, threshold, division, settle,
                     max_iterations, Rt, weights, valid, inliers, num_inliers, num_corr, iterations);
  return dh3d_launch_status();
}
