// ISS keypoints (Intrinsic Shape Signatures, Zhong 2009) of P clouds for gfx950 (include/dh3d_hip.h dh3d_iss_keypoints
// states the rule): per point the float64 scatter of ALL points within a radius, its eigenvalues, a saliency, then a
// radius non-maximum suppression and the M most salient survivors.  Five launches, one after the other on the caller's
// stream -- pack, sort, moments, nms, select -- no host sync, no allocation, no floating-point atomics, no workgroup waits
// for another: graph-capturable.
//   cloud_pack_kernel   (cloud_pack.h, icp.hip's) rows behind the count become copies of rows below it, then
//                       dh3d_spatial_sort_cells builds the cell table once per call.
//   iss_walk            the one walk both kernels make, LANE = POINT: cell_walk.h's cell_walk (icp_grid_kernel's too) over
//                       the cells that the box x_i +- r meets (ball_cells), a box of more than 512 cells over the 64-point
//                       groups whose gbox the ball meets.  The lanes of a workgroup are 256 consecutive points OF THE SORTED
//                       ORDER, so the lanes of a wave are neighbours walking the same few cells.  The sort's crowded flag
//                       is not looked at: a dense cell costs its records and no more (not measured against the group walk
//                       on crowded clouds).
//                       The other form, WAVE = QUERY (ball_grid_kernel's: a lane per cell for the ranges, the ranges
//                       flattened, a lane per record, a butterfly for the wave's eleven sums, the solve lane = point after
//                       64 walks), was built first and lost: 1.77 ms against 1.19 ms for the whole call on 64 x 8192 street
//                       scenes at 2.0 / 1.5 m (74 members a ball), 3.60 against 2.61 ms at 292 members (DEADENDS.md).
//   iss_moments_kernel  one walk at max(r_s, r_n) gives both counts and, for the members of S_i, the nine float64 sums of e
//                       and e e^T in the lane's registers; then the covariance, the Jacobi solve (rigid_fit.h
//                       eigenvalues_3_descending) and the saliency.  Bound, as icp_grid_kernel, by the steps of a wave's
//                       slowest lane times the instructions of a step (here the float32 test and, for a member, 21 float64
//                       operations).  60 VGPRs, 768 bytes of LDS, no scratch.
//   iss_nms_kernel      the same walk at r_n over the saliencies in sorted order (written by the moments kernel next to the
//                       records' order); only points with a positive saliency walk, and a lane stops at the first
//                       neighbour that beats it.  A 64-bit key per point, (ordered bits of s) << 32 | ~index, or 0 when the
//                       point is not kept.  29 VGPRs, 768 bytes of LDS, no scratch.
//   iss_select_kernel   one 1024-lane workgroup per cloud, block_ops.h's compaction, radix select of the M-th largest key and
//                       LDS sort, as keypoints.hip's nms_select_kernel; ~index in the low bits makes the lowest index the
//                       largest key among equal saliencies.  32 VGPRs, 33.9 KiB of LDS, no scratch.
// Compiled without contraction (csrc/Makefile EXACT): the memberships depend on every rounding of d2.
#include <math.h>

#include "block_ops.h"
#include "cell_walk.h"
#include "cloud_pack.h"
#include "common.h"
#include "keys.h"
#include "rigid_fit.h"
#include "wave_ops.h"
#include "workspace.h"

namespace {

constexpr int kMaxN = 16384;        // dh3d_spatial_sort_cells
constexpr int kMaxClouds = 65535;
constexpr int kMaxKeep = 4096;      // M limit: the winners' sort buffer in LDS (32 KiB)
constexpr int kThreads = 256;
constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / 64;

__device__ __forceinline__ float iss_d2(const float4 c, const float *q) {
  const float dx = c.x - q[0], dy = c.y - q[1], dz = c.z - q[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// What both kernels set up alike: one cloud as the walk reads it (uniform over the workgroup), the lane's own point and
// the deposit tables.  Ends in a barrier: every thread of the workgroup must reach it.
struct IssLane {
  const float4 *sc;  // the sorted records: x y z and the plain original index in w
  const float *gb;   // the boxes of the 64-record groups
  CellGrid g;
  int N, n;          // rows, valid rows
  float rs, rn;      // the radii, 0 for one that is <= 0 or NaN (no members: d2 < 0 is never true)
  int s, k;          // the lane's sorted position, and its point's original index (-1 for a lane beyond the cloud's end)
  float q[3];
};
__device__ __forceinline__ IssLane iss_lane(const float4 *sorted, const float *gbox, const int *cells, const int32_t *count,
                                            const float *radii, int N, unsigned (*s_dep)[64]) {
  const int p = blockIdx.y;
  IssLane L;
  L.sc = sorted + (size_t)p * N;
  L.gb = gbox + (size_t)p * ((N + 63) / 64) * 8;
  L.g = cell_grid(cells, p);
  L.N = N;
  L.n = count ? clamp_count(count[p], N) : N;
  const float rs = radii[2 * p], rn = radii[2 * p + 1];
  L.rs = rs > 0.f ? rs : 0.f;
  L.rn = rn > 0.f ? rn : 0.f;
  cell_deposit_tables(L.g, s_dep);  // axis value -> its bits at their places in the cell's 12-bit code
  L.s = blockIdx.x * kThreads + threadIdx.x;
  const float4 rec = L.sc[L.s < N ? L.s : 0];
  L.k = L.s < N ? __float_as_int(rec.w) : -1;
  L.q[0] = rec.x; L.q[1] = rec.y; L.q[2] = rec.z;
  return L;
}

// The walk of one lane around its point at radius r (cell_walk.h cell_walk states the contract): take(pos, record) for
// every sorted position whose record can pass the float32 test d2 < r * r, and for others, until take returns false.  A
// group is walked when the ball meets its box: 1e-5 relative margin on the box distance, as ball_grid_kernel's; it dwarfs
// the roundings of both chains.
template <class Take>
__device__ __forceinline__ void iss_walk(const IssLane &L, const unsigned (*s_dep)[64], bool walks, float r, Take take) {
  const float r2hi = r * r * 1.000001f;
  cell_walk(L.sc, L.gb, L.g.ct, L.N, s_dep, ball_cells(L.g, L.q, r), walks, [&](const float4 lo, const float4 hi) {
    const float dx = fmaxf(fmaxf(lo.x - L.q[0], L.q[0] - hi.x), 0.f), dy = fmaxf(fmaxf(lo.y - L.q[1], L.q[1] - hi.y), 0.f),
                dz = fmaxf(fmaxf(lo.z - L.q[2], L.q[2] - hi.z), 0.f);
    return ((dx * dx + dy * dy) + dz * dz) * 0.99999f <= r2hi;
  }, take);
}

// ------------------------------------------------------------------------------------------------------------- moments
__global__ __launch_bounds__(kThreads) void iss_moments_kernel(
    const float4 *__restrict__ sorted, const float *__restrict__ gbox, const int *__restrict__ cells,
    const int32_t *__restrict__ count, const float *__restrict__ radii, const float *__restrict__ saliency_in, int N, double g21,
    double g32, int min_nb, float *__restrict__ saliency, int32_t *__restrict__ num_nbr, double *__restrict__ lam,
    float *__restrict__ sal_sorted) {
  __shared__ unsigned s_dep[3][64];
  const IssLane L = iss_lane(sorted, gbox, cells, count, radii, N, s_dep);
  const int p = blockIdx.y, n = L.n;
  const float rs2 = L.rs * L.rs, rn2 = L.rn * L.rn, R = fmaxf(L.rs, L.rn);
  const bool moments = saliency_in == nullptr;
  const double q0 = (double)L.q[0], q1 = (double)L.q[1], q2 = (double)L.q[2];
  int ms = 0, mt = 0;
  double a[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // e0 e1 e2, e0e0 e0e1 e0e2 e1e1 e1e2 e2e2
  // a copy behind the count walks nothing, nor does anyone when neither radius is one
  iss_walk(L, s_dep, (unsigned)L.k < (unsigned)n && R > 0.f, R, [&](int, const float4 c) {
    if ((unsigned)__float_as_int(c.w) >= (unsigned)n) return true;  // copies are never members
    const float d2 = iss_d2(c, L.q);
    mt += d2 < rn2 ? 1 : 0;
    if (d2 < rs2) {
      ++ms;
      if (moments) {  // float64 differences of their own: not the float32 ones of the test
        const double e0 = (double)c.x - q0, e1 = (double)c.y - q1, e2 = (double)c.z - q2;
        a[0] += e0; a[1] += e1; a[2] += e2;
        a[3] += e0 * e0; a[4] += e0 * e1; a[5] += e0 * e2;
        a[6] += e1 * e1; a[7] += e1 * e2; a[8] += e2 * e2;
      }
    }
    return true;
  });
  if ((unsigned)L.k >= (unsigned)N) return;  // (a lane beyond the cloud's end)
  const long long row = (long long)p * N + L.k;
  float sal = 0.f;
  double l[3] = {0.0, 0.0, 0.0};
  if (L.k < n) {
    if (!moments) {
      sal = saliency_in[row];
    } else if (ms >= 1) {
      const double dm = (double)ms, u0 = a[0] / dm, u1 = a[1] / dm, u2 = a[2] / dm;
      const double C[6] = {a[3] / dm - u0 * u0, a[4] / dm - u0 * u1, a[5] / dm - u0 * u2,
                           a[6] / dm - u1 * u1, a[7] / dm - u1 * u2, a[8] / dm - u2 * u2};
      eigenvalues_3_descending(C, l);
      if (ms >= min_nb && l[1] < g21 * l[0] && l[2] < g32 * l[1] && l[2] > 0.0) sal = (float)l[2];
    }
  }
  saliency[row] = sal;
  num_nbr[2 * row] = ms;
  num_nbr[2 * row + 1] = mt;
  if (lam) {
    lam[3 * row] = l[0]; lam[3 * row + 1] = l[1]; lam[3 * row + 2] = l[2];
  }
  sal_sorted[(long long)p * N + L.s] = sal;
}

// ----------------------------------------------------------------------------------------------------------------- nms
__global__ __launch_bounds__(kThreads) void iss_nms_kernel(
    const float4 *__restrict__ sorted, const float *__restrict__ gbox, const int *__restrict__ cells,
    const int32_t *__restrict__ count, const float *__restrict__ radii, const float *__restrict__ sal_sorted,
    const int32_t *__restrict__ num_nbr, int N, int min_nb, unsigned long long *__restrict__ keys) {
  __shared__ unsigned s_dep[3][64];
  const IssLane L = iss_lane(sorted, gbox, cells, count, radii, N, s_dep);
  const int p = blockIdx.y, n = L.n, k = L.k;
  const float rn2 = L.rn * L.rn;
  const float *ss = sal_sorted + (long long)p * N;
  const bool live = (unsigned)k < (unsigned)n;  // (false for a copy behind the count and for a lane beyond the end)
  const float si = live ? ss[L.s] : 0.f;
  // a candidate: a valid row with a positive saliency (not 0, not NaN) and enough points in T_i (none when r_n is no radius)
  const bool cand = live && si > 0.f && num_nbr[2 * ((long long)p * N + k) + 1] >= min_nb;
  bool kept = cand;
  iss_walk(L, s_dep, cand, L.rn, [&](int pos, const float4 c) {
    const int kj = __float_as_int(c.w);
    const float sj = ss[pos];  // (0 for a copy; a NaN compares false)
    if ((unsigned)kj < (unsigned)n && kj != k && iss_d2(c, L.q) < rn2 && (sj > si || (sj == si && kj < k))) kept = false;
    return kept;  // beaten: the walk ends
  });
  if (L.s < N)
    keys[(long long)p * N + L.s] = kept ? ((unsigned long long)f32_order_bits(si) << 32) | (0xFFFFFFFFu - (unsigned)k) : 0ull;
}

// -------------------------------------------------------------------------------------------------------------- select
// The keys are distinct (the index sits in the low bits), so the order is total: the largest saliency first, the lowest
// index first among equal ones.
__global__ __launch_bounds__(kSelThreads) void iss_select_kernel(unsigned long long *__restrict__ keys, int N, int M,
                                                                 int32_t *__restrict__ ids, int32_t *__restrict__ kp_count) {
  __shared__ unsigned long long s_win[kMaxKeep];
  __shared__ int s_hist[256];
  __shared__ int s_wave[kSelWaves];
  __shared__ int s_sel[2], s_n;
  const int b = blockIdx.x, tid = threadIdx.x;
  unsigned long long *ck = keys + (long long)b * N;

  // (1) compact the non-zero keys to the front, in place: every store of a chunk lands below the chunk's end and the chunk
  //     was read before the barriers of block_compact_slot
  int c = 0;
  for (int base = 0; base < N; base += kSelThreads) {
    const int i = base + tid;
    const unsigned long long key = i < N ? ck[i] : 0ull;
    int tot;
    const int slot = c + block_compact_slot<kSelThreads>(key != 0ull, s_wave, tot);
    if (key) ck[slot] = key;
    c += tot;
  }

  // (2) the M-th largest key = the (c - M + 1)-th smallest; with c <= M every survivor is a winner
  unsigned long long thr = 1ull;
  if (c > M)  // exactly M keys are >= it: the keys are distinct
    thr = block_radix_select<kSelThreads>(c, c - M + 1, [&](int j, bool &) { return ck[j]; }, s_hist, s_sel).key;
  const int nw = c < M ? c : M;

  // (3) the winners into LDS (any order), sorted descending
  if (tid == 0) s_n = 0;
  __syncthreads();
  for (int base = 0; base < c; base += kSelThreads) {
    const int j = base + tid;
    const unsigned long long key = j < c ? ck[j] : 0ull;
    const bool win = j < c && key >= thr;
    const unsigned long long bal = __ballot(win);
    int slot0 = 0;
    if (bal && (tid & 63) == __builtin_ffsll((long long)bal) - 1) slot0 = atomicAdd(&s_n, __popcll(bal));
    slot0 = __shfl(slot0, __builtin_ffsll((long long)bal) - 1);
    const int slot = slot0 + __popcll(bal & lanes_below());
    if (win && slot < nw) s_win[slot] = key;  // (exactly nw winners; the bound only guards the LDS buffer)
  }
  block_sort<kSelThreads>(s_win, nw, [](unsigned long long x, unsigned long long y) { return x > y; });
  for (int j = tid; j < M; j += kSelThreads)
    ids[(long long)b * M + j] = j < nw ? (int32_t)(0xFFFFFFFFu - (unsigned)(s_win[j] & 0xffffffffull)) : -1;
  if (tid == 0) kp_count[b] = nw;
}

// ----------------------------------------------------------------------------------------------------------- workspace
struct IssWs {
  float4 *sorted;  // the cloud's spatial sort
  float *gbox;
  int *cells;
  float *packed;   // [P, N, 3] what the sort reads: the cloud without its stride and without the rows behind its count
  float *ssort;    // [P, N] the saliencies in the order of `sorted`
  unsigned long long *keys;  // [P, N]
  IssWs(Carve &c, int P, int N) {
    sorted = c.take<float4>((size_t)P * N, 16);
    gbox = c.take<float>((size_t)P * ((N + 63) / 64) * 8, 16);
    cells = c.take<int>((size_t)P * kCellInts, 16);
    packed = c.take<float>((size_t)P * N * 3, 16);
    ssort = c.take<float>((size_t)P * N, 16);
    keys = c.take<unsigned long long>((size_t)P * N, 16);
  }
};

bool iss_served(int P, int N, int M) {
  return P > 0 && N > 0 && M > 0 && P <= kMaxClouds && N <= kMaxN && M <= kMaxKeep;
}

}  // namespace

DH3D_API size_t dh3d_iss_keypoints_ws_bytes(int P, int N, int M) { return iss_served(P, N, M) ? carve_bytes<IssWs>(P, N) : 0; }

DH3D_API int dh3d_iss_keypoints(const float *xyz, long long stride, const int32_t *count, const float *radii,
                                const float *saliency_in, int P, int N, double gamma_21, double gamma_32, int min_neighbors, int M,
                                float *saliency, int32_t *num_nbr, double *lam, int32_t *ids, int32_t *kp_count, void *ws,
                                size_t ws_bytes, void *stream) {
  DH3D_REQUIRE(xyz && radii && saliency && num_nbr && ids && kp_count && ws);
  DH3D_REQUIRE(stride >= 3 && P > 0 && N > 0 && M > 0 && min_neighbors >= 1);
  DH3D_REQUIRE(gamma_21 > 0.0 && gamma_21 <= 1.0 && gamma_32 > 0.0 && gamma_32 <= 1.0);  // (NaN fails both)
  DH3D_SUPPORTED(iss_served(P, N, M));
  DH3D_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 15) == 0 && ws_bytes >= carve_bytes<IssWs>(P, N));
  Carve carve(ws);
  const IssWs w(carve, P, N);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cloud_pack_kernel, dim3(dh3d_cdiv(N, kPackThreads), P), dim3(kPackThreads), 0, s, xyz, stride, N, count,
                     w.packed);
  const int st = dh3d_spatial_sort_cells(w.packed, P, N, reinterpret_cast<float *>(w.sorted), w.gbox, w.cells, stream);
  if (st != DH3D_OK) return st;
  const dim3 grid(dh3d_cdiv(N, kThreads), P);
  hipLaunchKernelGGL(iss_moments_kernel, grid, dim3(kThreads), 0, s, w.sorted, w.gbox, w.cells, count, radii, saliency_in, N,
                     gamma_21, gamma_32, min_neighbors, saliency, num_nbr, lam, w.ssort);
  hipLaunchKernelGGL(iss_nms_kernel, grid, dim3(kThreads), 0, s, w.sorted, w.gbox, w.cells, count, radii, w.ssort, num_nbr, N,
                     min_neighbors, w.keys);
  hipLaunchKernelGGL(iss_select_kernel, dim3(P), dim3(kSelThreads), 0, s, w.keys, N, M, ids, kp_count);
  return dh3d_launch_status();
}
