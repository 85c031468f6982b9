// Scan Context for gfx950 (Kim & Kim, "Scan Context: Egocentric Spatial Descriptor for Place Recognition within 3D Point
// Cloud Map", IROS 2018): the rings x sectors polar height image of a cloud with its ring key, and the column-shifted
// cosine distance of such images.  include/dh3d_hip.h dh3d_scan_context / dh3d_scan_context_distance state the contract; no
// allocation, no host sync, launches one after the other on the caller's stream (graph-capturable, no parallel branches).
//   scan_context_clear_kernel desc = 0: an empty bin, and the identity of the unsigned maximum below.  A kernel, not
//                             hipMemsetAsync: captured in a graph together with the allocation of desc, the memset node left
//                             stale words in desc on replays that followed an eager call (seen on an MI355X; the
//                             kernel node does not, tests/test_scan_context_gpu.py replays between eager calls).
//   scan_context_bins_kernel  grid (ceil(N / 2048), P), 256 threads.  A workgroup takes 2048 rows of one cloud (8 a thread, read
//                             once, coalesced), keeps the Nr x Ns bins in LDS as the bit patterns of the heights -- a counted
//                             height is > 0, so its bits order as an unsigned integer -- and folds every point in with an LDS
//                             atomicMax.  The two tables sit in LDS; ring and sector are found by bisection (at most 5 + 6
//                             steps), which returns the count the header defines: the ring predicate is exactly monotone, the
//                             sector predicate is monotone in k for every input (see sector_of).  Then one global atomicMax
//                             per non-empty bin: a maximum does not depend on arrival order, so desc is bit-defined (the rule
//                             for integer atomics prepare.hip follows).  Several workgroups per cloud: P = 1 at N = 131072
//                             still makes 64 of them.
//   scan_context_keys_kernel  grid P, 64 threads: the cloud's image through LDS, thread r sums ring r in sector order.
//   scan_context_distance_kernel  grid Q, 256 threads.  The query's columns, each divided by its norm (an empty column: zeros),
//                             stay in LDS as float64 [ring][sector] for all C candidates; a candidate is read from the map
//                             once, coalesced, and scaled in LDS.  With W = Ns / 4, thread (g, part) owns the four shifts
//                             g + k W and, per pass, the four query columns j0 + u W: the candidate column of (u, k) is
//                             j0 + g + (u + k) W, so a ring costs 4 + 7 LDS reads for 16 fma (1.4 fma per read instead of
//                             0.5), and lanes with consecutive g read consecutive candidate addresses.  Partial sums meet
//                             in LDS and are added in part order, so a result does not depend on the run; wave 0 takes the
//                             minimum by (d, shift), and after the last candidate ranks the C slots by (dist, id, slot).
//                             The sums use fma: the header leaves their rounding free.
// Compiled without contraction (csrc/Makefile EXACT): the sector predicate is two products and a subtraction.
#include "common.h"
#include "keys.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 2048;        // rows of a cloud per workgroup
constexpr int kMaxRings = 32;
constexpr int kMaxSectors = 128;
constexpr int kMaxBins = kMaxRings * kMaxSectors;
constexpr int kMaxCand = 64;

// the number of i in 1 .. n-1 with r2 >= edge2[i]; edge2 ascends (rounding is monotone), so the predicate is true up to
// that count and false after it
__device__ __forceinline__ int ring_of(const double *edge2, int n, double r2) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (r2 >= edge2[mid]) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// the number of k in 1 .. half-1 with c_k * Y - s_k * X >= 0 for (X, Y) in the upper half plane.  The sign of the rounded
// difference of two rounded products is the sign of their comparison, and a rounded product compares wrongly with another
// only where the exact ones agree to 2^-52: the direction of (X, Y) within 3e-16 rad of direction k.  Directions are at least
// 2 pi / 128 apart, so at most ONE k can deviate from the exact predicate, which is true for k up to some k* and false
// after; whatever that k answers, the computed predicate is true-then-false too, and bisection returns its count.
__device__ __forceinline__ int sector_of(const double *dir, int half, double X, double Y) {
  int lo = 0, hi = half - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    const double a = dir[2 * (mid - 1)] * Y, b = dir[2 * (mid - 1) + 1] * X;
    if (a - b >= 0.0) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void scan_context_clear_kernel(unsigned *__restrict__ desc, long long n) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e < n) desc[e] = 0u;
}

__global__ __launch_bounds__(kThreads) void scan_context_bins_kernel(const float *__restrict__ xyz, long long xyz_stride,
                                                                     const int32_t *__restrict__ count,
                                                                     const float *__restrict__ center,
                                                                     const double *__restrict__ sector_dir,
                                                                     const double *__restrict__ ring_edge2, int N, int Nr, int Ns,
                                                                     float z_offset, unsigned *__restrict__ desc) {
  __shared__ unsigned s_bin[kMaxBins];
  __shared__ double s_dir[kMaxSectors];          // (cos, sin) of k = 1 .. Ns/2 - 1
  __shared__ double s_edge[kMaxRings + 1];
  const int tid = threadIdx.x, p = blockIdx.y;
  const int n = count ? clamp_count(count[p], N) : N;
  const int begin = blockIdx.x * kChunk;
  if (begin >= n) return;                        // (uniform: nothing of this chunk exists)
  const int end = begin + kChunk < n ? begin + kChunk : n;
  const int bins = Nr * Ns, half = Ns >> 1;
  for (int e = tid; e < bins; e += kThreads) s_bin[e] = 0u;
  for (int e = tid; e < 2 * (half - 1); e += kThreads) s_dir[e] = sector_dir[e];
  for (int e = tid; e <= Nr; e += kThreads) s_edge[e] = ring_edge2[e];
  const float cx = center ? center[2 * p] : 0.f, cy = center ? center[2 * p + 1] : 0.f;
  __syncthreads();
  const double limit = s_edge[Nr];
  const float *rows = xyz + (long long)p * N * xyz_stride;
  for (int i = begin + tid; i < end; i += kThreads) {
    const float *row = rows + (long long)i * xyz_stride;
    const float dx = row[0] - cx, dy = row[1] - cy, h = row[2] + z_offset;
    if (!(isfinite(dx) && isfinite(dy) && isfinite(h) && h > 0.f)) continue;
    double X = (double)dx, Y = (double)dy;
    const double r2 = X * X + Y * Y;
    if (!(r2 < limit)) continue;
    const int ring = ring_of(s_edge, Nr, r2);
    int sector = 0;
    if (!(Y > 0.0 || (Y == 0.0 && X > 0.0))) sector = half, X = -X, Y = -Y;
    sector += sector_of(s_dir, half, X, Y);
    atomicMax(&s_bin[ring * Ns + sector], __float_as_uint(h));
  }
  __syncthreads();
  unsigned *out = desc + (long long)p * bins;
  for (int e = tid; e < bins; e += kThreads) {
    const unsigned v = s_bin[e];
    if (v) atomicMax(&out[e], v);
  }
}

__global__ __launch_bounds__(64) void scan_context_keys_kernel(const float *__restrict__ desc, int Nr, int Ns,
                                                               float *__restrict__ ring_key) {
  __shared__ float s_d[kMaxBins];
  const int tid = threadIdx.x, p = blockIdx.x, bins = Nr * Ns;
  const float *d = desc + (long long)p * bins;
  for (int e = tid; e < bins; e += 64) s_d[e] = d[e];
  __syncthreads();
  if (tid < Nr) {
    double sum = 0.0;
    for (int j = 0; j < Ns; ++j) sum += (double)s_d[tid * Ns + j];
    ring_key[(long long)p * Nr + tid] = (float)(sum / (double)Ns);
  }
}

// One descriptor [Nr, Ns] float32 from global memory (read once, coalesced) into LDS as float64 columns of unit length:
// w_j = the sum over the rings (ascending) of D[i, j]^2; s_nz[j] = w_j != 0; s_n[i, j] = D[i, j] / sqrt(w_j), zeros for an
// empty column.  s_inv: Ns doubles.  Three barriers; the first comes before anything is written.
__device__ __forceinline__ void load_unit_columns(const float *__restrict__ d, int Nr, int Ns, double *s_n, double *s_inv,
                                                  int *s_nz) {
  const int tid = threadIdx.x, bins = Nr * Ns;
  float v[kMaxBins / kThreads];
#pragma unroll
  for (int u = 0; u < kMaxBins / kThreads; ++u) v[u] = tid + u * kThreads < bins ? d[tid + u * kThreads] : 0.f;
  __syncthreads();  // the previous descriptor in s_n has been read
#pragma unroll
  for (int u = 0; u < kMaxBins / kThreads; ++u)
    if (tid + u * kThreads < bins) s_n[tid + u * kThreads] = (double)v[u];
  __syncthreads();
  if (tid < Ns) {
    double w = 0.0;
    for (int i = 0; i < Nr; ++i) {
      const double x = s_n[i * Ns + tid];
      w += x * x;
    }
    s_nz[tid] = w != 0.0;
    s_inv[tid] = w != 0.0 ? 1.0 / sqrt(w) : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kMaxBins / kThreads; ++u) {
    const int e = tid + u * kThreads;
    if (e < bins) s_n[e] *= s_inv[e % Ns];
  }
  __syncthreads();
}

size_t distance_lds_bytes(int Nr, int Ns) {
  // qn, cn [Nr][Ns] double; partial sums [<= 1024] double; inv [Ns] double; d_n [Ns] double; counts [<= 1024] int;
  // nzq, nzc [Ns] int; the row's keys [64] (double, int)
  return (size_t)(2 * Nr * Ns + 1024 + 2 * Ns + kMaxCand) * sizeof(double) + (size_t)(1024 + 2 * Ns + kMaxCand) * sizeof(int);
}

__global__ __launch_bounds__(kThreads) void scan_context_distance_kernel(const float *__restrict__ qry,
                                                                         const float *__restrict__ map,
                                                                         const int32_t *__restrict__ map_count,
                                                                         const int32_t *__restrict__ cand, int R, int C, int Nr,
                                                                         int Ns, double *__restrict__ dist,
                                                                         int32_t *__restrict__ shift, int32_t *__restrict__ order) {
  extern __shared__ __align__(16) unsigned char s_raw[];
  const int bins = Nr * Ns;
  double *s_q = reinterpret_cast<double *>(s_raw);   // [Nr][Ns] the query's unit columns
  double *s_c = s_q + bins;                          // [Nr][Ns] the candidate's
  double *s_acc = s_c + bins;                        // [parts][Ns] partial sums
  double *s_inv = s_acc + 1024;                      // [Ns]
  double *s_d = s_inv + Ns;                          // [Ns] d_n
  double *s_kd = s_d + Ns;                           // [64] the row's distances
  int *s_m = reinterpret_cast<int *>(s_kd + kMaxCand);  // [parts][Ns] partial counts
  int *s_nzq = s_m + 1024;                           // [Ns]
  int *s_nzc = s_nzq + Ns;                           // [Ns]
  int *s_kid = s_nzc + Ns;                           // [64] the row's ids
  const int tid = threadIdx.x, lane = tid & 63, q = blockIdx.x;
  const int r = map_count ? clamp_count(*map_count, R) : R;
  const int W = Ns >> 2;                             // shift groups: thread g owns g, g + W, g + 2W, g + 3W
  const int parts = kThreads / W < W ? kThreads / W : W;     // parts * Ns <= 1024; part p owns query column groups p, p + parts, ..
  const int g = tid % W, part = tid / W;

  load_unit_columns(qry + (long long)q * bins, Nr, Ns, s_q, s_inv, s_nzq);

  for (int c = 0; c < C; ++c) {
    const int id = cand[(long long)q * C + c];
    const bool some = id >= 0 && id < r;             // (uniform)
    if (some) {
      load_unit_columns(map + (long long)id * bins, Nr, Ns, s_c, s_inv, s_nzc);
      if (part < parts) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        int m[4] = {0, 0, 0, 0};
        for (int j0 = part; j0 < W; j0 += parts) {
          int cj[7];  // candidate columns (j0 + g + t W) % Ns: query column j0 + u W under shift g + k W meets t = u + k
#pragma unroll
          for (int t = 0; t < 7; ++t) {
            cj[t] = j0 + g + t * W;                  // < 2 Ns
            if (cj[t] >= Ns) cj[t] -= Ns;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] += s_nzq[j0 + u * W] & s_nzc[cj[u + k]];
          for (int i = 0; i < Nr; ++i) {
            double qv[4], cv[7];
#pragma unroll
            for (int u = 0; u < 4; ++u) qv[u] = s_q[i * Ns + j0 + u * W];
#pragma unroll
            for (int t = 0; t < 7; ++t) cv[t] = s_c[i * Ns + cj[t]];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
              for (int k = 0; k < 4; ++k) acc[k] = fma(qv[u], cv[u + k], acc[k]);
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) s_acc[part * Ns + g + k * W] = acc[k], s_m[part * Ns + g + k * W] = m[k];
      }
      __syncthreads();
      if (tid < Ns) {
        double sum = 0.0;
        int m = 0;
        for (int pt = 0; pt < parts; ++pt) sum += s_acc[pt * Ns + tid], m += s_m[pt * Ns + tid];
        s_d[tid] = m ? 1.0 - sum / (double)m : 1.0;
      }
      __syncthreads();
    }
    if (tid < 64) {
      double bd = __longlong_as_double(0x7FF0000000000000ll);
      int bn = -1;
      if (some) {
        for (int n = lane; n < Ns; n += 64) {        // ascending n: a tie keeps the smaller shift
          const double d = s_d[n];
          if (bn < 0 || d < bd) bd = d, bn = n;
        }
        for (int off = 32; off > 0; off >>= 1) {
          const double od = __shfl_xor(bd, off, 64);
          const int on = __shfl_xor(bn, off, 64);
          if (on >= 0 && (bn < 0 || od < bd || (od == bd && on < bn))) bd = od, bn = on;
        }
      }
      if (lane == 0) {
        dist[(long long)q * C + c] = bd;
        shift[(long long)q * C + c] = bn;
        s_kd[c] = bd;
        s_kid[c] = id;
      }
    }
    // (the next candidate's first barrier, inside load_unit_columns, comes before anything of this one is overwritten that
    // wave 0 still reads: s_d is written only after two more barriers)
  }
  __syncthreads();
  if (tid < C) {                                     // C <= 64: rank slot tid by (dist, id, slot)
    const double d = s_kd[tid];
    const int id = s_kid[tid];
    int rank = 0;
    for (int o = 0; o < C; ++o) {
      const double od = s_kd[o];
      const int oid = s_kid[o];
      rank += od < d || (od == d && (oid < id || (oid == id && o < tid)));
    }
    order[(long long)q * C + rank] = tid;
  }
}

}  // namespace

static int grid_ok(int Nr, int Ns) {
  return Nr >= 4 && Nr <= kMaxRings && Nr % 4 == 0 && Ns >= 8 && Ns <= kMaxSectors && Ns % 4 == 0;
}

DH3D_API int dh3d_scan_context(const float *xyz, long long xyz_stride, const int32_t *count, const float *center,
                               const double *sector_dir, const double *ring_edge2, int P, int N, int Nr, int Ns, float z_offset,
                               float *desc, float *ring_key, void *stream) {
  DH3D_REQUIRE(xyz && sector_dir && ring_edge2 && desc && ring_key);
  DH3D_REQUIRE(xyz_stride >= 3 && P > 0 && N > 0 && grid_ok(Nr, Ns));
  DH3D_SUPPORTED(N <= (1 << 20) && P <= 65535);
  hipStream_t s = (hipStream_t)stream;
  const long long cells = (long long)P * Nr * Ns;
  hipLaunchKernelGGL(scan_context_clear_kernel, dim3(dh3d_cdiv(cells, kThreads)), dim3(kThreads), 0, s,
                     reinterpret_cast<unsigned *>(desc), cells);
  if (dh3d_launch_status() != DH3D_OK) return DH3D_ERR_LAUNCH;
  hipLaunchKernelGGL(scan_context_bins_kernel, dim3(dh3d_cdiv(N, kChunk), P), dim3(kThreads), 0, s, xyz, xyz_stride, count,
                     center, sector_dir, ring_edge2, N, Nr, Ns, z_offset, reinterpret_cast<unsigned *>(desc));
  if (dh3d_launch_status() != DH3D_OK) return DH3D_ERR_LAUNCH;
  hipLaunchKernelGGL(scan_context_keys_kernel, dim3(P), dim3(64), 0, s, desc, Nr, Ns, ring_key);
  return dh3d_launch_status();
}

DH3D_API int dh3d_scan_context_distance(const float *qry, const float *map, const int32_t *map_count, const int32_t *cand,
                                        int Q, int R, int C, int Nr, int Ns, double *dist, int32_t *shift, int32_t *order,
                                        void *stream) {
  DH3D_REQUIRE(qry && map && cand && dist && shift && order);
  DH3D_REQUIRE(Q > 0 && R > 0 && C > 0 && C <= kMaxCand && grid_ok(Nr, Ns));
  DH3D_SUPPORTED(Q <= (1 << 20) && R <= (1 << 24));
  DH3D_ALLOW_BIG_LDS(scan_context_distance_kernel);
  hipLaunchKernelGGL(scan_context_distance_kernel, dim3(Q), dim3(kThreads), distance_lds_bytes(Nr, Ns), (hipStream_t)stream, qry,
                     map, map_count, cand, R, C, Nr, Ns, dist, shift, order);
  return dh3d_launch_status();
}
