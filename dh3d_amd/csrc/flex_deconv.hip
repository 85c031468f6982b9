// flex_convolution_transpose (FlexDeconv, user_ops/ops/flex_deconv.cc): every source point n SPREADS its centre's features
// to its neighbours.  With s = nbr[b,0,n] (the centre) and m = nbr[b,k,n] (the target), for every (n, k):
//     out[b,:,m] += sum_din f[b,din,s] * (bias[din,:] + sum_dp theta[dp,din,:] * (p[b,dp,m] - p[b,dp,s]))
//
// Section A (any shape, f32 and f64): the reference formulation, one thread per (point, 16 output channels), the din sum
// in registers and one f32/f64 atomic per (n, k, dout) into the zeroed output.
//
// Section A' (Dp = 3, Din % 4 == 0, Dout % 4 == 0): the factorised form of flex_bwd.hip read through INVERTED neighbour
// lists, so that nothing is scattered:
//   forward   out = S' @ Wcat,  S'0[m] = sum_{(n,k)->m} f[s_n],  S'd[m] = sum_{(n,k)->m} (p[m] - p[s_n])_d f[s_n]
//   backward  Q[n] = [sum_k g[m_k] | sum_k (p[m_k] - p[s_n])_d g[m_k]]       (flex_S_kernel of flex_bwd.hip, rank0 = 1)
//             Q~[c] = sum_{n: s_n = c} Q[n]                                    (the rank-0 inverted lists, K = 1)
//             grad_f = Q~ @ Wcat'  (Wcat' [4*Dout, Din]: the blocks of Wcat transposed),  [bias; theta]' = Q~^T f
// The inverted lists are a CSR per batch: in-degree count, exclusive scan, atomic fill, then every list re-ordered by
// edge id n*K + k (a rank sort: an entry's place = the number of smaller edge ids in its list), so every sum over a
// list runs in one fixed order and the forward and grad_features are bitwise reproducible (as long as the GEMM's
// reduction, 4*Din resp. 4*Dout, is not split: <= 256).
// Skew: a list of more than kChunk entries (a "hub") is summed in kChunk-entry chunks by separate lanes into partial
// rows, which a second pass adds per target in chunk order (cdna_hip_programming.md, Appendix B "Scatter / gather"):
// the main gather skips such targets, so a kNN neighbourhood (in-degree ~K) pays two empty launches for it.
#include "flex_common.h"
#include "wave_ops.h"

namespace {

constexpr int kChunk = 64;  // inverted-list entries one lane sums; longer lists are split
constexpr int kScanThreads = 1024;

// ------------------------------------------------------------------ section A: reference formulation
template <typename T>
__global__ __launch_bounds__(kPts) void flex_deconv_fwd_generic(const T *__restrict__ feat, const T *__restrict__ theta,
                                                              const T *__restrict__ bias, const int32_t *__restrict__ nbr,
                                                              const T *__restrict__ pos, int N, int K, int Dp, int Din,
                                                              int Dout, T *__restrict__ out) {
  const int b = blockIdx.z;
  const int n = blockIdx.x * kPts + threadIdx.x;
  const int o0 = blockIdx.y * kDT;
  if (n >= N) return;
  const int s = AT3(nbr, b, 0, n, K, N);
  T ps[kMaxDp];
  for (int dp = 0; dp < Dp; ++dp) ps[dp] = AT3(pos, b, dp, s, Dp, N);
  for (int k = 0; k < K; ++k) {
    const int m = AT3(nbr, b, k, n, K, N);
    T q[kMaxDp];
    for (int dp = 0; dp < Dp; ++dp) q[dp] = AT3(pos, b, dp, m, Dp, N) - ps[dp];
    T res[kDT];
#pragma unroll
    for (int o = 0; o < kDT; ++o) res[o] = T(0);
    for (int i = 0; i < Din; ++i) {
      const T fs = AT3(feat, b, i, s, Din, N);
#pragma unroll
      for (int o = 0; o < kDT; ++o) {
        if (o0 + o < Dout) {
          T w = bias[(size_t)i * Dout + o0 + o];
          for (int dp = 0; dp < Dp; ++dp) w += q[dp] * theta[((size_t)dp * Din + i) * Dout + o0 + o];
          res[o] += w * fs;
        }
      }
    }
#pragma unroll
    for (int o = 0; o < kDT; ++o)
      if (o0 + o < Dout) atomicAdd(&AT3(out, b, o0 + o, m, Dout, N), res[o]);
  }
}

// grad_f[s_n, j] += sum_k sum_l (bias[j,l] + sum_dp theta[dp,j,l] q_dp) g[m_k, l]: one thread per (point, din), one atomic
template <typename T>
__global__ __launch_bounds__(kPts) void flex_deconv_bwd_feat_generic(const T *__restrict__ theta,
                                                                   const T *__restrict__ bias,
                                                                   const int32_t *__restrict__ nbr,
                                                                   const T *__restrict__ pos, const T *__restrict__ top,
                                                                   int N, int K, int Dp, int Din, int Dout,
                                                                   T *__restrict__ gfeat) {
  const int b = blockIdx.z;
  const int n = blockIdx.x * kPts + threadIdx.x;
  const int j = blockIdx.y;
  if (n >= N) return;
  const int s = AT3(nbr, b, 0, n, K, N);
  T ps[kMaxDp];
  for (int dp = 0; dp < Dp; ++dp) ps[dp] = AT3(pos, b, dp, s, Dp, N);
  T acc = T(0);
  for (int k = 0; k < K; ++k) {
    const int m = AT3(nbr, b, k, n, K, N);
    T q[kMaxDp];
    for (int dp = 0; dp < Dp; ++dp) q[dp] = AT3(pos, b, dp, m, Dp, N) - ps[dp];
    for (int l = 0; l < Dout; ++l) {
      T w = bias[(size_t)j * Dout + l];
      for (int dp = 0; dp < Dp; ++dp) w += theta[((size_t)dp * Din + j) * Dout + l] * q[dp];
      acc += w * AT3(top, b, l, m, Dout, N);
    }
  }
  atomicAdd(&AT3(gfeat, b, j, s, Din, N), acc);
}

// grad_bias[j,l] / grad_theta[dp,j,l]: one block per (din j, dout l), reduced over (b, n, k); plain stores
template <typename T>
__global__ __launch_bounds__(256) void flex_deconv_bwd_theta_generic(const T *__restrict__ feat,
                                                                    const int32_t *__restrict__ nbr,
                                                                    const T *__restrict__ pos, const T *__restrict__ top,
                                                                    int B, int N, int K, int Dp, int Din, int Dout,
                                                                    T *__restrict__ gtheta, T *__restrict__ gbias) {
  __shared__ T s_red[4];
  const int l = blockIdx.x, j = blockIdx.y;
  T sb = T(0), st[kMaxDp];
  for (int dp = 0; dp < kMaxDp; ++dp) st[dp] = T(0);
  for (long long e = threadIdx.x; e < (long long)B * N; e += 256) {
    const int b = (int)(e / N), n = (int)(e % N);
    const int s = AT3(nbr, b, 0, n, K, N);
    const T f = AT3(feat, b, j, s, Din, N);
    for (int k = 0; k < K; ++k) {
      const int m = AT3(nbr, b, k, n, K, N);
      const T ft = f * AT3(top, b, l, m, Dout, N);
      sb += ft;
      for (int dp = 0; dp < Dp; ++dp) st[dp] += ft * (AT3(pos, b, dp, m, Dp, N) - AT3(pos, b, dp, s, Dp, N));
    }
  }
  const T rb = block_sum_256(sb, s_red);
  if (threadIdx.x == 0) gbias[(size_t)j * Dout + l] = rb;
  for (int dp = 0; dp < Dp; ++dp) {
    const T r = block_sum_256(st[dp], s_red);
    if (threadIdx.x == 0) gtheta[((size_t)dp * Din + j) * Dout + l] = r;
  }
}

template <typename T>
int fwd_launch(const T *features, const T *theta, const T *bias, const int32_t *neighborhood, const T *positions, int B,
               int N, int K, int Dp, int Din, int Dout, T *output, void *stream) {
  DH3D_REQUIRE(features && theta && bias && neighborhood && positions && output);
  DH3D_REQUIRE(B > 0 && N > 0 && K > 0 && Dp > 0 && Din > 0 && Dout > 0);
  DH3D_SUPPORTED(Dp <= kMaxDp && B <= 65535 && dh3d_cdiv(Dout, kDT) <= 65535);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(output, 0, sizeof(T) * (size_t)B * Dout * N, s) != hipSuccess) return DH3D_ERR_LAUNCH;
  hipLaunchKernelGGL(flex_deconv_fwd_generic<T>, dim3(dh3d_cdiv(N, kPts), dh3d_cdiv(Dout, kDT), B), dim3(kPts), 0, s,
                     features, theta, bias, neighborhood, positions, N, K, Dp, Din, Dout, output);
  return dh3d_launch_status();
}

template <typename T>
int bwd_launch(const T *features, const T *theta, const T *bias, const int32_t *neighborhood, const T *positions,
               const T *topdiff, int B, int N, int K, int Dp, int Din, int Dout, T *grad_features, T *grad_theta,
               T *grad_bias, void *stream) {
  DH3D_REQUIRE(features && theta && bias && neighborhood && positions && topdiff && grad_features && grad_theta &&
               grad_bias);
  DH3D_REQUIRE(B > 0 && N > 0 && K > 0 && Dp > 0 && Din > 0 && Dout > 0);
  DH3D_SUPPORTED(Dp <= kMaxDp && B <= 65535 && Din <= 65535 && Dout <= 65535);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(grad_features, 0, sizeof(T) * (size_t)B * Din * N, s) != hipSuccess) return DH3D_ERR_LAUNCH;
  hipLaunchKernelGGL(flex_deconv_bwd_feat_generic<T>, dim3(dh3d_cdiv(N, kPts), Din, B), dim3(kPts), 0, s, theta, bias,
                     neighborhood, positions, topdiff, N, K, Dp, Din, Dout, grad_features);
  hipLaunchKernelGGL(flex_deconv_bwd_theta_generic<T>, dim3(Dout, Din), dim3(256), 0, s, features, neighborhood,
                     positions, topdiff, B, N, K, Dp, Din, Dout, grad_theta, grad_bias);
  return dh3d_launch_status();
}

// ------------------------------------------------------------------ section A': inverted neighbour lists
// A "view" of the point-major lists nbr [R, K]: the first Ku ranks of every row (Ku = K: all edges; Ku = 1: the centres).
// Edge e = row * Ku + k, its target t = cloud base + nbr[row * K + k]; entries are stored as the edge's id WITHIN its
// cloud ((row - base) * Ku + k < N * Ku < 2^31), which orders them as the global edge ids do.

__global__ __launch_bounds__(256) void csr_count_kernel(const int32_t *__restrict__ nbr, long long R, int N, int K, int Ku,
                                                       int32_t *__restrict__ cnt) {
  const long long E = R * Ku;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
    const long long row = e / Ku;
    const int k = (int)(e - row * Ku);
    atomicAdd(&cnt[(row / N) * N + nbr[row * K + k]], 1);
  }
}

// Exclusive scans of the in-degree (off, 64-bit) and of the partial rows of lists longer than kChunk (part); resets cnt
// to 0 for the fill's cursors.  One workgroup: every thread owns a contiguous segment of the R targets.
__device__ __forceinline__ long long parts_of(int d) { return d > kChunk ? (d + kChunk - 1) / kChunk : 0; }

__global__ __launch_bounds__(kScanThreads) void csr_scan_kernel(int32_t *__restrict__ cnt, long long R,
                                                               long long *__restrict__ off, long long *__restrict__ part) {
  __shared__ long long s_a[kScanThreads / 64], s_b[kScanThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long seg = (R + kScanThreads - 1) / kScanThreads;
  const long long lo = tid * seg, hi = lo + seg < R ? lo + seg : R;
  long long a = 0, p = 0;
  for (long long t0 = lo; t0 < hi; t0 += 16) {  // 16 loads in flight per thread
    int d[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) d[u] = t0 + u < hi ? cnt[t0 + u] : 0;
#pragma unroll
    for (int u = 0; u < 16; ++u) { a += d[u]; p += parts_of(d[u]); }
  }
  // inclusive scan of the (a, p) pairs over the workgroup
  const long long ia = wave_incl_scan(a), ip = wave_incl_scan(p);
  if (lane == 63) { s_a[wave] = ia; s_b[wave] = ip; }
  __syncthreads();
  long long ba = 0, bp = 0, ta = 0, tp = 0;
  for (int w = 0; w < kScanThreads / 64; ++w) {
    if (w < wave) { ba += s_a[w]; bp += s_b[w]; }
    ta += s_a[w]; tp += s_b[w];
  }
  long long ra = ba + ia - a, rp = bp + ip - p;  // exclusive prefix of this thread's segment
  for (long long t0 = lo; t0 < hi; t0 += 16) {
    int d[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) d[u] = t0 + u < hi ? cnt[t0 + u] : 0;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      if (t0 + u < hi) {
        off[t0 + u] = ra;
        part[t0 + u] = rp;
        cnt[t0 + u] = 0;
      }
      ra += d[u];
      rp += parts_of(d[u]);
    }
  }
  if (tid == 0) { off[R] = ta; part[R] = tp; }
}

__global__ __launch_bounds__(256) void csr_fill_kernel(const int32_t *__restrict__ nbr, long long R, int N, int K, int Ku,
                                                      const long long *__restrict__ off, int32_t *__restrict__ cur,
                                                      int32_t *__restrict__ ids) {
  const long long E = R * Ku;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
    const long long row = e / Ku;
    const int k = (int)(e - row * Ku);
    const long long base = (row / N) * N;
    const long long t = base + nbr[row * K + k];
    ids[off[t] + atomicAdd(&cur[t], 1)] = (int32_t)((row - base) * Ku + k);
  }
}

// Puts every entry at its place in ascending edge-id order (ids within a list are distinct) and stores its PAYLOAD:
// the source point's centre nbr[row * K] (centre = 1) or the source point itself (centre = 0), as a cloud-local index.
__global__ __launch_bounds__(256) void csr_order_kernel(const int32_t *__restrict__ nbr, long long R, int N, int K, int Ku,
                                                       int centre, const long long *__restrict__ off,
                                                       const int32_t *__restrict__ ids, int32_t *__restrict__ payload) {
  const long long E = R * Ku;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
    const long long row = e / Ku;
    const int k = (int)(e - row * Ku);
    const long long base = (row / N) * N;
    const long long t = base + nbr[row * K + k];
    const int32_t v = (int32_t)((row - base) * Ku + k);
    const long long b0 = off[t], b1 = off[t + 1];
    long long rank = 0;
#pragma unroll 8
    for (long long i = b0; i < b1; ++i) rank += ids[i] < v;
    payload[b0 + rank] = centre ? nbr[row * K] : (int32_t)(row - base);
  }
}

// Sum of one list range [i0, i1) for target t and channels [c4, c4 + 4).  FLEX: the four components of S' (rows of
// 4*D: S'0 | S'x | S'y | S'z); else the plain sum (rows of D).
template <bool FLEX>
struct ListSum {
  float4 s0, sx, sy, sz;
  __device__ __forceinline__ void zero() {
    s0 = make_float4(0.f, 0.f, 0.f, 0.f); sx = s0; sy = s0; sz = s0;
  }
  __device__ __forceinline__ void run(const float *__restrict__ feat, const float *__restrict__ xyz,
                                      const int32_t *__restrict__ payload, long long base, long long t, long long i0,
                                      long long i1, int D, int c4) {
    float px = 0.f, py = 0.f, pz = 0.f;
    if (FLEX) { px = xyz[t * 3]; py = xyz[t * 3 + 1]; pz = xyz[t * 3 + 2]; }
#pragma unroll 4
    for (long long i = i0; i < i1; ++i) {
      const long long g = base + payload[i];
      const float4 f = *reinterpret_cast<const float4 *>(feat + g * D + c4);
      s0.x += f.x; s0.y += f.y; s0.z += f.z; s0.w += f.w;
      if (FLEX) {  // (p[m] - p[s]) per edge, as flex_S_kernel forms it
        const float dx = px - xyz[g * 3], dy = py - xyz[g * 3 + 1], dz = pz - xyz[g * 3 + 2];
        sx.x = fmaf(dx, f.x, sx.x); sx.y = fmaf(dx, f.y, sx.y); sx.z = fmaf(dx, f.z, sx.z); sx.w = fmaf(dx, f.w, sx.w);
        sy.x = fmaf(dy, f.x, sy.x); sy.y = fmaf(dy, f.y, sy.y); sy.z = fmaf(dy, f.z, sy.z); sy.w = fmaf(dy, f.w, sy.w);
        sz.x = fmaf(dz, f.x, sz.x); sz.y = fmaf(dz, f.y, sz.y); sz.z = fmaf(dz, f.z, sz.z); sz.w = fmaf(dz, f.w, sz.w);
      }
    }
  }
  __device__ __forceinline__ void add(const float *row, int D) {
    auto acc = [](float4 &a, const float *p) {
      const float4 v = *reinterpret_cast<const float4 *>(p);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    };
    acc(s0, row);
    if (FLEX) { acc(sx, row + D); acc(sy, row + 2 * D); acc(sz, row + 3 * D); }
  }
  __device__ __forceinline__ void store(float *row, int D) const {
    *reinterpret_cast<float4 *>(row) = s0;
    if (FLEX) {
      *reinterpret_cast<float4 *>(row + D) = sx;
      *reinterpret_cast<float4 *>(row + 2 * D) = sy;
      *reinterpret_cast<float4 *>(row + 3 * D) = sz;
    }
  }
};

// One lane = (target, 4 channels), lists of up to kChunk entries; longer ones are left to the two kernels below.
template <bool FLEX>
__global__ __launch_bounds__(256) void csr_gather_kernel(const float *__restrict__ feat, const float *__restrict__ xyz,
                                                        const long long *__restrict__ off,
                                                        const int32_t *__restrict__ payload, long long R, int N, int D,
                                                        float *__restrict__ out) {
  const int lpr = D / 4, W = FLEX ? 4 * D : D;
  const long long total = R * lpr;
  for (long long e = (long long)dh3d_xcd_remap(blockIdx.x, gridDim.x) * 256 + threadIdx.x; e < total;
       e += (long long)gridDim.x * 256) {
    const long long t = e / lpr;
    const int c4 = (int)(e - t * lpr) * 4;
    const long long i0 = off[t], i1 = off[t + 1];
    if (i1 - i0 > kChunk) continue;
    ListSum<FLEX> acc;
    acc.zero();
    acc.run(feat, xyz, payload, (t / N) * N, t, i0, i1, D, c4);
    acc.store(out + t * W + c4, D);
  }
}

// the target whose partial rows hold row j: the last t with part[t] <= j
__device__ __forceinline__ long long part_owner(const long long *__restrict__ part, long long R, long long j) {
  long long lo = 0, hi = R;  // part[lo] <= j < part[hi]
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (part[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

// Long lists, pass 1: partial row j = the sum of chunk (j - part[t]) of target t's list.  The number of partial rows is
// read on the device (part[R]): a fixed grid, no host round trip.
template <bool FLEX>
__global__ __launch_bounds__(256) void csr_chunk_kernel(const float *__restrict__ feat, const float *__restrict__ xyz,
                                                       const long long *__restrict__ off,
                                                       const long long *__restrict__ part,
                                                       const int32_t *__restrict__ payload, long long R, int N, int D,
                                                       float *__restrict__ partial) {
  const int lpr = D / 4, W = FLEX ? 4 * D : D;
  const long long total = part[R] * lpr;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long j = e / lpr;
    const int c4 = (int)(e - j * lpr) * 4;
    const long long t = part_owner(part, R, j);
    const long long i0 = off[t] + (j - part[t]) * kChunk, i1 = min(i0 + kChunk, off[t + 1]);
    ListSum<FLEX> acc;
    acc.zero();
    acc.run(feat, xyz, payload, (t / N) * N, t, i0, i1, D, c4);
    acc.store(partial + j * W + c4, D);
  }
}

// Long lists, pass 2: each target's partial rows added in chunk order (by the lanes of its first partial row).
template <bool FLEX>
__global__ __launch_bounds__(256) void csr_combine_kernel(const long long *__restrict__ part, long long R, int D,
                                                         const float *__restrict__ partial, float *__restrict__ out) {
  const int lpr = D / 4, W = FLEX ? 4 * D : D;
  const long long total = part[R] * lpr;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const long long j = e / lpr;
    const int c4 = (int)(e - j * lpr) * 4;
    const long long t = part_owner(part, R, j);
    if (part[t] != j) continue;
    ListSum<FLEX> acc;
    acc.zero();
    for (long long r = j; r < part[t + 1]; ++r) acc.add(partial + r * W + c4, D);
    acc.store(out + t * W + c4, D);
  }
}

// Workspace of one inverted-list sum over the first Ku ranks of R rows, rows of W floats.
struct CsrWs {
  int32_t *cnt, *ids, *payload;
  long long *off, *part;
  long long P;  // partial rows: a list of d > kChunk entries has < 2d / kChunk
  float *partial;
  CsrWs() = default;
  CsrWs(Carve &c, size_t R, size_t Ku, size_t W) {
    const size_t E = R * Ku;
    P = (long long)(2 * (E / kChunk) + 1);
    cnt = c.take<int32_t>(R, 256);
    off = c.take<long long>(R + 1, 256);
    part = c.take<long long>(R + 1, 256);
    ids = c.take<int32_t>(E, 256);
    payload = c.take<int32_t>(E, 256);
    partial = c.take<float>((size_t)P * W, 256);
  }
};

// out[t, :] (rows of 4*D when flex, else D) = the sum over t's inverted list (first Ku ranks of nbr) of feat rows, in
// ascending edge order.  `w`: CsrWs(R, Ku, FLEX ? 4 * D : D).
template <bool FLEX>
int csr_sum(const float *feat, const float *xyz, const int32_t *nbr, long long R, int N, int K, int Ku, int centre, int D,
            const CsrWs &w, float *out, hipStream_t s) {
  const long long E = R * Ku;
  if (hipMemsetAsync(w.cnt, 0, sizeof(int32_t) * R, s) != hipSuccess) return DH3D_ERR_LAUNCH;
  hipLaunchKernelGGL(csr_count_kernel, dim3(flat_grid256(E, 4096)), dim3(256), 0, s, nbr, R, N, K, Ku, w.cnt);
  hipLaunchKernelGGL(csr_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, w.cnt, R, w.off, w.part);
  hipLaunchKernelGGL(csr_fill_kernel, dim3(flat_grid256(E, 4096)), dim3(256), 0, s, nbr, R, N, K, Ku, w.off, w.cnt, w.ids);
  hipLaunchKernelGGL(csr_order_kernel, dim3(flat_grid256(E, 4096)), dim3(256), 0, s, nbr, R, N, K, Ku, centre, w.off,
                     w.ids, w.payload);
  hipLaunchKernelGGL(csr_gather_kernel<FLEX>, dim3(flat_grid256(R * (D / 4), 8192)), dim3(256), 0, s, feat, xyz, w.off,
                     w.payload, R, N, D, out);
  hipLaunchKernelGGL(csr_chunk_kernel<FLEX>, dim3(flat_grid256(w.P * (D / 4), 1024)), dim3(256), 0, s, feat, xyz, w.off,
                     w.part, w.payload, R, N, D, w.partial);
  hipLaunchKernelGGL(csr_combine_kernel<FLEX>, dim3(flat_grid256(w.P * (D / 4), 1024)), dim3(256), 0, s, w.part, R, D,
                     w.partial, out);
  return dh3d_launch_status();
}

// Shapes A' serves: Dp = 3, channel counts multiples of four, edge ids and GEMM extents within 32 bits.
bool fast_shape(int B, int N, int K, int Dp, int Din, int Dout) {
  if (B <= 0 || N <= 0 || K <= 0 || Dp != 3 || Din <= 0 || Dout <= 0 || Din % 4 || Dout % 4) return false;
  const size_t R = (size_t)B * N, Cmax = (size_t)(Din > Dout ? Din : Dout);
  return (size_t)N * K < (1ull << 31) && R * K < (1ull << 40) && R * 4 * Cmax < (1ull << 31);
}

}  // namespace

// ------------------------------------------------------------------ section A entry points
#define DH3D_FLEX_DECONV_API(SUFFIX, T)                                                                               \
  DH3D_API int dh3d_flex_deconv_fwd##SUFFIX(const T *features, const T *theta, const T *bias,                        \
                                            const int32_t *neighborhood, const T *positions, int B, int N, int K,    \
                                            int Dp, int Din, int Dout, T *output, void *stream) {                    \
    return fwd_launch<T>(features, theta, bias, neighborhood, positions, B, N, K, Dp, Din, Dout, output, stream);    \
  }                                                                                                                   \
  DH3D_API int dh3d_flex_deconv_bwd##SUFFIX(const T *features, const T *theta, const T *bias,                        \
                                            const int32_t *neighborhood, const T *positions, const T *topdiff, int B, \
                                            int N, int K, int Dp, int Din, int Dout, T *grad_features, T *grad_theta, \
                                            T *grad_bias, void *stream) {                                            \
    return bwd_launch<T>(features, theta, bias, neighborhood, positions, topdiff, B, N, K, Dp, Din, Dout,            \
                         grad_features, grad_theta, grad_bias, stream);                                              \
  }
DH3D_FLEX_DECONV_API(, float)
DH3D_FLEX_DECONV_API(_f64, double)
#undef DH3D_FLEX_DECONV_API

// ------------------------------------------------------------------ section A' entry points
namespace {

// Both layouts: R = B * N point-major rows, each segment rounded up to 256 bytes.
struct DeconvFwdWs {
  PointMajor in{};
  float *Wcat, *out, *S;
  CsrWs csr;
  DeconvFwdWs(Carve &c, size_t R, int K, int Din, int Dout) {
    in.f = c.take<float>(R * Din, 256);
    in.nbr = c.take<int32_t>(R * K, 256);
    in.xyz = c.take<float>(R * 3, 256);
    Wcat = c.take<float>((size_t)4 * Din * Dout, 256);  // [bias; theta]: [4*Din, Dout]
    out = c.take<float>(R * Dout, 256);
    S = c.take<float>(R * 4 * Din, 256);
    csr = CsrWs(c, R, K, 4 * (size_t)Din);
  }
};

struct DeconvBwdWs {
  PointMajor in{};
  float *df, *Q, *Qc, *WT, *dW;
  CsrWs csr;
  DeconvBwdWs(Carve &c, size_t R, int K, int Din, int Dout) {
    in.f = c.take<float>(R * Din, 256);
    df = c.take<float>(R * Din, 256);
    in.nbr = c.take<int32_t>(R * K, 256);
    in.xyz = c.take<float>(R * 3, 256);
    in.g = c.take<float>(R * Dout, 256);
    Q = c.take<float>(R * 4 * Dout, 256);
    Qc = c.take<float>(R * 4 * Dout, 256);
    WT = c.take<float>((size_t)4 * Dout * Din, 256);  // [bias'; theta_d']: [4*Dout, Din]
    dW = c.take<float>((size_t)4 * Dout * Din, 256);  // Q~^T f: [4*Dout, Din]
    csr = CsrWs(c, R, 1, 4 * (size_t)Dout);
  }
};

// [rows, cols] -> [cols, rows] of one plane (b) and of three (t): [bias; theta] <-> [bias'; theta_d']
int transpose_planes(const float *b_in, const float *t_in, float *b_out, float *t_out, int rows, int cols, hipStream_t s) {
  const int st = dh3d_internal_transpose32(b_in, b_out, 1, rows, cols, 0, 0, s);
  return st != DH3D_OK ? st : dh3d_internal_transpose32(t_in, t_out, 3, rows, cols, 0, 0, s);
}

}  // namespace

DH3D_API size_t dh3d_flex_deconv_fwd_workspace_bytes(int B, int N, int K, int Dp, int Din, int Dout) {
  if (!fast_shape(B, N, K, Dp, Din, Dout)) return 0;
  return carve_bytes<DeconvFwdWs>((size_t)B * N, K, Din, Dout);
}

DH3D_API int dh3d_flex_deconv_fwd_ws(const float *features, const float *theta, const float *bias,
                                     const int32_t *neighborhood, const float *positions, int B, int N, int K, int Dp,
                                     int Din, int Dout, float *output, void *workspace, size_t workspace_bytes,
                                     void *stream) {
  DH3D_REQUIRE(features && theta && bias && neighborhood && positions && output && workspace);
  DH3D_REQUIRE(B > 0 && N > 0 && K > 0 && Dp > 0 && Din > 0 && Dout > 0);
  DH3D_SUPPORTED(fast_shape(B, N, K, Dp, Din, Dout));
  const size_t R = (size_t)B * N;
  Carve c(workspace);
  const DeconvFwdWs w(c, R, K, Din, Dout);
  DH3D_REQUIRE(workspace_bytes >= c.bytes());
  hipStream_t s = (hipStream_t)stream;
  int st = flex_to_point_major(w.in, features, neighborhood, positions, nullptr, B, N, K, Din, Dout, s);
  if (st != DH3D_OK) return st;
  if ((st = flex_build_wcat(bias, theta, Din, Dout, w.Wcat, s)) != DH3D_OK) return st;
  if ((st = csr_sum<true>(w.in.f, w.in.xyz, w.in.nbr, (long long)R, N, K, K, 1, Din, w.csr, w.S, s)) != DH3D_OK) return st;
  st = dh3d_internal_gemm(false, w.S, 4 * Din, w.Wcat, Dout, w.out, Dout, (int)R, Dout, 4 * Din, nullptr, 0, false, s);
  if (st != DH3D_OK) return st;
  return dh3d_internal_transpose32(w.out, output, B, N, Dout, 0, 0, s);
}

DH3D_API size_t dh3d_flex_deconv_bwd_workspace_bytes(int B, int N, int K, int Dp, int Din, int Dout) {
  if (!fast_shape(B, N, K, Dp, Din, Dout)) return 0;
  return carve_bytes<DeconvBwdWs>((size_t)B * N, K, Din, Dout);
}

DH3D_API int dh3d_flex_deconv_bwd_ws(const float *features, const float *theta, const float *bias,
                                     const int32_t *neighborhood, const float *positions, const float *topdiff, int B,
                                     int N, int K, int Dp, int Din, int Dout, float *grad_features, float *grad_theta,
                                     float *grad_bias, void *workspace, size_t workspace_bytes, void *stream) {
  DH3D_REQUIRE(features && theta && bias && neighborhood && positions && topdiff && grad_features && grad_theta &&
               grad_bias && workspace);
  DH3D_REQUIRE(B > 0 && N > 0 && K > 0 && Dp > 0 && Din > 0 && Dout > 0);
  DH3D_SUPPORTED(fast_shape(B, N, K, Dp, Din, Dout));
  const size_t R = (size_t)B * N;
  const int KQ = 4 * Dout;
  Carve c(workspace);
  const DeconvBwdWs w(c, R, K, Din, Dout);
  DH3D_REQUIRE(workspace_bytes >= c.bytes());
  hipStream_t s = (hipStream_t)stream;
  const size_t plane = (size_t)Dout * Din;
  int st = flex_to_point_major(w.in, features, neighborhood, positions, topdiff, B, N, K, Din, Dout, s);
  if (st != DH3D_OK) return st;
  // Q[n] = [sum_k g[m_k] | sum_k (p[m_k] - p[s_n])_d g[m_k]]: flex_conv's S of the upstream gradient, centred on rank 0
  if ((st = dh3d_internal_flex_S(w.in.g, w.in.xyz, w.in.nbr, (long long)R, N, K, Dout, 1, w.Q, s)) != DH3D_OK) return st;
  // Q~[c] = sum over the points n whose centre is c (the rank-0 inverted lists) of Q[n]
  if ((st = csr_sum<false>(w.Q, nullptr, w.in.nbr, (long long)R, N, K, 1, 0, KQ, w.csr, w.Qc, s)) != DH3D_OK) return st;
  if ((st = transpose_planes(bias, theta, w.WT, w.WT + plane, Din, Dout, s)) != DH3D_OK) return st;
  // grad_f = Q~ @ [bias'; theta_d'] ;  [grad_bias'; grad_theta'] = Q~^T f  (split-K tn GEMM: f32 atomics)
  st = dh3d_internal_gemm(false, w.Qc, KQ, w.WT, Din, w.df, Din, (int)R, Din, KQ, nullptr, 0, false, s);
  if (st != DH3D_OK) return st;
  st = dh3d_internal_gemm(true, w.Qc, KQ, w.in.f, Din, w.dW, Din, KQ, Din, (int)R, nullptr, 0, false, s);
  if (st != DH3D_OK) return st;
  if ((st = transpose_planes(w.dW, w.dW + plane, grad_bias, grad_theta, Dout, Din, s)) != DH3D_OK) return st;
  return dh3d_internal_transpose32(w.df, grad_features, B, N, Din, 0, 0, s);
}
