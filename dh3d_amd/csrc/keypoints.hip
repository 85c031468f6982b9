// Batched keypoint non-maximum suppression for gfx950 (localdesc_extract.py --perform_nms; core/utils.py:15-43) and the
// row gather that fetches only the keypoints' rows.  Same ids, cloud by cloud, as dh3d_amd/utils.py:single_nms, which
// runs the same rule one cloud at a time with host syncs.  Three launches per call, no atomics on global memory, no
// memset, no host sync (graph-capturable):
//   K1 nms_mute_kernel    one thread per point: a' = score (or 1 - score), muted to 0 when the 8th neighbour lies beyond
//                         2.0; one maximum of a' per 256-point block (wave DPP reduction + LDS);
//   K2 nms_keys_kernel    every block reduces its cloud's block maxima -> thr = max * ratio; one thread per point walks its
//                         K neighbours: a point is kept iff no neighbour inside the radius beats rank 0 and a' > thr.  The
//                         point's key is (f32_order_bits(a') << 32) | i, or 0 when it is not kept;
//   K3 nms_select_kernel  one 1024-lane workgroup per cloud: compact the non-zero keys (in place), radix-select the M-th
//                         largest, bitonic-sort the <= M winners in LDS (keys are unique -- the index sits in the low bits
//                         -- so the order is total), write count and ids; all three steps are block_ops.h's.
// Only comparisons, one f32 multiply and 1 - x: exact by construction (compiled without contraction, csrc/Makefile EXACT).
#include "common.h"
#include "keys.h"
#include "block_ops.h"
#include "workspace.h"

namespace {

constexpr int kPtThreads = 256;     // K1 / K2: points per block
constexpr int kSelThreads = 1024;   // K3: one workgroup per cloud
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kMaxKeep = 4096;      // M limit: the winners' sort buffer in LDS (32 KB)
constexpr int kMaxK = 64;           // the kNN kernels' limit

// max over a 256-lane block; every lane must call it (DPP reads all 64 lanes)
__device__ __forceinline__ float block256_max(float v, float *s_red) {
  const float w = wave_max_f32(v);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = w;
  __syncthreads();
  return fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
}

__global__ __launch_bounds__(kPtThreads) void nms_mute_kernel(const float *__restrict__ score, long long sstride, int invert,
                                                              const float *__restrict__ dist, int K,
                                                              const int32_t *__restrict__ num_valid, int N, int remove_noise,
                                                              float *__restrict__ ap, float *__restrict__ bmax) {
  __shared__ float s_red[kPtThreads / 64];
  const int b = blockIdx.y, i = blockIdx.x * kPtThreads + threadIdx.x;
  const int nb = num_valid ? clamp_count(num_valid[b], N) : N;
  float m = -INFINITY;
  if (i < N) {
    const long long p = (long long)b * N + i;
    float a = score[p * sstride];
    if (invert) a = 1.f - a;
    if (remove_noise && K > 7 && dist[p * K + 7] > 2.0f) a = 0.f;
    if (a == 0.f) a = 0.f;  // -0.0 -> +0.0: the key order below must not tell them apart
    ap[p] = a;
    if (i < nb) m = a;
  }
  m = block256_max(m, s_red);
  if (threadIdx.x == 0) bmax[(long long)b * gridDim.x + blockIdx.x] = m;
}

__global__ __launch_bounds__(kPtThreads) void nms_keys_kernel(const float *__restrict__ ap, const float *__restrict__ bmax,
                                                              const int32_t *__restrict__ nn, const float *__restrict__ dist,
                                                              int K, const int32_t *__restrict__ num_valid, int N, float radius,
                                                              float ratio, unsigned long long *__restrict__ keys) {
  __shared__ float s_red[kPtThreads / 64];
  const int b = blockIdx.y, i = blockIdx.x * kPtThreads + threadIdx.x, nblk = gridDim.x;
  const int nb = num_valid ? clamp_count(num_valid[b], N) : N;
  float m = -INFINITY;
  for (int j = threadIdx.x; j < nblk; j += kPtThreads) m = fmaxf(m, bmax[(long long)b * nblk + j]);
  const float thr = block256_max(m, s_red) * ratio;  // f32(max a') * f32(ratio)
  if (i >= N) return;
  const long long p = (long long)b * N + i;
  const float *cloud = ap + (long long)b * N;
  unsigned long long key = 0;
  const float a = ap[p];
  if (i < nb && a > thr) {
    const int32_t *row = nn + p * K;
    const float *drow = dist + p * K;
    // s[r] = a'[nn[r]] inside the ball (a real point), else 0; kept iff s[r] <= s[0] for every r >= 1 (first max wins)
    const int j0 = row[0];
    const float s0 = (drow[0] > radius || j0 < 0 || j0 >= nb) ? 0.f : cloud[j0];
    bool is_max = true;
    for (int r = 1; r < K && is_max; ++r) {
      const int j = row[r];
      const float s = (drow[r] > radius || j < 0 || j >= nb) ? 0.f : cloud[j];
      is_max = !(s > s0);
    }
    if (is_max) key = ((unsigned long long)f32_order_bits(a) << 32) | (unsigned)i;  // (K1 wrote -0 as +0)
  }
  keys[p] = key;
}

__global__ __launch_bounds__(kSelThreads) void nms_select_kernel(unsigned long long *__restrict__ keys, int N, int M,
                                                                 int32_t *__restrict__ count, int32_t *__restrict__ inds) {
  __shared__ unsigned long long s_win[kMaxKeep];
  __shared__ int s_hist[256];
  __shared__ int s_wave[kSelWaves];
  __shared__ int s_sel[2], s_n;
  const int b = blockIdx.x, tid = threadIdx.x;
  unsigned long long *ck = keys + (long long)b * N;

  // (1) compact the non-zero keys to the front, in place, in index order: every store of a chunk lands below the chunk's
  //     end and the chunk was read before the barriers of block_compact_slot
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

  // (3) the winners into LDS (any order), bitonic-sorted descending
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
    inds[(long long)b * M + j] = j < nw ? (int32_t)(unsigned)(s_win[j] & 0xffffffffull) : -1;
  if (tid == 0) count[b] = nw;
}

// dst[b, j, :] = src[b, inds[b, j], :] for j < count[b], zero rows after that (and for an id outside [0, N)); one wave
// per row, 4-byte elements: any C (131 is not 16-byte aligned per row)
__global__ __launch_bounds__(256) void gather_rows_kernel(const float *__restrict__ src, int N, int C,
                                                          const int32_t *__restrict__ inds, const int32_t *__restrict__ count,
                                                          int M, long long rows, float *__restrict__ dst) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int b = (int)(r / M), j = (int)(r % M);
  int id = j < count[b] ? inds[r] : -1;
  if (id >= N) id = -1;
  const float *s = src + ((long long)b * N + (id < 0 ? 0 : id)) * C;
  float *d = dst + r * C;
  for (int c = threadIdx.x & 63; c < C; c += 64) d[c] = id >= 0 ? s[c] : 0.f;
}

struct NmsWs {
  float *ap, *bmax;
  unsigned long long *keys;
  int nblk;
  NmsWs(Carve &c, int B, int N) : nblk(dh3d_cdiv(N, kPtThreads)) {
    ap = c.take<float>((size_t)B * N, 256);
    bmax = c.take<float>((size_t)B * nblk, 256);
    keys = c.take<unsigned long long>((size_t)B * N, 256);
  }
};

}  // namespace

DH3D_API size_t dh3d_keypoint_nms_workspace_bytes(int B, int N, int M) {
  if (B <= 0 || N <= 0 || M <= 0 || M > kMaxKeep) return 0;
  return carve_bytes<NmsWs>(B, N);
}

DH3D_API int dh3d_keypoint_nms(const float *score, long long score_stride, int invert, const int32_t *nn, const float *dist,
                               const int32_t *num_valid, int B, int N, int K, float radius, float ratio, int M,
                               int remove_noise, int32_t *count, int32_t *inds, void *workspace, size_t workspace_bytes,
                               void *stream) {
  DH3D_REQUIRE(score && nn && dist && count && inds && workspace);
  DH3D_REQUIRE(B > 0 && N > 0 && K > 0 && M > 0 && score_stride >= 1);
  DH3D_SUPPORTED(M <= kMaxKeep && K <= kMaxK && B <= 65535);
  Carve c(workspace);
  const NmsWs w(c, B, N);
  DH3D_REQUIRE(workspace_bytes >= c.bytes());
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(nms_mute_kernel, dim3(w.nblk, B), dim3(kPtThreads), 0, s, score, score_stride, invert, dist, K,
                     num_valid, N, remove_noise, w.ap, w.bmax);
  hipLaunchKernelGGL(nms_keys_kernel, dim3(w.nblk, B), dim3(kPtThreads), 0, s, w.ap, w.bmax, nn, dist, K, num_valid, N,
                     radius, ratio, w.keys);
  hipLaunchKernelGGL(nms_select_kernel, dim3(B), dim3(kSelThreads), 0, s, w.keys, N, M, count, inds);
  return dh3d_launch_status();
}

DH3D_API int dh3d_gather_rows(const float *src, int B, int N, int C, const int32_t *inds, const int32_t *count, int M,
                              float *dst, void *stream) {
  DH3D_REQUIRE(src && inds && count && dst);
  DH3D_REQUIRE(B > 0 && N > 0 && C > 0 && M > 0);
  const long long rows = (long long)B * M;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(dh3d_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, src, N, C, inds,
                     count, M, rows, dst);
  return dh3d_launch_status();
}
