// Training batches on the device for gfx950: the host loaders of core/datasets.py (Local_train_dataset_selfpair.loadPair,
// Global_train_dataset_triplet.loadPC) between prepare_clouds and the trainers.  include/dh3d_hip.h "Training batches"
// states the contract; every random draw is a pure function of (seed, stream, cloud, element) through splitmix64, so no
// key array, no sort and no generator state exist anywhere.  The seed is read from device memory: a captured graph draws a
// fresh batch on every replay once the caller bumps that scalar.
//   resample_select_kernel  grid B, 1024 threads.  n >= targetnum: the targetnum-th smallest key of the cloud by a radix
//                           select, 8 bits a pass, the keys recomputed on every pass (two 64-bit multiplies each); then the
//                           number of chosen rows in every chunk of 1024 source rows, as an exclusive prefix -> workspace.
//   resample_write_kernel   grid (chunks, B), 1024 threads.  n >= targetnum: a stable compaction of one source chunk behind
//                           its prefix (ballot + wave totals).  n < targetnum: one chunk of output rows -- the cloud, then the
//                           pad draws, or 100000.0 for an empty cloud.
//   augment_kernel          grid (ceil(N / 1024), B), 256 threads x 4 points.  Thread 0 derives the cloud's parameters (they
//                           are outputs too), every thread runs the float64 chain on its points and rounds once.
//   pair_rotate_kernel      loadPair's z-rotation of pc2: float64 row times matrix, rounded once; R as float32.
//   pair_fps_kernel         grid B, 1024 threads: radix select of the N / 2 subset keys, stable compaction of the subset's
//                           coordinates into LDS (96 KB at N = 16384), FarthestSampler.sample with the running minima in
//                           registers (8 positions a thread) and one barrier a pick (the wave maxima are double-buffered).
//   pair_nn_kernel          grid (ceil(M / 16), B), 256 threads: the float64 1-NN of 16 anchors in pc2, each pc2 row loaded
//                           once for the 16; kept out of the FPS workgroup so that B pairs fill more than B compute units.
// Compiled without contraction (csrc/Makefile EXACT): the picks and the neighbours depend on every rounding of d2.
#include "common.h"
#include "keys.h"
#include "workspace.h"

namespace {

typedef unsigned long long u64;

constexpr int kBig = 1024;          // threads of the select / compaction / FPS workgroups; also rows per compaction chunk
constexpr int kMaxSrc = 131072;
constexpr int kMaxTarget = 1 << 20;
constexpr int kMaxBatch = 65535;    // grid.y
constexpr int kMaxPairN = 16384;
constexpr int kFpsPer = kMaxPairN / 2 / kBig;  // subset positions per thread
constexpr int kAugThreads = 256, kAugPer = 4;
constexpr int kNnThreads = 256, kNnAnchors = 16;
constexpr double kTwoPi = 6.283185307179586;
constexpr double kPi = 3.141592653589793;

enum Stream : unsigned {  // include/dh3d_hip.h lists these
  kResample = 1, kPad = 2, kRotate1D = 3, kJitter = 4, kScale = 5, kRotateSmall = 6, kShift = 7, kPairRot = 8, kSubset = 9,
  kFirst = 10
};

// (stream_h, unit_co, unit_oc: keys.h)
__device__ __forceinline__ double normal(u64 h, u64 e) {  // Box-Muller, cosine branch
  const double u1 = unit_oc(splitmix64(h + 2 * e)), u2 = unit_co(splitmix64(h + 2 * e + 1));
  return sqrt(-2.0 * log(u1)) * cos(kTwoPi * u2);
}
__device__ __forceinline__ double clipd(double v, double c) { return fmin(fmax(v, -c), c); }

// The m-th smallest (1 <= m <= n) of the keys splitmix64(h + i), i < n, returned to every thread of a 1024-thread
// workgroup.  splitmix64 is a bijection, so the keys are distinct: exactly m of them are <= the result, and the order by
// (key, i) is the order by key.  s_hist: 256 counters, s_sel: 2.
__device__ u64 block_select(u64 h, int n, int m, unsigned *s_hist, unsigned *s_sel) {
  const int tid = threadIdx.x, lane = tid & 63;
  u64 prefix = 0;
  unsigned k = (unsigned)m;
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (tid < 256) s_hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kBig) {
      const u64 key = splitmix64(h + (u64)i);
      const bool cand = shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8));
      if (cand) atomicAdd(&s_hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid < 64) {  // lane l owns bins 4l .. 4l+3
      const unsigned c0 = s_hist[4 * lane], c1 = s_hist[4 * lane + 1], c2 = s_hist[4 * lane + 2], c3 = s_hist[4 * lane + 3];
      const unsigned sum = c0 + c1 + c2 + c3;
      unsigned incl = sum;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
      }
      unsigned before = incl - sum;
      if (before < k && k <= incl) {  // one lane
        unsigned bin = 4 * lane;
        if (k > before + c0) { before += c0, ++bin;
          if (k > before + c1) { before += c1, ++bin;
            if (k > before + c2) before += c2, ++bin; } }
        s_sel[0] = bin;
        s_sel[1] = k - before;
      }
    }
    __syncthreads();
    prefix |= (u64)s_sel[0] << shift;
    k = s_sel[1];
  }
  return prefix;
}

struct ResampleWs {  // per cloud: the threshold key; per source chunk of 1024 rows: the chosen rows before it
  u64 *thr;
  int32_t *base;
  ResampleWs(Carve &c, int B, int Nsrc) : thr(c.take<u64>((size_t)B, 16)), base(c.take<int32_t>((size_t)B * dh3d_cdiv(Nsrc, kBig), 16)) {}
};

__global__ __launch_bounds__(kBig) void resample_select_kernel(const int32_t *__restrict__ num_valid, int Nsrc, int targetnum,
                                                               const u64 *__restrict__ seed, u64 *__restrict__ thr,
                                                               int32_t *__restrict__ base) {
  __shared__ unsigned s_hist[256], s_sel[2], s_cnt[kMaxSrc / kBig];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int n = clamp_count(num_valid[b], Nsrc), nch = (Nsrc + kBig - 1) / kBig;
  if (n < targetnum) {  // (workgroup-uniform) the write kernel reads neither; written so that the workspace is defined
    if (tid == 0) thr[b] = ~0ull;
    for (int c = tid; c < nch; c += kBig) base[(size_t)b * nch + c] = 0;
    return;
  }
  const u64 h = stream_h(*seed, kResample, (unsigned)b);
  const u64 t = block_select(h, n, targetnum, s_hist, s_sel);
  if (tid < kMaxSrc / kBig) s_cnt[tid] = 0;
  __syncthreads();
  for (int c = 0; c * kBig < n; ++c) {
    const int i = c * kBig + tid;
    const u64 mask = __ballot(i < n && splitmix64(h + (u64)i) <= t);
    if (lane == 0 && mask) atomicAdd(&s_cnt[c], (unsigned)__popcll(mask));
  }
  __syncthreads();
  if (tid == 0) {
    thr[b] = t;
    int run = 0;
    for (int c = 0; c < nch; ++c) {
      base[(size_t)b * nch + c] = run;
      run += (int)s_cnt[c];
    }
  }
}

__global__ __launch_bounds__(kBig) void resample_write_kernel(const float *__restrict__ src, const int32_t *__restrict__ num_valid,
                                                              int Nsrc, int targetnum, const u64 *__restrict__ seed,
                                                              const u64 *__restrict__ thr, const int32_t *__restrict__ base,
                                                              float *__restrict__ out, int32_t *__restrict__ num_orig) {
  __shared__ unsigned s_w[kBig / 64];
  const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = clamp_count(num_valid[b], Nsrc);
  const float *in = src + (size_t)b * Nsrc * 3;
  float *o = out + (size_t)b * targetnum * 3;
  if (c == 0 && tid == 0) num_orig[b] = n < targetnum ? n : targetnum;
  if (n >= targetnum) {
    if (c * kBig >= n) return;  // (workgroup-uniform)
    const u64 h = stream_h(*seed, kResample, (unsigned)b);
    const int i = c * kBig + tid;
    const bool sel = i < n && splitmix64(h + (u64)i) <= thr[b];
    const u64 mask = __ballot(sel);
    if (lane == 0) s_w[wave] = (unsigned)__popcll(mask);
    __syncthreads();
    int pos = base[(size_t)b * ((Nsrc + kBig - 1) / kBig) + c] + __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += (int)s_w[w];
    if (sel && pos < targetnum) {
      o[3 * (size_t)pos] = in[3 * (size_t)i];
      o[3 * (size_t)pos + 1] = in[3 * (size_t)i + 1];
      o[3 * (size_t)pos + 2] = in[3 * (size_t)i + 2];
    }
    return;
  }
  const int j = c * kBig + tid;
  if (j >= targetnum) return;
  float x = 100000.0f, y = 100000.0f, z = 100000.0f;
  if (n > 0) {
    int r = j;
    if (j >= n) r = (int)(splitmix64(stream_h(*seed, kPad, (unsigned)b) + (u64)(j - n)) % (u64)n);
    x = in[3 * (size_t)r], y = in[3 * (size_t)r + 1], z = in[3 * (size_t)r + 2];
  }
  o[3 * (size_t)j] = x, o[3 * (size_t)j + 1] = y, o[3 * (size_t)j + 2] = z;
}

struct AugArgs {
  unsigned mask;
  double sigma, clip, scale_low, scale_high, angle_sigma, angle_clip, shift_range;
};

// C = A * B, 3 x 3 row-major, every element (a0 b0 + a1 b1) + a2 b2
__device__ __forceinline__ void mat3_mul(const double *A, const double *B, double *C) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
// row * R
__device__ __forceinline__ void row_mat3(double &x, double &y, double &z, const double *R) {
  const double a = (x * R[0] + y * R[3]) + z * R[6], b = (x * R[1] + y * R[4]) + z * R[7], c = (x * R[2] + y * R[5]) + z * R[8];
  x = a, y = b, z = c;
}
__device__ __forceinline__ void rot_z(double angle, double *R) {  // augment.py RotateZ, datasets.py loadPair
  const double c = cos(angle), s = sin(angle);
  R[0] = c, R[1] = s, R[2] = 0.0, R[3] = -s, R[4] = c, R[5] = 0.0, R[6] = 0.0, R[7] = 0.0, R[8] = 1.0;
}

__global__ __launch_bounds__(kAugThreads) void augment_kernel(const float *__restrict__ in, int N, AugArgs a,
                                                              const u64 *__restrict__ seed, float *__restrict__ out,
                                                              double *__restrict__ rot1d, double *__restrict__ scale,
                                                              double *__restrict__ rot_small, double *__restrict__ shift) {
  __shared__ double s_p[22];  // rot1d 9, rot_small 9, shift 3, scale 1
  const int b = blockIdx.y, tid = threadIdx.x;
  const u64 sd = *seed;
  if (tid == 0) {
    double R1[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Rs[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, sh[3] = {0, 0, 0}, sc = 1.0;
    if (a.mask & DH3D_AUG_ROTATE1D) rot_z(unit_co(splitmix64(stream_h(sd, kRotate1D, b))) * 2.0 * kPi, R1);
    if (a.mask & DH3D_AUG_SCALE) sc = a.scale_low + (a.scale_high - a.scale_low) * unit_co(splitmix64(stream_h(sd, kScale, b)));
    if (a.mask & DH3D_AUG_ROTATESMALL) {
      const u64 h = stream_h(sd, kRotateSmall, b);
      double c[3], s[3];
      for (int e = 0; e < 3; ++e) {
        const double ang = clipd(a.angle_sigma * normal(h, (u64)e), a.angle_clip);
        c[e] = cos(ang), s[e] = sin(ang);
      }
      const double Rx[9] = {1, 0, 0, 0, c[0], -s[0], 0, s[0], c[0]}, Ry[9] = {c[1], 0, s[1], 0, 1, 0, -s[1], 0, c[1]},
                   Rz[9] = {c[2], -s[2], 0, s[2], c[2], 0, 0, 0, 1};
      double T[9];
      mat3_mul(Ry, Rx, T);
      mat3_mul(Rz, T, Rs);
    }
    if (a.mask & DH3D_AUG_SHIFT) {
      const u64 h = stream_h(sd, kShift, b);
      for (int c = 0; c < 3; ++c) sh[c] = -a.shift_range + (a.shift_range - -a.shift_range) * unit_co(splitmix64(h + (u64)c));
    }
    for (int e = 0; e < 9; ++e) s_p[e] = R1[e], s_p[9 + e] = Rs[e];
    for (int e = 0; e < 3; ++e) s_p[18 + e] = sh[e];
    s_p[21] = sc;
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    if (tid < 9) rot1d[(size_t)b * 9 + tid] = s_p[tid], rot_small[(size_t)b * 9 + tid] = s_p[9 + tid];
    if (tid < 3) shift[(size_t)b * 3 + tid] = s_p[18 + tid];
    if (tid == 0) scale[b] = s_p[21];
  }
  const u64 hj = stream_h(sd, kJitter, b);
  for (int k = 0; k < kAugPer; ++k) {
    const int i = (blockIdx.x * kAugPer + k) * kAugThreads + tid;
    if (i >= N) break;
    const size_t at = ((size_t)b * N + i) * 3;
    double x = (double)in[at], y = (double)in[at + 1], z = (double)in[at + 2];
    if (a.mask & DH3D_AUG_ROTATE1D) row_mat3(x, y, z, s_p);
    if (a.mask & DH3D_AUG_JITTER) {
      const u64 e = 3ull * (u64)i;
      x = clipd(a.sigma * normal(hj, e), a.clip) + x;
      y = clipd(a.sigma * normal(hj, e + 1), a.clip) + y;
      z = clipd(a.sigma * normal(hj, e + 2), a.clip) + z;
    }
    if (a.mask & DH3D_AUG_SCALE) x *= s_p[21], y *= s_p[21], z *= s_p[21];
    if (a.mask & DH3D_AUG_ROTATESMALL) row_mat3(x, y, z, s_p + 9);
    if (a.mask & DH3D_AUG_SHIFT) x += s_p[18], y += s_p[19], z += s_p[20];
    out[at] = (float)x, out[at + 1] = (float)y, out[at + 2] = (float)z;
  }
}

__global__ __launch_bounds__(256) void pair_rotate_kernel(const float *__restrict__ pc2, int N, double rot_maxv,
                                                          const u64 *__restrict__ seed, float *__restrict__ pc2_trans,
                                                          float *__restrict__ R) {
  __shared__ double s_r[9];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (tid == 0) {
    double M[9];
    rot_z((2.0 * unit_co(splitmix64(stream_h(*seed, kPairRot, b))) - 1.0) * rot_maxv, M);
    for (int e = 0; e < 9; ++e) s_r[e] = M[e];
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid < 9) R[(size_t)b * 9 + tid] = (float)s_r[tid];
  const int i = blockIdx.x * 256 + tid;
  if (i >= N) return;
  const size_t at = ((size_t)b * N + i) * 3;
  double x = (double)pc2[at], y = (double)pc2[at + 1], z = (double)pc2[at + 2];
  row_mat3(x, y, z, s_r);
  pc2_trans[at] = (float)x, pc2_trans[at + 1] = (float)y, pc2_trans[at + 2] = (float)z;
}

__device__ __forceinline__ double dist2(double ax, double ay, double az, float bx, float by, float bz) {
  const double dx = ax - (double)bx, dy = ay - (double)by, dz = az - (double)bz;
  return (dx * dx + dy * dy) + dz * dz;
}

struct FpsHead {  // the small arrays of pair_fps_kernel, in front of the subset
  double rv[2][kBig / 64];   // the waves' maxima, double-buffered
  int rp[2][kBig / 64];      // and their positions
  unsigned hist[256], sel[2], w[kBig / 64];
  unsigned pad[2];           // (a multiple of 16 bytes)
};
static_assert(sizeof(FpsHead) % 16 == 0, "the subset's floats start aligned");

size_t fps_lds_bytes(int N) { return sizeof(FpsHead) + (size_t)(N / 2) * (3 * sizeof(float) + sizeof(unsigned short)); }
static_assert(sizeof(FpsHead) + (size_t)(kMaxPairN / 2) * 14 <= 159 * 1024, "the largest cloud fits the raised LDS cap");

__global__ __launch_bounds__(kBig) void pair_fps_kernel(const float *__restrict__ pc1, int N, int M,
                                                        const u64 *__restrict__ seed, int32_t *__restrict__ anc) {
  // all of the LDS is dynamic: DH3D_ALLOW_BIG_LDS raises the dynamic cap to 159 KiB, which leaves no room for static arrays
  extern __shared__ __align__(16) unsigned char s_raw[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = N / 2;
  FpsHead *hd = reinterpret_cast<FpsHead *>(s_raw);
  unsigned *s_hist = hd->hist, *s_sel = hd->sel, *s_w = hd->w;
  double(*s_rv)[kBig / 64] = hd->rv;
  int(*s_rp)[kBig / 64] = hd->rp;
  float *s_xyz = reinterpret_cast<float *>(s_raw + sizeof(FpsHead));                 // [half][3] the subset, in index order
  unsigned short *s_idx = reinterpret_cast<unsigned short *>(s_xyz + 3 * (size_t)half);  // [half] its rows in the cloud
  const float *p1 = pc1 + (size_t)b * N * 3;
  const u64 sd = *seed;

  const u64 h = stream_h(sd, kSubset, (unsigned)b);
  const u64 t = block_select(h, N, half, s_hist, s_sel);
  int run = 0;
  for (int c = 0; c * kBig < N; ++c) {
    const int i = c * kBig + tid;
    const bool sel = i < N && splitmix64(h + (u64)i) <= t;
    const u64 mask = __ballot(sel);
    if (lane == 0) s_w[wave] = (unsigned)__popcll(mask);
    __syncthreads();
    int pos = run + __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < kBig / 64; ++w) {
      const int v = (int)s_w[w];
      if (w < wave) pos += v;
      total += v;
    }
    if (sel && pos < half) {
      s_xyz[3 * pos] = p1[3 * (size_t)i], s_xyz[3 * pos + 1] = p1[3 * (size_t)i + 1], s_xyz[3 * pos + 2] = p1[3 * (size_t)i + 2];
      s_idx[pos] = (unsigned short)i;
    }
    run += total;
    __syncthreads();
  }

  float px[kFpsPer], py[kFpsPer], pz[kFpsPer];
  double md[kFpsPer];
#pragma unroll
  for (int k = 0; k < kFpsPer; ++k) {
    const int p = k * kBig + tid;
    const bool in = p < half;
    px[k] = in ? s_xyz[3 * p] : 0.f, py[k] = in ? s_xyz[3 * p + 1] : 0.f, pz[k] = in ? s_xyz[3 * p + 2] : 0.f;
    md[k] = in ? __longlong_as_double(0x7FF0000000000000ll) : -1.0;  // (-1: below every distance, never the maximum)
  }
  int cur = (int)(splitmix64(stream_h(sd, kFirst, (unsigned)b)) % (u64)half);
  for (int it = 0; it < M; ++it) {
    if (tid == 0) anc[(size_t)b * M + it] = (int32_t)s_idx[cur];
    if (it == M - 1) break;
    const double cx = (double)s_xyz[3 * cur], cy = (double)s_xyz[3 * cur + 1], cz = (double)s_xyz[3 * cur + 2];
    double bv = -1.0;
    int bp = 0x7FFFFFFF;
#pragma unroll
    for (int k = 0; k < kFpsPer; ++k) {
      if (k * kBig < half) {  // (workgroup-uniform)
        const double d = dist2(cx, cy, cz, px[k], py[k], pz[k]);
        if (md[k] >= 0.0) md[k] = fmin(md[k], d);
        if (md[k] > bv) bv = md[k], bp = k * kBig + tid;  // ascending positions: the first maximum stays
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(bv, off, 64);
      const int op = __shfl_xor(bp, off, 64);
      if (ov > bv || (ov == bv && op < bp)) bv = ov, bp = op;
    }
    const int par = it & 1;  // two buffers: a wave may write the next pick's maximum while another still reads this one's
    if (lane == 0) s_rv[par][wave] = bv, s_rp[par][wave] = bp;
    __syncthreads();
    bv = s_rv[par][lane & 15], bp = s_rp[par][lane & 15];
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
      const double ov = __shfl_xor(bv, off, 64);
      const int op = __shfl_xor(bp, off, 64);
      if (ov > bv || (ov == bv && op < bp)) bv = ov, bp = op;
    }
    cur = bp;
  }
}

__global__ __launch_bounds__(kNnThreads) void pair_nn_kernel(const float *__restrict__ pc1, const float *__restrict__ pc2, int N,
                                                            int M, const int32_t *__restrict__ anc, int32_t *__restrict__ pos) {
  __shared__ double s_a[kNnAnchors][3];
  __shared__ double s_bd[kNnThreads / 64][kNnAnchors];
  __shared__ int s_bj[kNnThreads / 64][kNnAnchors];
  const int b = blockIdx.y, m0 = blockIdx.x * kNnAnchors, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float *p2 = pc2 + (size_t)b * N * 3;
  if (tid < kNnAnchors * 3) {  // (a padding anchor repeats the last one; it writes nothing)
    const int a = tid / 3, c = tid - 3 * a, m = m0 + a < M ? m0 + a : M - 1;
    int row = anc[(size_t)b * M + m];
    row = row < 0 ? 0 : (row >= N ? N - 1 : row);
    s_a[a][c] = (double)pc1[((size_t)b * N + row) * 3 + c];
  }
  __syncthreads();
  double bd[kNnAnchors];
  int bj[kNnAnchors];
#pragma unroll
  for (int a = 0; a < kNnAnchors; ++a) bd[a] = __longlong_as_double(0x7FF0000000000000ll), bj[a] = 0x7FFFFFFF;
  for (int j = tid; j < N; j += kNnThreads) {
    const float x = p2[3 * (size_t)j], y = p2[3 * (size_t)j + 1], z = p2[3 * (size_t)j + 2];
#pragma unroll
    for (int a = 0; a < kNnAnchors; ++a) {
      const double d = dist2(s_a[a][0], s_a[a][1], s_a[a][2], x, y, z);
      if (d < bd[a]) bd[a] = d, bj[a] = j;  // ascending j: the lowest stays on ties
    }
  }
#pragma unroll
  for (int a = 0; a < kNnAnchors; ++a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_xor(bd[a], off, 64);
      const int oj = __shfl_xor(bj[a], off, 64);
      if (od < bd[a] || (od == bd[a] && oj < bj[a])) bd[a] = od, bj[a] = oj;
    }
    if (lane == 0) s_bd[wave][a] = bd[a], s_bj[wave][a] = bj[a];
  }
  __syncthreads();
  if (tid < kNnAnchors && m0 + tid < M) {
    double d = s_bd[0][tid];
    int j = s_bj[0][tid];
    for (int w = 1; w < kNnThreads / 64; ++w)
      if (s_bd[w][tid] < d || (s_bd[w][tid] == d && s_bj[w][tid] < j)) d = s_bd[w][tid], j = s_bj[w][tid];
    pos[(size_t)b * M + m0 + tid] = j;
  }
}

bool finite_nonneg(double v) { return v >= 0.0 && v < __builtin_inf(); }

}  // namespace

DH3D_API size_t dh3d_resample_clouds_ws_bytes(int B, int Nsrc, int targetnum) {
  if (B <= 0 || Nsrc <= 0 || targetnum <= 0 || B > kMaxBatch || Nsrc > kMaxSrc || targetnum > kMaxTarget) return 0;
  return carve_bytes<ResampleWs>(B, Nsrc);
}

DH3D_API int dh3d_resample_clouds(int B, int Nsrc, int targetnum, const float *points, const int32_t *num_valid,
                                  const unsigned long long *seed, float *out, int32_t *num_orig, void *workspace,
                                  size_t workspace_bytes, void *stream) {
  DH3D_REQUIRE(B > 0 && Nsrc > 0 && targetnum > 0);
  DH3D_REQUIRE(points && num_valid && seed && out && num_orig);
  DH3D_SUPPORTED(B <= kMaxBatch && Nsrc <= kMaxSrc && targetnum <= kMaxTarget);
  DH3D_REQUIRE(workspace && workspace_bytes >= carve_bytes<ResampleWs>(B, Nsrc) && ((uintptr_t)workspace & 15) == 0);
  Carve carve(workspace);
  const ResampleWs w(carve, B, Nsrc);
  hipLaunchKernelGGL(resample_select_kernel, dim3(B), dim3(kBig), 0, (hipStream_t)stream, num_valid, Nsrc, targetnum, seed, w.thr,
                     w.base);
  if (dh3d_launch_status() != DH3D_OK) return DH3D_ERR_LAUNCH;
  const int chunks = dh3d_cdiv(Nsrc > targetnum ? Nsrc : targetnum, kBig);
  hipLaunchKernelGGL(resample_write_kernel, dim3(chunks, B), dim3(kBig), 0, (hipStream_t)stream, points, num_valid, Nsrc,
                     targetnum, seed, w.thr, w.base, out, num_orig);
  return dh3d_launch_status();
}

DH3D_API int dh3d_augment_clouds(int B, int N, const float *points, unsigned aug_mask, double sigma, double clip,
                                 double scale_low, double scale_high, double angle_sigma, double angle_clip, double shift_range,
                                 const unsigned long long *seed, float *out, double *rot1d, double *scale, double *rot_small,
                                 double *shift, void *stream) {
  DH3D_REQUIRE(B > 0 && N > 0);
  DH3D_REQUIRE(points && seed && out && rot1d && scale && rot_small && shift);
  DH3D_REQUIRE((aug_mask & ~(unsigned)DH3D_AUG_ALL) == 0);
  DH3D_REQUIRE(finite_nonneg(sigma) && clip > 0.0 && finite_nonneg(clip) && scale_low > 0.0 && finite_nonneg(scale_high) &&
               scale_low <= scale_high && finite_nonneg(angle_sigma) && finite_nonneg(angle_clip) && finite_nonneg(shift_range));
  DH3D_SUPPORTED(B <= kMaxBatch);
  const AugArgs a{aug_mask, sigma, clip, scale_low, scale_high, angle_sigma, angle_clip, shift_range};
  hipLaunchKernelGGL(augment_kernel, dim3(dh3d_cdiv(N, kAugThreads * kAugPer), B), dim3(kAugThreads), 0, (hipStream_t)stream,
                     points, N, a, seed, out, rot1d, scale, rot_small, shift);
  return dh3d_launch_status();
}

DH3D_API int dh3d_pair_rotate(int B, int N, const float *pc2, double rot_maxv, const unsigned long long *seed, float *pc2_trans,
                              float *R, void *stream) {
  DH3D_REQUIRE(B > 0 && N > 0);
  DH3D_REQUIRE(pc2 && seed && pc2_trans && R);
  DH3D_REQUIRE(finite_nonneg(rot_maxv));
  DH3D_SUPPORTED(B <= kMaxBatch);
  hipLaunchKernelGGL(pair_rotate_kernel, dim3(dh3d_cdiv(N, 256), B), dim3(256), 0, (hipStream_t)stream, pc2, N, rot_maxv, seed,
                     pc2_trans, R);
  return dh3d_launch_status();
}

DH3D_API int dh3d_sample_pair_nodes(int B, int N, int sample_nodes, const float *pc1, const float *pc2,
                                    const unsigned long long *seed, int32_t *anc, int32_t *pos, void *stream) {
  DH3D_REQUIRE(B > 0 && N > 0);
  DH3D_REQUIRE(pc1 && pc2 && seed && anc && pos);
  DH3D_SUPPORTED(B <= kMaxBatch && N <= kMaxPairN && sample_nodes >= 1 && sample_nodes <= N / 2);
  DH3D_ALLOW_BIG_LDS(pair_fps_kernel);
  hipLaunchKernelGGL(pair_fps_kernel, dim3(B), dim3(kBig), fps_lds_bytes(N), (hipStream_t)stream, pc1, N, sample_nodes, seed, anc);
  if (dh3d_launch_status() != DH3D_OK) return DH3D_ERR_LAUNCH;
  hipLaunchKernelGGL(pair_nn_kernel, dim3(dh3d_cdiv(sample_nodes, kNnAnchors), B), dim3(kNnThreads), 0, (hipStream_t)stream, pc1,
                     pc2, N, sample_nodes, anc, pos);
  return dh3d_launch_status();
}
