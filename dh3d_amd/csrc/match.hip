// Two-nearest, reverse-nearest, ratio-test and mutual descriptor matching of cloud pairs for gfx950
// (include/dh3d_hip.h dh3d_match_descriptors2).  The ids and distances come from registration.hip's rule alone -- the f32
// sum over d ascending of (x_d - y_d)^2, every operation rounded on its own -- but only a few pairs per row ever reach
// it: the f32 MFMA screens the rest.
//
//   match2_kernel    grid (ceil(max(Ma, Mb) / 64), P, directions), 256 lanes.  Direction 0 searches the positives for
//                    every anchor (nn1, nn2, the ratio test), direction 1 the anchors for every positive (rev): the same
//                    code with the operands swapped, S being symmetric in f32.  A block keeps 64 rows x in LDS and sweeps
//                    the other cloud's rows y 64 at a time; the next 64 travel from memory in registers while this step
//                    computes.  Per step, wave w owns the 32 x 32 tile (w >> 1, w & 1):
//                      (1) s(i, j) = (nx_i + ny_j) - 2 dot(i, j): dot on v_mfma_f32_32x32x2_f32, the norms once per staged row;
//                      (2) (i, j) survives while s - E(i, j) <= T_i, the row's current second-best rule value (the rows'
//                          keys only fall, so a running T is safe); on the first step, where no key exists yet, T_i is the
//                          second smallest s + E of the wave's own 32 columns, which bounds two rule values from above;
//                      (3) the survivors are compacted into an LDS list (it holds a whole step: every pair may survive)
//                          and evaluated by the rule, one lane per pair, the operations and their order as match_kernel;
//                      (4) a rule value enters the row's two keys (S bits << 32 | j; S >= +0, so the unsigned order is the
//                          order of (S, j)) by two integer LDS minima: k1 <- min(k1, key), and whichever of the two lost
//                          goes to k2 <- min(k2, loser).  Every key but the smallest loses exactly once, so k2 ends as
//                          the second smallest whatever the order of arrival.
//                    S = +inf or NaN is never a neighbour (match_kernel's strict `<` against +inf).
//   match2_finalize_kernel  one block per pair: the mutual check rev[match[i]] == i on the ratio-filtered ids, num_kept.
//
// THE BOUND.  u = 2^-24, gamma_n = n u / (1 - n u), x and y two rows of D <= 256 floats, X = |x|^2, Y = |y|^2 and
// S* = |x - y|^2 in real arithmetic, T = X + Y; S* <= 2 T and sum_d |x_d y_d| <= T / 2.  Without underflow:
//   rule     every term (x_d - y_d)^2 carries two roundings, the sum D - 1 more, all terms >= 0:
//            |S - S*| <= gamma_(D+1) S* <= 2 gamma_(D+1) T;
//   norms    nx = X (1 + t), |t| <= gamma_D (a product and at most D - 1 additions per term, any order, terms >= 0);
//   fma chain  the MFMA result is a k-ordered fmaf chain from 0, one rounding per step (zero padding adds exact zeros), so in
//            any order of k: |dot - x.y| <= gamma_D sum |x_d y_d| <= gamma_D T / 2;
//   combining  t = fl(nx + ny): |t - T| <= gamma_(D+1) T;  s = fl(t - 2 dot) (2 dot is exact): its rounding is at most
//            u (|t| + 2 |dot|) <= 2 u (1 + gamma_(D+1)) T.
//   Together |s - S| <= (gamma_(D+1) + gamma_D + 2 u (1 + gamma_(D+1)) + 2 gamma_(D+1)) T <= (4 D + 6.1) u T  (n u <= 1.6e-5).
//   The test itself rounds: E^ = fl(fl(c t) + tiny) >= c T (1 - gamma_(D+3)), and fl(s -+ E^) moves by at most
//   u |s -+ E^| <= 2.1 u T.  So s - E^ <= S <= s + E^ holds after rounding when c (1 - 1.7e-5) >= (4 D + 8.2) u:
//   c = 4 (D + 4) u = (4 D + 16) u, exact in f32.  Underflow adds at most 2^-150 per product or fma, fewer than 2^-138 in
//   all: tiny = 2^-100 covers it.  Overflow gives s or E^ = inf / NaN: the tests are written so that NaN survives (2) and
//   never lowers a threshold.
// Compiled without contraction (csrc/Makefile EXACT): the ids depend on every rounding of the rule.
#include "common.h"
#include "keys.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;          // rows of x per block, rows of y per step
constexpr int kMaxDim = 256;       // descriptor length limit, as dh3d_match_descriptors
constexpr int kMaxKp = 4096;       // keypoints per cloud
constexpr unsigned long long kNoKey = ~0ull;

struct Match2Args {
  const float *a, *b;              // anchor / positive descriptors
  long long a_stride, b_stride;
  const int32_t *a_count, *b_count;
  int Ma, Mb, D;
  float c_bound, ratio2;           // 4 (D + 4) 2^-24; <= 0: no ratio test
  int32_t *nn1, *nn2, *match, *rev;
  float *dist1, *dist2, *rev_dist;
};

__host__ __device__ inline int padded_dim(int D) { return (D + 7) & ~7; }   // whole k-groups of 8
__host__ __device__ inline int row_ld(int D) { return padded_dim(D) + 4; }  // 16-byte rows, 4 banks of skew per row
size_t match2_lds_bytes(int D) {
  return (size_t)2 * kTile * row_ld(D) * sizeof(float) + 2 * kTile * sizeof(float) + 2 * kTile * sizeof(unsigned long long) +
         kTile * kTile * sizeof(unsigned short) + 16;
}

// Rows [r0, r0 + 64) of a cloud on their way into a tile: thread t holds columns (t & 31) + 32 m of the rows (t >> 5) + 8 k,
// rows >= n and columns >= D as zeros.  All 64 loads are in flight at once, and those of the next step are issued ahead of
// this step's MFMAs and stored after its rule pass.  C = ceil(D / 32) column chunks: the kernel is compiled for 2, 4 and 8.
template <int C>
struct RowRegs { float v[C][kTile / 8]; };
template <int C>
__device__ __forceinline__ void load_rows(const float *__restrict__ src, long long stride, int r0, int n, int D, RowRegs<C> &q) {
  const int c0 = threadIdx.x & 31, rr = threadIdx.x >> 5;
#pragma unroll
  for (int k = 0; k < kTile / 8; ++k) {
    const bool live = r0 + rr + 8 * k < n;
    const float *row = src + (long long)(r0 + rr + 8 * k) * stride;  // (rows may not be 16-byte aligned: column 3 of 132)
#pragma unroll
    for (int m = 0; m < C; ++m) q.v[m][k] = (live && c0 + 32 * m < D) ? row[c0 + 32 * m] : 0.f;
  }
}
template <int C>
__device__ __forceinline__ void store_rows(const RowRegs<C> &q, int Dp, int ld, float *__restrict__ tile) {
  const int c0 = threadIdx.x & 31, rr = threadIdx.x >> 5;
#pragma unroll
  for (int m = 0; m < C; ++m) {
    if (c0 + 32 * m < Dp) {
#pragma unroll
      for (int k = 0; k < kTile / 8; ++k) tile[(rr + 8 * k) * ld + c0 + 32 * m] = q.v[m][k];
    }
  }
}
// the squared norms of a staged tile's rows: four lanes per row, each over every fourth float4, combined by a butterfly
// (any order satisfies the bound)
__device__ __forceinline__ void row_norms(const float *__restrict__ tile, int Dp, int ld, float *__restrict__ norm) {
  const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
  float acc = 0.f;
  for (int c = 4 * q; c < Dp; c += 16) {
    const float4 v = *reinterpret_cast<const float4 *>(&tile[r * ld + c]);
    acc = acc + v.x * v.x;
    acc = acc + v.y * v.y;
    acc = acc + v.z * v.z;
    acc = acc + v.w * v.w;
  }
  acc = acc + __shfl_xor(acc, 1, 64);
  acc = acc + __shfl_xor(acc, 2, 64);
  if (q == 0) norm[r] = acc;
}

// (m1, m2) <- the two smallest of the multiset {m1, m2, p1, p2}, m1 <= m2 and p1 <= p2 (no NaN)
__device__ __forceinline__ void merge_two_smallest(float &m1, float &m2, float p1, float p2) {
  const float lo = fminf(m1, p1), hi = fmaxf(m1, p1);
  m2 = fminf(hi, fminf(m2, p2));
  m1 = lo;
}

template <int C>
__global__ __launch_bounds__(kThreads) void match2_kernel(Match2Args g) {
  extern __shared__ __align__(16) unsigned char s_raw[];
  const int dir = blockIdx.z, p = blockIdx.y, i0 = blockIdx.x * kTile;
  // x: the cloud whose rows search, y: the cloud searched
  const int Mx = dir ? g.Mb : g.Ma, My = dir ? g.Ma : g.Mb;
  if (i0 >= Mx) return;
  const float *x = (dir ? g.b : g.a) + (long long)p * Mx * (dir ? g.b_stride : g.a_stride);
  const float *y = (dir ? g.a : g.b) + (long long)p * My * (dir ? g.a_stride : g.b_stride);
  const long long x_stride = dir ? g.b_stride : g.a_stride, y_stride = dir ? g.a_stride : g.b_stride;
  const int na = clamp_count(g.a_count[p], g.Ma), nb = clamp_count(g.b_count[p], g.Mb);
  const int nx = dir ? nb : na, ny = dir ? na : nb;
  const int D = g.D, Dp = padded_dim(D), ld = row_ld(D);

  unsigned long long *s_k1 = reinterpret_cast<unsigned long long *>(s_raw);
  unsigned long long *s_k2 = s_k1 + kTile;
  float *s_x = reinterpret_cast<float *>(s_k2 + kTile);
  float *s_y = s_x + kTile * ld;
  float *s_nx = s_y + kTile * ld;
  float *s_ny = s_nx + kTile;
  unsigned short *s_list = reinterpret_cast<unsigned short *>(s_ny + kTile);
  int *s_cnt = reinterpret_cast<int *>(s_list + kTile * kTile);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rg = wave >> 1, cg = wave & 1, r = lane & 31, h = lane >> 5;

  if (threadIdx.x < kTile) s_k1[threadIdx.x] = s_k2[threadIdx.x] = kNoKey;
  if (i0 < nx && ny > 0) {  // (block-uniform) else no row of this block has a neighbour
    RowRegs<C> regs;
    load_rows(x, x_stride, i0, nx, D, regs);
    store_rows(regs, Dp, ld, s_x);
    load_rows(y, y_stride, 0, ny, D, regs);
    __syncthreads();
    row_norms(s_x, Dp, ld, s_nx);
    for (int j0 = 0; j0 < ny; j0 += kTile) {
      __syncthreads();  // the previous step's rows have been read, its keys are in
      store_rows(regs, Dp, ld, s_y);
      if (threadIdx.x == 0) *s_cnt = 0;
      __syncthreads();
      row_norms(s_y, Dp, ld, s_ny);
      if (j0 + kTile < ny) load_rows(y, y_stride, j0 + kTile, ny, D, regs);  // lands under the MFMAs
      __syncthreads();
      if (i0 + rg * 32 < nx && j0 + cg * 32 < ny) {  // (wave-uniform)
        // (1) lane (r, h) feeds row r of both operands; k-group g is d = 8 g .. 8 g + 7, MFMA t of it takes d = 8 g + t
        // from the lanes h = 0 and d = 8 g + 4 + t from h = 1: one 16-byte LDS read per operand and four MFMAs
        const float *xp = s_x + (rg * 32 + r) * ld + 4 * h, *yp = s_y + (cg * 32 + r) * ld + 4 * h;
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
        float4 vx = *reinterpret_cast<const float4 *>(xp), vy = *reinterpret_cast<const float4 *>(yp);
        for (int c = 0; c < Dp; c += 8) {
          const int cn = c + 8 < Dp ? c + 8 : c;  // the next group's operands arrive under this group's MFMAs
          const float4 wx = *reinterpret_cast<const float4 *>(xp + cn), wy = *reinterpret_cast<const float4 *>(yp + cn);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(vx.x, vy.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(vx.y, vy.y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(vx.z, vy.z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(vx.w, vy.w, acc, 0, 0, 0);
          vx = wx;
          vy = wy;
        }
        // (2) the lane holds column jl = cg * 32 + r of the rows il(q) = rg * 32 + (q & 3) + 8 (q >> 2) + 4 h
        const int jl = cg * 32 + r;
        const bool col_live = j0 + jl < ny;
        const float nyj = s_ny[jl];
        float low[16], thr[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int il = rg * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
          const float t = s_nx[il] + nyj;
          const float s = t - 2.f * acc[q];
          const float e = g.c_bound * t + 0x1p-100f;
          low[q] = s - e;
          const unsigned long long k2 = s_k2[il];
          thr[q] = k2 == kNoKey ? INFINITY : __uint_as_float((unsigned)(k2 >> 32));
          if (j0 == 0) {  // (block-uniform) no key yet: the second smallest upper bound of the wave's 32 columns
            float m1 = s + e, m2 = INFINITY;
            if (!col_live || !(m1 < INFINITY)) m1 = INFINITY;  // (a NaN bound says nothing)
#pragma unroll
            for (int off = 1; off < 32; off <<= 1) {
              const float p1 = __shfl_xor(m1, off, 64), p2 = __shfl_xor(m2, off, 64);
              merge_two_smallest(m1, m2, p1, p2);
            }
            thr[q] = m2;
          }
        }
        // (3) compaction: one list slot per survivor
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int il = rg * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
          if (col_live && i0 + il < nx && !(low[q] > thr[q])) s_list[atomicAdd(s_cnt, 1)] = (unsigned short)(il << 6 | jl);
        }
      }
      __syncthreads();
      // (3, 4) the rule, one lane per surviving pair, into the row's keys
      const int n = *s_cnt;
      for (int e = threadIdx.x; e < n; e += kThreads) {
        const int il = s_list[e] >> 6, jl = s_list[e] & 63;
        const float *xr = s_x + il * ld, *yr = s_y + jl * ld;
        float s = 0.f;
        for (int c = 0; c < D; c += 4) {
          const float4 u = *reinterpret_cast<const float4 *>(xr + c), v = *reinterpret_cast<const float4 *>(yr + c);
          const float d0 = u.x - v.x, d1 = u.y - v.y, d2 = u.z - v.z, d3 = u.w - v.w;
          s = s + d0 * d0;
          s = s + d1 * d1;
          s = s + d2 * d2;
          s = s + d3 * d3;
        }
        if (s < INFINITY) {
          const unsigned long long key = (unsigned long long)__float_as_uint(s) << 32 | (unsigned)(j0 + jl);
          const unsigned long long old = atomicMin(&s_k1[il], key);
          const unsigned long long loser = old > key ? old : key;
          if (loser != kNoKey) atomicMin(&s_k2[il], loser);
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < kTile && i0 + threadIdx.x < Mx) {
    const unsigned long long k1 = s_k1[threadIdx.x], k2 = s_k2[threadIdx.x];
    const float s1 = k1 == kNoKey ? INFINITY : __uint_as_float((unsigned)(k1 >> 32));
    const float s2 = k2 == kNoKey ? INFINITY : __uint_as_float((unsigned)(k2 >> 32));
    const int j1 = k1 == kNoKey ? -1 : (int)(unsigned)k1, j2 = k2 == kNoKey ? -1 : (int)(unsigned)k2;
    const long long o = (long long)p * Mx + i0 + threadIdx.x;
    if (dir) {
      g.rev[o] = j1;
      g.rev_dist[o] = j1 >= 0 ? sqrtf(s1) : INFINITY;
    } else {
      g.nn1[o] = j1;
      g.dist1[o] = j1 >= 0 ? sqrtf(s1) : INFINITY;
      g.nn2[o] = j2;
      g.dist2[o] = j2 >= 0 ? sqrtf(s2) : INFINITY;
      bool keep = j1 >= 0;
      if (g.ratio2 > 0.f) {
        const float bound = g.ratio2 * s2;  // one rounded product; +inf without a second neighbour
        keep = keep && s1 < bound;
      }
      g.match[o] = keep ? j1 : -1;
    }
  }
}

// match [P, Ma] holds the ratio-filtered ids: drop those whose positive does not choose the anchor back, count the rest
__global__ __launch_bounds__(kThreads) void match2_finalize_kernel(int32_t *__restrict__ match, const int32_t *__restrict__ rev,
                                                                   int Ma, int Mb, int mutual,
                                                                   int32_t *__restrict__ num_kept) {
  __shared__ int s_red[4];
  const int p = blockIdx.x;
  int kept = 0;
  for (int i = threadIdx.x; i < Ma; i += kThreads) {
    const long long o = (long long)p * Ma + i;
    int m = match[o];
    if (mutual && m >= 0 && rev[(long long)p * Mb + m] != i) match[o] = m = -1;
    kept += m >= 0;
  }
  kept = block_sum_256(kept, s_red);
  if (threadIdx.x == 0) num_kept[p] = kept;
}

}  // namespace

DH3D_API int dh3d_match_descriptors2(const float *anchor_desc, long long anchor_stride, const int32_t *anchor_count,
                                     const float *positive_desc, long long positive_stride, const int32_t *positive_count,
                                     int P, int Ma, int Mb, int D, float ratio2, int mutual, int32_t *nn1, float *dist1,
                                     int32_t *nn2, float *dist2, int32_t *rev, float *rev_dist, int32_t *match,
                                     int32_t *num_kept, void *stream) {
  DH3D_REQUIRE(anchor_desc && anchor_count && positive_desc && positive_count && nn1 && dist1 && nn2 && dist2 && match &&
               num_kept);
  DH3D_REQUIRE((rev != nullptr) == (rev_dist != nullptr) && (rev || !mutual));
  DH3D_REQUIRE(P > 0 && Ma > 0 && Mb > 0 && D > 0 && anchor_stride >= D && positive_stride >= D);
  DH3D_REQUIRE(ratio2 == ratio2 && ratio2 <= 1.f);
  DH3D_SUPPORTED(D <= kMaxDim && D % 4 == 0 && Ma <= kMaxKp && Mb <= kMaxKp && P <= 65535);
  DH3D_ALLOW_BIG_LDS(match2_kernel<4>);  // (77 KB at D = 128, 143 KB at D = 256; D <= 64 stays below the default cap)
  DH3D_ALLOW_BIG_LDS(match2_kernel<8>);
  Match2Args g{anchor_desc, positive_desc, anchor_stride, positive_stride, anchor_count, positive_count, Ma, Mb, D,
               ldexpf(4.f * (float)(D + 4), -24), ratio2, nn1, nn2, match, rev, dist1, dist2, rev_dist};
  const int rows = rev && Mb > Ma ? Mb : Ma;
  const dim3 grid(dh3d_cdiv(rows, kTile), P, rev ? 2 : 1);
  const size_t lds = match2_lds_bytes(D);
  if (D <= 64) hipLaunchKernelGGL(match2_kernel<2>, grid, dim3(kThreads), lds, (hipStream_t)stream, g);
  else if (D <= 128) hipLaunchKernelGGL(match2_kernel<4>, grid, dim3(kThreads), lds, (hipStream_t)stream, g);
  else hipLaunchKernelGGL(match2_kernel<8>, grid, dim3(kThreads), lds, (hipStream_t)stream, g);
  if (hipGetLastError() != hipSuccess) return DH3D_ERR_LAUNCH;
  hipLaunchKernelGGL(match2_finalize_kernel, dim3(P), dim3(kThreads), 0, (hipStream_t)stream, match, rev, Ma, Mb, mutual,
                     num_kept);
  return dh3d_launch_status();
}
