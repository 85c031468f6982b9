// QueryBallPoint / QueryBallPoint2 (tf_ops/grouping: tf_grouping_g.cu:3-92, CPU twin test/query_ball_point.cpp:19-47) for
// gfx950.  Per query j the reference walks the dataset points k = 0 .. n-1 in index order,
//   d = max(sqrtf((x2-x1)^2 + (y2-y1)^2 + (z2-z1)^2), 1e-20f),   hit: d < radius (strict),
// and stops at nsample hits: a row is the min(hits, nsample) SMALLEST indices inside the ball in ascending order, then the
// first of them repeated; pts_cnt = min(hits, nsample).  An empty ball's row is nsample copies of the index of the point
// nearest to the query (same d, strict <, lowest index on ties), pts_cnt = 0.
// Rounding: the twin's -- ((dx*dx + dy*dy) + dz*dz) in f32 without contraction (this file is built with
// -ffp-contract=off), IEEE sqrtf.  A squared-distance screen only ever lets extra candidates through; the decision is
// taken on the sqrtf value.
// Two kernels, one result:
//   ball_scan_kernel  the reference formulation made parallel -- lane = query, one wave per tile of 64 consecutive
//                     queries, the cloud staged through LDS in index order and broadcast; a wave leaves when all its
//                     lanes are full.  Any shape.
//   ball_grid_kernel  one wave per query on the cell table of dh3d_spatial_sort_cells (n <= 16384): the cells the ball's
//                     box meets, hits marked in a bit set over ORIGINAL indices in LDS, the nsample lowest bits read out.
#include <float.h>
#include <math.h>

#include "cell_walk.h"
#include "common.h"
#include "wave_ops.h"

namespace {

constexpr int kChunk = 1024;     // candidates staged per step of the scan (12 KiB of LDS)

// Everything at or below this squared distance goes to the exact test: d < r needs s < r^2 (1 + 2^-22) at most, and s = 0
// (d = 1e-20) must pass for every r > 1e-20 even where r * r underflows.
__device__ __forceinline__ float ball_screen(float r) { return fmaxf(r * r * 1.000001f, FLT_MIN); }

__device__ __forceinline__ float ball_sq(float qx, float qy, float qz, float x, float y, float z) {
  const float dx = qx - x, dy = qy - y, dz = qz - z;
  return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ float ball_dist(float s) { return fmaxf(sqrtf(s), 1e-20f); }

// ------------------------------------------------------------------------------------------------ scan
// One wave per workgroup: the early exit is then the workgroup's, and a barrier costs nothing.  Blocks are numbered
// (cloud, tile) and dealt to the XCDs in contiguous ranges, so a cloud's 12 n bytes are fetched into one L2 (or two).
template <bool PER_QUERY>
__global__ __launch_bounds__(64) void ball_scan_kernel(const float *__restrict__ xyz1, const float *__restrict__ xyz2,
                                                       const float *__restrict__ radii, float radius, int n, int m,
                                                       int nsample, int tiles, int32_t *__restrict__ idx,
                                                       int32_t *__restrict__ pts_cnt) {
  __shared__ __attribute__((aligned(16))) float s_c[3 * kChunk];  // x[kChunk] | y[kChunk] | z[kChunk]
  const int bid = dh3d_xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int b = bid / tiles, lane = threadIdx.x;
  const int j = (bid - b * tiles) * 64 + lane;
  const bool valid = j < m;
  const float *pc = xyz1 + (size_t)b * n * 3;
  const size_t qrow = (size_t)b * m + (valid ? j : m - 1);
  const float qx = xyz2[qrow * 3], qy = xyz2[qrow * 3 + 1], qz = xyz2[qrow * 3 + 2];
  const float r = PER_QUERY ? radii[qrow] : radius;
  const float r2hi = ball_screen(r);
  int32_t *row = idx + qrow * nsample;

  int cnt = 0, first = 0, best_k = 0;
  float best_s = INFINITY, best_d = INFINITY;  // the nearest point so far: tracked only while the lane has no hit
  bool active = valid;                         // still walking: fewer than nsample hits
  bool done = false;
  for (int base = 0; base < n && !done; base += kChunk) {
    const int len = min(kChunk, n - base);
    const int len4 = (len + 3) & ~3;
    __syncthreads();
    for (int e = lane; e < len4 * 3; e += 64) {
      const int c = e / 3, comp = e - c * 3;
      s_c[comp * kChunk + c] = c < len ? pc[(size_t)base * 3 + e] : INFINITY;
    }
    __syncthreads();
    for (int jj = 0; jj < len4; jj += 4) {
      const float4 X = *reinterpret_cast<const float4 *>(s_c + jj);
      const float4 Y = *reinterpret_cast<const float4 *>(s_c + kChunk + jj);
      const float4 Z = *reinterpret_cast<const float4 *>(s_c + 2 * kChunk + jj);
      const float s[4] = {ball_sq(qx, qy, qz, X.x, Y.x, Z.x), ball_sq(qx, qy, qz, X.y, Y.y, Z.y),
                          ball_sq(qx, qy, qz, X.z, Y.z, Z.z), ball_sq(qx, qy, qz, X.w, Y.w, Z.w)};
      // nothing above `lim` is a hit, and nothing above best_s is nearer than the nearest so far
      const float lim = cnt == 0 ? fmaxf(r2hi, best_s) : r2hi;
      const float mn = fminf(fminf(s[0], s[1]), fminf(s[2], s[3]));
      const bool need = active && mn <= lim;
      if (__any(need)) {  // wave-uniform: the exact test, in index order
        if (need) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int k = base + jj + u;
            if (active && s[u] <= lim && k < n) {
              const float d = ball_dist(s[u]);
              if (d < r) {
                if (cnt == 0) first = k;
                row[cnt] = k;
                ++cnt;
                active = cnt < nsample;
              } else if (cnt == 0 && d < best_d) {
                best_d = d; best_s = s[u]; best_k = k;
              }
            }
          }
        }
        if (!__any(active)) { done = true; break; }  // every ball of the wave is full
      }
    }
  }
  if (valid) {
    const int fill = cnt > 0 ? first : best_k;
    for (int l = cnt; l < nsample; ++l) row[l] = fill;
    pts_cnt[qrow] = cnt;
  }
}

// ------------------------------------------------------------------------------------------------ cell lists
constexpr int kGridWaves = 4;  // queries per workgroup; a ball whose box meets more than kWalkMaxCells cells (cell_walk.h)
                               // goes over the 64-point group boxes

__global__ __launch_bounds__(64 * kGridWaves) void ball_grid_kernel(
    const float4 *__restrict__ sorted, const float *__restrict__ gbox, const int *__restrict__ cells,
    const float *__restrict__ xyz2, const float *__restrict__ radii, int per_query, int n, int m, int nsample, int wpl,
    int32_t *__restrict__ idx, int32_t *__restrict__ pts_cnt) {
  extern __shared__ unsigned s_dyn[];  // per wave: bits[64 * wpl] | pre[64] | beg[64]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int b = blockIdx.y, j = (int)blockIdx.x * kGridWaves + wave;
  if (j >= m) return;  // (wave-uniform; the waves of a workgroup never meet at a barrier)
  unsigned *bits = s_dyn + wave * (64 * wpl + 128);
  int *s_pre = reinterpret_cast<int *>(bits + 64 * wpl), *s_beg = s_pre + 64;
  for (int i = 0; i < wpl; ++i) bits[i * 64 + lane] = 0u;
  wave_lds_sync();  // the zeroes are in place before any lane's atomicOr

  const float4 *sc = sorted + (size_t)b * n;
  const size_t qrow = (size_t)b * m + j;
  const float q[3] = {xyz2[qrow * 3], xyz2[qrow * 3 + 1], xyz2[qrow * 3 + 2]};
  const float r = radii[per_query ? qrow : 0];
  const float r2hi = ball_screen(r);
  auto test = [&](int i) {
    const float4 p = sc[i];
    const float s = ball_sq(q[0], q[1], q[2], p.x, p.y, p.z);
    if (s <= r2hi && ball_dist(s) < r) {
      const unsigned k = __float_as_uint(p.w);  // (the plain original index, < 16384: spatial.hip)
      if (k < (unsigned)n) atomicOr(&bits[k >> 5], 1u << (k & 31u));
    }
  };

  if (r > 0.f) {  // (a radius <= 0 or NaN has no hits)
    // This kernel counts the schedule's bits again itself, cell_grid.h's sched_bits restated as a loop: with the shared
    // population counts the compiler builds another cell loop below, and a ball whose box meets ~500 cells took 39.4 us
    // against 35.6 (profiles/cell_grid_header.txt).
    CellGrid g = cell_grid(cells, b);
    const int *ct = g.ct;
    g.nb[0] = g.nb[1] = g.nb[2] = 0;
#pragma unroll
    for (int s = 0; s < kGridSteps; ++s) {
      const int a = sched_axis(g.sched, s);
      g.nb[0] += (int)(a == 0); g.nb[1] += (int)(a == 1); g.nb[2] += (int)(a == 2);
    }
    // The cells the ball's axis-aligned box meets: cell_walk.h's ball_cells, to the letter (its comment has the argument
    // for the margin).  Written out here because with the shared function the kernel's preamble came out 3 instructions
    // longer (1490 against 1487; the loops are the same) and cube_m1024_r0.1_k32 of tools/ball_query_bench.py measured 12.60
    // us against 12.48 with a spread of 0.08: over the bar by one tick of the timer (profiles/cell_walk.txt section 4).
    int c0[3], cn[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float marg = r * 1e-5f + fabsf(q[a]) * 1e-6f;
      c0[a] = grid_cell(g, a, (q[a] - r) - marg);
      cn[a] = grid_cell(g, a, (q[a] + r) + marg) - c0[a] + 1;
    }
    const int total = cn[0] * cn[1] * cn[2];
    if (!ct[kCellFlag] && total <= kWalkMaxCells) {
      for (int t0 = 0; t0 < total; t0 += 64) {
        // a lane per cell: its range of the order; then the ranges of the 64 cells flattened, a lane per record
        const int t = t0 + lane;
        int beg = 0, len = 0;
        if (t < total) {
          const int ix = c0[0] + t % cn[0], iy = c0[1] + (t / cn[0]) % cn[1], iz = c0[2] + t / (cn[0] * cn[1]);
          const unsigned code = cell_code(g.sched, g.nb, ix, iy, iz);
          beg = max(ct[code], 0);
          len = max(min(ct[code + 1], n) - beg, 0);
        }
        const int inc = wave_incl_scan(len);
        s_pre[lane] = inc;
        s_beg[lane] = beg - (inc - len);
        wave_lds_sync();
        const int recs = __builtin_amdgcn_readlane(inc, 63);
        for (int rr = lane; rr < recs; rr += 64) {
          int o = 0;  // the first cell whose inclusive prefix exceeds rr
#pragma unroll
          for (int step = 32; step > 0; step >>= 1)
            if (s_pre[o + step - 1] <= rr) o += step;
          test(s_beg[o] + rr);
        }
        wave_lds_sync();
      }
    } else {
      // crowded cloud or wide ball: every 64-point group of the order whose box the ball meets (1e-5 relative margin on
      // the box distance, as the pruned kNN scan's; it dwarfs the roundings of both chains)
      const int NG = (n + 63) / 64;
      const float *gb = gbox + (size_t)b * NG * 8;
      for (int g0 = 0; g0 < NG; g0 += 64) {
        const int g = g0 + lane;
        bool meet = false;
        if (g < NG) {
          const float4 lo = *reinterpret_cast<const float4 *>(gb + (size_t)g * 8);
          const float4 hi = *reinterpret_cast<const float4 *>(gb + (size_t)g * 8 + 4);
          const float dx = fmaxf(fmaxf(lo.x - q[0], q[0] - hi.x), 0.f), dy = fmaxf(fmaxf(lo.y - q[1], q[1] - hi.y), 0.f),
                      dz = fmaxf(fmaxf(lo.z - q[2], q[2] - hi.z), 0.f);
          meet = ((dx * dx + dy * dy) + dz * dz) * 0.99999f <= r2hi;
        }
        unsigned long long mask = __ballot(meet);
        while (mask) {
          const int i = (g0 + __builtin_ctzll(mask)) * 64 + lane;
          mask &= mask - 1ull;
          if (i < n) test(i);
        }
      }
    }
  }
  wave_lds_sync();

  // ---- read out: lane l owns the words [l * wpl, (l + 1) * wpl) -- ascending indices across the wave
  int c = 0;
  unsigned lowest = ~0u;
  for (int i = wpl - 1; i >= 0; --i) {
    const unsigned w = bits[lane * wpl + i];
    c += __popc(w);
    if (w) lowest = (unsigned)((lane * wpl + i) * 32 + __builtin_ctz(w));
  }
  const int inc = wave_incl_scan(c);
  const int hits = __builtin_amdgcn_readlane(inc, 63);
  const int cnt = min(hits, nsample);
  int32_t *row = idx + qrow * nsample;
  unsigned first;
  if (hits > 0) {
    first = wave_min_u32(lowest);
    int pos = inc - c;
    for (int i = 0; i < wpl && pos < nsample; ++i) {
      unsigned w = bits[lane * wpl + i];
      while (w && pos < nsample) {
        row[pos++] = (lane * wpl + i) * 32 + __builtin_ctz(w);
        w &= w - 1u;
      }
    }
  } else {
    // empty ball: the nearest point of the whole cloud, ties to the lowest index -- the minimum of (bits(d), index)
    unsigned long long best = ~0ull;
    for (int i = lane; i < n; i += 64) {
      const float4 p = sc[i];
      const float d = ball_dist(ball_sq(q[0], q[1], q[2], p.x, p.y, p.z));
      const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | __float_as_uint(p.w);
      best = key < best ? key : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off, 64);
      best = o < best ? o : best;
    }
    first = (unsigned)best;
    if (first >= (unsigned)n) first = 0u;
  }
  for (int l = cnt + lane; l < nsample; l += 64) row[l] = (int)first;
  if (lane == 0) pts_cnt[qrow] = cnt;
}

// The one rule of the dispatcher (shapes only): cell lists from this many dataset points on.  The cell lists enter the
// rule for the shapes where sort + cell lists is MEASURED below the scan by more than their spread
// (tools/ball_query_bench.py); no such measurement exists yet, so no shape qualifies and the operator runs the scan.
constexpr int kGridMinN = 1 << 30;

int scan_launch(int b, int n, int m, float radius, const float *radii, int nsample, const float *xyz1, const float *xyz2,
                int32_t *idx, int32_t *pts_cnt, void *stream) {
  const int tiles = dh3d_cdiv(m, 64);
  DH3D_SUPPORTED((long long)b * tiles <= 0x7FFFFFFFll);
  hipStream_t s = (hipStream_t)stream;
  if (radii)
    hipLaunchKernelGGL(ball_scan_kernel<true>, dim3(b * tiles), dim3(64), 0, s, xyz1, xyz2, radii, 0.f, n, m, nsample, tiles,
                       idx, pts_cnt);
  else
    hipLaunchKernelGGL(ball_scan_kernel<false>, dim3(b * tiles), dim3(64), 0, s, xyz1, xyz2, nullptr, radius, n, m, nsample,
                       tiles, idx, pts_cnt);
  return dh3d_launch_status();
}

}  // namespace

DH3D_API int dh3d_query_ball_point(int b, int n, int m, float radius, int nsample, const float *xyz1, const float *xyz2,
                                   int32_t *idx, int32_t *pts_cnt, void *stream) {
  DH3D_REQUIRE(xyz1 && xyz2 && idx && pts_cnt && b > 0 && n > 0 && m > 0 && nsample > 0 && radius > 0.f);
  return scan_launch(b, n, m, radius, nullptr, nsample, xyz1, xyz2, idx, pts_cnt, stream);
}

DH3D_API int dh3d_query_ball_point2(int b, int n, int m, int nsample, const float *xyz1, const float *xyz2,
                                    const float *radii, int32_t *idx, int32_t *pts_cnt, void *stream) {
  DH3D_REQUIRE(xyz1 && xyz2 && radii && idx && pts_cnt && b > 0 && n > 0 && m > 0 && nsample > 0);
  return scan_launch(b, n, m, 0.f, radii, nsample, xyz1, xyz2, idx, pts_cnt, stream);
}

DH3D_API int dh3d_query_ball_point_grid(int b, int n, int m, const float *radius_or_radii, int per_query, int nsample,
                                        const float *sorted1, const float *gbox1, const int32_t *cells1, const float *xyz2,
                                        int32_t *idx, int32_t *pts_cnt, void *stream) {
  DH3D_REQUIRE(radius_or_radii && sorted1 && gbox1 && cells1 && xyz2 && idx && pts_cnt && b > 0 && n > 0 && m > 0 &&
               nsample > 0);
  DH3D_SUPPORTED(n <= 16384 && b <= 65535);
  const int wpl = dh3d_cdiv(dh3d_cdiv(n, 32), 64);  // <= 8 words of the bit set per lane
  const size_t lds = sizeof(unsigned) * kGridWaves * (64 * (size_t)wpl + 128);
  hipLaunchKernelGGL(ball_grid_kernel, dim3(dh3d_cdiv(m, kGridWaves), b), dim3(64 * kGridWaves), lds, (hipStream_t)stream,
                     reinterpret_cast<const float4 *>(sorted1), gbox1, cells1, xyz2, radius_or_radii, per_query != 0, n, m,
                     nsample, wpl, idx, pts_cnt);
  return dh3d_launch_status();
}

DH3D_API int dh3d_query_ball_point_plan(int n, int m, int nsample) {
  if (n <= 0 || m <= 0 || nsample <= 0) return -1;
  return n >= kGridMinN && n <= 16384 ? 1 : 0;
}
