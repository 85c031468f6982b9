// Place retrieval for gfx950: the exact float64 top-k search of Q query descriptors in a map of R reference descriptors
// (evaluate/global_eval/evaluation_retrieval.py:37-40, cKDTree(database).query(queries, k), run there on the host).
// include/dh3d_hip.h dh3d_retrieve states the contract; no [Q, R] matrix is formed, no atomics on global memory, no host
// sync, one or two launches on the caller's stream (graph-capturable, no parallel branches):
//   retrieve_scan_kernel   grid (ceil(Q / 16), S), 256 threads.  A workgroup takes 16 queries against one contiguous slice of
//                          the map.  The queries sit in LDS as float64 for the whole slice; the slice streams through LDS in
//                          tiles of 256 rows x 32 columns (stored column-major, so a lane reads its four rows with one
//                          ds_read_b128), the next chunk's global loads in flight under the current chunk's arithmetic.
//                          Wave w owns queries 4w .. 4w+3, lane l rows 4l .. 4l+3 of the tile: 16 float64 accumulators per
//                          lane, a converted value used four times.  The column chunks are walked in ascending order, so every
//                          accumulator is the sum over c ascending.  After a tile's last chunk each distance is compared with
//                          its query's threshold (the current k-th key); survivors are appended to the wave's 64-entry LDS
//                          buffer of that query by ballot + prefix count, and a full buffer is folded into the sorted k-list
//                          (one entry per lane) by a wave-wide bitonic sort + merge -- wave_fold (wave_ops.h), which
//                          knn3_fused_kernel (knn_point.hip) runs on 64-bit keys, here on 96-bit ones.  Keys (d2 bits, id) are
//                          all distinct and a non-negative double orders as its bit pattern, so a list is a function of the
//                          SET of rows scanned: it depends neither on the order in which survivors arrive nor on S.
//   retrieve_merge_kernel  S > 1 only: one wave per query merges the S partial lists [S, Q, k] of the workspace by the same key.
// Bound: 3 float64 VALU operations (subtract, multiply, add -- no contraction) per (query, row, column) plus one conversion
// per 4 of them; the map is read once per 16 queries.  Compiled without contraction (csrc/Makefile EXACT).
#include "common.h"
#include "keys.h"
#include "wave_ops.h"
#include "workspace.h"

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kQw = 4;                       // queries per wave
constexpr int kQb = kWaves * kQw;            // queries per workgroup
constexpr int kTile = 256;                   // map rows per tile (4 per lane)
constexpr int kChunk = 32;                   // columns per LDS chunk
constexpr int kTileStride = kTile + 4;       // floats between two columns of the tile: 16-byte aligned, spreads the banks
constexpr int kLoads = kTile * kChunk / kThreads;  // 32 elements per thread per chunk
constexpr int kMaxDim = 256;
constexpr int kMaxK = 64;                    // the k-list is one entry per lane
constexpr int kTargetBlocks = 512;           // two workgroups (78 KB of LDS each) per CU on 256 CUs

typedef Key96 Key;  // (wave_ops.h) ascending by (d, id); d = the bits of a non-negative double
constexpr u64 kNoDist = kNoKey96;
__device__ __forceinline__ Key no_key() { return key96_none(); }

__device__ __forceinline__ void write_entry(const Key &e, long long o, int32_t *idx, double *dist2) {
  const bool some = e.d != kNoDist;
  idx[o] = some ? (int32_t)e.id : -1;
  dist2[o] = some ? __longlong_as_double((long long)e.d) : __longlong_as_double(0x7FF0000000000000ll);
}

size_t scan_lds_bytes(int D) {
  return (size_t)D * kQb * sizeof(double) + (size_t)kChunk * kTileStride * sizeof(float) +
         (size_t)kQb * 64 * (sizeof(u64) + sizeof(unsigned));
}

__global__ __launch_bounds__(kThreads) void retrieve_scan_kernel(const float *__restrict__ ref, long long ref_stride,
                                                                 const int32_t *__restrict__ ref_count,
                                                                 const float *__restrict__ qry, long long qry_stride, int Q,
                                                                 int R, int D, int k, int slice_rows, int32_t *__restrict__ idx,
                                                                 double *__restrict__ dist2, u64 *__restrict__ part_d,
                                                                 unsigned *__restrict__ part_id) {
  extern __shared__ __align__(16) unsigned char s_raw[];
  double *s_q = reinterpret_cast<double *>(s_raw);                      // [D][16] queries, float64
  float *s_t = reinterpret_cast<float *>(s_q + (size_t)D * kQb);        // [32][260] one chunk of the tile, column-major
  u64 *s_bd = reinterpret_cast<u64 *>(s_t + kChunk * kTileStride);      // [16][64] survivors: distance bits
  unsigned *s_bi = reinterpret_cast<unsigned *>(s_bd + kQb * 64);       // [16][64] survivors: ids
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = blockIdx.x * kQb;
  const int r = ref_count ? clamp_count(*ref_count, R) : R;
  const long long begin = (long long)blockIdx.y * slice_rows;
  const long long end = begin + slice_rows < r ? begin + slice_rows : r;   // (begin >= end: an empty slice, nothing is read)
  const int ntiles = end > begin ? (int)((end - begin + kTile - 1) / kTile) : 0;
  const int nchunks = (D + kChunk - 1) / kChunk, total = ntiles * nchunks;

  for (int e = tid; e < D * kQb; e += kThreads) {   // (a padding query repeats the last one; it writes nothing)
    const int qi = e / D, c = e - qi * D;
    const int q = q0 + qi < Q ? q0 + qi : Q - 1;
    s_q[c * kQb + qi] = (double)qry[(long long)q * qry_stride + c];
  }

  Key list[kQw], tau[kQw];
  int cnt[kQw];
#pragma unroll
  for (int qi = 0; qi < kQw; ++qi) list[qi] = no_key(), tau[qi] = no_key(), cnt[qi] = 0;
  auto flush = [&](int qi) {
    const int slot = (wave * kQw + qi) * 64 + lane;
    wave_lds_sync();
    Key bv = no_key();
    if (lane < cnt[qi]) bv = Key{s_bd[slot], s_bi[slot]};
    wave_lds_sync();
    list[qi] = wave_fold(list[qi], bv, lane);
    tau[qi] = key_shfl(list[qi], k - 1);
    cnt[qi] = 0;
  };

  // the chunk's elements of this thread: element i is row i * 8 + tid / 32 of the tile, column tid % 32 of the chunk
  const int lc = tid & 31, lr = tid >> 5;
  float pf[kLoads];
  auto load = [&](int it) {
    const int tile = it / nchunks, c = (it - tile * nchunks) * kChunk + lc;
    const long long row0 = begin + (long long)tile * kTile + lr;
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const long long row = row0 + i * 8;
      pf[i] = row < end && c < D ? ref[row * ref_stride + c] : 0.f;
    }
  };

  double acc[kQw][4];
  if (total > 0) load(0);
  for (int it = 0; it < total; ++it) {
    const int tile = it / nchunks, chunk = it - tile * nchunks;
    __syncthreads();  // the previous chunk has been read (first pass: nothing)
#pragma unroll
    for (int i = 0; i < kLoads; ++i) s_t[lc * kTileStride + lr + i * 8] = pf[i];
    __syncthreads();  // (also orders the queries' staging before the first read)
    if (it + 1 < total) load(it + 1);
    if (chunk == 0) {
#pragma unroll
      for (int qi = 0; qi < kQw; ++qi)
#pragma unroll
        for (int ri = 0; ri < 4; ++ri) acc[qi][ri] = 0.0;
    }
    const int c0 = chunk * kChunk, cols = D - c0 < kChunk ? D - c0 : kChunk;
    const double *sq = s_q + (size_t)c0 * kQb + wave * kQw;
    const float *st = s_t + 4 * lane;
    for (int c = 0; c < cols; ++c) {
      const double2 qa = *reinterpret_cast<const double2 *>(sq + c * kQb);
      const double2 qb = *reinterpret_cast<const double2 *>(sq + c * kQb + 2);
      const float4 v = *reinterpret_cast<const float4 *>(st + c * kTileStride);
      const double qv[kQw] = {qa.x, qa.y, qb.x, qb.y};
      const double rv[4] = {(double)v.x, (double)v.y, (double)v.z, (double)v.w};
#pragma unroll
      for (int qi = 0; qi < kQw; ++qi) {
#pragma unroll
        for (int ri = 0; ri < 4; ++ri) {
          const double d = qv[qi] - rv[ri];
          acc[qi][ri] = acc[qi][ri] + d * d;
        }
      }
    }
    if (chunk != nchunks - 1) continue;
    const long long row0 = begin + (long long)tile * kTile + 4 * lane;
#pragma unroll
    for (int qi = 0; qi < kQw; ++qi) {
#pragma unroll
      for (int ri = 0; ri < 4; ++ri) {
        const Key key{(u64)__double_as_longlong(acc[qi][ri]), (unsigned)(row0 + ri)};
        const bool take = row0 + ri < end && key_lt(key, tau[qi]);
        const u64 mask = __ballot(take);
        if (mask) {  // wave-uniform
          const int pcnt = __popcll(mask);
          if (cnt[qi] + pcnt > 64) flush(qi);  // (what the new threshold would now refuse is still correct to keep)
          if (take) {
            const int slot = (wave * kQw + qi) * 64 + cnt[qi] + __popcll(mask & ((1ull << lane) - 1ull));
            s_bd[slot] = key.d;
            s_bi[slot] = key.id;
          }
          cnt[qi] += pcnt;
        }
      }
    }
  }

#pragma unroll
  for (int qi = 0; qi < kQw; ++qi) {
    flush(qi);
    const int q = q0 + wave * kQw + qi;
    if (q < Q && lane < k) {
      if (gridDim.y == 1) {
        write_entry(list[qi], (long long)q * k + lane, idx, dist2);
      } else {
        const long long o = ((long long)blockIdx.y * Q + q) * k + lane;
        part_d[o] = list[qi].d;
        part_id[o] = list[qi].id;
      }
    }
  }
}

// one wave per query: the S * k keys of its partial lists, 64 at a time, folded into one list
__global__ __launch_bounds__(kThreads) void retrieve_merge_kernel(const u64 *__restrict__ part_d,
                                                                  const unsigned *__restrict__ part_id, int S, int Q, int k,
                                                                  int32_t *__restrict__ idx, double *__restrict__ dist2) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int q = blockIdx.x * kWaves + wave;
  if (q >= Q) return;  // (wave-uniform; no workgroup barrier below)
  Key list = no_key(), tau = no_key();
  const int n = S * k;
  for (int base = 0; base < n; base += 64) {
    const int t = base + lane;
    Key bv = no_key();
    if (t < n) {
      const int s = t / k, e = t - s * k;
      const long long o = ((long long)s * Q + q) * k + e;
      bv = Key{part_d[o], part_id[o]};
    }
    if (!__ballot(key_lt(bv, tau))) continue;  // nothing here can enter the list
    list = wave_fold(list, bv, lane);
    tau = key_shfl(list, k - 1);
  }
  if (lane < k) write_entry(list, (long long)q * k + lane, idx, dist2);
}

struct RetrieveWs {  // the partial lists [S, Q, k]
  u64 *part_d;
  unsigned *part_id;
  RetrieveWs(Carve &c, int S, int Q, int k)
      : part_d(c.take<u64>((size_t)S * Q * k, 16)), part_id(c.take<unsigned>((size_t)S * Q * k, 16)) {}
};

// rows per slice for S slices: whole tiles
int slice_rows_for(int R, int S) {
  const long long tiles = ((long long)R + kTile - 1) / kTile;
  return (int)((tiles + S - 1) / S) * kTile;
}

}  // namespace

DH3D_API int dh3d_retrieve_plan(int Q, int R, int D, int k) {
  if (Q <= 0 || R <= 0 || D <= 0 || k <= 0 || D % 4 != 0 || D > kMaxDim || k > kMaxK) return -1;
  const long long qblocks = ((long long)Q + kQb - 1) / kQb, tiles = ((long long)R + kTile - 1) / kTile;
  long long S = kTargetBlocks / qblocks;  // enough workgroups for two per CU, never less than a tile each
  if (S < 1) S = 1;
  if (S > tiles) S = tiles;
  const long long per = (tiles + S - 1) / S;
  return (int)((tiles + per - 1) / per);  // no empty slice: slice s is rows [s * 256 * per, (s + 1) * 256 * per)
}

DH3D_API size_t dh3d_retrieve_ws_bytes(int Q, int R, int D, int k) {
  const int S = dh3d_retrieve_plan(Q, R, D, k);
  return S < 0 ? 0 : carve_bytes<RetrieveWs>(S, Q, k);
}

DH3D_API int dh3d_retrieve(const float *ref, long long ref_stride, const int32_t *ref_count, const float *qry,
                           long long qry_stride, int Q, int R, int D, int k, int32_t *idx, double *dist2, void *ws,
                           size_t ws_bytes, void *stream) {
  DH3D_REQUIRE(ref && qry && idx && dist2);
  DH3D_REQUIRE(Q > 0 && R > 0 && D > 0 && k > 0);
  const int S = dh3d_retrieve_plan(Q, R, D, k);
  DH3D_SUPPORTED(S > 0);
  DH3D_REQUIRE(ref_stride >= D && qry_stride >= D);
  DH3D_REQUIRE(ws && ws_bytes >= carve_bytes<RetrieveWs>(S, Q, k) && ((uintptr_t)ws & 15) == 0);
  Carve carve(ws);
  const RetrieveWs w(carve, S, Q, k);
  DH3D_ALLOW_BIG_LDS(retrieve_scan_kernel);
  hipLaunchKernelGGL(retrieve_scan_kernel, dim3(dh3d_cdiv(Q, kQb), S), dim3(kThreads), scan_lds_bytes(D), (hipStream_t)stream,
                     ref, ref_stride, ref_count, qry, qry_stride, Q, R, D, k, slice_rows_for(R, S), idx, dist2, w.part_d,
                     w.part_id);
  if (S > 1) {
    if (dh3d_launch_status() != DH3D_OK) return DH3D_ERR_LAUNCH;
    hipLaunchKernelGGL(retrieve_merge_kernel, dim3(dh3d_cdiv(Q, kWaves)), dim3(kThreads), 0, (hipStream_t)stream, w.part_d,
                       w.part_id, S, Q, k, idx, dist2);
  }
  return dh3d_launch_status();
}
