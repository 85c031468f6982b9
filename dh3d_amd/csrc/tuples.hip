// Training tuples on the device for gfx950: which places form a quadruplet, decided from the map's positions (and, for
// hard negatives, its descriptors) -- Global_train_dataset_triplet.__iter__ (core/datasets.py:202-233), which runs Python
// set differences over the whole training set per tuple.  include/dh3d_hip.h "Training tuples" states the contract; the
// draws are the counter RNG of "Training batches" (keys.h stream_h), the seed is read from device memory, nothing
// synchronises, allocates or branches into parallel launches, so bank -> tuple -> batch -> step is one capturable chain.
//   tuple_counts_kernel   grid ceil(M / 256), 256 threads, a place per thread; the live places stream through LDS in tiles
//                         of 256 positions, read as broadcasts.  The only O(M^2) piece; it runs once per map.
//   draw_select_kernel    one workgroup of 1024: the number of eligible places, the Q-th smallest stream-15 key among them by
//                         a radix select (block_ops.h; the keys recomputed on every pass, as in pairs.hip -- here under
//                         a predicate), then a stable compaction of the chosen (key, id) into the workspace.
//   draw_rank_kernel      grid ceil(Q / 256): a chosen place's slot is the number of chosen keys below its own.
//   sample_tuples_kernel  one 256-thread workgroup per query slot.  Pass 1: the four waves each stream a quarter of the
//                         places (16 B per lane, coalesced), test d2 against the two radii and keep one sorted 64-entry list
//                         per role (positives by stream 11, negatives by stream 12, pool members by descriptor distance), one
//                         key per lane: a candidate below the list's k-th key goes to the wave's LDS buffer by ballot +
//                         prefix count, a full buffer is folded by wave_fold (wave_ops.h), as retrieve_scan_kernel does.  Pool
//                         members are compacted to 64 ids per wave; their descriptor rows are staged through the wave's LDS
//                         tile in chunks of 32 columns (float4 loads, eight lanes a row) and lane l sums row l over ascending
//                         columns in one float64 accumulator -- dh3d_retrieve's rule.  The four waves' lists merge through
//                         LDS; wave 0 assembles [hard | random] and stages the up to 65 barring positions.  Pass 2 (other
//                         negative): a place's stream-14 key is compared with the wave's best so far BEFORE any distance; only
//                         a key that would win pays the 65 distance tests, about ln(M / 4) times per wave.
// A list is a function of the SET of places scanned, so nothing depends on which wave saw a place or in what order
// survivors arrived.  Compiled without contraction (csrc/Makefile EXACT): every id depends on the roundings of d2 and D2.
#include "common.h"
#include "keys.h"
#include "block_ops.h"
#include "workspace.h"

namespace {

typedef unsigned long long u64;
typedef Key96 Key;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBig = 1024;                  // threads of draw_select_kernel
constexpr int kMaxPlaces = 1 << 20;
constexpr int kMaxQueries = 65535;          // grid.x of sample_tuples_kernel stays far below its limit; the header's number
constexpr int kMaxPick = 64;                // a role's list is one entry per lane
constexpr int kMaxDim = 256;
constexpr int kChunk = 32;                  // descriptor columns per LDS chunk
constexpr int kTileStride = 66;             // floats between two columns of a wave's tile.  A read takes column c of rows
                                            // 0 .. 63: bank (2c + l) % 64, one lane each.  A store takes column 4a + k of row
                                            // 8i + b (a = lane & 7, b = lane >> 3): bank (8a + b + 2k + 8i) % 64, one lane each
constexpr unsigned kNoId = 0xFFFFFFFFu;

enum Stream : unsigned { kPosKeys = 11, kNegKeys = 12, kPool = 13, kOtherKeys = 14, kQueryKeys = 15 };  // include/dh3d_hip.h

// the lower of two keys, member by member (a select between two structs goes through memory)
__device__ __forceinline__ Key lower_of(const Key &a, const Key &b) {
  const bool lt = key_lt(b, a);
  return Key{lt ? b.d : a.d, lt ? b.id : a.id};
}

__device__ __forceinline__ double plane_d2(const double2 &from, const double2 &to) {
  const double dx = to.x - from.x, dy = to.y - from.y;
  return dx * dx + dy * dy;
}

__global__ __launch_bounds__(kThreads) void tuple_counts_kernel(const double2 *__restrict__ pos, const int32_t *__restrict__ count,
                                                                int M, double rp2, double rn2, int32_t *__restrict__ n_pos,
                                                                int32_t *__restrict__ n_neg) {
  __shared__ double2 s_p[kThreads];
  const int tid = threadIdx.x, i = blockIdx.x * kThreads + tid;
  const int n = count ? clamp_count(*count, M) : M;
  const bool live = i < n;
  const double2 me = live ? pos[i] : make_double2(0.0, 0.0);
  int np = 0, nn = 0;
  if (blockIdx.x * kThreads < n) {  // (workgroup-uniform)
    for (int j0 = 0; j0 < n; j0 += kThreads) {
      __syncthreads();
      if (j0 + tid < n) s_p[tid] = pos[j0 + tid];
      __syncthreads();
      const int m = n - j0 < kThreads ? n - j0 : kThreads;
      for (int t = 0; t < m; ++t) {
        const double d2 = plane_d2(me, s_p[t]);
        np += (d2 <= rp2 && j0 + t != i) ? 1 : 0;
        nn += d2 > rn2 ? 1 : 0;
      }
    }
  }
  if (i < M) n_pos[i] = live ? np : 0, n_neg[i] = live ? nn : 0;
}

struct DrawWs {  // the chosen places in index order: key, id; how many there are
  u64 *key;
  int32_t *id;
  int32_t *chosen;
  DrawWs(Carve &c, int Q) : key(c.take<u64>((size_t)Q, 16)), id(c.take<int32_t>((size_t)Q, 16)), chosen(c.take<int32_t>(1, 16)) {}
};

__global__ __launch_bounds__(kBig) void draw_select_kernel(const int32_t *__restrict__ n_pos, const int32_t *__restrict__ n_neg,
                                                           const int32_t *__restrict__ count, int M, int Q, int num_pos,
                                                           int num_neg, const u64 *__restrict__ seed, u64 *__restrict__ ws_key,
                                                           int32_t *__restrict__ ws_id, int32_t *__restrict__ ws_chosen,
                                                           int32_t *__restrict__ ok) {
  __shared__ int s_hist[256], s_sel[2], s_w[kBig / 64];
  __shared__ unsigned s_total;
  const int tid = threadIdx.x, lane = tid & 63;
  const int n = count ? clamp_count(*count, M) : M;
  const u64 h = stream_h(*seed, kQueryKeys, 0u);
  auto eligible = [&](int i) { return i < n && n_pos[i] >= num_pos && n_neg[i] >= num_neg; };

  if (tid == 0) s_total = 0;
  __syncthreads();
  unsigned mine = 0;
  for (int i = tid; i < n; i += kBig) mine += eligible(i) ? 1u : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if (lane == 0 && mine) atomicAdd(&s_total, mine);
  __syncthreads();
  const unsigned total = s_total;
  const unsigned want = total < (unsigned)Q ? total : (unsigned)Q;
  if (tid == 0) *ok = total >= (unsigned)Q ? 1 : 0, *ws_chosen = (int32_t)want;
  if (want == 0) return;  // (workgroup-uniform)

  // the want-th smallest key of the eligible places: the keys are distinct (splitmix64 is a bijection), so exactly `want`
  // of them are <= the result
  const u64 thr = block_radix_select<kBig>(n, (int)want, [&](int i, bool &valid) {
    valid = eligible(i);
    return splitmix64(h + (u64)i);
  }, s_hist, s_sel).key;

  int run = 0;
  for (int c = 0; c * kBig < n; ++c) {
    const int i = c * kBig + tid;
    const u64 key = splitmix64(h + (u64)i);
    const bool sel = eligible(i) && key <= thr;
    int all;
    const int at = run + block_compact_slot<kBig>(sel, s_w, all);
    if (sel && at < Q) ws_key[at] = key, ws_id[at] = i;
    run += all;
  }
}

__global__ __launch_bounds__(kThreads) void draw_rank_kernel(const u64 *__restrict__ ws_key, const int32_t *__restrict__ ws_id,
                                                             const int32_t *__restrict__ ws_chosen, int Q,
                                                             int32_t *__restrict__ queries) {
  __shared__ u64 s_k[kThreads];
  const int tid = threadIdx.x, t = blockIdx.x * kThreads + tid;
  int chosen = *ws_chosen;
  chosen = chosen < 0 ? 0 : (chosen > Q ? Q : chosen);
  const bool have = t < chosen;
  const u64 mine = have ? ws_key[t] : 0ull;
  int rank = 0;
  if (blockIdx.x * kThreads < chosen) {  // (workgroup-uniform)
    for (int j0 = 0; j0 < chosen; j0 += kThreads) {
      __syncthreads();
      if (j0 + tid < chosen) s_k[tid] = ws_key[j0 + tid];
      __syncthreads();
      const int m = chosen - j0 < kThreads ? chosen - j0 : kThreads;
      for (int e = 0; e < m; ++e) rank += s_k[e] < mine ? 1 : 0;
    }
  }
  if (have) queries[rank] = ws_id[t];   // the chosen keys are distinct: the ranks are 0 .. chosen-1, each once
  else if (t < Q) queries[t] = -1;
}

struct Shared {
  double q[kMaxDim];                       // the query's descriptor, float64
  float tile[kWaves][kChunk * kTileStride];  // per wave: one chunk of 64 pool rows, column-major
  u64 buf_k[kWaves][2][64];                // per wave and role (0 positives, 1 negatives): survivors' keys
  unsigned buf_i[kWaves][2][64];           //   and ids
  int pool[kWaves][64];                    // per wave: pool members awaiting their distance
  u64 list_k[kWaves][3][64];               // the waves' final lists (2: hard), for the merge
  unsigned list_i[kWaves][3][64];
  int cnt[kWaves][3];                      // |POS|, |NEG|, |POOL| seen by each wave
  double2 bar[kMaxPick + 1];               // the query and the negative row
  int negrow[kMaxPick];
  int filled;                              // bit 0: positives, bit 1: negatives
  u64 other_k[kWaves];
  unsigned other_i[kWaves];
};
static_assert(sizeof(Shared) <= 64 * 1024, "static LDS");

__global__ __launch_bounds__(kThreads) void sample_tuples_kernel(
    const double2 *__restrict__ pos, const int32_t *__restrict__ count, int M, const int32_t *__restrict__ queries, int num_pos,
    int num_neg, double rp2, double rn2, const float *__restrict__ desc, long long desc_stride, int D, int num_hard,
    double pool_fraction, const u64 *__restrict__ seed, int32_t *__restrict__ pos_idx, int32_t *__restrict__ neg_idx,
    int32_t *__restrict__ other_idx, int32_t *__restrict__ valid) {
  __shared__ __align__(16) Shared s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = count ? clamp_count(*count, M) : M;
  const int q = queries[b];
  const bool hard = desc != nullptr && num_hard > 0;
  int32_t *prow = pos_idx + (size_t)b * num_pos, *nrow = neg_idx + (size_t)b * num_neg;
  if (q < 0 || q >= n) {  // (workgroup-uniform)
    if (tid < num_pos) prow[tid] = -1;
    if (tid < num_neg) nrow[tid] = -1;
    if (tid == 0) {
      if (other_idx) other_idx[b] = -1;
      valid[b] = 0;
    }
    return;
  }
  const u64 sd = *seed;
  const u64 hp = stream_h(sd, kPosKeys, (unsigned)b), hn = stream_h(sd, kNegKeys, (unsigned)b);
  const u64 hl = stream_h(sd, kPool, (unsigned)b), ho = stream_h(sd, kOtherKeys, (unsigned)b);
  const double2 pq = pos[q];
  if (hard) {
    for (int c = tid; c < D; c += kThreads) s.q[c] = (double)desc[(long long)q * desc_stride + c];
    __syncthreads();
  }

  // ---------------------------------------------------------------------------------------------------------- pass 1
  Key list_p = key96_none(), list_n = key96_none(), list_h = key96_none();
  Key tau_p = key96_none(), tau_n = key96_none(), tau_h = key96_none();
  int cnt_p = 0, cnt_n = 0, cnt_pool = 0;  // entries waiting in the wave's buffers
  int np = 0, nn = 0, npool = 0;           // the sets' sizes over this wave's places
  auto flush = [&](Key &list, Key &tau, int &cnt, int role, int k) {
    wave_lds_sync();
    Key bv = key96_none();
    if (lane < cnt) bv = Key{s.buf_k[wave][role][lane], s.buf_i[wave][role][lane]};
    wave_lds_sync();
    list = wave_fold(list, bv, lane);
    tau = key_shfl(list, k - 1);
    cnt = 0;
  };
  auto offer = [&](const Key &key, bool take, Key &list, Key &tau, int &cnt, int role, int k) {
    const u64 mask = __ballot(take);
    if (!mask) return;  // (wave-uniform)
    const int add = __popcll(mask);
    if (cnt + add > 64) flush(list, tau, cnt, role, k);  // (what the new threshold would now refuse is still correct to keep)
    if (take) {
      const int slot = cnt + __popcll(mask & lanes_below());
      s.buf_k[wave][role][slot] = key.d;
      s.buf_i[wave][role][slot] = key.id;
    }
    cnt += add;
  };
  // the descriptor distance of the wave's cnt_pool waiting pool members, lane l summing row l, folded into the hard list
  auto measure_pool = [&]() {
    wave_lds_sync();
    const int mine = lane < cnt_pool ? s.pool[wave][lane] : -1;
    float *tile = s.tile[wave];
    const int lr = lane >> 3, lc = 4 * (lane & 7);
    double acc = 0.0;
    for (int c0 = 0; c0 < D; c0 += kChunk) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {  // row i * 8 + lr of the tile, columns c0 + lc .. + 3: eight lanes read 128 B of a row
        const int row = i * 8 + lr;
        const int rid = __shfl(mine, row, 64);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rid >= 0 && c0 + lc < D) v = *reinterpret_cast<const float4 *>(desc + (long long)rid * desc_stride + c0 + lc);
        tile[(lc + 0) * kTileStride + row] = v.x;
        tile[(lc + 1) * kTileStride + row] = v.y;
        tile[(lc + 2) * kTileStride + row] = v.z;
        tile[(lc + 3) * kTileStride + row] = v.w;
      }
      wave_lds_sync();
      const int cols = D - c0 < kChunk ? D - c0 : kChunk;
      for (int c = 0; c < cols; ++c) {
        const double d = s.q[c0 + c] - (double)tile[c * kTileStride + lane];
        acc = acc + d * d;
      }
      wave_lds_sync();
    }
    const Key key = mine >= 0 ? Key{(u64)__double_as_longlong(acc), (unsigned)mine} : key96_none();
    if (__ballot(key_lt(key, tau_h))) {
      list_h = wave_fold(list_h, key, lane);
      tau_h = key_shfl(list_h, num_hard - 1);
    }
    cnt_pool = 0;
  };

  for (int j0 = wave * 64; j0 < n; j0 += kThreads) {
    const int j = j0 + lane;
    const bool in = j < n;
    const double2 p = in ? pos[j] : pq;
    const double d2 = plane_d2(pq, p);
    const bool is_p = in && j != q && d2 <= rp2, is_n = in && d2 > rn2;
    const u64 mp = __ballot(is_p), mn = __ballot(is_n);
    np += __popcll(mp), nn += __popcll(mn);
    if (mp) {
      const Key key{splitmix64(hp + (u64)j), (unsigned)j};
      offer(key, is_p && key_lt(key, tau_p), list_p, tau_p, cnt_p, 0, num_pos);
    }
    if (mn) {
      const Key key{splitmix64(hn + (u64)j), (unsigned)j};
      offer(key, is_n && key_lt(key, tau_n), list_n, tau_n, cnt_n, 1, num_neg);
      if (hard) {
        const bool member = is_n && unit_co(splitmix64(hl + (u64)j)) < pool_fraction;
        const u64 mm = __ballot(member);
        if (mm) {
          const int add = __popcll(mm);
          npool += add;
          if (cnt_pool + add > 64) measure_pool();
          if (member) s.pool[wave][cnt_pool + __popcll(mm & lanes_below())] = j;
          cnt_pool += add;
        }
      }
    }
  }
  flush(list_p, tau_p, cnt_p, 0, num_pos);
  flush(list_n, tau_n, cnt_n, 1, num_neg);
  if (hard && cnt_pool) measure_pool();

  // ------------------------------------------------------------------------------------------- merge, rows, barring set
  s.list_k[wave][0][lane] = list_p.d, s.list_i[wave][0][lane] = list_p.id;
  s.list_k[wave][1][lane] = list_n.d, s.list_i[wave][1][lane] = list_n.id;
  s.list_k[wave][2][lane] = list_h.d, s.list_i[wave][2][lane] = list_h.id;
  if (lane == 0) s.cnt[wave][0] = np, s.cnt[wave][1] = nn, s.cnt[wave][2] = npool;
  __syncthreads();
  if (wave == 0) {
    int tp = np, tn = nn, tpool = npool;
    for (int w = 1; w < kWaves; ++w) {
      list_p = wave_fold(list_p, Key{s.list_k[w][0][lane], s.list_i[w][0][lane]}, lane);
      list_n = wave_fold(list_n, Key{s.list_k[w][1][lane], s.list_i[w][1][lane]}, lane);
      if (hard) list_h = wave_fold(list_h, Key{s.list_k[w][2][lane], s.list_i[w][2][lane]}, lane);
      tp += s.cnt[w][0], tn += s.cnt[w][1], tpool += s.cnt[w][2];
    }
    const bool pos_filled = tp >= num_pos, neg_filled = tn >= num_neg;
    if (lane < num_pos) prow[lane] = pos_filled ? (int32_t)list_p.id : -1;
    const int nh = hard ? (tpool < num_hard ? tpool : num_hard) : 0;  // h'
    bool is_hard = false;
    for (int t = 0; t < nh; ++t) is_hard = is_hard || __shfl(list_h.id, t, 64) == list_n.id;
    const bool keep = lane < num_neg && !is_hard;   // (neg_filled: the first num_neg entries of list_n are places)
    const u64 mk = __ballot(keep);
    const int at = nh + __popcll(mk & lanes_below());
    if (neg_filled) {
      if (lane < nh) s.negrow[lane] = (int)list_h.id;
      if (keep && at < num_neg) s.negrow[at] = (int)list_n.id;
    }
    wave_lds_sync();
    if (lane < num_neg) {
      const int g = neg_filled ? s.negrow[lane] : -1;
      nrow[lane] = g;
      if (neg_filled && other_idx) s.bar[1 + lane] = pos[g];
    }
    if (lane == 0) s.bar[0] = pq, s.filled = (pos_filled ? 1 : 0) | (neg_filled ? 2 : 0);
  }
  __syncthreads();
  const int filled = s.filled;
  if (!other_idx || !(filled & 2)) {  // (workgroup-uniform)
    if (tid == 0) {
      if (other_idx) other_idx[b] = -1;
      valid[b] = (filled == 3 && !other_idx) ? 1 : 0;
    }
    return;
  }

  // ---------------------------------------------------------------------------------------------------------- pass 2
  const int nbar = 1 + num_neg;
  Key best = key96_none();  // wave-uniform: the smallest stream-14 key of an unbarred place so far
  for (int j0 = wave * 64; j0 < n; j0 += kThreads) {
    const int j = j0 + lane;
    const bool in = j < n;
    const Key mine{splitmix64(ho + (u64)j), (unsigned)j};
    const bool cand = in && key_lt(mine, best);  // (no key: above every place's)
    if (!__ballot(cand)) continue;  // (wave-uniform)
    const double2 p = cand ? pos[j] : pq;
    bool barred = false;
    for (int t = 0; t < nbar; ++t) barred = barred || plane_d2(s.bar[t], p) <= rp2;
    const bool free_place = cand && !barred;
    if (!__ballot(free_place)) continue;
    Key low{free_place ? mine.d : kNoKey96, free_place ? mine.id : kNoId};
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) low = lower_of(low, key_shfl_xor(low, off));
    best = low;  // (every candidate was below the old best)
  }
  if (lane == 0) s.other_k[wave] = best.d, s.other_i[wave] = best.id;
  __syncthreads();
  if (tid == 0) {
    Key low{s.other_k[0], s.other_i[0]};
    for (int w = 1; w < kWaves; ++w) low = lower_of(low, Key{s.other_k[w], s.other_i[w]});
    const int other = low.id != kNoId ? (int)low.id : -1;
    other_idx[b] = other;
    valid[b] = (filled == 3 && other >= 0) ? 1 : 0;
  }
}

bool radii_ok(double pos_radius, double neg_radius) {
  return pos_radius > 0.0 && neg_radius > 0.0 && pos_radius < __builtin_inf() && neg_radius < __builtin_inf() &&
         neg_radius >= pos_radius;
}

}  // namespace

DH3D_API int dh3d_tuple_counts(const double *pos, const int32_t *count, int M, double pos_radius, double neg_radius,
                               int32_t *n_pos, int32_t *n_neg, void *stream) {
  DH3D_REQUIRE(pos && n_pos && n_neg && M > 0);
  DH3D_REQUIRE(radii_ok(pos_radius, neg_radius));
  DH3D_REQUIRE(((uintptr_t)pos & 15) == 0);
  DH3D_SUPPORTED(M <= kMaxPlaces);
  hipLaunchKernelGGL(tuple_counts_kernel, dim3(dh3d_cdiv(M, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const double2 *>(pos), count, M, pos_radius * pos_radius, neg_radius * neg_radius, n_pos,
                     n_neg);
  return dh3d_launch_status();
}

DH3D_API size_t dh3d_draw_queries_ws_bytes(int M, int Q) {
  if (M <= 0 || Q <= 0 || M > kMaxPlaces || Q > kMaxQueries) return 0;
  return carve_bytes<DrawWs>(Q);
}

DH3D_API int dh3d_draw_queries(const int32_t *n_pos, const int32_t *n_neg, const int32_t *count, int M, int Q, int num_pos,
                               int num_neg, const unsigned long long *seed, int32_t *queries, int32_t *ok, void *workspace,
                               size_t workspace_bytes, void *stream) {
  DH3D_REQUIRE(n_pos && n_neg && seed && queries && ok);
  DH3D_REQUIRE(M > 0 && Q > 0 && num_pos > 0 && num_neg > 0);
  DH3D_SUPPORTED(M <= kMaxPlaces && Q <= kMaxQueries && num_pos <= kMaxPick && num_neg <= kMaxPick);
  DH3D_REQUIRE(workspace && workspace_bytes >= carve_bytes<DrawWs>(Q) && ((uintptr_t)workspace & 15) == 0);
  Carve carve(workspace);
  const DrawWs w(carve, Q);
  hipLaunchKernelGGL(draw_select_kernel, dim3(1), dim3(kBig), 0, (hipStream_t)stream, n_pos, n_neg, count, M, Q, num_pos, num_neg,
                     seed, w.key, w.id, w.chosen, ok);
  if (dh3d_launch_status() != DH3D_OK) return DH3D_ERR_LAUNCH;
  hipLaunchKernelGGL(draw_rank_kernel, dim3(dh3d_cdiv(Q, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, w.key, w.id, w.chosen,
                     Q, queries);
  return dh3d_launch_status();
}

DH3D_API int dh3d_sample_tuples(const double *pos, const int32_t *count, int M, const int32_t *queries, int Q, int num_pos,
                                int num_neg, double pos_radius, double neg_radius, const float *desc, long long desc_stride, int D,
                                int num_hard, double pool_fraction, const unsigned long long *seed, int32_t *pos_idx,
                                int32_t *neg_idx, int32_t *other_idx, int32_t *valid, void *stream) {
  DH3D_REQUIRE(pos && queries && seed && pos_idx && neg_idx && valid);
  DH3D_REQUIRE(M > 0 && Q > 0 && num_pos > 0 && num_neg > 0 && num_hard >= 0);
  DH3D_REQUIRE(radii_ok(pos_radius, neg_radius));
  DH3D_REQUIRE(((uintptr_t)pos & 15) == 0);
  DH3D_SUPPORTED(M <= kMaxPlaces && Q <= kMaxQueries && num_pos <= kMaxPick && num_neg <= kMaxPick && num_hard <= num_neg);
  if (desc && num_hard > 0) {
    DH3D_REQUIRE(D > 0 && pool_fraction >= 0.0 && pool_fraction <= 1.0);
    DH3D_SUPPORTED(D <= kMaxDim && D % 4 == 0);
    DH3D_REQUIRE(desc_stride >= D && desc_stride % 4 == 0 && ((uintptr_t)desc & 15) == 0);
  }
  hipLaunchKernelGGL(sample_tuples_kernel, dim3(Q), dim3(kThreads), 0, (hipStream_t)stream,
                     reinterpret_cast<const double2 *>(pos), count, M, queries, num_pos, num_neg, pos_radius * pos_radius,
                     neg_radius * neg_radius, desc, desc_stride, D, num_hard, pool_fraction, seed, pos_idx, neg_idx, other_idx,
                     valid);
  return dh3d_launch_status();
}
