// Preparation of raw clouds for gfx950: voxel-grid down-sampling, radius-outlier removal, crop / pad to a fixed size
// (get_fixednum_pcd, core/utils.py:87-110, with open3d's voxel_down_sample and remove_radius_outlier in front).  The
// semantics are the project's own, stated in include/dh3d_hip.h (dh3d_prepare_clouds) and restated in numpy in
// tests/prepare_reference.py; every output is bit-exact against that restatement.  What is taken from open3d 0.9 / nanoflann
// from memory, not from a source on this tree, is marked INFERRED there and here:
//   INFERRED  the voxel origin is min_bound - voxel/2;
//   INFERRED  a voxel's point is the sum of its members in point order over their count;
//   INFERRED  the radius test is strict (d2 < r2);
//   INFERRED  a point is kept iff MORE than nb_points lie inside, the point itself counted.
// A point exactly on a voxel face or on a shell is the only place another reading would show.
//
// Every size is on the device (num_raw, the voxel count, the survivor count), so every launch covers the Nraw the caller
// declares and each kernel reads its cloud's count from the state words.  Kernel boundaries are the only grid-wide
// ordering; inside a kernel workgroups meet only through integer atomics whose result does not depend on arrival order.
//
//   stage 1   hash table on the 63-bit cell key (atomicCAS claims a slot, linear probing; 2 slots per point at least); per
//             slot the lowest member index (atomicMin), the member count and a linked list of the members (atomicExch on
//             the head; the list's order is arrival order and is never trusted).  A point is its voxel's representative iff it
//             is the slot's lowest index; the representatives compacted in index order number the voxels.  One thread per
//             voxel collects the list, sorts it by index and sums in double (up to 16 members, in private memory); larger
//             voxels are copied to a member array and sorted by a workgroup (bitonic, in LDS up to 4096 members).
//   stage 2   the same table keyed by cells of edge radius * (1 + 2^-20) over the stage-1 points (lists only); a point walks
//             the 27 cells around its own and leaves as soon as it has counted more than nb_points.
//   stage 3   float64 centroid by a fixed tree (tile partial sums, then the tiles in order); the targetnum smallest
//             (d2, index) by a radix select on the double's bit pattern (block_ops.h), one workgroup per cloud; ties on the
//             threshold go to the lowest indices through the same prefix scan that compacts.
// All three compactions: per-tile counts, a scan of the tile counts per cloud, in-tile ranks by a workgroup scan.
// This file is built with -ffp-contract=off: the double expressions below are evaluated as written.
#include "common.h"
#include "keys.h"
#include "block_ops.h"
#include "workspace.h"

namespace {

typedef unsigned long long u64;

constexpr int kMaxN = 131072;        // points per cloud
constexpr int kMaxTarget = 1 << 20;  // rows per output cloud
constexpr int kTile = 1024;          // points per workgroup in the tiled kernels
constexpr int kThreads = 256;
constexpr int kPer = kTile / kThreads;
constexpr u64 kEmpty = ~0ull;        // no 63-bit key
constexpr double kCellLimit = 2097152.0;  // 2^21 cells per axis
constexpr int kSmallVox = 16;        // members a single thread sorts
constexpr int kBigLds = 4096;        // members a workgroup sorts in LDS
constexpr int kBigBlocks = 64;       // workgroups per cloud over the list of large voxels
constexpr int kSelThreads = 1024;
constexpr float kPad = 100000.0f;

// state words of a cloud
enum { ST_N0 = 0, ST_N1, ST_N2, ST_ERR, ST_BUMP, ST_NBIG, ST_NEED, ST_LO, ST_INTS = 16 };

struct Ws {
  u64 *hkey, *dkey;
  double *tpart;
  int *head, *hrep, *hcnt, *slot, *next, *members, *flag, *big, *tsum, *toff, *st;
  float *p1, *p2;
  int N, H, T;
};

// The workspace of B clouds of N raw points, every segment rounded up to 16 bytes: fills every field of Ws.
Ws make_layout(Carve &c, int B, int N) {
  Ws w;
  w.N = N, w.H = 64;
  while (w.H < 2 * N) w.H <<= 1;
  w.T = dh3d_cdiv(N, kTile);
  const size_t b = (size_t)B, H = w.H, T = w.T, n = N;
  w.hkey = c.take<u64>(b * H, 16), w.dkey = c.take<u64>(b * n, 16), w.tpart = c.take<double>(b * T * 3, 16);
  w.head = c.take<int>(b * H, 16), w.hrep = c.take<int>(b * H, 16), w.hcnt = c.take<int>(b * H, 16);
  w.slot = c.take<int>(b * n, 16), w.next = c.take<int>(b * n, 16), w.members = c.take<int>(b * n, 16);
  w.flag = c.take<int>(b * n, 16), w.big = c.take<int>(b * (N / kSmallVox + 1) * 3, 16);
  w.tsum = c.take<int>(b * T * 2, 16), w.toff = c.take<int>(b * T * 2, 16), w.st = c.take<int>(b * ST_INTS, 16);
  w.p1 = c.take<float>(b * n * 3, 16), w.p2 = c.take<float>(b * n * 3, 16);
  return w;
}

__device__ __forceinline__ double sqdist(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }

// The flags (0, 1 or 2) of this thread's kPer consecutive points and their exclusive in-tile ranks, flag 1 in the low and
// flag 2 in the high 16 bits (a tile holds 1024 points: neither field overflows).
__device__ __forceinline__ void tile_ranks(const int *flag, int n, int i0, int (&f)[kPer], int (&r)[kPer], int *s_w) {
  int loc = 0;
#pragma unroll
  for (int e = 0; e < kPer; ++e) {
    f[e] = i0 + e < n ? flag[i0 + e] : 0;
    r[e] = loc;
    loc += (f[e] == 1) + ((f[e] == 2) << 16);
  }
  int total;
  const int base = block_excl_scan<kThreads>(loc, s_w, total);
#pragma unroll
  for (int e = 0; e < kPer; ++e) r[e] += base;
}

// ------------------------------------------------------------------------------------------------ table
// stage 1: the whole table and the state words; stage 2: keys, heads and the bounds again
__global__ __launch_bounds__(kThreads) void prep_init_kernel(Ws w, const int32_t *__restrict__ num_raw, int stage) {
  const int b = blockIdx.y, s = blockIdx.x * kThreads + threadIdx.x;
  if (s < w.H) {
    const size_t at = (size_t)b * w.H + s;
    w.hkey[at] = kEmpty;
    w.head[at] = -1;
    if (stage == 1) w.hrep[at] = 0x7FFFFFFF, w.hcnt[at] = 0;
  }
  if (s < ST_INTS) {
    int *st = w.st + b * ST_INTS;
    if (stage == 1) {
      int v = 0;
      if (s == ST_N0) v = min(max(num_raw[b], 0), w.N);  // (not keys.h clamp_count: the select form compiles to other code here)
      if (s >= ST_LO && s < ST_LO + 3) v = -1;
      st[s] = v;
    } else if (s >= ST_LO && s < ST_LO + 3) {
      st[s] = -1;
    }
  }
}

// per-axis minimum of a cloud's points: ordered bits, atomicMin (the result does not depend on the order)
__global__ __launch_bounds__(kThreads) void prep_min_kernel(Ws w, const float *__restrict__ src, int st_n) {
  const int b = blockIdx.y;
  int *st = w.st + b * ST_INTS;
  const int n = st[st_n];
  const float *p = src + (size_t)b * w.N * 3;
  unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  const int i0 = blockIdx.x * kTile + threadIdx.x;
  for (int e = 0; e < kPer; ++e) {
    const int i = i0 + e * kThreads;
    if (i < n) {
#pragma unroll
      for (int a = 0; a < 3; ++a) lo[a] = min(lo[a], f32_order_bits_nz(p[(size_t)i * 3 + a]));
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lo[a] = min(lo[a], (unsigned)__shfl_xor((int)lo[a], off, 64));
    if ((threadIdx.x & 63) == 0 && lo[a] != 0xFFFFFFFFu) atomicMin(reinterpret_cast<unsigned *>(st + ST_LO + a), lo[a]);
  }
}

// cell = floor((double(p) - origin) / edge) per axis, origin = double(lo) - half; false (and cell 0) outside [0, 2^21)
__device__ __forceinline__ bool cell_of(const float *p, const int *st, double half, double edge, int (&c)[3]) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double origin = (double)f32_from_order_bits((unsigned)st[ST_LO + a]) - half;
    const double q = floor(((double)p[a] - origin) / edge);
    const bool in = q >= 0.0 && q < kCellLimit;   // (false for a NaN)
    c[a] = in ? (int)q : 0;
    ok = ok && in;
  }
  return ok;
}
__device__ __forceinline__ u64 cell_key(int cx, int cy, int cz) { return (u64)cx | ((u64)cy << 21) | ((u64)cz << 42); }

// the slot of a key: found or claimed (insert), found or -1 (lookup)
__device__ __forceinline__ int table_insert(u64 *hkey, int H, u64 key) {
  int s = (int)(mix64(key) & (u64)(H - 1));
  for (int probe = 0; probe < H; ++probe) {
    const u64 prev = atomicCAS(hkey + s, kEmpty, key);
    if (prev == kEmpty || prev == key) return s;
    s = (s + 1) & (H - 1);
  }
  return -1;  // (never: the table has two slots per point)
}
__device__ __forceinline__ int table_find(const u64 *hkey, int H, u64 key) {
  int s = (int)(mix64(key) & (u64)(H - 1));
  for (int probe = 0; probe < H; ++probe) {
    const u64 k = hkey[s];
    if (k == key) return s;
    if (k == kEmpty) return -1;
    s = (s + 1) & (H - 1);
  }
  return -1;
}

template <bool STAGE1>
__global__ __launch_bounds__(kThreads) void prep_insert_kernel(Ws w, const float *__restrict__ src, int st_n, double half,
                                                               double edge) {
  const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
  int *st = w.st + b * ST_INTS;
  if (i >= st[st_n]) return;
  int c[3];
  if (!cell_of(src + ((size_t)b * w.N + i) * 3, st, half, edge, c)) atomicOr(st + ST_ERR, 1);
  const size_t tb = (size_t)b * w.H;
  int s = table_insert(w.hkey + tb, w.H, cell_key(c[0], c[1], c[2]));
  if (s < 0) {
    atomicOr(st + ST_ERR, 1);
    s = 0;
  }
  w.next[(size_t)b * w.N + i] = atomicExch(w.head + tb + s, i);
  if (STAGE1) {
    w.slot[(size_t)b * w.N + i] = s;
    atomicMin(w.hrep + tb + s, i);
    atomicAdd(w.hcnt + tb + s, 1);
  }
}

// ------------------------------------------------------------------------------------------------ compaction
__global__ __launch_bounds__(kThreads) void prep_rep_flag_kernel(Ws w) {
  const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= w.st[b * ST_INTS + ST_N0]) return;
  const size_t at = (size_t)b * w.N + i;
  w.flag[at] = w.hrep[(size_t)b * w.H + w.slot[at]] == i;
}

__global__ __launch_bounds__(kThreads) void prep_tile_sums_kernel(Ws w, int st_n) {
  __shared__ int s_w[4];
  const int b = blockIdx.y, n = w.st[b * ST_INTS + st_n];
  const int i0 = blockIdx.x * kTile + threadIdx.x * kPer;
  const int *flag = w.flag + (size_t)b * w.N;
  int one = 0, two = 0;
  for (int e = 0; e < kPer; ++e) {
    const int f = i0 + e < n ? flag[i0 + e] : 0;
    one += f == 1, two += f == 2;
  }
  int t1, t2;
  block_excl_scan<kThreads>(one, s_w, t1);
  block_excl_scan<kThreads>(two, s_w, t2);
  if (threadIdx.x == 0) {
    int *ts = w.tsum + ((size_t)b * w.T + blockIdx.x) * 2;
    ts[0] = t1, ts[1] = t2;
  }
}

// exclusive scan of a cloud's tile counts (T <= 128); the total of flag 1 goes to state word st_total (if >= 0)
__global__ __launch_bounds__(kThreads) void prep_tile_scan_kernel(Ws w, int st_total) {
  __shared__ int s_w[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const int *ts = w.tsum + (size_t)b * w.T * 2;
  const int a = t < w.T ? ts[t * 2] : 0, c = t < w.T ? ts[t * 2 + 1] : 0;
  int ta, tc;
  const int ea = block_excl_scan<kThreads>(a, s_w, ta);
  const int ec = block_excl_scan<kThreads>(c, s_w, tc);
  if (t < w.T) {
    int *to = w.toff + ((size_t)b * w.T + t) * 2;
    to[0] = ea, to[1] = ec;
  }
  if (t == 0 && st_total >= 0) w.st[b * ST_INTS + st_total] = ta;
}

// ------------------------------------------------------------------------------------------------ stage 1
// the mean of members m[0 .. c) (ascending) of cloud p: sums in double in that order, one division, rounded to f32
__device__ __forceinline__ void voxel_point(const float *p, const int *m, int c, float *out) {
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int k = 0; k < c; ++k) {
    const float *q = p + (size_t)m[k] * 3;
    sx += (double)q[0], sy += (double)q[1], sz += (double)q[2];
  }
  out[0] = (float)(sx / (double)c), out[1] = (float)(sy / (double)c), out[2] = (float)(sz / (double)c);
}

__global__ __launch_bounds__(kThreads) void prep_voxel_kernel(Ws w, const float *__restrict__ raw) {
  __shared__ int s_w[4];
  const int b = blockIdx.y, tile = blockIdx.x;
  int *st = w.st + b * ST_INTS;
  const int n = st[ST_N0], i0 = tile * kTile + threadIdx.x * kPer;
  const size_t pb = (size_t)b * w.N, tb = (size_t)b * w.H;
  int f[kPer], r[kPer];
  tile_ranks(w.flag + pb, n, i0, f, r, s_w);
  const int base = w.toff[((size_t)b * w.T + tile) * 2];
  const float *p = raw + pb * 3;
  for (int e = 0; e < kPer; ++e) {
    if (f[e] != 1) continue;
    const int v = base + (r[e] & 0xFFFF), s = w.slot[pb + i0 + e], c = w.hcnt[tb + s];
    if (c <= kSmallVox) {
      int m[kSmallVox];
      int k = 0;
      for (int j = w.head[tb + s]; j >= 0 && k < c; j = w.next[pb + j]) {  // insertion into the sorted prefix
        int at = k++;
        for (; at > 0 && m[at - 1] > j; --at) m[at] = m[at - 1];
        m[at] = j;
      }
      voxel_point(p, m, k, w.p1 + (pb + v) * 3);
    } else {
      const int off = atomicAdd(st + ST_BUMP, c);      // (the voxels' counts add up to n <= N: the array never overflows)
      int k = 0;
      for (int j = w.head[tb + s]; j >= 0 && k < c; j = w.next[pb + j]) w.members[pb + off + k++] = j;
      int *rec = w.big + ((size_t)b * (w.N / kSmallVox + 1) + atomicAdd(st + ST_NBIG, 1)) * 3;
      rec[0] = v, rec[1] = off, rec[2] = k;
    }
  }
}

__global__ __launch_bounds__(kThreads) void prep_big_voxel_kernel(Ws w, const float *__restrict__ raw) {
  __shared__ int s_m[kBigLds];
  const int b = blockIdx.y;
  const int *st = w.st + b * ST_INTS;
  const int nbig = min(st[ST_NBIG], w.N / kSmallVox + 1);
  const size_t pb = (size_t)b * w.N;
  for (int q = blockIdx.x; q < nbig; q += gridDim.x) {   // (uniform)
    const int *rec = w.big + ((size_t)b * (w.N / kSmallVox + 1) + q) * 3;
    const int v = rec[0], off = rec[1], c = rec[2];
    int *m = w.members + pb + off;
    __syncthreads();
    if (c <= kBigLds) {
      for (int k = threadIdx.x; k < c; k += kThreads) s_m[k] = m[k];
      m = s_m;
    }
    block_sort<kThreads>(m, c);  // (in LDS, or in place in the member array)
    if (threadIdx.x < 3) {                               // one axis per thread, each in member order
      const float *p = raw + pb * 3 + threadIdx.x;
      double s = 0.0;
      for (int k = 0; k < c; ++k) s += (double)p[(size_t)m[k] * 3];
      w.p1[(pb + v) * 3 + threadIdx.x] = (float)(s / (double)c);
    }
  }
}

// stage 1 switched off: the stage-1 points are the raw ones
__global__ __launch_bounds__(kThreads) void prep_copy_kernel(Ws w, const float *__restrict__ raw) {
  const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
  int *st = w.st + b * ST_INTS;
  const int n = st[ST_N0];
  if (i == 0) st[ST_N1] = n;
  if (i >= n) return;
  const size_t at = ((size_t)b * w.N + i) * 3;
  w.p1[at] = raw[at], w.p1[at + 1] = raw[at + 1], w.p1[at + 2] = raw[at + 2];
}

// ------------------------------------------------------------------------------------------------ stage 2
// flag[i] = more than nb points of the cloud lie at d2 < r2 of point i (i included); on = 0: every point is kept
__global__ __launch_bounds__(kThreads) void prep_radius_kernel(Ws w, int on, double edge, double r2, int nb) {
  const int b = blockIdx.y, i = blockIdx.x * kThreads + threadIdx.x;
  int *st = w.st + b * ST_INTS;
  if (i >= st[ST_N1]) return;
  const size_t pb = (size_t)b * w.N, tb = (size_t)b * w.H;
  if (!on) {
    w.flag[pb + i] = 1;
    return;
  }
  const float *p = w.p1 + pb * 3;
  const double x = (double)p[(size_t)i * 3], y = (double)p[(size_t)i * 3 + 1], z = (double)p[(size_t)i * 3 + 2];
  int c[3];
  cell_of(p + (size_t)i * 3, st, 0.0, edge, c);
  int cnt = 0;
  for (int o = 0; o < 27 && cnt <= nb; ++o) {
    // the point's own cell first: offsets 0, -1, +1 on every axis
    const int ox = o % 3, oy = (o / 3) % 3, oz = o / 9;
    const int cx = c[0] + (ox == 2 ? 1 : -ox), cy = c[1] + (oy == 2 ? 1 : -oy), cz = c[2] + (oz == 2 ? 1 : -oz);
    if (cx < 0 || cy < 0 || cz < 0 || cx >= (1 << 21) || cy >= (1 << 21) || cz >= (1 << 21)) continue;
    const int s = table_find(w.hkey + tb, w.H, cell_key(cx, cy, cz));
    if (s < 0) continue;
    int steps = 0;
    for (int j = w.head[tb + s]; j >= 0 && cnt <= nb && steps < w.N; j = w.next[pb + j], ++steps) {
      const float *q = p + (size_t)j * 3;
      cnt += sqdist(x - (double)q[0], y - (double)q[1], z - (double)q[2]) < r2;
    }
  }
  w.flag[pb + i] = cnt > nb;
}

// the survivors in order, and each tile's float64 partial sums of them (thread: its points in order; then a fixed tree)
__global__ __launch_bounds__(kThreads) void prep_survivors_kernel(Ws w) {
  __shared__ int s_w[4];
  __shared__ double s_red[4];
  const int b = blockIdx.y, tile = blockIdx.x;
  const int n = w.st[b * ST_INTS + ST_N1], i0 = tile * kTile + threadIdx.x * kPer;
  const size_t pb = (size_t)b * w.N;
  int f[kPer], r[kPer];
  tile_ranks(w.flag + pb, n, i0, f, r, s_w);
  const int base = w.toff[((size_t)b * w.T + tile) * 2];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int e = 0; e < kPer; ++e) {
    if (f[e] != 1) continue;
    const float *q = w.p1 + (pb + i0 + e) * 3;
    float *o = w.p2 + (pb + base + (r[e] & 0xFFFF)) * 3;
    o[0] = q[0], o[1] = q[1], o[2] = q[2];
    sx += (double)q[0], sy += (double)q[1], sz += (double)q[2];
  }
  sx = block_sum_256(sx, s_red), sy = block_sum_256(sy, s_red), sz = block_sum_256(sz, s_red);
  if (threadIdx.x == 0) {
    double *tp = w.tpart + ((size_t)b * w.T + tile) * 3;
    tp[0] = sx, tp[1] = sy, tp[2] = sz;
  }
}

// ------------------------------------------------------------------------------------------------ stage 3
// One workgroup per cloud: the centroid; then, where the cloud is cropped by distance, the targetnum-th smallest key
// (the bits of d2, which order as d2 does: it is never negative) by a radix select and the number of keys equal to it to
// take; flag = 1 below the threshold, 2 on it.  Elsewhere every survivor gets flag 1 (prep_output_kernel cuts at
// targetnum).
__global__ __launch_bounds__(kSelThreads) void prep_select_kernel(Ws w, int targetnum, int sortby, double *__restrict__ centroid) {
  __shared__ int s_hist[256], s_sel[2];
  __shared__ double s_c[3];
  const int b = blockIdx.x, tid = threadIdx.x;
  int *st = w.st + b * ST_INTS;
  const int m = st[ST_ERR] ? 0 : st[ST_N2];
  const size_t pb = (size_t)b * w.N;
  if (tid < 3) {
    double s = 0.0;
    const int tiles = (st[ST_N1] + kTile - 1) / kTile;
    for (int t = 0; t < tiles; ++t) s += w.tpart[((size_t)b * w.T + t) * 3 + tid];
    s_c[tid] = m > 0 ? s / (double)m : 0.0;
    centroid[b * 3 + tid] = s_c[tid];
  }
  __syncthreads();
  int *flag = w.flag + pb;
  if (!(sortby && m > targetnum)) {
    for (int i = tid; i < m; i += kSelThreads) flag[i] = 1;
    return;
  }
  const double cx = s_c[0], cy = s_c[1], cz = s_c[2];
  u64 *key = w.dkey + pb;
  const float *p = w.p2 + pb * 3;
  for (int i = tid; i < m; i += kSelThreads)
    key[i] = (u64)__double_as_longlong(sqdist((double)p[(size_t)i * 3] - cx, (double)p[(size_t)i * 3 + 1] - cy,
                                              (double)p[(size_t)i * 3 + 2] - cz));
  const BlockSelected sel = block_radix_select<kSelThreads>(m, targetnum, [&](int i, bool &) { return key[i]; }, s_hist, s_sel);
  const u64 tau = sel.key;
  if (tid == 0) st[ST_NEED] = sel.need;
  for (int i = tid; i < m; i += kSelThreads) flag[i] = key[i] < tau ? 1 : key[i] == tau ? 2 : 0;
}

// The kept rows in order, then the padding rows, num_valid and counts.  A cloud whose cells passed 2^21 on an axis is void:
// num_valid 0, every row padding, counts (n, -1, -1).
__global__ __launch_bounds__(kThreads) void prep_output_kernel(Ws w, int targetnum, float *__restrict__ points,
                                                               int32_t *__restrict__ num_valid, int32_t *__restrict__ counts) {
  __shared__ int s_w[4];
  const int b = blockIdx.y, tile = blockIdx.x;
  const int *st = w.st + b * ST_INTS;
  const bool err = st[ST_ERR] != 0;
  const int m = err ? 0 : st[ST_N2], nv = min(m, targetnum), need = st[ST_NEED];
  const size_t pb = (size_t)b * w.N;
  float *out = points + (size_t)b * targetnum * 3;
  if (tile < w.T) {                                      // (uniform)
    const int i0 = tile * kTile + threadIdx.x * kPer;
    int f[kPer], r[kPer];
    tile_ranks(w.flag + pb, m, i0, f, r, s_w);
    const int *to = w.toff + ((size_t)b * w.T + tile) * 2;
    for (int e = 0; e < kPer; ++e) {
      const int below = to[0] + (r[e] & 0xFFFF), on = to[1] + (r[e] >> 16);
      const bool keep = f[e] == 1 || (f[e] == 2 && on < need);
      const int at = below + min(on, need);
      if (keep && at < nv) {
        const float *q = w.p2 + (pb + i0 + e) * 3;
        out[(size_t)at * 3] = q[0], out[(size_t)at * 3 + 1] = q[1], out[(size_t)at * 3 + 2] = q[2];
      }
    }
  }
  for (int e = 0; e < kPer; ++e) {
    const int j = tile * kTile + e * kThreads + threadIdx.x;
    if (j >= nv && j < targetnum) out[(size_t)j * 3] = kPad, out[(size_t)j * 3 + 1] = kPad, out[(size_t)j * 3 + 2] = kPad;
  }
  if (tile == 0 && threadIdx.x == 0) {
    num_valid[b] = nv;
    counts[b * 3] = st[ST_N0], counts[b * 3 + 1] = err ? -1 : st[ST_N1], counts[b * 3 + 2] = err ? -1 : st[ST_N2];
  }
}

bool shape_ok(int B, int Nraw, int targetnum) { return B > 0 && Nraw > 0 && targetnum > 0; }
bool shape_served(int B, int Nraw, int targetnum) { return B <= 65535 && Nraw <= kMaxN && targetnum <= kMaxTarget; }

}  // namespace

DH3D_API size_t dh3d_prepare_clouds_workspace(int B, int Nraw, int targetnum) {
  if (!shape_ok(B, Nraw, targetnum) || !shape_served(B, Nraw, targetnum)) return 0;
  Carve c(nullptr);
  make_layout(c, B, Nraw);
  return c.bytes();
}

DH3D_API int dh3d_prepare_clouds(int B, int Nraw, int targetnum, const float *raw, const int32_t *num_raw, double voxel_size,
                                 double radius, int nb_points, int sortby_dis, float *points, int32_t *num_valid,
                                 int32_t *counts, double *centroid, void *workspace, size_t workspace_bytes, void *stream) {
  DH3D_REQUIRE(shape_ok(B, Nraw, targetnum) && raw && num_raw && points && num_valid && counts && centroid && workspace);
  DH3D_REQUIRE(voxel_size >= 0.0 && voxel_size < 1e300 && radius >= 0.0 && radius < 1e150 && nb_points >= 0);
  DH3D_SUPPORTED(shape_served(B, Nraw, targetnum));
  Carve c(workspace);
  const Ws w = make_layout(c, B, Nraw);
  DH3D_REQUIRE(workspace_bytes >= c.bytes() && ((uintptr_t)workspace & 15) == 0);

  hipStream_t s = (hipStream_t)stream;
  const dim3 blk(kThreads), per_slot(dh3d_cdiv(w.H, kThreads), B), per_point(dh3d_cdiv(Nraw, kThreads), B), per_tile(w.T, B);
  hipLaunchKernelGGL(prep_init_kernel, per_slot, blk, 0, s, w, num_raw, 1);
  if (voxel_size > 0.0) {
    hipLaunchKernelGGL(prep_min_kernel, per_tile, blk, 0, s, w, raw, (int)ST_N0);
    hipLaunchKernelGGL(prep_insert_kernel<true>, per_point, blk, 0, s, w, raw, (int)ST_N0, voxel_size / 2.0, voxel_size);
    hipLaunchKernelGGL(prep_rep_flag_kernel, per_point, blk, 0, s, w);
    hipLaunchKernelGGL(prep_tile_sums_kernel, per_tile, blk, 0, s, w, (int)ST_N0);
    hipLaunchKernelGGL(prep_tile_scan_kernel, dim3(B), blk, 0, s, w, (int)ST_N1);
    hipLaunchKernelGGL(prep_voxel_kernel, per_tile, blk, 0, s, w, raw);
    hipLaunchKernelGGL(prep_big_voxel_kernel, dim3(kBigBlocks, B), blk, 0, s, w, raw);
  } else {
    hipLaunchKernelGGL(prep_copy_kernel, per_point, blk, 0, s, w, raw);
  }
  const double edge = radius * (1.0 + 1.0 / 1048576.0);  // a little over the radius: rounding never splits a ball over 3 cells
  if (radius > 0.0) {
    hipLaunchKernelGGL(prep_init_kernel, per_slot, blk, 0, s, w, num_raw, 2);
    hipLaunchKernelGGL(prep_min_kernel, per_tile, blk, 0, s, w, (const float *)w.p1, (int)ST_N1);
    hipLaunchKernelGGL(prep_insert_kernel<false>, per_point, blk, 0, s, w, (const float *)w.p1, (int)ST_N1, 0.0, edge);
  }
  hipLaunchKernelGGL(prep_radius_kernel, per_point, blk, 0, s, w, radius > 0.0 ? 1 : 0, edge, radius * radius, nb_points);
  hipLaunchKernelGGL(prep_tile_sums_kernel, per_tile, blk, 0, s, w, (int)ST_N1);
  hipLaunchKernelGGL(prep_tile_scan_kernel, dim3(B), blk, 0, s, w, (int)ST_N2);
  hipLaunchKernelGGL(prep_survivors_kernel, per_tile, blk, 0, s, w);
  hipLaunchKernelGGL(prep_select_kernel, dim3(B), dim3(kSelThreads), 0, s, w, targetnum, sortby_dis != 0 ? 1 : 0, centroid);
  hipLaunchKernelGGL(prep_tile_sums_kernel, per_tile, blk, 0, s, w, (int)ST_N2);
  hipLaunchKernelGGL(prep_tile_scan_kernel, dim3(B), blk, 0, s, w, -1);
  const int out_tiles = dh3d_cdiv(Nraw > targetnum ? Nraw : targetnum, kTile);
  hipLaunchKernelGGL(prep_output_kernel, dim3(out_tiles, B), blk, 0, s, w, targetnum, points, num_valid, counts);
  return dh3d_launch_status();
}
