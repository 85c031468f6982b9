// Exact workgroup building blocks for gfx950: prefix sum, ordered compaction, radix select and an LDS sort, for a
// workgroup of NT threads (a multiple of 64, one-dimensional).  Every result is an integer prefix, an order statistic or
// a permutation, so none depends on how the work is split.  Every function must be reached by ALL threads of the
// workgroup (barriers inside); the barriers each one contains and what the caller may assume are stated with it.
// Two files keep copies of their own on purpose: pairs.hip (select and compaction in front of pair_fps_kernel's pick loop)
// and registration.hip (the compaction in front of ransac_kernel's trial loop).  With these helpers inlined the compiler
// allocates those long loops differently and both kernels measured 1.5 to 2.5 % slower; wave_incl_scan alone did the same
// to pair_fps_kernel.
#pragma once
#include "wave_ops.h"

// The sum of the totals of the waves below this one, and of all waves; wave_total is read from lane 63 of each wave.
// s_w: NT / 64 ints.  Barriers: one before s_w is written, one after.  Entry: a slower wave may still be reading s_w (an
// earlier call's).  Exit: s_w is still being read; only another call of this header may write it with no barrier between.
template <int NT>
__device__ __forceinline__ int block_waves_below(int wave_total, int *s_w, int &total) {
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 63) s_w[wave] = wave_total;
  __syncthreads();
  int below = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const int t = s_w[w];
    below += w < wave ? t : 0;
    total += t;
  }
  return below;
}

// Exclusive prefix of v over the workgroup in thread order; the workgroup's total to every thread.  s_w, barriers and
// contract: block_waves_below's.
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int *s_w, int &total) {
  const int inc = wave_incl_scan(v);
  return block_waves_below<NT>(inc, s_w, total) + inc - v;
}

// Ordered compaction: the number of threads below this one whose `keep` is set, and the number of all that are.  One
// ballot per wave in place of the wave's scan; s_w, barriers and contract: block_waves_below's.
template <int NT>
__device__ __forceinline__ int block_compact_slot(bool keep, int *s_w, int &total) {
  const unsigned long long bal = __ballot(keep);
  return block_waves_below<NT>(__popcll(bal), s_w, total) + __popcll(bal & lanes_below());
}

// The k-th smallest (1 <= k <= n, both workgroup-uniform) of the 64-bit keys key_of(i, valid), i < n, to every thread;
// `need` = how many keys EQUAL to it belong to the k smallest (1 when the keys are distinct).  key_of(i, valid) returns
// the key of element i and sets valid = false for an element that does not take part (its return value is ignored then);
// at least k elements must take part.  It is called eight times per element, so it is either a load or cheap to recompute.
// MSB-first, 8 passes of 8 bits.  A pass: every thread adds its candidates (the keys that agree with the digits found so
// far) to the 256-bin histogram -- one LDS atomic per wave when all the wave's candidates share a bin, which is the rule
// for the top bytes of ordered float bits; wave 0 then owns 4 bins a lane, finds the bin where the running count reaches
// k by one wave scan, and zeroes the bins for the next pass.
// s_hist: 256 ints, s_sel: 2 ints.  Barriers: one after the histogram is first zeroed (it precedes the first key_of, so
// what the caller wrote before the call -- LDS or global -- is visible to key_of), then two per pass.  Entry: no thread
// may still be using s_hist or s_sel.  Exit: s_hist is all zero; s_sel is still being read, so a barrier must come
// before anything but another call of this function writes it.
struct BlockSelected {
  unsigned long long key;
  int need;
};
template <int NT, class KeyOf>
__device__ __forceinline__ BlockSelected block_radix_select(int n, int k, KeyOf key_of, int *s_hist, int *s_sel) {
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 256) s_hist[tid] = 0;
  __syncthreads();
  unsigned long long prefix = 0ull, mask = 0ull;
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int base = 0; base < n; base += NT) {  // (uniform trip count: the ballots see whole waves)
      const int i = base + tid;
      bool in = i < n;
      const unsigned long long key = in ? key_of(i, in) : 0ull;
      in = in && (key & mask) == prefix;
      const int bin = (int)((key >> shift) & 255ull);
      const unsigned long long act = __ballot(in);
      if (!act) continue;  // (wave-uniform)
      const int first = __builtin_amdgcn_readlane(bin, __builtin_ctzll(act));  // the bin of the lowest candidate lane
      const unsigned long long same = __ballot(in && bin == first);
      if (same == act) {
        if (in && (same & lanes_below()) == 0ull) atomicAdd(&s_hist[first], __popcll(act));
      } else if (in) {
        atomicAdd(&s_hist[bin], 1);
      }
    }
    __syncthreads();
    if (tid < 64) {  // lane l owns bins 4l .. 4l+3
      const int c0 = s_hist[4 * lane], c1 = s_hist[4 * lane + 1], c2 = s_hist[4 * lane + 2], c3 = s_hist[4 * lane + 3];
      s_hist[4 * lane] = 0, s_hist[4 * lane + 1] = 0, s_hist[4 * lane + 2] = 0, s_hist[4 * lane + 3] = 0;
      const int sum = c0 + c1 + c2 + c3, incl = wave_incl_scan(sum);
      int before = incl - sum;
      if (before < k && k <= incl) {  // one lane
        int bin = 4 * lane;
        if (k > before + c0) { before += c0, ++bin;
          if (k > before + c1) { before += c1, ++bin;
            if (k > before + c2) before += c2, ++bin; } }
        s_sel[0] = bin;
        s_sel[1] = k - before;
      }
    }
    __syncthreads();
    prefix |= (unsigned long long)s_sel[0] << shift;
    mask |= 255ull << shift;
    k = s_sel[1];
  }
  return BlockSelected{prefix, k};
}

// Ascending (by `less`, a strict weak order) bitonic sort of s[0 .. n) by the workgroup, any n (workgroup-uniform): every
// comparator puts the lesser at the lower position (flip, then disperse), so positions >= n act as +inf and their
// comparators are skipped -- no padding.  s: LDS, or global memory that only this workgroup touches.
// Barriers: one on entry (what any thread wrote to s before the call is sorted), one after every step; on exit s is
// sorted and visible to every thread.
template <int NT, typename T, class Less>
__device__ __forceinline__ void block_sort(T *s, int n, Less less) {
  __syncthreads();
  for (int k2 = 2; k2 < 2 * n; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += NT) {
        const int l = j == (k2 >> 1) ? i ^ (k2 - 1) : i ^ j;
        if (l > i && l < n) {
          const T x = s[i], y = s[l];
          if (less(y, x)) s[i] = y, s[l] = x;
        }
      }
      __syncthreads();
    }
  }
}
template <int NT, typename T>
__device__ __forceinline__ void block_sort(T *s, int n) {
  block_sort<NT>(s, n, [](const T &a, const T &b) { return a < b; });
}
