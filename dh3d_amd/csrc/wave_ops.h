// Wave64 reductions on the DPP crossbar (no LDS round trip, ONE VALU op per step) for gfx950.
//   quad_perm [1,0,3,2] -> quad_perm [2,3,0,1] -> row_half_mirror -> row_mirror   : every lane of a
//   16-lane row holds the row result; row_bcast:15 (rows 1,3) -> row_bcast:31 (rows 2,3): lane 63 holds
//   the wave result, which v_readlane broadcasts through an SGPR.  Valid for idempotent ops (max / min).
// Written as inline asm so that each step is a single v_max_f32_dpp / v_min_i32_dpp (hipcc emits
// v_mov_b32_dpp + op + a canonicalising v_max per step); the `s_nop 1` in front of every step is the
// gfx9 "VALU write -> DPP read of the same VGPR" hazard (2 wait states), which the compiler does not
// pad inside an asm statement.  Rows disabled by row_mask keep their value (dst == src).
#pragma once
#include <hip/hip_runtime.h>

#define DH3D_DPP_ROW16(OP)                                                      \
  "s_nop 1\n\t" OP " %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t" \
  "s_nop 1\n\t" OP " %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t" \
  "s_nop 1\n\t" OP " %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"     \
  "s_nop 1\n\t" OP " %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
#define DH3D_DPP_ROWS(OP)                                                       \
  "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"    \
  "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"    \
  "s_nop 1\n\t"

// The same chains on a NAMED asm operand (for hand-written loops): wave result in lane 63 of %[R].
#define DH3D_DPP_WAVE_N(OP, R)                                                                   \
  "s_nop 1\n\t" OP " %[" R "], %[" R "], %[" R "] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t" \
  "s_nop 1\n\t" OP " %[" R "], %[" R "], %[" R "] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t" \
  "s_nop 1\n\t" OP " %[" R "], %[" R "], %[" R "] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"     \
  "s_nop 1\n\t" OP " %[" R "], %[" R "], %[" R "] row_mirror row_mask:0xf bank_mask:0xf\n\t"          \
  "s_nop 1\n\t" OP " %[" R "], %[" R "], %[" R "] row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"        \
  "s_nop 1\n\t" OP " %[" R "], %[" R "], %[" R "] row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"

// max / min over each 16-lane row, result in every lane of the row
__device__ __forceinline__ float row16_max_f32(float v) {
  asm volatile(DH3D_DPP_ROW16("v_max_f32_dpp") "s_nop 1\n\t" : "+v"(v));
  return v;
}
__device__ __forceinline__ int row16_min_i32(int v) {
  asm volatile(DH3D_DPP_ROW16("v_min_i32_dpp") "s_nop 1\n\t" : "+v"(v));
  return v;
}
// wave-wide, result uniform (SGPR)
__device__ __forceinline__ float wave_max_f32(float v) {
  asm volatile(DH3D_DPP_ROW16("v_max_f32_dpp") DH3D_DPP_ROWS("v_max_f32_dpp") : "+v"(v));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ int wave_min_i32(int v) {
  asm volatile(DH3D_DPP_ROW16("v_min_i32_dpp") DH3D_DPP_ROWS("v_min_i32_dpp") : "+v"(v));
  return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
  asm volatile(DH3D_DPP_ROW16("v_min_u32_dpp") DH3D_DPP_ROWS("v_min_u32_dpp") : "+v"(v));
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

__device__ __forceinline__ float wave_min_f32(float v) {
  asm volatile(DH3D_DPP_ROW16("v_min_f32_dpp") DH3D_DPP_ROWS("v_min_f32_dpp") : "+v"(v));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float row16_min_f32(float v) {
  asm volatile(DH3D_DPP_ROW16("v_min_f32_dpp") "s_nop 1\n\t" : "+v"(v));
  return v;
}
// The largest of the eight 8-lane minima (lanes 8g .. 8g+7), wave-uniform: three min steps leave every lane of a half
// row with its group's minimum, row_mirror pairs the two groups of a row, the row_bcast steps carry the maximum to
// lane 63.  No input may be a NaN (v_min would drop it, v_max would not).
__device__ __forceinline__ float wave_max_of_min8_f32(float v) {
  asm volatile(
      "s_nop 1\n\tv_min_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_min_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_min_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
      "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf\n\t"
      DH3D_DPP_ROWS("v_max_f32_dpp")
      : "+v"(v));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// Sums (not idempotent, but every step pairs DISJOINT partial groups, so nothing is counted twice):
// after the four row steps every lane of a 16-lane row holds the row's sum; row_bcast:15 adds row 0's (2's) sum into
// row 1 (3).  Result: lanes 16..31 hold the sum of lanes 0..31, lanes 48..63 the sum of lanes 32..63.
__device__ __forceinline__ float row16_sum_f32(float v) {  // every lane: the sum over its 16-lane row
  asm volatile(DH3D_DPP_ROW16("v_add_f32_dpp") "s_nop 1\n\t" : "+v"(v));
  return v;
}
__device__ __forceinline__ float half32_sum_f32(float v) {
  asm volatile(DH3D_DPP_ROW16("v_add_f32_dpp")
               "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\ts_nop 1\n\t"
               : "+v"(v));
  return v;
}
// Two per-lane partial sums a, b (one value per lane each) -> lanes 16..31: sum of a over the wave, lanes 48..63: sum
// of b over the wave.  v_permlane32_swap (gfx950) exchanges a's upper half with b's lower half in one instruction.
__device__ __forceinline__ float pair_wave_sum_f32(float a, float b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  return half32_sum_f32(__uint_as_float(r[0]) + __uint_as_float(r[1]));
}

// ---------------------------------------------------------------------------------------------- lanes, LDS, broadcast
// The lanes of the wave below this one, as a ballot mask (kept in this form: the shift-and-decrement form compiles to
// other code in the kernels that use it).
__device__ __forceinline__ unsigned long long lanes_below() {
  const unsigned lane = threadIdx.x & 63;
  return lane ? (~0ull >> (64 - lane)) : 0ull;
}

// Inclusive prefix sum of v over the wave (int, unsigned, long long).
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = __shfl_up(v, off, 64);
    if (lane >= off) v += o;
  }
  return v;
}

// Orders the LDS traffic of ONE wave: what a lane wrote before is visible to every lane of the wave after.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// v of lane `lane` (wave-uniform) to every lane, through an SGPR.
__device__ __forceinline__ float wave_bcast_f32(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// ------------------------------------------------------------------------------------- sorted lists, one key per lane
// wave_sort / wave_merge / wave_fold work on any key type K that supplies, next to its definition,
//   bool key_lt(a, b)   a strict total order,     K key_shfl_xor(v, j)   v of lane ^ j,     K key_shfl(v, src)   v of lane src.
// unsigned long long is a key as it is.  Its min / max are overloads, not the generic form below: `a < b ? a : b` and
// `b < a ? b : a` are the same function and compile to different code.
__device__ __forceinline__ bool key_lt(unsigned long long a, unsigned long long b) { return a < b; }
__device__ __forceinline__ unsigned long long key_min(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long key_max(unsigned long long a, unsigned long long b) { return a < b ? b : a; }
__device__ __forceinline__ unsigned long long key_shfl_xor(unsigned long long v, int j) { return __shfl_xor(v, j, 64); }
__device__ __forceinline__ unsigned long long key_shfl(unsigned long long v, int src) { return __shfl(v, src, 64); }

// A 96-bit key, ascending by (d, id): d = the bits of a non-negative double (retrieval.hip) or a 64-bit random key
// (tuples.hip), id = the row it belongs to.
struct Key96 {
  unsigned long long d;
  unsigned id;
};
constexpr unsigned long long kNoKey96 = ~0ull;  // above the bits of +inf
__device__ __forceinline__ Key96 key96_none() { return Key96{kNoKey96, 0xFFFFFFFFu}; }
__device__ __forceinline__ bool key_lt(const Key96 &a, const Key96 &b) { return a.d < b.d || (a.d == b.d && a.id < b.id); }
__device__ __forceinline__ Key96 key_shfl_xor(const Key96 &v, int j) { return Key96{__shfl_xor(v.d, j, 64), __shfl_xor(v.id, j, 64)}; }
__device__ __forceinline__ Key96 key_shfl(const Key96 &v, int src) { return Key96{__shfl(v.d, src, 64), __shfl(v.id, src, 64)}; }

template <typename K>
__device__ __forceinline__ K key_min(const K &a, const K &b) { return key_lt(b, a) ? b : a; }
template <typename K>
__device__ __forceinline__ K key_max(const K &a, const K &b) { return key_lt(b, a) ? a : b; }

// ascending bitonic sort of one key per lane over the wave
template <typename K>
__device__ __forceinline__ K wave_sort(K v, int lane) {
#pragma unroll
  for (int k2 = 2; k2 <= 64; k2 <<= 1) {
#pragma unroll
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      const K o = key_shfl_xor(v, j);
      const bool take_min = ((lane & k2) == 0) == ((lane & j) == 0);
      v = take_min ? key_min(v, o) : key_max(v, o);
    }
  }
  return v;
}
// a bitonic sequence over the wave -> ascending
template <typename K>
__device__ __forceinline__ K wave_merge(K v, int lane) {
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    const K o = key_shfl_xor(v, j);
    v = (lane & j) == 0 ? key_min(v, o) : key_max(v, o);
  }
  return v;
}
// fold 64 keys (one per lane, any order) into the ascending list: sort them, reverse them against the list (the elementwise
// minimum is a bitonic sequence holding the 64 smallest of both), merge
template <typename K>
__device__ __forceinline__ K wave_fold(const K &list, K batch, int lane) {
  batch = wave_sort(batch, lane);
  return wave_merge(key_min(list, key_shfl(batch, 63 - lane)), lane);
}
