// Scalar helpers that several kernel files key, hash and index by.  One definition each: the restatements under tests/
// pin their results bit for bit, so a second copy that differs in a detail (-0, the increment) is a silent bug.
#pragma once
#include <hip/hip_runtime.h>

// Monotone map f32 -> u32: unsigned order of the result == float order of the argument (NaN outside the contract).
// -0 orders below +0; f32_order_bits_nz makes them one value first.  (fps.hip keeps an XOR form of its own, see there.)
__device__ __forceinline__ unsigned f32_order_bits(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned f32_order_bits_nz(float v) {
  if (v == 0.f) v = 0.f;  // -0.0 -> +0.0
  return f32_order_bits(v);
}
__device__ __forceinline__ float f32_from_order_bits(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// splitmix64's finaliser (a bijection of 64-bit words), and the generator's step on the counter z.
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) { return mix64(z + 0x9E3779B97F4A7C15ull); }

// The counter RNG of include/dh3d_hip.h "Training batches": h(stream, b), the draw u(stream, b, j) = splitmix64(h + j),
// and a draw as a double in [0, 1) / (0, 1].
__device__ __forceinline__ unsigned long long stream_h(unsigned long long seed, unsigned stream, unsigned b) {
  return splitmix64(splitmix64(seed) ^ (((unsigned long long)stream << 32) | (unsigned long long)b));
}
__device__ __forceinline__ double unit_co(unsigned long long u) { return (double)(u >> 11) * 0x1p-53; }            // [0, 1)
__device__ __forceinline__ double unit_oc(unsigned long long u) { return (double)(u >> 11) * 0x1p-53 + 0x1p-53; }  // (0, 1]

// A per-cloud count read from the device, held to [0, cap].
__device__ __forceinline__ int clamp_count(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

// LDS slot of component comp (0:x 1:y 2:z) of candidate c in the packed image of 4 consecutive candidates c0..c3
// (12 floats, three 16-byte reads):  [x0 x1 y0 y1] [z0 z1 x2 x3] [y2 y3 z2 z3]   -> pairs feed v_pk_* directly
__device__ __forceinline__ int cand4_slot(int c, int comp) {
  const int g = c >> 2, r = c & 3;
  return g * 12 + ((r < 2) ? (2 * comp + r) : (4 + 2 * comp + r));
}
