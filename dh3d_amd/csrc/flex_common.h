// Shared by the reference-layout flex operators (flex_generic.hip, flex_bwd.hip, flex_deconv.hip): the tile constants of
// the reference formulation's kernels, and the host steps every workspace path starts with.
#pragma once
#include "internal.h"
#include "workspace.h"

constexpr int kPts = 128;  // reference formulation: points per block (one per lane)
constexpr int kDT = 16;    // reference formulation: output channels held in registers per thread
constexpr int kMaxDp = 4;

#define AT3(p, b, c, n, C, N) (p)[((size_t)(b) * (C) + (c)) * (size_t)(N) + (n)]

// blocks of 256 threads for a grid-stride loop over `work` items, at most `cap`
static inline int flat_grid256(long long work, int cap) {
  long long g = (work + 255) / 256;
  return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

// Point-major copies of the reference-layout (channels-first) inputs; xyz / g stay null where an op has none.
struct PointMajor {
  float *f;      // [R, Din]
  int32_t *nbr;  // [R, K]
  float *xyz;    // [R, 3]
  float *g;      // [R, Dout]: the top gradient
};

// features [B,Din,N], neighborhood [B,K,N], positions [B,3,N] (may be null), topdiff [B,Dout,N] (may be null) -> pm
static inline int flex_to_point_major(const PointMajor &pm, const float *features, const int32_t *neighborhood,
                                      const float *positions, const float *topdiff, int B, int N, int K, int Din,
                                      int Dout, hipStream_t s) {
  int st;
  if ((st = dh3d_internal_transpose32(features, pm.f, B, Din, N, 0, 0, s)) != DH3D_OK) return st;
  if ((st = dh3d_internal_transpose32(neighborhood, pm.nbr, B, K, N, 0, 0, s)) != DH3D_OK) return st;
  if (positions && (st = dh3d_internal_transpose32(positions, pm.xyz, B, 3, N, 0, 0, s)) != DH3D_OK) return st;
  if (topdiff && (st = dh3d_internal_transpose32(topdiff, pm.g, B, Dout, N, 0, 0, s)) != DH3D_OK) return st;
  return DH3D_OK;
}

// Wcat = [bias; theta_x; theta_y; theta_z]: [4*Din, Dout]
static inline int flex_build_wcat(const float *bias, const float *theta, int Din, int Dout, float *Wcat, hipStream_t s) {
  const size_t plane = (size_t)Din * Dout;
  if (hipMemcpyAsync(Wcat, bias, sizeof(float) * plane, hipMemcpyDeviceToDevice, s) != hipSuccess ||
      hipMemcpyAsync(Wcat + plane, theta, sizeof(float) * 3 * plane, hipMemcpyDeviceToDevice, s) != hipSuccess)
    return DH3D_ERR_LAUNCH;
  return DH3D_OK;
}
