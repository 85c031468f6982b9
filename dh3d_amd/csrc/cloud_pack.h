// What a cloud batch looks like to dh3d_spatial_sort_cells when its rows carry a stride and a count: icp.hip (the anchor's
// cell table) and iss.hip (the detector's) hand the sort the same packed copy.  One definition: the copies' rule -- which
// row stands in for a row behind the count -- decides the grid's extent and which cells the stand-ins fill, and both
// readers refuse the stand-ins by their index.
#pragma once
#include <hip/hip_runtime.h>

#include "keys.h"

namespace {

constexpr int kPackThreads = 256;

// rows with an element stride -> [P, N, 3] for the sort.  Row r >= n becomes a copy of row r % n: whatever lies behind the
// count (prepare_clouds pads with 100000.0) stays out of the grid's extent, and the copies spread over the cloud's cells
// instead of crowding one.  The copies keep their own index r >= n, which the readers refuse.  n = 0: the rows as they are.
// Launch: dim3(cdiv(N, kPackThreads), P) x kPackThreads.
__global__ __launch_bounds__(kPackThreads) void cloud_pack_kernel(const float *__restrict__ a, long long stride, int N,
                                                                  const int32_t *__restrict__ count, float *__restrict__ out) {
  const int p = blockIdx.y, r = blockIdx.x * kPackThreads + threadIdx.x;
  if (r >= N) return;
  const int n = count ? clamp_count(count[p], N) : N;
  const float *src = a + ((long long)p * N + (r < n || n == 0 ? r : r % n)) * stride;
  float *dst = out + ((long long)p * N + r) * 3;
  dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
}

}  // namespace
