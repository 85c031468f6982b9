// The boxes of the spatial sort's 64-point groups, and the two tests the pruned searches make against them (knn.hip,
// pointnet2.hip, fps.hip).
//
// Layout, as dh3d_spatial_sort writes it: 8 floats per group of 64 consecutive records of the order,
//   [lo.x, lo.y, lo.z, _ | hi.x, hi.y, hi.z, _]
// the componentwise minimum and maximum of the group's points (the last group of a cloud may hold fewer than 64).
//
// Both tests return a LOWER bound of the squared distance between anything inside the one box and anything inside the
// other (or the point): per axis the gap e = max(lo - qhi, qlo - hi, 0) is exact up to one rounding, and the sum of the
// squares is scaled by (1 - 1e-5).  Why skipping on it is exact: the callers compare the result with a screening bound
// that a candidate's own squared distance s = fma(dz, dz, fma(dy, dy, dx * dx)) is compared with as well.  For a
// candidate inside the box every |d| is at least the axis' true gap, so s is at least the true gap sum up to the roundings
// of both chains, a few 1e-7 relative; the 1e-5 margin dwarfs them.  Hence gap2 > bound implies s > bound for every point
// of the box: a group skipped on `gap2 > bound` holds nothing the per-candidate screen `s <= bound` would have let
// through, ties at exactly the bound included (the callers skip on '>' and keep on '<=').
//
// For translation units built without contraction (the Makefile's EXACT list); the sums below are not to be fused either
// way, so the functions say so themselves and do not depend on where the header is included.
#pragma once

__device__ __forceinline__ float group_box_gap2(float lx, float ly, float lz, float hx, float hy, float hz,  //
                                                float qlx, float qly, float qlz, float qhx, float qhy, float qhz) {
#pragma clang fp contract(off)
  const float ex = fmaxf(fmaxf(lx - qhx, qlx - hx), 0.f);
  const float ey = fmaxf(fmaxf(ly - qhy, qly - hy), 0.f);
  const float ez = fmaxf(fmaxf(lz - qhz, qlz - hz), 0.f);
  return (ex * ex + ey * ey + ez * ez) * 0.99999f;
}
__device__ __forceinline__ float group_box_gap2(const float4 &lo, const float4 &hi, const float4 &qlo, const float4 &qhi) {
  return group_box_gap2(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, qlo.x, qlo.y, qlo.z, qhi.x, qhi.y, qhi.z);
}

// the box [q, q]
__device__ __forceinline__ float point_box_gap2(float lx, float ly, float lz, float hx, float hy, float hz,  //
                                                float qx, float qy, float qz) {
  return group_box_gap2(lx, ly, lz, hx, hy, hz, qx, qy, qz, qx, qy, qz);
}
__device__ __forceinline__ float point_box_gap2(const float4 &lo, const float4 &hi, float qx, float qy, float qz) {
  return group_box_gap2(lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, qx, qy, qz, qx, qy, qz);
}
