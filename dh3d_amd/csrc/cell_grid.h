// The cell table of dh3d_spatial_sort_cells (include/dh3d_hip.h states the layout for callers), device side: the slots, the
// header's decode, the cell of a coordinate and the table index of a cell.  One definition each: spatial.hip writes the
// table, knn.hip, ball_query.hip, icp.hip, iss.hip, pointnet2.hip and fps.hip read it, and tests/spatial_reference.py pins
// every slot bit for bit -- a reader with its own copy that differs in a clamp, a slot or a bit position returns a wrong
// neighbour on one kind of cloud only.  (cell_walk.h: what the radius searches do with the table.)
#pragma once
#include <hip/hip_runtime.h>

#include "dh3d_hip.h"

// ---- layout: ints of one cloud's table
constexpr int kGridCells = 4096;  // [0, kGridCells]: first sorted position of every cell in code order; [kGridCells] = N
constexpr int kCellCopy = 4097;   // from here on a table holds the GRID, not the points: fps.hip copies it to a subset's table
constexpr int kCellHead = 4100;   // as floats: origin x y z, then the quantisation scale per axis (a cell = 4 steps)
constexpr int kCellFlag = 4106;   // 1 = the points crowd into few cells: not a cloud for cell lists (the one slot not copied)
constexpr int kCellSched = 4107;  // the bit schedule: 12 x 2 bits, field s = the axis of code bit 11 - s
constexpr int kCellInts = 4112;   // ints per cloud
constexpr int kGridSteps = 12;    // schedule steps = bits of a cell's code
static_assert(kCellInts == DH3D_CELL_INTS && kCellSched < kCellInts && (1 << kGridSteps) == kGridCells, "cell table layout");

// Axis of step s of the 18-step bit schedule (step 0 = the sort key's most significant bit): the 12 grid steps from `sched`
// (2 bits each), then the sub-cell bits z y x z y x.
__device__ __forceinline__ int sched_axis(unsigned sched, int s) {
  return s < kGridSteps ? (int)((sched >> (2 * s)) & 3u) : 2 - (s - kGridSteps) % 3;
}

// Grid bits per axis over the schedule's first `steps` steps.  All 12: the grid, 2^nb[0] x 2^nb[1] x 2^nb[2] cells.  12 - D:
// the coarser grid without the code's D low bits, whose cells are 2^D consecutive cells of the table.
// (A field is 0, 1 or 2: with one mask bit per counted step, an axis' bits are a population count.)
__device__ __forceinline__ void sched_bits(unsigned sched, int nb[3], int steps = kGridSteps) {
  const unsigned f0 = sched, f1 = sched >> 1, m = 0x555555u & ((1u << (2 * steps)) - 1u);
  nb[0] = __popc(~(f0 | f1) & m); nb[1] = __popc(f0 & ~f1 & m); nb[2] = __popc(~f0 & f1 & m);
}

// One cloud's table with its header decoded.  (The table is uniform over a workgroup: all of this lives in scalar registers.)
struct CellGrid {
  const int *ct;           // the cloud's kCellInts ints
  float lo[3], scl[3];     // origin and quantisation scale
  unsigned sched;
  int nb[3];               // grid bits per axis
};
__device__ __forceinline__ CellGrid cell_grid(const int *cells, size_t cloud) {
  CellGrid g;
  g.ct = cells + cloud * kCellInts;
  const float *hd = reinterpret_cast<const float *>(g.ct) + kCellHead;
#pragma unroll
  for (int a = 0; a < 3; ++a) { g.lo[a] = hd[a]; g.scl[a] = hd[3 + a]; }
  g.sched = (unsigned)g.ct[kCellSched];
  sched_bits(g.sched, g.nb);
  return g;
}

// The cell of coordinate p on axis a: the sort's own expression (spatial.hip: (int)((p - lo) * scale), clamped to the axis'
// 2^(nb + 2) quantisation steps, >> 2).  The float clamp changes nothing inside the grid and keeps the conversion defined
// for a far, infinite or NaN p.  PINNED: every step -- the subtraction, the product with a positive scale, the clamps, the
// truncation, the shift -- is monotone in p IN FLOAT ARITHMETIC, so a point with x >= p lies in a cell >= grid_cell(p)
// whatever was rounded: a point of [plo, phi] lies in a cell of [grid_cell(plo), grid_cell(phi)].  The exactness arguments
// of icp_grid_kernel, ball_grid_kernel and three_nn_pruned_kernel_cells rest on this being the expression the points were
// binned with.
__device__ __forceinline__ int grid_cell(const CellGrid &g, int a, float p) {
  const float t = fminf(fmaxf((p - g.lo[a]) * g.scl[a], 0.f), 1.0e6f);
  return min((4 << g.nb[a]) - 1, (int)t) >> 2;
}

// The code of cell (ix, iy, iz): step s of the schedule puts the next lower bit of its axis' cell number at code bit
// 11 - s.  Two forms of the one rule.
// A lane's own cell, by the bit loop (the schedule is uniform: scalar branches).  D > 0: a cell of the coarser grid with
// nc = sched_bits(12 - D) bits per axis; its 12 - D bit code c is the table's cells [c << D, (c + 1) << D).
template <int D = 0>
__device__ __forceinline__ unsigned cell_code(unsigned sched, const int nc[3], int ix, int iy, int iz) {
  unsigned code = 0;
  int r0 = nc[0], r1 = nc[1], r2 = nc[2];
#pragma unroll
  for (int s = 0; s < kGridSteps - D; ++s) {
    const int a = sched_axis(sched, s);
    unsigned bit;
    if (a == 0) bit = (unsigned)(ix >> --r0) & 1u;
    else if (a == 1) bit = (unsigned)(iy >> --r1) & 1u;
    else bit = (unsigned)(iz >> --r2) & 1u;
    code |= bit << (kGridSteps - 1 - D - s);
  }
  return code;
}
// One axis' share, for a per-axis table in LDS (a cell's code = the OR of its three entries): the `bits` bits of axis a's
// value v that the schedule's first `steps` steps hold, step s at bit top - s.  The grid: (12, nb[a], 11); without D low
// bits: (12 - D, nc[a], 11), a table index at once; the sort's 18-bit key: (18, nb[a] + 2, 17).
__device__ __forceinline__ unsigned cell_deposit(unsigned sched, int a, int v, int steps, int bits, int top) {
  unsigned code = 0;
  for (int s = 0; s < steps; ++s)
    if (sched_axis(sched, s) == a && bits > 0) {
      --bits;
      code |= (unsigned)((v >> bits) & 1) << (top - s);
    }
  return code;
}
