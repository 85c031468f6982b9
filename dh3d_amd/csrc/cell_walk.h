// What the radius searches do with the cell table of cell_grid.h, one definition each: the per-axis deposit tables in LDS
// (icp.hip, iss.hip, knn.hip), the box of cells of a float32 ball (iss.hip; ball_grid_kernel writes the same lines out, for
// a measured reason its comment gives) and the lane-per-query walk over a box (icp.hip, iss.hip).  Each carries an exactness
// argument; a search with its own copy would have to restate it, and a copy that differs in a clamp or a margin loses a
// neighbour on one kind of cloud only.
#pragma once
#include "cell_grid.h"

// A box that meets more cells than this walks the 64-point groups instead (cell_walk, ball_grid_kernel).
constexpr int kWalkMaxCells = 512;

// ---- the deposit tables: tab[a][v] = the bits of axis a's cell number v at their places in the cell's code over the
// schedule's first `steps` steps (cell_grid.h cell_deposit), n0 n1 n2 = sched_bits(sched, ., steps).  The code of cell
// (ix, iy, iz) is then tab[0][ix] | tab[1][iy] | tab[2][iz].  Threads 0 .. 191 fill; ENDS IN A BARRIER: every thread of
// the workgroup must reach it.  The arguments are scalars on purpose: handed the CellGrid of a struct still under
// construction by reference, the barrier in here made the compiler keep that struct in scratch memory (112 bytes a lane in
// both ISS kernels); copies taken before the branch stay in scalar registers.
__device__ __forceinline__ void cell_deposit_tables(unsigned sched, int n0, int n1, int n2, int steps, unsigned (*tab)[64]) {
  if (threadIdx.x < 192) {
    const int ax = threadIdx.x >> 6;
    tab[ax][threadIdx.x & 63] =
        cell_deposit(sched, ax, threadIdx.x & 63, steps, ax == 0 ? n0 : ax == 1 ? n1 : n2, kGridSteps - 1);
  }
  __syncthreads();
}
// all twelve steps: the grid's own cells
__device__ __forceinline__ void cell_deposit_tables(const CellGrid &g, unsigned (*tab)[64]) {
  const unsigned sched = g.sched;
  const int n0 = g.nb[0], n1 = g.nb[1], n2 = g.nb[2];
  cell_deposit_tables(sched, n0, n1, n2, kGridSteps, tab);
}

// ---- a box of cells: c0 = its first cell per axis, cn = its cells per axis (>= 1; the product is at most kGridCells)
struct CellBox {
  int c0[3], cn[3];
};

// The cells that the box of the ball [q - r, q + r] meets, for a float32 membership test d2 < r * r (or sqrtf(d2) < r) on
// ((dx * dx + dy * dy) + dz * dz).  A point that passes has |x - q| < r (1 + 5 * 2^-24) on every axis; the margin covers
// that and the two roundings of q -+ r -+ margin, and the cell function is monotone (cell_grid.h grid_cell), so the
// point's cell lies in the box.  (A float64 test has another argument and its own edges: icp_grid_kernel.)
__device__ __forceinline__ CellBox ball_cells(const CellGrid &g, const float q[3], float r) {
  CellBox box;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float marg = r * 1e-5f + fabsf(q[a]) * 1e-6f;
    box.c0[a] = grid_cell(g, a, (q[a] - r) - marg);
    box.cn[a] = grid_cell(g, a, (q[a] + r) + marg) - box.c0[a] + 1;
  }
  return box;
}

// ---- the walk of one lane, LANE = QUERY, over one cloud: sc its N sorted records, gb the boxes of its 64-record groups,
// ct its table, tab the deposit tables of all twelve steps.  The contract:
//   * every lane of the wave must call it (the group walk is a wave-uniform loop); a lane whose `walks` is false takes
//     nothing;
//   * take(pos, sc[pos]) is called at most once per sorted position, in no promised order, until it returns false, which
//     ends the lane's walk;
//   * unless ended, a lane whose box has at most kWalkMaxCells cells takes every position of every cell of its box; any
//     other lane takes every position of every 64-record group for which reach(lo, hi) -- the caller's own test of the
//     group's box corners, in the caller's own precision -- is true.  So every record is taken that lies in a cell of the
//     box AND in a group that reach accepts: the caller's box and reach must each be conservative for its membership test.
// A lane's cells: one step = one read, the next cell's range while the lane has none, else the next record (what bounds
// these kernels is the instructions of a step times the steps of the wave's slowest lane).  The clamps keep a table of
// garbage inside the records.  The groups: the records are read as broadcasts; a lane that walked its cells, or whose walk
// has ended, only skips them.
template <class Reach, class Take>
__device__ __forceinline__ void cell_walk(const float4 *sc, const float *gb, const int *ct, int N, const unsigned (*tab)[64],
                                          const CellBox &box, bool walks, Reach reach, Take take) {
  const int *c0 = box.c0, *cn = box.cn;
  const bool by_cells = cn[0] * cn[1] * cn[2] <= kWalkMaxCells;
  if (walks && by_cells) {
    int pos = 0, end = 0, ox = 0, oy = 0, oz = 0;
    while (pos < end || oz < cn[2]) {
      if (pos < end) {
        if (!take(pos, sc[pos])) break;
        ++pos;
      } else {
        const unsigned code = tab[0][c0[0] + ox] | tab[1][c0[1] + oy] | tab[2][c0[2] + oz];
        if (++ox == cn[0]) {
          ox = 0;
          if (++oy == cn[1]) { oy = 0; ++oz; }
        }
        pos = max(ct[code], 0);
        end = min(ct[code + 1], N);
      }
    }
  }
  bool more = walks && !by_cells;
  if (__any(more)) {
    const int NG = (N + 63) / 64;
    for (int gi = 0; gi < NG; ++gi) {
      const float4 lo = *reinterpret_cast<const float4 *>(gb + (size_t)gi * 8);
      const float4 hi = *reinterpret_cast<const float4 *>(gb + (size_t)gi * 8 + 4);
      bool meet = more && reach(lo, hi);
      if (!__any(meet)) continue;
      const int len = min(64, N - gi * 64);
      for (int e = 0; e < len; ++e) {
        const float4 rec = sc[gi * 64 + e];
        if (meet && !take(gi * 64 + e, rec)) meet = more = false;  // (a take that never ends a walk leaves no flag to carry)
      }
    }
  }
}
