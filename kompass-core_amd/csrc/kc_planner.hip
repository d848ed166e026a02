// Grid planner on gfx950: occupancy grid -> footprint validity -> exact 8-connected cost field from the goal ->
// steepest-descent path.  Everything is integer work on cells; the world <-> cell conversions
// and the radius -> R2 rule live in the host class (csrc/host/src/grid_planner.cpp).
//
// The reference has no counterpart: its planning submodule wraps OMPL (planning/ompl.h), which stays out of
// scope.  The yardstick is the heap Dijkstra of tests/planner_ref.py, bit for bit.
//
//  (a) validity.  planner_classify_kernel turns the grid's cells (int32 as the mapper writes them, int8 as
//      kc_cloud_grid_fill does) into a class byte; planner_rowdist_kernel takes, per cell, the distance in cells
//      to the nearest blocking cell of its own row (255: none within R); planner_valid_kernel asks the 2 R + 1
//      rows around a cell for rowdist^2 + dy^2 <= R2.  The nearest blocker of a row is the one that decides that
//      row, so the two passes are the disc test exactly, at O(R) loads a cell instead of O(R^2).
//  (b) cost field.  planner_relax_kernel is a tile pass (below) whose rule is the 8-connected step with the corner
//      rule.  The host launches passes in batches of kPlanBatch and reads the changed word back once per batch; a word
//      older than the batch's last pass means that pass changed nothing, i.e. both buffers hold the fixed point.
//  (c) path.  planner_walk_kernel is a walk (below) over cells: eight lanes load the eight neighbours of the current cell.
//
//  A tile pass: one workgroup per 64 x 64 tile, the tile and a one-cell halo in LDS (plan_tile_origin, plan_load_halo),
//  Jacobi iterations in LDS until the tile stops changing (or 256 iterations), the tile written to the OTHER of two field
//  buffers.  A pass reads one buffer and writes the other: no workgroup reads what another one writes in the same launch,
//  none waits for another, and the field after k passes is the same on every run.  A workgroup that changed a cell stores
//  the pass number into one device word, the changed word.  A walk: one wavefront walks down a converged field, a state an
//  iteration; a shuffle reduction (plan_min_key) takes the smallest (value, lane) pair among the lanes' candidates.
//  (d) clearance cost (rules 6 to 8; off unless kc_planner_set_clearance_cost gave a table).  The row pass reaches
//      max(R, Rc) cells; planner_clear_kernel takes min(rowdist^2 + dy^2) over the rows in reach and writes clear2,
//      the table's penalty and the validity map in one go.  planner_relax_kernel<true> adds the penalty of the cell
//      a step leaves, one register per owned cell; planner_walk_kernel<true> follows field + step and keeps the
//      smallest clear2 it visits.  The <false> instantiations are the code of the planner without the cost.
//  (e) any-angle path (rules 9 to 12; on request, kc_planner_shortcut).  planner_shortcut_kernel: one workgroup behind
//      the walk loops over the anchors; the window of the walk behind an anchor sits in LDS, its candidates go one
//      to a wavefront from the far end in rounds of 16, the lanes of a wavefront stride over the columns of their
//      segment and test the up to three touched cells of a column, and the largest clear index of the first round
//      that has one is the next anchor.
//  (f) oriented box footprint (rules 13 to 18; off unless kc_planner_set_oriented gave a box).  The state is (cell,
//      class), four classes.  The turning disc goes through the row and column passes of (a) with r2 = T2;
//      planner_oriented_valid_kernel tests the four host-built offset lists, nearest offsets first, and skips the cells
//      the disc already cleared (T2 contains every mask); a byte a cell holds the four class bits and the turn bit.
//      planner_relax4_kernel is a tile pass over four layers, 16 states a lane; layers 0 and 2 couple along rows and
//      columns, 1 and 3 along the diagonals, all four at the same cell by a turn.  planner_walk4_kernel is a walk over
//      states: four lanes, the two moves of the class and the two turns.
//
//  (g) replan (rules 19 and 20; kc_planner_replan).  The context keeps the field of its last solve, and through a new
//      grid its validity map and penalty.  planner_touched_kernel compares them with the new grid's and reduces the
//      rollback threshold T; planner_rollback_kernel puts every value below T back into both buffers and marks the tiles
//      that hold a cell that may still change; planner_relax_list_kernel is (b) over those tiles only.
//
//  (h) exploration (rules 21 to 26; kc_planner_explore).  The validity of (a) with unknown not blocking, then
//      planner_known_kernel takes the unknown cells out; the field of (b) rooted at the robot's cell;
//      planner_frontier_mark_kernel writes the frontier bytes, both label planes and the tiles that hold a frontier cell;
//      planner_label_kernel is a tile pass with "the smallest label among my eight frontier neighbours and me" as its
//      rule, over the listed tiles; sizes, kept roots and the records go by vector
//      atomics from plain HIP (32-bit add at the root, 64-bit add and min at the record); planner_walk_kernel<false, true>
//      walks from an entry cell down to the robot by field + step, so that the path costs what the record says.
//
//  (i) car motion (rules 27 to 36; off unless kc_planner_set_car gave a turn length).  The state is (cell, one of eight
//      directed headings); the transitions are one straight step and 45-degree arcs of n cells a leg, backward at a price
//      or not at all, no turn in place.  planner_car_steps_kernel writes a byte a cell (bit h: the unit step along +D[h] is
//      allowed) from the validity map of (a) or (f); planner_car_moves_kernel walks every arc's polyline over those bytes
//      once a solve and writes a byte a state (bits 0 .. 5: S, L, R, B, BL, BR).  planner_relax8_kernel is a tile pass with
//      a workgroup per (tile, heading): its rule is the straight moves, which couple one layer along one line; the arc
//      candidates, which reach up to 2 n cells into the two neighbouring layers, are taken once a pass from the read-only
//      input.  planner_walk8_kernel is a walk over states: six lanes, a primitive each.
//
// Plain vector loads and stores only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

#include "kc_internal.h"
#include "kompass_hip.h"

namespace kc {

constexpr uint32_t kPlanInf = 0xFFFFFFFFu;
constexpr int kPlanTile = 64;                  // cells per side of a tile
constexpr int kPlanHalo = kPlanTile + 2;       // ... with the one-cell ring around it
constexpr int kPlanThreads = 1024;             // 16 wavefronts, four cells a lane
constexpr int kPlanRows = kPlanTile * kPlanTile / kPlanThreads;
constexpr int kPlanLocalIters = 4 * kPlanTile; // Jacobi iterations per tile and pass at the most
constexpr int kPlanBatch = 8;                  // passes per read-back of the changed word
constexpr int kPlanBlock = 256;
constexpr int kPlanMaxBlocks = 2048;
constexpr int kShortThreads = 1024;            // the shortcut's one workgroup: 16 wavefronts, a candidate each
constexpr int kShortWaves = kShortThreads / 64;

// the neighbour order of the walk (ties go to the first): E, N, W, S, NE, NW, SW, SE
__constant__ const int kPlanDx[8] = {1, 0, -1, 0, 1, -1, -1, 1};
__constant__ const int kPlanDy[8] = {0, 1, 0, -1, 1, 1, -1, -1};

template <typename T>
__global__ __launch_bounds__(kPlanBlock) void planner_classify_kernel(const T *grid, uint8_t *cls, long long n) {
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
    const int v = static_cast<int>(grid[i]);
    cls[i] = v == KC_OCCUPIED ? 2 : (v == KC_UNEXPLORED ? 1 : 0);
  }
}

__device__ __forceinline__ bool plan_blocks(uint8_t c, int block_unknown) { return c == 2 || (c == 1 && block_unknown); }

__global__ __launch_bounds__(kPlanBlock) void planner_rowdist_kernel(const uint8_t *cls, uint8_t *rowd, int W, int H, int R,
                                                                     int block_unknown) {
  const long long n = static_cast<long long>(W) * H;
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
    const int x = static_cast<int>(i % W);
    const uint8_t *row = cls + (i - x);
    int found = 255;
    for (int d = 0; d <= R; ++d) {
      const bool l = x - d >= 0 && plan_blocks(row[x - d], block_unknown);   // cells outside the grid do not block
      const bool r = x + d < W && plan_blocks(row[x + d], block_unknown);
      if (l || r) {
        found = d;
        break;
      }
    }
    rowd[i] = static_cast<uint8_t>(found);
  }
}

__global__ __launch_bounds__(kPlanBlock) void planner_valid_kernel(const uint8_t *rowd, uint8_t *valid, int W, int H, int R,
                                                                   uint32_t R2) {
  const long long n = static_cast<long long>(W) * H;
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
    const int y = static_cast<int>(i / W);
    const int lo = max(-R, -y), hi = min(R, H - 1 - y);
    uint8_t ok = 1;
    for (int dy = lo; dy <= hi; ++dy) {
      const uint32_t d = rowd[i + static_cast<long long>(dy) * W];
      if (d != 255u && d * d + static_cast<uint32_t>(dy * dy) <= R2) {
        ok = 0;
        break;
      }
    }
    valid[i] = ok;
  }
}

// rule 6 and the table of rule 7 in one column pass: rowd holds the row distances within Rm = max(R, Rc) cells
__global__ __launch_bounds__(kPlanBlock) void planner_clear_kernel(const uint8_t *rowd, const uint32_t *pen_by_d2, uint16_t *clear2,
                                                                   uint32_t *pen, uint8_t *valid, int W, int H, int Rm,
                                                                   uint32_t R2, uint32_t C2) {
  const long long n = static_cast<long long>(W) * H;
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
    const int y = static_cast<int>(i / W);
    const int lo = max(-Rm, -y), hi = min(Rm, H - 1 - y);
    uint32_t best = kPlanInf;  // the nearest blocking cell within Rm columns and Rm rows
    for (int dy = lo; dy <= hi; ++dy) {
      const uint32_t d = rowd[i + static_cast<long long>(dy) * W];
      if (d != 255u) best = min(best, d * d + static_cast<uint32_t>(dy * dy));
    }
    // Rm covers both discs: a blocking cell within R2 or C2 is within Rm of the cell in both directions
    const bool near = best <= C2;
    clear2[i] = near ? static_cast<uint16_t>(best) : static_cast<uint16_t>(KC_PLANNER_CLEAR_FAR);
    pen[i] = near ? pen_by_d2[best] : 0u;
    valid[i] = best <= R2 ? 0 : 1;
  }
}

__global__ __launch_bounds__(kPlanBlock) void planner_init_kernel(uint32_t *a, uint32_t *b, const uint8_t *valid, long long n,
                                                                  long long goal) {
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
    const uint32_t v = (i == goal && valid[i]) ? 0u : kPlanInf;
    a[i] = v;
    b[i] = v;
  }
}

// ---- what the tile passes (planner_relax_kernel, planner_label_kernel, planner_relax4_kernel, planner_relax8_kernel) share
constexpr int kPlanRegion = kPlanHalo * kPlanHalo;  // values of one layer's halo region in LDS

// the grid cell of the halo region's corner.  The tiles are numbered row by row along gridDim.x: a 1 x 2^28 grid has more
// tile rows than gridDim.y holds
__device__ __forceinline__ void plan_tile_origin(unsigned tile, unsigned tiles_x, int *x0, int *y0) {
  *x0 = static_cast<int>(tile % tiles_x) * kPlanTile - 1;
  *y0 = static_cast<int>(tile / tiles_x) * kPlanTile - 1;
}

// the halo region of L layers (layer l of `in` is its cells [l * n, (l + 1) * n)) into f[l * kPlanRegion + k].  MAP: v[k]
// takes the cell's byte of `map`, 0 outside the grid; with one layer the byte is that layer's own, with more bit l is
// layer l's.  Invalid cells and cells outside the grid never carry a distance: INF.  Ends with the barrier behind the stores.
template <int L, bool MAP>
__device__ __forceinline__ void plan_load_halo(const uint32_t *__restrict__ in, size_t n, const uint8_t *__restrict__ map, int W, int H,
                                               int x0, int y0, uint32_t *f, uint8_t *v) {
  for (int k = threadIdx.x; k < kPlanRegion; k += kPlanThreads) {
    const int gx = x0 + k % kPlanHalo, gy = y0 + k / kPlanHalo;
    const bool inside = gx >= 0 && gx < W && gy >= 0 && gy < H;
    const size_t g = inside ? static_cast<size_t>(gy) * static_cast<size_t>(W) + static_cast<size_t>(gx) : 0;
    uint32_t bits = inside ? 1u : 0u;
    if constexpr (MAP) {
      bits = inside ? map[g] : 0u;
      v[k] = static_cast<uint8_t>(bits);
    }
#pragma unroll
    for (int l = 0; l < L; ++l) {
      const bool on = L == 1 ? bits != 0u : (bits >> l & 1u) != 0u;
      f[l * kPlanRegion + k] = on ? in[static_cast<size_t>(l) * n + g] : kPlanInf;
    }
  }
  __syncthreads();
}

// one pass over one tile: `in` is only read, `out` only written (the tile's own cells).  PEN: a step pays the
// penalty of the cell it leaves (rule 7), which is the cell that is relaxed: one more register per owned cell, the
// same LDS traffic.
// `tile`: the tile's number, row by row; planner_relax_kernel takes it from blockIdx.x, planner_relax_list_kernel from
// a list (rule 20).
template <bool PEN>
__device__ __forceinline__ void plan_relax_tile(unsigned tile, const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                const uint8_t *__restrict__ valid, const uint32_t *__restrict__ pen, int W, int H,
                                                unsigned tiles_x, uint32_t *changed_word, uint32_t pass) {
  __shared__ uint32_t f[kPlanRegion];
  __shared__ uint8_t v[kPlanRegion];
  int x0, y0;
  plan_tile_origin(tile, tiles_x, &x0, &y0);
  plan_load_halo<1, true>(in, 0, valid, W, H, x0, y0, f, v);
  const int tx = threadIdx.x & (kPlanTile - 1), ty = threadIdx.x / kPlanTile;
  const int off[8] = {1, kPlanHalo, -1, -kPlanHalo, kPlanHalo + 1, kPlanHalo - 1, -kPlanHalo - 1, -kPlanHalo + 1};
  int idx[kPlanRows];
  uint32_t cur[kPlanRows], orig[kPlanRows], mask[kPlanRows];
  uint32_t leave[PEN ? kPlanRows : 1];
#pragma unroll
  for (int r = 0; r < kPlanRows; ++r) {
    const int k = (1 + ty + r * (kPlanThreads / kPlanTile)) * kPlanHalo + 1 + tx;
    idx[r] = k;
    if constexpr (PEN) {
      const int gx = x0 + 1 + tx, gy = y0 + 1 + ty + r * (kPlanThreads / kPlanTile);
      leave[r] = (gx < W && gy < H) ? pen[static_cast<size_t>(gy) * static_cast<size_t>(W) + static_cast<size_t>(gx)] : 0u;
    }
    cur[r] = orig[r] = f[k];
    uint32_t m = 0;
    if (v[k]) {
      const bool e = v[k + 1], n = v[k + kPlanHalo], w = v[k - 1], s = v[k - kPlanHalo];
      // a diagonal step needs both orthogonal neighbours it passes between
      m = (e ? 1u : 0u) | (n ? 2u : 0u) | (w ? 4u : 0u) | (s ? 8u : 0u) |
          ((e && n && v[k + kPlanHalo + 1]) ? 16u : 0u) | ((w && n && v[k + kPlanHalo - 1]) ? 32u : 0u) |
          ((w && s && v[k - kPlanHalo - 1]) ? 64u : 0u) | ((e && s && v[k - kPlanHalo + 1]) ? 128u : 0u);
    }
    mask[r] = m;
  }
  for (int it = 0; it < kPlanLocalIters; ++it) {
    int ch = 0;
#pragma unroll
    for (int r = 0; r < kPlanRows; ++r) {
      uint32_t best = cur[r];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (mask[r] & (1u << q)) {
          const uint32_t fn = f[idx[r] + off[q]];
          uint32_t c = fn + (q < 4 ? 10u : 14u);  // no wrap: 14 * cells < 2^32 (the cell cap)
          if constexpr (PEN) c += leave[r];       // nor here: (14 + max penalty) * cells < 2^32 (kc_planner_solve)
          if (fn != kPlanInf && c < best) best = c;
        }
      }
      if (best < cur[r]) {
        cur[r] = best;
        ch = 1;
      }
    }
    if (!__syncthreads_or(ch)) break;  // every lane has read this iteration's values
#pragma unroll
    for (int r = 0; r < kPlanRows; ++r) f[idx[r]] = cur[r];
    __syncthreads();
  }
  int changed = 0;
#pragma unroll
  for (int r = 0; r < kPlanRows; ++r) {
    const int gx = x0 + 1 + tx, gy = y0 + 1 + ty + r * (kPlanThreads / kPlanTile);
    if (gx < W && gy < H) out[static_cast<size_t>(gy) * static_cast<size_t>(W) + static_cast<size_t>(gx)] = cur[r];
    changed |= cur[r] != orig[r];
  }
  if (__syncthreads_or(changed) && threadIdx.x == 0) *changed_word = pass;
}

template <bool PEN>
__global__ __launch_bounds__(kPlanThreads) void planner_relax_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                                     const uint8_t *__restrict__ valid, const uint32_t *__restrict__ pen,
                                                                     int W, int H, unsigned tiles_x, uint32_t *changed_word,
                                                                     uint32_t pass) {
  plan_relax_tile<PEN>(blockIdx.x, in, out, valid, pen, W, H, tiles_x, changed_word, pass);
}

// rule 20: the same pass over the tiles of a list, one workgroup each; the tiles left out hold final values in both
// buffers, so the halo a listed tile reads from them is what a pass over every tile would have read
template <bool PEN>
__global__ __launch_bounds__(kPlanThreads) void planner_relax_list_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                                          const uint8_t *__restrict__ valid,
                                                                          const uint32_t *__restrict__ pen, int W, int H,
                                                                          unsigned tiles_x, const uint32_t *__restrict__ tiles,
                                                                          uint32_t *changed_word, uint32_t pass) {
  plan_relax_tile<PEN>(tiles[blockIdx.x], in, out, valid, pen, W, H, tiles_x, changed_word, pass);
}

// ---- the replan (rules 19 and 20) --------------------------------------------------------------------------------

// rule 19 in one pass over the cells: a cell whose validity differs, or (PEN) whose penalty differs while it is valid
// in both maps, is touched; its candidate is the smallest of its old value and its eight neighbours' old values + 10,
// validity and the corner rule ignored.  out[0] takes the smallest candidate (the host sets it to INF first), out[1]
// the number of touched cells: a wavefront reduction, then one atomic each per workgroup that saw a touched cell.
// No wrap: a finite value is at most (14 + max penalty) * (cells - 1), and (14 + max penalty) * cells fits (kc_planner_solve).
template <bool PEN>
__global__ __launch_bounds__(kPlanBlock) void planner_touched_kernel(const uint32_t *__restrict__ old, const uint8_t *__restrict__ valid_old,
                                                                     const uint8_t *__restrict__ valid_new,
                                                                     const uint32_t *__restrict__ pen_old,
                                                                     const uint32_t *__restrict__ pen_new, int W, int H, uint32_t *out) {
  __shared__ uint32_t wave_min[kPlanBlock / 64], wave_cnt[kPlanBlock / 64];
  const long long n = static_cast<long long>(W) * H;
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  uint32_t best = kPlanInf, cnt = 0;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
    const bool was = valid_old[i] != 0, is = valid_new[i] != 0;
    bool touched = was != is;
    if constexpr (PEN) touched = touched || (was && is && pen_old[i] != pen_new[i]);
    if (!touched) continue;
    ++cnt;
    const int x = static_cast<int>(i % W), y = static_cast<int>(i / W);
    best = min(best, old[i]);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int nx = x + kPlanDx[q], ny = y + kPlanDy[q];
      if (nx >= 0 && nx < W && ny >= 0 && ny < H) {
        const uint32_t u = old[static_cast<size_t>(ny) * static_cast<size_t>(W) + static_cast<size_t>(nx)];
        if (u != kPlanInf) best = min(best, u + 10u);
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    best = min(best, static_cast<uint32_t>(__shfl_xor(static_cast<int>(best), d, 64)));
    cnt += static_cast<uint32_t>(__shfl_xor(static_cast<int>(cnt), d, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    wave_min[threadIdx.x >> 6] = best;
    wave_cnt[threadIdx.x >> 6] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 1; k < kPlanBlock / 64; ++k) {
      best = min(best, wave_min[k]);
      cnt += wave_cnt[k];
    }
    if (cnt) {
      atomicMin(&out[0], best);
      atomicAdd(&out[1], cnt);
    }
  }
}

// rule 20's start state, into both field buffers as planner_init_kernel writes its own: the old value where the cell
// is valid in the new map and below T, INF elsewhere, 0 at a valid goal.  `old` is one of a and b: a lane reads its
// cell before it writes it, and no lane reads another's.  A valid cell that gets INF (the goal does not) may still
// change: it marks every tile whose 66 x 66 halo region holds it, i.e. its own and, from a tile's edge, the ones
// beside it (bytes, zero before the launch; every writer stores a 1).
__global__ __launch_bounds__(kPlanBlock) void planner_rollback_kernel(const uint32_t *old, uint32_t *a, uint32_t *b,
                                                                      const uint8_t *__restrict__ valid, int W, int H, long long goal,
                                                                      uint32_t T, int tiles_x, int tiles_y, uint8_t *active) {
  const long long n = static_cast<long long>(W) * H;
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
    const bool ok = valid[i] != 0;
    const uint32_t o = old[i];
    uint32_t v = (ok && o < T) ? o : kPlanInf;
    if (i == goal && ok) v = 0u;
    a[i] = v;
    b[i] = v;
    if (ok && v == kPlanInf) {
      const int x = static_cast<int>(i % W), y = static_cast<int>(i / W);
      const int tx = x / kPlanTile, ty = y / kPlanTile, lx = x % kPlanTile, ly = y % kPlanTile;
      const int tx0 = (lx == 0 && tx > 0) ? tx - 1 : tx, tx1 = (lx == kPlanTile - 1 && tx + 1 < tiles_x) ? tx + 1 : tx;
      const int ty0 = (ly == 0 && ty > 0) ? ty - 1 : ty, ty1 = (ly == kPlanTile - 1 && ty + 1 < tiles_y) ? ty + 1 : ty;
      for (int u = ty0; u <= ty1; ++u)
        for (int t = tx0; t <= tx1; ++t) active[static_cast<size_t>(u) * static_cast<size_t>(tiles_x) + static_cast<size_t>(t)] = 1;
    }
  }
}

// the marked tiles' numbers, in no particular order (a tile writes its own cells only, so the order decides nothing)
__global__ __launch_bounds__(kPlanBlock) void planner_compact_kernel(const uint8_t *__restrict__ active, unsigned ntiles,
                                                                     uint32_t *__restrict__ list, uint32_t *count) {
  const unsigned stride = gridDim.x * kPlanBlock;
  for (unsigned t = blockIdx.x * kPlanBlock + threadIdx.x; t < ntiles; t += stride)
    if (active[t]) list[atomicAdd(count, 1u)] = t;
}

// ---- exploration (rules 21 to 26) --------------------------------------------------------------------------------

// rule 21's second half: an unknown cell is not explore-valid (the row and column passes ran with unknown not blocking)
__global__ __launch_bounds__(kPlanBlock) void planner_known_kernel(const uint8_t *__restrict__ cls, uint8_t *valid, long long n) {
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride)
    if (cls[i] == 1) valid[i] = 0;
}

// rule 23, one lane a cell: the frontier byte, the start of both label planes (the cell's own flat index, INF for the
// rest) and a 1 into the byte of the tile that holds a frontier cell (bytes, zero before the launch).  A tile without
// one holds INF in both planes and never changes, so only a cell's own tile is marked.
__global__ __launch_bounds__(kPlanBlock) void planner_frontier_mark_kernel(const uint8_t *__restrict__ cls, const uint8_t *__restrict__ valid,
                                                                           const uint32_t *__restrict__ field, uint32_t min_cost, int W,
                                                                           int H, int tiles_x, uint8_t *__restrict__ front,
                                                                           uint32_t *__restrict__ la, uint32_t *__restrict__ lb,
                                                                           uint8_t *tile_on) {
  const long long n = static_cast<long long>(W) * H;
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
    const uint32_t f = field[i];
    bool fr = valid[i] != 0 && f != kPlanInf && f >= min_cost;
    const int x = static_cast<int>(i % W), y = static_cast<int>(i / W);
    if (fr)  // the four neighbours inside the grid, in the walk's order
      fr = (x + 1 < W && cls[i + 1] == 1) || (y + 1 < H && cls[i + W] == 1) || (x > 0 && cls[i - 1] == 1) || (y > 0 && cls[i - W] == 1);
    front[i] = fr ? 1 : 0;
    const uint32_t l = fr ? static_cast<uint32_t>(i) : kPlanInf;  // the cell cap keeps a flat index below INF
    la[i] = l;
    lb[i] = l;
    if (fr) tile_on[static_cast<size_t>(y / kPlanTile) * static_cast<size_t>(tiles_x) + static_cast<size_t>(x / kPlanTile)] = 1;
  }
}

// rule 24, one tile pass over one listed tile.  A frontier cell takes the smallest label among itself and its eight
// neighbours; the cells that are no frontier cells hold INF in both label planes from the mark kernel on, as the ring
// outside the grid does in LDS, and so never win: no byte plane is read.
__global__ __launch_bounds__(kPlanThreads) void planner_label_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, int W, int H,
                                                                     unsigned tiles_x, const uint32_t *__restrict__ tiles, uint32_t *changed_word, uint32_t pass) {
  __shared__ uint32_t f[kPlanRegion];
  int x0, y0;
  plan_tile_origin(tiles[blockIdx.x], tiles_x, &x0, &y0);
  plan_load_halo<1, false>(in, 0, nullptr, W, H, x0, y0, f, nullptr);
  const int tx = threadIdx.x & (kPlanTile - 1), ty = threadIdx.x / kPlanTile;
  const int off[8] = {1, kPlanHalo, -1, -kPlanHalo, kPlanHalo + 1, kPlanHalo - 1, -kPlanHalo - 1, -kPlanHalo + 1};
  int idx[kPlanRows];
  uint32_t cur[kPlanRows], orig[kPlanRows];
#pragma unroll
  for (int r = 0; r < kPlanRows; ++r) {
    idx[r] = (1 + ty + r * (kPlanThreads / kPlanTile)) * kPlanHalo + 1 + tx;
    cur[r] = orig[r] = f[idx[r]];
  }
  for (int it = 0; it < kPlanLocalIters; ++it) {
    int ch = 0;
#pragma unroll
    for (int r = 0; r < kPlanRows; ++r) {
      if (cur[r] == kPlanInf) continue;  // no frontier cell
      uint32_t best = cur[r];
#pragma unroll
      for (int q = 0; q < 8; ++q) best = min(best, f[idx[r] + off[q]]);
      if (best < cur[r]) {
        cur[r] = best;
        ch = 1;
      }
    }
    if (!__syncthreads_or(ch)) break;  // every lane has read this iteration's values
#pragma unroll
    for (int r = 0; r < kPlanRows; ++r) f[idx[r]] = cur[r];
    __syncthreads();
  }
  int changed = 0;
#pragma unroll
  for (int r = 0; r < kPlanRows; ++r) {
    const int gx = x0 + 1 + tx, gy = y0 + 1 + ty + r * (kPlanThreads / kPlanTile);
    if (gx < W && gy < H) out[static_cast<size_t>(gy) * static_cast<size_t>(W) + static_cast<size_t>(gx)] = cur[r];
    changed |= cur[r] != orig[r];
  }
  if (__syncthreads_or(changed) && threadIdx.x == 0) *changed_word = pass;
}

// rule 24's cell counts: `size` is a plane of zeros; a frontier cell adds one at its root (the label is a flat index)
__global__ __launch_bounds__(kPlanBlock) void planner_frontier_size_kernel(const uint32_t *__restrict__ label, uint32_t *size, long long n) {
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
    const uint32_t l = label[i];
    if (l != kPlanInf) atomicAdd(&size[l], 1u);
  }
}

// a root is the cell that holds its own index.  out[0] += roots, out[1] += roots of at least min_size cells: a
// wavefront reduction, then one atomic each per wavefront that saw a root.
__global__ __launch_bounds__(kPlanBlock) void planner_frontier_count_kernel(const uint32_t *__restrict__ label, const uint32_t *__restrict__ size,
                                                                            long long n, uint32_t min_size, uint32_t *out) {
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  uint32_t roots = 0, kept = 0;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride)
    if (label[i] == static_cast<uint32_t>(i)) {
      ++roots;
      kept += size[i] >= min_size ? 1u : 0u;
    }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    roots += static_cast<uint32_t>(__shfl_xor(static_cast<int>(roots), d, 64));
    kept += static_cast<uint32_t>(__shfl_xor(static_cast<int>(kept), d, 64));
  }
  if ((threadIdx.x & 63) == 0 && roots) {
    atomicAdd(&out[0], roots);
    atomicAdd(&out[1], kept);
  }
}

// rule 25's record as the device fills it; key = field << 32 | flat index of the entry cell
struct PlanFrontierRec {
  unsigned long long sum_i, sum_j, key;
  uint32_t root, size;
};

// a kept root takes the next slot (any order: the host sorts) and starts its record; afterwards size[root] is the
// slot of a kept root and INF for a dropped one.  rec holds as many records as planner_frontier_count_kernel counted.
__global__ __launch_bounds__(kPlanBlock) void planner_frontier_slot_kernel(const uint32_t *__restrict__ label, uint32_t *size, long long n,
                                                                           uint32_t min_size, PlanFrontierRec *rec, uint32_t *counter) {
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
    if (label[i] != static_cast<uint32_t>(i)) continue;
    const uint32_t cells = size[i];
    uint32_t slot = kPlanInf;
    if (cells >= min_size) {
      slot = atomicAdd(counter, 1u);
      rec[slot] = PlanFrontierRec{0ull, 0ull, ~0ull, static_cast<uint32_t>(i), cells};
    }
    size[i] = slot;
  }
}

// rule 25: the cells of kept frontiers add their indices to their record and offer their (field, flat index)
__global__ __launch_bounds__(kPlanBlock) void planner_frontier_record_kernel(const uint32_t *__restrict__ label, const uint32_t *__restrict__ slot,
                                                                             const uint32_t *__restrict__ field, int W, long long n,
                                                                             PlanFrontierRec *rec) {
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
    const uint32_t l = label[i];
    if (l == kPlanInf) continue;
    const uint32_t s = slot[l];
    if (s == kPlanInf) continue;
    atomicAdd(&rec[s].sum_i, static_cast<unsigned long long>(i % W));
    atomicAdd(&rec[s].sum_j, static_cast<unsigned long long>(i / W));
    atomicMin(&rec[s].key, (static_cast<unsigned long long>(field[i]) << 32) | static_cast<unsigned long long>(i));
  }
}

// what the three walks share: the smallest key among the lanes 0 .. 2^K - 1, in every lane
template <int K>
__device__ __forceinline__ unsigned long long plan_min_key(unsigned long long key) {
#pragma unroll
  for (int d = 1 << (K - 1); d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(key, d, 64);
    key = o < key ? o : key;
  }
  return __shfl(key, 0, 64);
}

// status words of the walk: out[0] = cells written, out[1] = 0 done / 1 capacity / 2 no descending neighbour.
// PEN (rule 8): the key is field + step, its minimum must be field - penalty of the cell left, and out[2] = the
// smallest clear2 among the cells visited.  STEP without PEN (rule 26): rule 8's key and test with no penalty plane,
// the walk that realises the field; <false> and <true> are <false, false> and <true, true>.
template <bool PEN, bool STEP = PEN>
__global__ __launch_bounds__(64) void planner_walk_kernel(const uint32_t *field, const uint8_t *valid, const uint32_t *pen,
                                                          const uint16_t *clear2, int W, int H, int sx, int sy, int32_t *cells,
                                                          uint32_t cap, uint32_t *out) {
  const int lane = threadIdx.x;
  int cx = sx, cy = sy;
  uint32_t n = 0, status = 0, min_clear = KC_PLANNER_CLEAR_FAR;
  for (;;) {
    const size_t c = static_cast<size_t>(cy) * static_cast<size_t>(W) + static_cast<size_t>(cx);
    if (n >= cap) {
      status = 1;
      break;
    }
    if (lane == 0) cells[n] = static_cast<int32_t>(c);
    ++n;
    const uint32_t fc = field[c];
    if constexpr (PEN) min_clear = min(min_clear, static_cast<uint32_t>(clear2[c]));
    if (fc == 0u) break;
    unsigned long long key = ~0ull;
    if (lane < 8) {
      const int dx = kPlanDx[lane], dy = kPlanDy[lane];
      const int nx = cx + dx, ny = cy + dy;
      if (nx >= 0 && nx < W && ny >= 0 && ny < H) {
        const size_t g = static_cast<size_t>(ny) * static_cast<size_t>(W) + static_cast<size_t>(nx);
        bool ok = valid[g] != 0;
        if (ok && lane >= 4)
          ok = valid[static_cast<size_t>(cy) * static_cast<size_t>(W) + static_cast<size_t>(nx)] != 0 &&
               valid[static_cast<size_t>(ny) * static_cast<size_t>(W) + static_cast<size_t>(cx)] != 0;
        // 64 bits hold an unreached neighbour's 0xFFFFFFFF + 14 as well
        const unsigned long long step = STEP ? (lane < 4 ? 10ull : 14ull) : 0ull;
        if (ok) key = ((static_cast<unsigned long long>(field[g]) + step) << 3) | static_cast<unsigned long long>(lane);
      }
    }
    key = plan_min_key<3>(key);
    bool off_field;  // not on a converged field with a reachable start
    if constexpr (PEN)
      off_field = key == ~0ull || (key >> 3) + static_cast<unsigned long long>(pen[c]) != static_cast<unsigned long long>(fc);
    else if constexpr (STEP)
      off_field = key == ~0ull || (key >> 3) != static_cast<unsigned long long>(fc);
    else
      off_field = key == ~0ull || static_cast<uint32_t>(key >> 3) >= fc;
    if (off_field) {
      status = 2;
      break;
    }
    const int q = static_cast<int>(key & 7ull);
    cx += kPlanDx[q];
    cy += kPlanDy[q];
  }
  if (lane == 0) {
    out[0] = n;
    out[1] = status;
    if constexpr (PEN) out[2] = min_clear;
  }
}

// status words of the shortcut: out[0] = kept indices written, out[1] = 0 done, out[2] = the smallest clear2 over the
// kept cells and the touched cells of the kept segments that were tested (CLEAR_FAR without CLR).
// Rule 11 over the walk path[0 .. n-1] (linear cells): from the anchor s the largest t <= min(n - 1, s + span) whose
// segment is clear (rules 9 and 10), s + 1 untested.  CLR: a touched cell must also hold clear2 >= m.
// Every touched cell lies in the bounding box of two cells of the walk, so no load leaves the grid.
template <bool CLR>
__global__ __launch_bounds__(kShortThreads) void planner_shortcut_kernel(const int32_t *__restrict__ path, uint32_t n, int span,
                                                                         const uint8_t *__restrict__ valid,
                                                                         const uint16_t *__restrict__ clear2, uint32_t m, int W,
                                                                         int32_t *__restrict__ keep, uint32_t *out) {
  __shared__ int32_t px[KC_PLANNER_MAX_SPAN + 1], py[KC_PLANNER_MAX_SPAN + 1];
  __shared__ uint32_t best;  // of a round: (index - s) << 16 | 0xFFFF - smallest touched clear2, 0 for none clear
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t s = 0, kept = 1, min_touched = KC_PLANNER_CLEAR_FAR;  // kept and min_touched are lane 0's
  if (tid == 0) {
    keep[0] = 0;
    if constexpr (CLR) min_touched = clear2[path[0]];
  }
  while (s + 1 < n) {
    const int hi = static_cast<int>(min(static_cast<uint32_t>(span), n - 1 - s));
    __syncthreads();  // the last anchor's window and its `best` have been read by everyone
    for (int k = tid; k <= hi; k += kShortThreads) {
      const int32_t c = path[s + k];
      px[k] = c % W;
      py[k] = c / W;
    }
    if (tid == 0) best = 0;
    __syncthreads();
    const int ax = px[0], ay = py[0];
    uint32_t found = 0;
    for (int top = hi; top >= 2 && !found; top -= kShortWaves) {
      const int rel = top - wave;  // this wavefront's candidate
      if (rel >= 2) {
        const int dx = px[rel] - ax, dy = py[rel] - ay;
        const int adx = abs(dx), ady = abs(dy);
        const bool xmaj = adx >= ady;
        const int M = xmaj ? adx : ady, mn = xmaj ? ady : adx;  // |dx|, |dy| <= rel <= 1024: the products fit
        const int sM = xmaj ? (dx > 0) - (dx < 0) : (dy > 0) - (dy < 0);
        const int sm = xmaj ? (dy > 0) - (dy < 0) : (dx > 0) - (dx < 0);
        const int den = 2 * max(M, 1);
        bool blocked = false;
        uint32_t wmin = KC_PLANNER_CLEAR_FAR;
        for (int k0 = 0; k0 <= M; k0 += 64) {
          const int k = k0 + lane;  // a column of the major axis
          if (k <= M) {
            const int q = mn * k;
            const int v1 = (2 * q + M) / den;  // the minor offset nearest to the segment: the touched ones are v1 - 1 .. v1 + 1
#pragma unroll
            for (int d = -1; d <= 1; ++d) {
              const int v = v1 + d;
              // rule 9: inside the bounding box and 2 |dx (j - ay) - dy (i - ax)| <= |dx| + |dy|
              if (v >= 0 && v <= mn && 2 * abs(M * v - q) <= M + mn) {
                const int cx = xmaj ? ax + sM * k : ax + sm * v, cy = xmaj ? ay + sm * v : ay + sM * k;
                const size_t g = static_cast<size_t>(cy) * static_cast<size_t>(W) + static_cast<size_t>(cx);
                blocked |= valid[g] == 0;
                if constexpr (CLR) {
                  const uint32_t c2 = clear2[g];
                  blocked |= c2 < m;
                  wmin = min(wmin, c2);
                }
              }
            }
          }
          if (__any(blocked)) break;
        }
        if (!__any(blocked)) {
          if constexpr (CLR) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) wmin = min(wmin, static_cast<uint32_t>(__shfl_xor(static_cast<int>(wmin), d, 64)));
          }
          if (lane == 0) atomicMax(&best, (static_cast<uint32_t>(rel) << 16) | (0xFFFFu - wmin));
        }
      }
      __syncthreads();
      found = best;
      __syncthreads();  // nobody raises `best` in the next round before everyone has read this one's
    }
    s += found ? found >> 16 : 1u;
    if (tid == 0) {
      keep[kept++] = static_cast<int32_t>(s);
      if constexpr (CLR) {
        if (found) min_touched = min(min_touched, 0xFFFFu - (found & 0xFFFFu));
        min_touched = min(min_touched, static_cast<uint32_t>(clear2[path[s]]));
      }
    }
  }
  if (tid == 0) {
    out[0] = kept;
    out[1] = 0;
    out[2] = min_touched;
  }
}

// ---- the oriented box footprint (rules 13 to 18) -----------------------------------------------------------------

// the length axis of class k: E, NE, N, NW, the first of the class's two directions in the walk's order
__constant__ const int kPlanClassDx[4] = {1, 1, 0, -1};
__constant__ const int kPlanClassDy[4] = {0, 1, 1, 1};
constexpr uint8_t kPlanTurnBit = 16;  // beside the four class bits of a cell's byte

struct PlanMaskEnds {
  uint32_t at[5];  // class k's offsets are offs[at[k] .. at[k + 1])
};

// rule 14: offs holds (di, dj) pairs, class after class, each class by rising di^2 + dj^2 so that a cell near a
// blocking one leaves early.  turn: rule 15's disc; it contains every mask, so its cells are valid in all four.
__global__ __launch_bounds__(kPlanBlock) void planner_oriented_valid_kernel(const uint8_t *__restrict__ cls,
                                                                            const uint8_t *__restrict__ turn,
                                                                            const int16_t *__restrict__ offs, PlanMaskEnds ends,
                                                                            uint8_t *__restrict__ valid4, int W, int H,
                                                                            int block_unknown) {
  const long long n = static_cast<long long>(W) * H;
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
    if (turn[i]) {
      valid4[i] = static_cast<uint8_t>(15 | kPlanTurnBit);
      continue;
    }
    const int x = static_cast<int>(i % W), y = static_cast<int>(i / W);
    uint32_t bits = 0;
    for (int k = 0; k < 4; ++k) {
      bool ok = true;
      for (uint32_t o = ends.at[k]; o < ends.at[k + 1]; ++o) {
        const int nx = x + offs[2 * o], ny = y + offs[2 * o + 1];
        // cells outside the grid do not block
        if (nx >= 0 && nx < W && ny >= 0 && ny < H &&
            plan_blocks(cls[static_cast<size_t>(ny) * static_cast<size_t>(W) + static_cast<size_t>(nx)], block_unknown)) {
          ok = false;
          break;
        }
      }
      bits |= ok ? 1u << k : 0u;
    }
    valid4[i] = static_cast<uint8_t>(bits);
  }
}

// layer k of a field buffer is its cells [k * n, (k + 1) * n)
__global__ __launch_bounds__(kPlanBlock) void planner_init4_kernel(uint32_t *a, uint32_t *b, const uint8_t *valid4, long long n,
                                                                   long long goal) {
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
    const uint32_t bits = i == goal ? valid4[i] : 0u;  // every valid class at the goal cell is a goal state
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t v = (bits >> k & 1u) ? 0u : kPlanInf;
      a[static_cast<size_t>(k) * static_cast<size_t>(n) + static_cast<size_t>(i)] = v;
      b[static_cast<size_t>(k) * static_cast<size_t>(n) + static_cast<size_t>(i)] = v;
    }
  }
}

// rule 16, one tile pass over four layers.  A lane owns four cells and their sixteen states.  The moves read the neighbours'
// values of the last iteration from LDS; the turns couple the four values of one cell, which one lane holds in registers.
__global__ __launch_bounds__(kPlanThreads) void planner_relax4_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                                      const uint8_t *__restrict__ valid4, int W, int H, size_t n,
                                                                      unsigned tiles_x, uint32_t turn10, uint32_t *changed_word,
                                                                      uint32_t pass) {
  __shared__ uint32_t f[4][kPlanRegion];
  __shared__ uint8_t v[kPlanRegion];
  int x0, y0;
  plan_tile_origin(blockIdx.x, tiles_x, &x0, &y0);
  plan_load_halo<4, true>(in, n, valid4, W, H, x0, y0, f[0], v);
  const int tx = threadIdx.x & (kPlanTile - 1), ty = threadIdx.x / kPlanTile;
  const int off[4] = {1, kPlanHalo + 1, kPlanHalo, kPlanHalo - 1};
  int idx[kPlanRows];
  uint32_t cur[kPlanRows][4], mask[kPlanRows];
#pragma unroll
  for (int r = 0; r < kPlanRows; ++r) {
    const int k = (1 + ty + r * (kPlanThreads / kPlanTile)) * kPlanHalo + 1 + tx;
    idx[r] = k;
    const uint32_t here = v[k];
    uint32_t m = (here & kPlanTurnBit) ? 256u : 0u;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      cur[r][l] = f[l][k];
      // a move needs both states valid; no corner rule: the swept lattice points lie in the footprint of one end
      if (here >> l & 1u) m |= ((v[k + off[l]] >> l & 1u) ? 1u << (2 * l) : 0u) | ((v[k - off[l]] >> l & 1u) ? 2u << (2 * l) : 0u);
    }
    mask[r] = m;
  }
  int changed = 0;
  for (int it = 0; it < kPlanLocalIters; ++it) {
    int ch = 0;
#pragma unroll
    for (int r = 0; r < kPlanRows; ++r) {
      uint32_t b[4];
#pragma unroll
      for (int l = 0; l < 4; ++l) {
        uint32_t best = cur[r][l];
        const uint32_t step = (l & 1) ? 14u : 10u;  // no wrap: max(14, turn10) * 4 * cells < 2^32 (kc_planner_solve_oriented)
        if (mask[r] & (1u << (2 * l))) {
          const uint32_t fn = f[l][idx[r] + off[l]];
          if (fn != kPlanInf && fn + step < best) best = fn + step;
        }
        if (mask[r] & (2u << (2 * l))) {
          const uint32_t fn = f[l][idx[r] - off[l]];
          if (fn != kPlanInf && fn + step < best) best = fn + step;
        }
        b[l] = best;
      }
      if (mask[r] & 256u) {
        uint32_t t[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) t[l] = min(b[(l + 1) & 3], b[(l + 3) & 3]);
#pragma unroll
        for (int l = 0; l < 4; ++l)
          if (t[l] != kPlanInf && t[l] + turn10 < b[l]) b[l] = t[l] + turn10;
      }
#pragma unroll
      for (int l = 0; l < 4; ++l)
        if (b[l] < cur[r][l]) {
          cur[r][l] = b[l];
          ch = 1;
        }
    }
    if (!__syncthreads_or(ch)) break;  // every lane has read this iteration's values
    changed |= ch;
#pragma unroll
    for (int r = 0; r < kPlanRows; ++r)
#pragma unroll
      for (int l = 0; l < 4; ++l) f[l][idx[r]] = cur[r][l];
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < kPlanRows; ++r) {
    const int gx = x0 + 1 + tx, gy = y0 + 1 + ty + r * (kPlanThreads / kPlanTile);
    if (gx < W && gy < H) {
      const size_t g = static_cast<size_t>(gy) * static_cast<size_t>(W) + static_cast<size_t>(gx);
#pragma unroll
      for (int l = 0; l < 4; ++l) out[static_cast<size_t>(l) * n + g] = cur[r][l];
    }
  }
  if (__syncthreads_or(changed) && threadIdx.x == 0) *changed_word = pass;
}

// rule 17: one wavefront, four lanes: the class's first direction, its opposite, the turn to k + 1, the turn to k - 1.
// states[] = 4 * cell + class; out[0] = states written, out[1] = 0 done / 1 capacity / 2 the minimum is not the field.
__global__ __launch_bounds__(64) void planner_walk4_kernel(const uint32_t *field, const uint8_t *valid4, int W, int H, size_t n,
                                                           int sx, int sy, int sk, uint32_t turn10, int32_t *states, uint32_t cap,
                                                           uint32_t *out) {
  const int lane = threadIdx.x;
  int cx = sx, cy = sy, ck = sk;
  uint32_t count = 0, status = 0;
  for (;;) {
    const size_t c = static_cast<size_t>(cy) * static_cast<size_t>(W) + static_cast<size_t>(cx);
    if (count >= cap) {
      status = 1;
      break;
    }
    if (lane == 0) states[count] = static_cast<int32_t>(4 * c + static_cast<size_t>(ck));
    ++count;
    const uint32_t fc = field[static_cast<size_t>(ck) * n + c];
    if (fc == 0u) break;
    unsigned long long key = ~0ull;
    if (lane < 2) {
      const int sgn = lane == 0 ? 1 : -1;
      const int nx = cx + sgn * kPlanClassDx[ck], ny = cy + sgn * kPlanClassDy[ck];
      if (nx >= 0 && nx < W && ny >= 0 && ny < H) {
        const size_t g = static_cast<size_t>(ny) * static_cast<size_t>(W) + static_cast<size_t>(nx);
        // 64 bits hold an unreached state's 0xFFFFFFFF + cost as well; it never equals field[current]
        if (valid4[g] >> ck & 1)
          key = ((static_cast<unsigned long long>(field[static_cast<size_t>(ck) * n + g]) + ((ck & 1) ? 14ull : 10ull)) << 2) |
                static_cast<unsigned long long>(lane);
      }
    } else if (lane < 4) {
      if (valid4[c] & kPlanTurnBit) {
        const int nk = lane == 2 ? (ck + 1) & 3 : (ck + 3) & 3;
        key = ((static_cast<unsigned long long>(field[static_cast<size_t>(nk) * n + c]) + turn10) << 2) | static_cast<unsigned long long>(lane);
      }
    }
    key = plan_min_key<2>(key);
    if (key == ~0ull || (key >> 2) != static_cast<unsigned long long>(fc)) {  // not on a converged field with a reachable start
      status = 2;
      break;
    }
    const int q = static_cast<int>(key & 3ull);
    if (q < 2) {
      const int sgn = q == 0 ? 1 : -1;
      cx += sgn * kPlanClassDx[ck];
      cy += sgn * kPlanClassDy[ck];
    } else {
      ck = q == 2 ? (ck + 1) & 3 : (ck + 3) & 3;
    }
  }
  if (lane == 0) {
    out[0] = count;
    out[1] = status;
  }
}

// ---- car motion (rules 27 to 36) ---------------------------------------------------------------------------------

// heading h = 0 .. 7 is the direction the robot's front points: E, NE, N, NW, W, SW, S, SE
__constant__ const int kCarDx[8] = {1, 1, 0, -1, -1, -1, 0, 1};
__constant__ const int kCarDy[8] = {0, 1, 1, 1, 0, -1, -1, -1};
constexpr int kCarS = 0, kCarL = 1, kCarR = 2, kCarB = 3, kCarBL = 4, kCarBR = 5;  // rule 30's order

// rule 28: `vmap` is the disc's validity byte (every heading) or, BOX, the four class bits of rule 14 (heading h & 3)
template <bool BOX>
__device__ __forceinline__ bool car_valid(const uint8_t *__restrict__ vmap, size_t g, int h) {
  if constexpr (BOX) return (vmap[g] >> (h & 3) & 1u) != 0;
  return vmap[g] != 0;
}

// rule 29, one lane a cell: bit h of steps[c] says that the unit step from (c, h) along +D[h] is allowed.  The step
// from (c, h) along -D[h] is the same pair of cells (and, for the disc, the same two corner cells) as the forward step
// out of c - D[h], so one plane serves both signs.  A cell outside the grid is never stepped on.
template <bool BOX>
__global__ __launch_bounds__(kPlanBlock) void planner_car_steps_kernel(const uint8_t *__restrict__ vmap, uint8_t *__restrict__ steps, int W,
                                                                       int H) {
  const long long n = static_cast<long long>(W) * H;
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
    const int x = static_cast<int>(i % W), y = static_cast<int>(i / W);
    uint32_t bits = 0;
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      const int nx = x + kCarDx[h], ny = y + kCarDy[h];
      if (nx < 0 || nx >= W || ny < 0 || ny >= H) continue;
      bool ok = car_valid<BOX>(vmap, static_cast<size_t>(i), h) &&
                car_valid<BOX>(vmap, static_cast<size_t>(ny) * static_cast<size_t>(W) + static_cast<size_t>(nx), h);
      if constexpr (!BOX) {  // rule 3's corner rule; both cells lie in the bounding box of two cells inside the grid
        if (ok && (h & 1))
          ok = vmap[static_cast<size_t>(y) * static_cast<size_t>(W) + static_cast<size_t>(nx)] != 0 &&
               vmap[static_cast<size_t>(ny) * static_cast<size_t>(W) + static_cast<size_t>(x)] != 0;
      }
      bits |= ok ? 1u << h : 0u;
    }
    steps[i] = static_cast<uint8_t>(bits);
  }
}

// `count` unit steps of sign sgn in heading h from (x, y), which is inside the grid: all allowed?  Moves (x, y) to the
// end of the leg when they are.  A forward step out of a cell inside the grid whose bit is set ends inside the grid; a
// backward step's bit is read at the cell it ends on, after the bounds test.
__device__ __forceinline__ bool car_leg(const uint8_t *__restrict__ steps, int W, int H, int &x, int &y, int h, int sgn, int count) {
  const int dx = sgn * kCarDx[h], dy = sgn * kCarDy[h];
  for (int k = 0; k < count; ++k) {
    const int nx = x + dx, ny = y + dy;
    if (nx < 0 || nx >= W || ny < 0 || ny >= H) return false;
    const int bx = sgn > 0 ? x : nx, by = sgn > 0 ? y : ny;
    if (!(steps[static_cast<size_t>(by) * static_cast<size_t>(W) + static_cast<size_t>(bx)] >> h & 1u)) return false;
    x = nx;
    y = ny;
  }
  return true;
}

// rule 30, one lane a state: bits 0 .. 5 of moves[h * n + c] say which of S, L, R, B, BL, BR are allowed out of (c, h).
// An arc is its polyline walked step by step over the steps plane, first leg in heading h, second in the new heading
// from the corner cell; the walk ends at the first step that is refused.  The 2 n tests of an arc happen here only.
__global__ __launch_bounds__(kPlanBlock) void planner_car_moves_kernel(const uint8_t *__restrict__ steps, uint8_t *__restrict__ moves, int W,
                                                                       int H, int turn, int reverse) {
  const long long n = static_cast<long long>(W) * H;
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long s = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; s < 8 * n; s += stride) {
    const int h = static_cast<int>(s / n);
    const long long i = s - static_cast<long long>(h) * n;
    const int x = static_cast<int>(i % W), y = static_cast<int>(i / W);
    uint32_t bits = 0;
    int px = x, py = y;
    if (car_leg(steps, W, H, px, py, h, 1, 1)) bits |= 1u << kCarS;
    px = x, py = y;
    if (car_leg(steps, W, H, px, py, h, 1, turn)) {
      int qx = px, qy = py;
      if (car_leg(steps, W, H, qx, qy, (h + 1) & 7, 1, turn)) bits |= 1u << kCarL;
      if (car_leg(steps, W, H, px, py, (h + 7) & 7, 1, turn)) bits |= 1u << kCarR;
    }
    if (reverse) {
      px = x, py = y;
      if (car_leg(steps, W, H, px, py, h, -1, 1)) bits |= 1u << kCarB;
      px = x, py = y;
      if (car_leg(steps, W, H, px, py, h, -1, turn)) {
        int qx = px, qy = py;
        if (car_leg(steps, W, H, qx, qy, (h + 7) & 7, -1, turn)) bits |= 1u << kCarBL;
        if (car_leg(steps, W, H, px, py, (h + 1) & 7, -1, turn)) bits |= 1u << kCarBR;
      }
    }
    moves[s] = static_cast<uint8_t>(bits);
  }
}

// where primitive p out of (x, y, h) ends, rule 30's table; turn = n
__device__ __forceinline__ void car_target(int x, int y, int h, int p, int turn, int *tx, int *ty, int *th) {
  const int sgn = p < kCarB ? 1 : -1;
  const bool arc = p != kCarS && p != kCarB;
  const int h2 = !arc ? h : ((p == kCarL || p == kCarBR) ? (h + 1) & 7 : (h + 7) & 7);
  const int len = arc ? turn : 1;
  *tx = x + sgn * len * (kCarDx[h] + (arc ? kCarDx[h2] : 0));
  *ty = y + sgn * len * (kCarDy[h] + (arc ? kCarDy[h2] : 0));
  *th = h2;
}

// rule 32's start state into both buffers: 0 at the goal cell's valid states of heading hg (every heading for hg < 0)
template <bool BOX>
__global__ __launch_bounds__(kPlanBlock) void planner_init8_kernel(uint32_t *a, uint32_t *b, const uint8_t *__restrict__ vmap, long long n,
                                                                   long long goal, int hg) {
  const long long stride = static_cast<long long>(gridDim.x) * kPlanBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kPlanBlock + threadIdx.x; i < n; i += stride) {
#pragma unroll
    for (int h = 0; h < 8; ++h) {
      const bool root = i == goal && (hg < 0 || h == hg) && car_valid<BOX>(vmap, static_cast<size_t>(i), h);
      const uint32_t v = root ? 0u : kPlanInf;
      a[static_cast<size_t>(h) * static_cast<size_t>(n) + static_cast<size_t>(i)] = v;
      b[static_cast<size_t>(h) * static_cast<size_t>(n) + static_cast<size_t>(i)] = v;
    }
  }
}

// rule 32, one tile pass over one (tile, heading): blockIdx.x = 8 * tile + h.  `in` is only read, `out` only written (the
// tile's own cells of layer h).  The layer's 66 x 66 halo region sits in LDS; the straight
// moves couple states of this layer alone, along the line +D[h] (S) and -D[h] (B), and are iterated there.  The arcs
// end in the layers h + 1 and h - 1, up to 2 n cells away: their candidates cost + in[target] are taken once from the
// read-only input, guarded by the moves byte, and are constants of the pass.  A value therefore crosses one arc a
// pass at the most; the fixed point is unique (every cost is positive), so the schedule does not decide it.
// No validity plane: an invalid state has no move and is no goal state, so it holds INF from the init on; the ring
// outside the grid is loaded as INF.
__global__ __launch_bounds__(kPlanThreads) void planner_relax8_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                                      const uint8_t *__restrict__ moves, int W, int H, size_t n,
                                                                      unsigned tiles_x, int turn, uint32_t rw, uint32_t *changed_word,
                                                                      uint32_t pass) {
  __shared__ uint32_t f[kPlanRegion];
  const int h = static_cast<int>(blockIdx.x & 7u);
  int x0, y0;
  plan_tile_origin(blockIdx.x >> 3, tiles_x, &x0, &y0);
  plan_load_halo<1, false>(in + static_cast<size_t>(h) * n, 0, nullptr, W, H, x0, y0, f, nullptr);
  const int tx = threadIdx.x & (kPlanTile - 1), ty = threadIdx.x / kPlanTile;
  const int off = kCarDy[h] * kPlanHalo + kCarDx[h];
  const uint32_t fwd = (h & 1) ? 14u : 10u, bwd = fwd * rw, arc_f = 24u * static_cast<uint32_t>(turn), arc_b = arc_f * rw;
  int idx[kPlanRows];
  uint32_t cur[kPlanRows], orig[kPlanRows], mask[kPlanRows];
#pragma unroll
  for (int r = 0; r < kPlanRows; ++r) {
    const int k = (1 + ty + r * (kPlanThreads / kPlanTile)) * kPlanHalo + 1 + tx;
    idx[r] = k;
    const int gx = x0 + 1 + tx, gy = y0 + 1 + ty + r * (kPlanThreads / kPlanTile);
    uint32_t m = 0, best = orig[r] = f[k];
    if (gx < W && gy < H) {
      m = moves[static_cast<size_t>(h) * n + static_cast<size_t>(gy) * static_cast<size_t>(W) + static_cast<size_t>(gx)];
#pragma unroll
      for (int p = kCarL; p <= kCarBR; ++p) {
        if (p == kCarB || !(m >> p & 1u)) continue;
        int ax, ay, ah;
        car_target(gx, gy, h, p, turn, &ax, &ay, &ah);  // inside the grid: the moves bit says that every step of the arc is
        const uint32_t fn = in[static_cast<size_t>(ah) * n + static_cast<size_t>(ay) * static_cast<size_t>(W) + static_cast<size_t>(ax)];
        const uint32_t c = fn + (p < kCarB ? arc_f : arc_b);  // no wrap: 24 n max(rw, 1) * 8 * cells < 2^32 (kc_planner_solve_car)
        if (fn != kPlanInf && c < best) best = c;
      }
    }
    cur[r] = best;
    mask[r] = m;
  }
  // an arc may have lowered an owned state below what LDS holds
#pragma unroll
  for (int r = 0; r < kPlanRows; ++r) f[idx[r]] = cur[r];
  __syncthreads();
  for (int it = 0; it < kPlanLocalIters; ++it) {
    int ch = 0;
#pragma unroll
    for (int r = 0; r < kPlanRows; ++r) {
      uint32_t best = cur[r];
      if (mask[r] & (1u << kCarS)) {
        const uint32_t fn = f[idx[r] + off];
        if (fn != kPlanInf && fn + fwd < best) best = fn + fwd;
      }
      if (mask[r] & (1u << kCarB)) {
        const uint32_t fn = f[idx[r] - off];
        if (fn != kPlanInf && fn + bwd < best) best = fn + bwd;
      }
      if (best < cur[r]) {
        cur[r] = best;
        ch = 1;
      }
    }
    if (!__syncthreads_or(ch)) break;  // every lane has read this iteration's values
#pragma unroll
    for (int r = 0; r < kPlanRows; ++r) f[idx[r]] = cur[r];
    __syncthreads();
  }
  int changed = 0;
#pragma unroll
  for (int r = 0; r < kPlanRows; ++r) {
    const int gx = x0 + 1 + tx, gy = y0 + 1 + ty + r * (kPlanThreads / kPlanTile);
    if (gx < W && gy < H) out[static_cast<size_t>(h) * n + static_cast<size_t>(gy) * static_cast<size_t>(W) + static_cast<size_t>(gx)] = cur[r];
    changed |= cur[r] != orig[r];
  }
  if (__syncthreads_or(changed) && threadIdx.x == 0) *changed_word = pass;
}

// rule 33: one wavefront, six lanes, a primitive each in rule 30's order.  states[k] = 8 * cell + heading of state k, and
// above that (from bit kCarMoveShift) the primitive taken out of it; the solve's range test keeps 8 * cells below that bit.
// out[0] = states written, out[1] = 0 done / 1 capacity / 2 the minimum is not the field.
constexpr int kCarMoveShift = 28;
__global__ __launch_bounds__(64) void planner_walk8_kernel(const uint32_t *field, const uint8_t *moves, int W, int H, size_t n, int sx, int sy,
                                                           int sh, int turn, uint32_t rw, int32_t *states, uint32_t cap, uint32_t *out) {
  const int lane = threadIdx.x;
  int cx = sx, cy = sy, chd = sh;
  uint32_t count = 0, status = 0;
  for (;;) {
    const size_t c = static_cast<size_t>(cy) * static_cast<size_t>(W) + static_cast<size_t>(cx);
    if (count >= cap) {
      status = 1;
      break;
    }
    const uint32_t fc = field[static_cast<size_t>(chd) * n + c];
    unsigned long long key = ~0ull;
    if (fc != 0u && lane < 6 && (moves[static_cast<size_t>(chd) * n + c] >> lane & 1u)) {
      int ax, ay, ah;
      car_target(cx, cy, chd, lane, turn, &ax, &ay, &ah);
      const uint32_t base = (lane == kCarS || lane == kCarB) ? ((chd & 1) ? 14u : 10u) : 24u * static_cast<uint32_t>(turn);
      const unsigned long long cost = static_cast<unsigned long long>(base) * (lane < kCarB ? 1ull : static_cast<unsigned long long>(rw));
      // 64 bits hold an unreached state's 0xFFFFFFFF + cost as well; it never equals field[current]
      key = ((static_cast<unsigned long long>(field[static_cast<size_t>(ah) * n + static_cast<size_t>(ay) * static_cast<size_t>(W) +
                                                    static_cast<size_t>(ax)]) + cost) << 3) | static_cast<unsigned long long>(lane);
    }
    key = plan_min_key<3>(key);
    const int q = static_cast<int>(key & 7ull);
    const bool last = fc == 0u;
    const bool off_field = !last && (key == ~0ull || (key >> 3) != static_cast<unsigned long long>(fc));
    if (lane == 0)
      states[count] = static_cast<int32_t>((8u * static_cast<uint32_t>(c) + static_cast<uint32_t>(chd)) |
                                           ((last || off_field) ? 0u : static_cast<uint32_t>(q) << kCarMoveShift));
    ++count;
    if (last) break;
    if (off_field) {  // not on a converged field with a reachable start
      status = 2;
      break;
    }
    int ax, ay, ah;
    car_target(cx, cy, chd, q, turn, &ax, &ay, &ah);
    cx = ax;
    cy = ay;
    chd = ah;
  }
  if (lane == 0) {
    out[0] = count;
    out[1] = status;
  }
}

// The kernels' status words, one struct on the device and in pinned memory: a read-back copies a member onto itself.
struct PlanWords {
  uint32_t changed;                                 // the last pass that changed a cell
  uint32_t walk_count, walk_status, walk_clear2;    // either walk's out[0..1]; out[2] of planner_walk_kernel<true>
  uint32_t short_count, short_status, short_clear2; // planner_shortcut_kernel's out[0..2]
  uint32_t rp_T, rp_touched, rp_listed;             // planner_touched_kernel's out[0..1], planner_compact_kernel's count
  uint32_t ex_listed;                               // planner_compact_kernel's count of the tiles that hold a frontier cell
  uint32_t ex_components, ex_kept, ex_slots;        // planner_frontier_count_kernel's out[0..1], planner_frontier_slot_kernel's counter
};
constexpr size_t kPlanSolveWords = 4;  // zeroed by one memset before the passes of a solve: changed and the walk's three
// what the memsets, the multi-word copies and the kernels' out[] rely on
static_assert(sizeof(PlanWords) == 56 && offsetof(PlanWords, changed) == 0 && offsetof(PlanWords, walk_count) == 4 &&
                  offsetof(PlanWords, walk_status) == 8 && offsetof(PlanWords, walk_clear2) == 12 && offsetof(PlanWords, short_count) == 16 &&
                  offsetof(PlanWords, short_status) == 20 && offsetof(PlanWords, short_clear2) == 24 && offsetof(PlanWords, rp_T) == 28 &&
                  offsetof(PlanWords, rp_touched) == 32 && offsetof(PlanWords, rp_listed) == 36 && offsetof(PlanWords, ex_listed) == 40 &&
                  offsetof(PlanWords, ex_components) == 44 && offsetof(PlanWords, ex_kept) == 48 && offsetof(PlanWords, ex_slots) == 52,
              "changed .. walk_clear2 are words 0 .. 3; each kernel's out[0..2] are neighbours in its order");
struct PlanPinned {
  PlanWords w;
  uint32_t start_field, start_valid, goal_valid;  // planner_finish's read-backs: field[start], a validity byte each
};

}  // namespace kc

using namespace kc;

struct kc_planner {
  int device = 0;
  hipStream_t stream = nullptr;
  int W = 0, H = 0;
  unsigned tiles_x = 0, tiles_y = 0;  // of kPlanTile cells; at most 2^28 / 64 tiles (a one-cell-wide grid), within gridDim.x
  bool have_grid = false;
  bool have_valid = false;   // d_valid holds the validity of (grid, valid_r2, valid_unknown), and with the clearance
                             // cost on d_clear2 / d_pen hold the clearance and penalty of (grid, clear_c2, table)
  uint32_t valid_r2 = 0;
  int valid_unknown = 0;
  bool solved = false;
  int final_buf = 0;         // which of d_field holds the fixed point
  int start[2] = {0, 0};
  int status = -1;
  uint32_t cost = kPlanInf;
  bool have_path = false;
  std::vector<int32_t> path; // linear cell indices, start first
  DevBuf<uint8_t> d_stage;   // a host grid on its way to the classifier
  DevBuf<uint8_t> d_cls, d_rowd, d_valid;
  DevBuf<uint32_t> d_field[2];
  uint32_t clear_c2 = 0;     // the clearance cost (rules 6 to 8): on while clear_c2 > 0
  uint32_t clear_max_pen = 0;
  uint32_t path_clear2 = KC_PLANNER_CLEAR_FAR;
  DevBuf<uint32_t> d_pen_by_d2, d_pen;
  DevBuf<uint16_t> d_clear2;
  DevBuf<PlanWords> d_word;  // one element each
  PinBuf<PlanPinned> h_word;
  DevBuf<int32_t> d_path;
  PinBuf<int32_t> h_path;
  bool have_short = false;   // short_idx holds rule 11's indices into `path` for short_span; only with have_path
  int short_span = 0;
  uint32_t short_clear2 = KC_PLANNER_CLEAR_FAR;
  std::vector<int32_t> short_idx;
  DevBuf<int32_t> d_keep;
  PinBuf<int32_t> h_keep;
  uint32_t or_a2 = 0, or_b2 = 0, or_turn10 = 0;  // the oriented footprint (rules 13 to 18): on while or_a2 > 0
  PlanMaskEnds or_ends = {};
  bool or_have_valid = false;  // d_turn / d_valid4 hold the maps of (grid, or_a2, or_b2, or_valid_unknown)
  int or_valid_unknown = 0;
  bool or_solve = false;       // the last solve was kc_planner_solve_oriented: d_field4, start_class, states
  int start_class = 0;
  std::vector<int32_t> states; // the walk's states, 4 * cell + class; `path` then holds its cells, turns collapsed
  DevBuf<int16_t> d_offs;
  DevBuf<uint8_t> d_turn, d_valid4;
  DevBuf<uint32_t> d_field4[2];
  // car motion (rules 27 to 36): on while car_turn > 0
  int car_turn = 0;            // n, the turn length in cells
  uint32_t car_rw = 0;         // the reverse weight, 0: no reverse
  uint32_t car_a2 = 0, car_b2 = 0;  // the box footprint's masks (d_offs, or_ends, d_valid4 as the oriented mode's); 0, 0: the disc
  bool car_solve = false;      // the last solve was kc_planner_solve_car: d_field8, d_moves, start_heading, car_states
  bool car_have_moves = false; // d_moves holds rule 30's bytes of (the validity map in use, car_turn, car_rw)
  int start_heading = 0;
  std::vector<int32_t> car_states;  // the walk's states, 8 * cell + heading; `path` then holds rule 34's expansion
  std::vector<int32_t> car_moves;   // the primitive taken out of each state but the last
  float car_ms[3] = {0.0f, 0.0f, 0.0f};  // host clock around the maps + moves, the field and the walk, each ended by its read-back
  DevBuf<uint8_t> d_steps, d_moves;
  DevBuf<uint32_t> d_field8[2];
  // the replan (rules 19 and 20)
  bool fld_ok = false;         // d_field[final_buf] is the fixed point of (fld_goal, valid_r2, valid_unknown, the table) on a
                               // W x H grid whose maps are d_valid (d_pen), the goal valid; a new grid of that shape leaves it
  int fld_goal[2] = {0, 0};
  DevBuf<uint8_t> d_valid_old; // the kept field's maps while the new grid's are made
  DevBuf<uint32_t> d_pen_old;
  DevBuf<uint8_t> d_tile_on;   // a byte a tile: its halo region holds a cell that may change
  DevBuf<uint32_t> d_tile_list;
  bool rp_kept = false;        // the last kc_planner_replan kept a field; T, touched cells, tiles relaxed
  uint32_t rp_T = kPlanInf, rp_touched = 0, rp_tiles = 0;
  // exploration (rules 21 to 26)
  bool explored = false;       // the last solve-type call was kc_planner_explore: d_field[final_buf] is rooted at the robot's
                               // cell `start`, d_valid is rule 21's map (have_valid stays false: no solve may take it for its own)
  int label_buf = 0;           // which of d_label holds rule 24's labels; the other one is the size / slot plane
  uint32_t ex_components = 0, ex_tiles = 0;
  float ex_ms[3] = {0.0f, 0.0f, 0.0f};  // host clock around the field, mark + label and records phases, each ended by its read-back
  std::vector<kc_planner_frontier> frontiers;  // the kept records, sorted by (cost, entry flat index)
  DevBuf<uint8_t> d_front;
  DevBuf<uint32_t> d_label[2];
  DevBuf<PlanFrontierRec> d_rec;
  PinBuf<PlanFrontierRec> h_rec;
};

namespace {

// What a context holds is a ladder: grid -> maps (the disc's, the oriented masks') -> field (with the kept field's
// fld_ok) -> walk -> shortcut.  Whatever changes a level calls the forget_* of the level below it, which drops that
// level and every one after it.
void forget_walk(kc_planner *c) { c->have_path = c->have_short = false; }

// also what a solve starts with: its outputs say "nothing" until it ends
void forget_solve(kc_planner *c, uint32_t *cost_out = nullptr, int *passes_out = nullptr) {
  c->solved = c->or_solve = c->car_solve = c->fld_ok = c->explored = false;
  c->frontiers.clear();
  c->status = -1;
  c->cost = kPlanInf;
  if (cost_out) *cost_out = kPlanInf;
  if (passes_out) *passes_out = 0;
  forget_walk(c);
}

void forget_maps(kc_planner *c, bool disc, bool oriented) {
  if (disc) c->have_valid = false;
  if (oriented) c->or_have_valid = false;
  c->car_have_moves = false;  // rule 30's bytes are made from a validity map
  forget_solve(c);
}

// f(std::true_type) or f(std::false_type): one launch statement for both instantiations of a <bool> kernel
template <typename F>
void with_bool(bool on, F &&f) { on ? f(std::true_type{}) : f(std::false_type{}); }

// floor(sqrt(v)) for v < (KC_PLANNER_MAX_RADIUS_CELLS + 1)^2, which kc_planner_solve and the two setters see to: at most
// KC_PLANNER_MAX_RADIUS_CELLS = 254, the largest distance a rowd byte holds beside its 255 of "none"
int plan_isqrt(uint32_t v) {
  int r = 0;
  while (static_cast<uint32_t>(r + 1) * static_cast<uint32_t>(r + 1) <= v) ++r;
  return r;
}

// the refusal of a disc footprint whose row distances a rowd byte does not hold
int check_radius(uint32_t r2) {
  if (r2 >= static_cast<uint32_t>(KC_PLANNER_MAX_RADIUS_CELLS + 1) * (KC_PLANNER_MAX_RADIUS_CELLS + 1))
    KC_FAIL(KC_ERR_RANGE, "a footprint of R2 = %u is wider than %d cells", r2, KC_PLANNER_MAX_RADIUS_CELLS);
  return KC_OK;
}
// the same for a box, whose turning disc T2 = A2 + B2 contains every mask; `what` names the sum in the caller's terms
int check_box(uint32_t a2, uint32_t b2, const char *what) {
  const unsigned long long t2 = static_cast<unsigned long long>(a2) + b2;
  if (t2 > static_cast<unsigned long long>(KC_PLANNER_MAX_RADIUS_CELLS) * KC_PLANNER_MAX_RADIUS_CELLS)
    KC_FAIL(KC_ERR_RANGE, "a %s = %llu is wider than %d cells", what, t2, KC_PLANNER_MAX_RADIUS_CELLS);
  return KC_OK;
}

// the host clock of a call's phases: lap() is the milliseconds since the last lap, or since the clock was made
struct PlanClock {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  float lap() {
    const auto now = std::chrono::steady_clock::now();
    const float ms = std::chrono::duration<float, std::milli>(now - t).count();
    t = now;
    return ms;
  }
};

// the linear index of a cell, -1 outside the grid
long long plan_cell_index(const kc_planner *c, const int cell[2]) {
  const bool in = cell[0] >= 0 && cell[0] < c->W && cell[1] >= 0 && cell[1] < c->H;
  return in ? static_cast<long long>(cell[1]) * c->W + cell[0] : -1;
}

// `count` status words from `first` on, device to pinned, on the stream
hipError_t plan_fetch_words(kc_planner *c, uint32_t PlanWords::*first, size_t count) {
  return hipMemcpyAsync(&(c->h_word.p->w.*first), &(c->d_word.p->*first), count * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
}

unsigned plan_blocks_for(long long work) {
  return static_cast<unsigned>(std::max<long long>(1, std::min<long long>(kPlanMaxBlocks, (work + kPlanBlock - 1) / kPlanBlock)));
}

int check_grid_shape(const void *grid, int elem_bytes, int width, int height) {
  if (!grid) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (elem_bytes != 1 && elem_bytes != 4) KC_FAIL(KC_ERR_INVALID, "grid cells are int8 (1) or int32 (4) bytes, got %d", elem_bytes);
  if (width <= 0 || height <= 0) KC_FAIL(KC_ERR_INVALID, "grid width and height must be positive, got %d x %d", width, height);
  if (static_cast<unsigned long long>(width) * static_cast<unsigned long long>(height) > KC_PLANNER_MAX_CELLS)
    KC_FAIL(KC_ERR_RANGE, "a %d x %d grid is above the cap of %u cells", width, height, static_cast<unsigned>(KC_PLANNER_MAX_CELLS));
  return KC_OK;
}

// dev: the grid on the context's device, complete
int planner_take_grid(kc_planner *c, const void *dev, int elem_bytes, int width, int height) {
  const long long n = static_cast<long long>(width) * height;
  const bool keep_field = c->fld_ok && width == c->W && height == c->H;  // a kept field (rule 20) is one of this shape
  c->have_grid = false;
  forget_maps(c, true, true);
  c->fld_ok = keep_field;
  KC_TRY(c->d_cls.reserve(static_cast<size_t>(n)));
  if (elem_bytes == 4)
    hipLaunchKernelGGL(planner_classify_kernel<int32_t>, dim3(plan_blocks_for(n)), dim3(kPlanBlock), 0, c->stream,
                       static_cast<const int32_t *>(dev), c->d_cls.p, n);
  else
    hipLaunchKernelGGL(planner_classify_kernel<int8_t>, dim3(plan_blocks_for(n)), dim3(kPlanBlock), 0, c->stream,
                       static_cast<const int8_t *>(dev), c->d_cls.p, n);
  KC_HIP(hipGetLastError());
  KC_HIP(hipStreamSynchronize(c->stream));  // the caller's grid is not read after the call returns
  c->W = width;
  c->H = height;
  c->tiles_x = static_cast<unsigned>((width + kPlanTile - 1) / kPlanTile);
  c->tiles_y = static_cast<unsigned>((height + kPlanTile - 1) / kPlanTile);
  c->have_grid = true;
  return KC_OK;
}

// rule 14's offsets of class k, by rising di^2 + dj^2 (then dj, then di); A2 + B2 within the radius cap
std::vector<int16_t> oriented_offsets(int k, uint32_t a2, uint32_t b2) {
  const int r = plan_isqrt(a2 + b2);  // T2 contains every mask
  std::vector<std::pair<int, int>> o;
  for (int dj = -r; dj <= r; ++dj)
    for (int di = -r; di <= r; ++di) {
      const uint32_t ii = static_cast<uint32_t>(di * di), jj = static_cast<uint32_t>(dj * dj);
      const uint32_t ss = static_cast<uint32_t>((di + dj) * (di + dj)), dd = static_cast<uint32_t>((dj - di) * (dj - di));
      const bool in = k == 0 ? ii <= a2 && jj <= b2 : k == 2 ? jj <= a2 && ii <= b2 : k == 1 ? ss <= 2 * a2 && dd <= 2 * b2 : dd <= 2 * a2 && ss <= 2 * b2;
      if (in) o.emplace_back(di, dj);
    }
  std::stable_sort(o.begin(), o.end(), [](const std::pair<int, int> &p, const std::pair<int, int> &q) {
    return p.first * p.first + p.second * p.second < q.first * q.first + q.second * q.second;
  });
  std::vector<int16_t> out;
  out.reserve(2 * o.size());
  for (const auto &p : o) {
    out.push_back(static_cast<int16_t>(p.first));
    out.push_back(static_cast<int16_t>(p.second));
  }
  return out;
}

// behind either walk kernel's launch: its count and status (and walk_clear2, a copy of its own) come back, then the
// `count` int32 it wrote to d_path arrive in h_path; "the <noun> walk stopped after .. <unit>"
int planner_walk_fetch(kc_planner *c, size_t cap, bool clear2_too, const char *noun, const char *unit, uint32_t *count_out) {
  hipStream_t s = c->stream;
  KC_HIP(hipGetLastError());
  KC_HIP(plan_fetch_words(c, &PlanWords::walk_count, 2));
  if (clear2_too) KC_HIP(plan_fetch_words(c, &PlanWords::walk_clear2, 1));
  KC_HIP(hipStreamSynchronize(s));
  const uint32_t count = c->h_word.p->w.walk_count, wst = c->h_word.p->w.walk_status;
  if (wst != 0u || count == 0u || count > cap)
    KC_FAIL(KC_ERR_STATE, "the %s walk stopped after %u %s with status %u", noun, count, unit, wst);
  KC_HIP(hipMemcpyAsync(c->h_path.p, c->d_path.p, count * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  KC_HIP(hipStreamSynchronize(s));
  *count_out = count;
  return KC_OK;
}

// rule 17 over the last oriented solve (status KC_PLAN_FOUND), once: c->states, and c->path with the turns collapsed
int planner_walk_oriented(kc_planner *c) {
  KC_HIP(hipSetDevice(c->device));
  const size_t n = static_cast<size_t>(c->W) * static_cast<size_t>(c->H);
  // every transition lowers the field by min(10, turn10) at least, and no state comes twice
  const size_t cap = std::min<size_t>(4 * n, static_cast<size_t>(c->cost / std::min<uint32_t>(10u, c->or_turn10))) + 2;
  KC_TRY(c->d_path.reserve(cap));
  KC_TRY(c->h_path.reserve(cap));
  hipLaunchKernelGGL(planner_walk4_kernel, dim3(1), dim3(64), 0, c->stream, c->d_field4[c->final_buf].p, c->d_valid4.p, c->W, c->H, n, c->start[0],
                     c->start[1], c->start_class, c->or_turn10, c->d_path.p, static_cast<uint32_t>(cap), &c->d_word.p->walk_count);
  uint32_t count = 0;
  KC_TRY(planner_walk_fetch(c, cap, false, "state", "states", &count));
  c->states.assign(c->h_path.p, c->h_path.p + count);
  c->path.clear();
  for (const int32_t st : c->states)
    if (c->path.empty() || c->path.back() != st / 4) c->path.push_back(st / 4);  // a turn stays in its cell
  c->path_clear2 = static_cast<uint32_t>(KC_PLANNER_CLEAR_FAR);
  c->have_path = true;
  return KC_OK;
}

int planner_walk_car(kc_planner *c);

// the walk of the last solve (status KC_PLAN_FOUND), once: c->path, and c->path_clear2 with the clearance cost on
int planner_walk(kc_planner *c) {
  if (c->have_path) return KC_OK;
  if (c->or_solve) return planner_walk_oriented(c);
  if (c->car_solve) return planner_walk_car(c);
  KC_HIP(hipSetDevice(c->device));
  const bool pen_on = c->clear_c2 > 0;
  const uint32_t *pen = pen_on ? c->d_pen.p : nullptr;
  const uint16_t *clear2 = pen_on ? c->d_clear2.p : nullptr;
  // every step lowers the field by 10 at least
  const size_t cap = static_cast<size_t>(c->cost / 10u) + 2;
  KC_TRY(c->d_path.reserve(cap));
  KC_TRY(c->h_path.reserve(cap));
  with_bool(pen_on, [&](auto on) {
    hipLaunchKernelGGL(planner_walk_kernel<decltype(on)::value>, dim3(1), dim3(64), 0, c->stream, c->d_field[c->final_buf].p, c->d_valid.p, pen,
                       clear2, c->W, c->H, c->start[0], c->start[1], c->d_path.p, static_cast<uint32_t>(cap), &c->d_word.p->walk_count);
  });
  uint32_t count = 0;
  KC_TRY(planner_walk_fetch(c, cap, pen_on, "path", "cells", &count));
  c->path.assign(c->h_path.p, c->h_path.p + count);
  c->path_clear2 = pen_on ? c->h_word.p->w.walk_clear2 : static_cast<uint32_t>(KC_PLANNER_CLEAR_FAR);
  c->have_path = true;
  return KC_OK;
}

// rules 9 to 12 over the walk of the last solve, once per (walk, max_span): c->short_idx, c->short_clear2
int planner_shortcut(kc_planner *c, int max_span) {
  KC_TRY(planner_walk(c));
  if (c->have_short && c->short_span == max_span) return KC_OK;
  c->have_short = false;
  KC_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const bool clr = c->clear_c2 > 0;
  const size_t n = c->path.size();  // d_path still holds these cells: only the walk writes it
  KC_TRY(c->d_keep.reserve(n));
  KC_TRY(c->h_keep.reserve(n));
  const uint16_t *clear2 = clr ? c->d_clear2.p : nullptr;
  with_bool(clr, [&](auto on) {
    hipLaunchKernelGGL(planner_shortcut_kernel<decltype(on)::value>, dim3(1), dim3(kShortThreads), 0, s, c->d_path.p, static_cast<uint32_t>(n),
                       max_span, c->d_valid.p, clear2, clr ? c->path_clear2 : 0u, c->W, c->d_keep.p, &c->d_word.p->short_count);
  });
  KC_HIP(hipGetLastError());
  KC_HIP(plan_fetch_words(c, &PlanWords::short_count, 3));
  KC_HIP(hipStreamSynchronize(s));
  const uint32_t count = c->h_word.p->w.short_count, sst = c->h_word.p->w.short_status;
  if (sst != 0u || count == 0u || count > n) KC_FAIL(KC_ERR_STATE, "the shortcut stopped after %u indices with status %u", count, sst);
  KC_HIP(hipMemcpyAsync(c->h_keep.p, c->d_keep.p, count * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  KC_HIP(hipStreamSynchronize(s));
  c->short_idx.assign(c->h_keep.p, c->h_keep.p + count);
  c->short_clear2 = c->h_word.p->w.short_clear2;
  c->short_span = max_span;
  c->have_short = true;
  return KC_OK;
}

// rules 2 and 6: the validity map of (grid, r2, unknown_blocks) into d_valid, and with the clearance cost on clear2 and the
// penalty beside it
int planner_validity(kc_planner *c, uint32_t r2, int unknown_blocks) {
  hipStream_t s = c->stream;
  const int W = c->W, H = c->H, R = plan_isqrt(r2);
  const long long n = static_cast<long long>(W) * H;
  const unsigned blocks = plan_blocks_for(n);
  c->have_valid = false;
  KC_TRY(c->d_rowd.reserve(static_cast<size_t>(n)));
  KC_TRY(c->d_valid.reserve(static_cast<size_t>(n)));
  if (c->clear_c2 > 0) {
    const int Rm = std::max(R, plan_isqrt(c->clear_c2));
    KC_TRY(c->d_clear2.reserve(static_cast<size_t>(n)));
    KC_TRY(c->d_pen.reserve(static_cast<size_t>(n)));
    hipLaunchKernelGGL(planner_rowdist_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, c->d_cls.p, c->d_rowd.p, W, H, Rm, unknown_blocks);
    hipLaunchKernelGGL(planner_clear_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, c->d_rowd.p, c->d_pen_by_d2.p, c->d_clear2.p,
                       c->d_pen.p, c->d_valid.p, W, H, Rm, r2, c->clear_c2);
  } else {
    hipLaunchKernelGGL(planner_rowdist_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, c->d_cls.p, c->d_rowd.p, W, H, R, unknown_blocks);
    hipLaunchKernelGGL(planner_valid_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, c->d_rowd.p, c->d_valid.p, W, H, R, r2);
  }
  KC_HIP(hipGetLastError());
  c->have_valid = true;
  c->valid_r2 = r2;
  c->valid_unknown = unknown_blocks;
  return KC_OK;
}

// rule 14's four offset lists of the box (a2, b2) into d_offs and or_ends; the caller drops the maps made from another box
int planner_upload_box(kc_planner *c, uint32_t a2, uint32_t b2) {
  std::vector<int16_t> all;
  PlanMaskEnds ends = {};
  for (int k = 0; k < 4; ++k) {
    const std::vector<int16_t> o = oriented_offsets(k, a2, b2);
    all.insert(all.end(), o.begin(), o.end());
    ends.at[k + 1] = static_cast<uint32_t>(all.size() / 2);
  }
  KC_HIP(hipSetDevice(c->device));
  KC_TRY(c->d_offs.reserve(all.size()));
  // pageable memory: the copy has left the vector when the call returns
  KC_HIP(hipMemcpyAsync(c->d_offs.p, all.data(), all.size() * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  c->or_ends = ends;
  return KC_OK;
}

// rules 14 and 15: the class bits and the turn bit of the box (a2, b2) whose offsets d_offs holds into d_valid4, the turning
// disc into d_turn, unless they are there
int planner_oriented_validity(kc_planner *c, uint32_t a2, uint32_t b2, int unknown_blocks) {
  if (c->or_have_valid && c->or_valid_unknown == unknown_blocks) return KC_OK;
  hipStream_t s = c->stream;
  const int W = c->W, H = c->H;
  const long long n = static_cast<long long>(W) * H;
  const unsigned blocks = plan_blocks_for(n);
  c->or_have_valid = false;
  const uint32_t t2 = a2 + b2;
  const int R = plan_isqrt(t2);
  KC_TRY(c->d_rowd.reserve(static_cast<size_t>(n)));
  KC_TRY(c->d_turn.reserve(static_cast<size_t>(n)));
  KC_TRY(c->d_valid4.reserve(static_cast<size_t>(n)));
  // rule 15 is rule 2's disc with r2 = T2: the row distances are scratch, the disc solve's d_valid is not touched
  hipLaunchKernelGGL(planner_rowdist_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, c->d_cls.p, c->d_rowd.p, W, H, R, unknown_blocks);
  hipLaunchKernelGGL(planner_valid_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, c->d_rowd.p, c->d_turn.p, W, H, R, t2);
  hipLaunchKernelGGL(planner_oriented_valid_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, c->d_cls.p, c->d_turn.p, c->d_offs.p,
                     c->or_ends, c->d_valid4.p, W, H, unknown_blocks);
  KC_HIP(hipGetLastError());
  c->or_have_valid = true;
  c->or_valid_unknown = unknown_blocks;
  return KC_OK;
}

// rule 34: the cell indices of every unit step of primitive p out of (cell, h), first leg then second, appended
void car_expand(const kc_planner *c, int32_t cell, int h, int p, std::vector<int32_t> *cells) {
  static const int dx[8] = {1, 1, 0, -1, -1, -1, 0, 1}, dy[8] = {0, 1, 1, 1, 0, -1, -1, -1};
  const int sgn = p < 3 ? 1 : -1;
  const bool arc = p != 0 && p != 3;
  const int h2 = !arc ? h : ((p == 1 || p == 5) ? (h + 1) & 7 : (h + 7) & 7);
  const int len = arc ? c->car_turn : 1;
  int x = cell % c->W, y = cell / c->W;
  for (int leg = 0; leg < (arc ? 2 : 1); ++leg) {
    const int hl = leg == 0 ? h : h2;
    for (int k = 0; k < len; ++k) {
      x += sgn * dx[hl];
      y += sgn * dy[hl];
      cells->push_back(y * c->W + x);
    }
  }
}

// rule 33 over the last car solve (status KC_PLAN_FOUND), once: c->car_states, c->car_moves, and c->path with rule 34's expansion
int planner_walk_car(kc_planner *c) {
  KC_HIP(hipSetDevice(c->device));
  PlanClock clock;
  const size_t n = static_cast<size_t>(c->W) * static_cast<size_t>(c->H);
  // every primitive lowers the field by 10 at least, and no state comes twice
  const size_t cap = std::min<size_t>(8 * n, static_cast<size_t>(c->cost / 10u)) + 2;
  KC_TRY(c->d_path.reserve(cap));
  KC_TRY(c->h_path.reserve(cap));
  hipLaunchKernelGGL(planner_walk8_kernel, dim3(1), dim3(64), 0, c->stream, c->d_field8[c->final_buf].p, c->d_moves.p, c->W, c->H, n, c->start[0],
                     c->start[1], c->start_heading, c->car_turn, c->car_rw, c->d_path.p, static_cast<uint32_t>(cap), &c->d_word.p->walk_count);
  uint32_t count = 0;
  KC_TRY(planner_walk_fetch(c, cap, false, "car", "states", &count));
  c->car_ms[2] = clock.lap();
  c->car_states.resize(count);
  c->car_moves.resize(count - 1);
  c->path.clear();
  for (uint32_t k = 0; k < count; ++k) {
    const uint32_t word = static_cast<uint32_t>(c->h_path.p[k]);
    const int32_t state = static_cast<int32_t>(word & ((1u << kCarMoveShift) - 1u));
    c->car_states[k] = state;
    if (k == 0) c->path.push_back(state / 8);
    if (k + 1 < count) {
      c->car_moves[k] = static_cast<int32_t>(word >> kCarMoveShift);
      car_expand(c, state / 8, state % 8, c->car_moves[k], &c->path);
    }
  }
  c->path_clear2 = static_cast<uint32_t>(KC_PLANNER_CLEAR_FAR);
  c->have_path = true;
  return KC_OK;
}

// the start of a field pair: both buffers hold `cells` values, init(a, b) queues the kernel that writes the start state
// into both, the solve's words are zero.  Both buffers hold the initial state, so pass 1 reads either: final_buf = 0.
template <typename Init>
int planner_start_pair(kc_planner *c, DevBuf<uint32_t> (&pair)[2], size_t cells, Init &&init) {
  KC_TRY(pair[0].reserve(cells));
  KC_TRY(pair[1].reserve(cells));
  init(pair[0].p, pair[1].p);
  KC_HIP(hipMemsetAsync(c->d_word.p, 0, kPlanSolveWords * sizeof(uint32_t), c->stream));
  KC_HIP(hipGetLastError());
  c->final_buf = 0;
  return KC_OK;
}

// rule 3's passes to the fixed point, in batches of kPlanBatch with one read-back of the changed word (zero before the
// first) a batch.  launch(k, b) queues pass k, which reads buffer b = (k - 1) & 1 of a field pair and writes the other.
// A pass that is not the last gives at least one more of the `states` cells or states its final value: states + 1
// passes always do.  *final_out: the buffer the last pass wrote; *passes_out: the passes a batch of one would have
// run, the last that changed a cell and the one that found nothing to change.  The labelling (rule 24) is the same
// loop: a pass that is not the last gives one more frontier cell its final label at least.
template <typename Launch>
int planner_relax(kc_planner *c, Launch &&launch, unsigned long long states, const char *noun, int *final_out, uint32_t *passes_out) {
  const unsigned long long cap = states + 1ull;
  for (uint32_t pass = 0;;) {
    for (int b = 0; b < kPlanBatch; ++b) {
      ++pass;
      launch(pass, static_cast<int>((pass - 1) & 1u));
    }
    KC_HIP(hipGetLastError());
    KC_HIP(plan_fetch_words(c, &PlanWords::changed, 1));
    KC_HIP(hipStreamSynchronize(c->stream));
    const uint32_t last_changed = c->h_word.p->w.changed;
    if (last_changed < pass) {
      *final_out = static_cast<int>(pass & 1u);
      *passes_out = last_changed + 1u;
      return KC_OK;
    }
    if (pass >= cap)
      KC_FAIL(KC_ERR_RANGE, "the %s field of a %d x %d grid still changed after %u passes (cap %llu)", noun, c->W, c->H, pass, cap);
  }
}

// the disc's pass over `blocks` tiles: all of them (list == nullptr) or those of a list
auto disc_pass(kc_planner *c, const uint32_t *list, unsigned blocks) {
  return [=](uint32_t pass, int b) {
    const bool pen_on = c->clear_c2 > 0;
    const uint32_t *in = c->d_field[b].p, *pen = pen_on ? c->d_pen.p : nullptr;
    uint32_t *out = c->d_field[b ^ 1].p, *changed = &c->d_word.p->changed;
    with_bool(pen_on, [&](auto on) {
      if (list)
        hipLaunchKernelGGL(planner_relax_list_kernel<decltype(on)::value>, dim3(blocks), dim3(kPlanThreads), 0, c->stream, in, out,
                           c->d_valid.p, pen, c->W, c->H, c->tiles_x, list, changed, pass);
      else
        hipLaunchKernelGGL(planner_relax_kernel<decltype(on)::value>, dim3(blocks), dim3(kPlanThreads), 0, c->stream, in, out,
                           c->d_valid.p, pen, c->W, c->H, c->tiles_x, changed, pass);
    });
  };
}

// `field` (a layer of the pair's buffer c->final_buf) holds the fixed point for goal_cell over the validity bytes
// `valid`: the start's status and cost (rule 4).  A cell is valid where its byte has a bit of its mask.  keep_field:
// the field may serve a replan, which needs to know its goal.
int planner_finish(kc_planner *c, const int start_cell[2], const int goal_cell[2], const uint32_t *field, const uint8_t *valid,
                   uint32_t start_mask, uint32_t goal_mask, bool keep_field, int *status_out, uint32_t *cost_out) {
  hipStream_t s = c->stream;
  const long long start = plan_cell_index(c, start_cell), goal = plan_cell_index(c, goal_cell);
  PlanPinned *h = c->h_word.p;
  c->solved = true;
  c->start[0] = start_cell[0];
  c->start[1] = start_cell[1];
  h->start_field = kPlanInf;
  h->start_valid = 0;
  h->goal_valid = 0;
  if (start >= 0) {
    KC_HIP(hipMemcpyAsync(&h->start_field, field + start, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    KC_HIP(hipMemcpyAsync(&h->start_valid, valid + start, 1, hipMemcpyDeviceToHost, s));
  }
  if (goal >= 0) KC_HIP(hipMemcpyAsync(&h->goal_valid, valid + goal, 1, hipMemcpyDeviceToHost, s));
  KC_HIP(hipStreamSynchronize(s));
  const bool start_ok = (h->start_valid & start_mask) != 0, goal_ok = (h->goal_valid & goal_mask) != 0;
  int st = KC_PLAN_FOUND;
  if (start < 0) st = KC_PLAN_START_OUTSIDE;
  else if (goal < 0) st = KC_PLAN_GOAL_OUTSIDE;
  else if (!start_ok) st = KC_PLAN_START_INVALID;
  else if (!goal_ok) st = KC_PLAN_GOAL_INVALID;
  else if (h->start_field == kPlanInf) st = KC_PLAN_UNREACHABLE;
  c->status = st;
  c->cost = st == KC_PLAN_FOUND ? h->start_field : kPlanInf;
  *status_out = st;
  if (cost_out) *cost_out = c->cost;
  // rule 19's proof starts from old(goal) = 0: a field of all INF under an invalid goal is not kept
  c->fld_ok = keep_field && goal_ok;
  c->fld_goal[0] = goal_cell[0];
  c->fld_goal[1] = goal_cell[1];
  return KC_OK;
}

}  // namespace

// DESIGN.md 4.12 rules 19 and 23: the field of the last solve-type call, where it lies, when that call was kc_planner_solve
// or kc_planner_replan.  The pair's buffers alternate between solves, so a reader asks at every use
int kc::planner_field_view(kc_planner *c, PlannerFieldView *out) {
  if (!c || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (!c->solved) KC_FAIL(KC_ERR_STATE, "the planner holds no cost field: kc_planner_solve or kc_planner_replan first");
  if (c->or_solve || c->car_solve || c->explored)
    KC_FAIL(KC_ERR_STATE, "the planner's last field is %s, not a goal-rooted disc-mode one",
            c->or_solve ? "an oriented solve's" : (c->car_solve ? "a car solve's" : "rooted at the robot by kc_planner_explore"));
  *out = PlannerFieldView{c->d_field[c->final_buf].p, c->W, c->H, c->stream, c->device};
  return KC_OK;
}

extern "C" {

int kc_planner_create(int device, kc_planner **out) {
  if (!out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *out = nullptr;
  hipStream_t stream = nullptr;
  KC_TRY(open_device_stream(device, &stream));
  auto *c = new kc_planner();
  c->device = device;
  c->stream = stream;
  int rc;
  if ((rc = c->d_word.reserve(1)) || (rc = c->h_word.reserve(1))) {
    kc_planner_destroy(c);
    return rc;
  }
  *out = c;
  return KC_OK;
}

void kc_planner_destroy(kc_planner *c) {
  if (!c) return;
  close_device_stream(c->device, &c->stream);
  delete c;
}

int kc_planner_set_grid_host(kc_planner *c, const void *grid, int elem_bytes, int width, int height) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  KC_TRY(check_grid_shape(grid, elem_bytes, width, height));
  KC_HIP(hipSetDevice(c->device));
  const size_t nbytes = static_cast<size_t>(width) * static_cast<size_t>(height) * static_cast<size_t>(elem_bytes);
  KC_TRY(c->d_stage.reserve(nbytes));
  KC_HIP(hipMemcpyAsync(c->d_stage.p, grid, nbytes, hipMemcpyHostToDevice, c->stream));
  return planner_take_grid(c, c->d_stage.p, elem_bytes, width, height);
}

int kc_planner_set_grid_device(kc_planner *c, const void *dev_grid, int elem_bytes, int width, int height) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  KC_TRY(check_grid_shape(dev_grid, elem_bytes, width, height));
  KC_HIP(hipSetDevice(c->device));
  const size_t nbytes = static_cast<size_t>(width) * static_cast<size_t>(height) * static_cast<size_t>(elem_bytes);
  // read in place: refused before any read unless all of it is this device's memory, aligned to its cells
  KC_TRY(check_device_range(c->device, dev_grid, 0, static_cast<long long>(nbytes), static_cast<size_t>(elem_bytes), "grid"));
  return planner_take_grid(c, dev_grid, elem_bytes, width, height);
}

int kc_planner_after_stream(kc_planner *c, void *stream) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  return stream_wait_for(c->device, c->stream, stream);
}

int kc_planner_solve(kc_planner *c, const int start_cell[2], const int goal_cell[2], uint32_t r2, int allow_unknown,
                     int *status_out, uint32_t *cost_out, int *passes_out) {
  if (!c || !start_cell || !goal_cell || !status_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (!c->have_grid) KC_FAIL(KC_ERR_STATE, "kc_planner_solve before a grid was set");
  if (c->or_a2 > 0) KC_FAIL(KC_ERR_STATE, "kc_planner_solve with the oriented footprint on: kc_planner_solve_oriented");
  if (c->car_turn > 0) KC_FAIL(KC_ERR_STATE, "kc_planner_solve with car motion on: kc_planner_solve_car");
  KC_TRY(check_radius(r2));
  const long long n = static_cast<long long>(c->W) * c->H;
  // field <= (14 + max penalty) * cells: the sums of the relaxation stay below the 0xFFFFFFFF of "no walk"
  if (c->clear_c2 > 0 && (14ull + c->clear_max_pen) * static_cast<unsigned long long>(n) > 0xFFFFFFFEull)
    KC_FAIL(KC_ERR_RANGE, "a clearance penalty of %u over %lld cells does not fit the 32-bit cost field", c->clear_max_pen, n);
  KC_HIP(hipSetDevice(c->device));
  forget_solve(c, cost_out, passes_out);
  const int unknown_blocks = allow_unknown ? 0 : 1;
  if (!c->have_valid || c->valid_r2 != r2 || c->valid_unknown != unknown_blocks) KC_TRY(planner_validity(c, r2, unknown_blocks));
  const long long goal = plan_cell_index(c, goal_cell);
  KC_TRY(planner_start_pair(c, c->d_field, static_cast<size_t>(n), [&](uint32_t *a, uint32_t *b) {
    hipLaunchKernelGGL(planner_init_kernel, dim3(plan_blocks_for(n)), dim3(kPlanBlock), 0, c->stream, a, b, c->d_valid.p, n, goal);
  }));
  uint32_t passes = 0;
  if (goal >= 0) KC_TRY(planner_relax(c, disc_pass(c, nullptr, c->tiles_x * c->tiles_y), n, "cost", &c->final_buf, &passes));
  KC_TRY(planner_finish(c, start_cell, goal_cell, c->d_field[c->final_buf].p, c->d_valid.p, 0xFFu, 0xFFu, true, status_out, cost_out));
  if (passes_out) *passes_out = static_cast<int>(passes);
  return KC_OK;
}

int kc_planner_replan(kc_planner *c, const int start_cell[2], const int goal_cell[2], uint32_t r2, int allow_unknown,
                      int *status_out, uint32_t *cost_out, int *passes_out) {
  if (!c || !start_cell || !goal_cell || !status_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  c->rp_kept = false;
  c->rp_T = kPlanInf;
  c->rp_touched = c->rp_tiles = 0;
  const int unknown_blocks = allow_unknown ? 0 : 1;
  // rule 20's fall-back: no kept field, or one of another problem; every refusal of kc_planner_solve is its own
  if (!c->have_grid || c->or_a2 > 0 || c->car_turn > 0 || !c->fld_ok || c->fld_goal[0] != goal_cell[0] || c->fld_goal[1] != goal_cell[1] ||
      c->valid_r2 != r2 || c->valid_unknown != unknown_blocks)
    return kc_planner_solve(c, start_cell, goal_cell, r2, allow_unknown, status_out, cost_out, passes_out);
  // r2, the penalty table and the shape are the kept solve's: its range checks hold
  KC_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int W = c->W, H = c->H;
  const long long n = static_cast<long long>(W) * H;
  const bool pen_on = c->clear_c2 > 0;
  PlanWords *d = c->d_word.p;
  forget_solve(c, cost_out, passes_out);
  uint32_t T = kPlanInf, touched = 0, listed = 0, passes = 0;
  if (!c->have_valid) {  // a grid was set since: rule 19 against its maps; otherwise nothing is touched
    const unsigned blocks = plan_blocks_for(n);
    std::swap(c->d_valid, c->d_valid_old);
    if (pen_on) std::swap(c->d_pen, c->d_pen_old);
    KC_TRY(planner_validity(c, r2, unknown_blocks));
    const uint32_t *old = c->d_field[c->final_buf].p, *pen_old = pen_on ? c->d_pen_old.p : nullptr, *pen_new = pen_on ? c->d_pen.p : nullptr;
    KC_HIP(hipMemsetAsync(&d->rp_T, 0xFF, sizeof(uint32_t), s));
    KC_HIP(hipMemsetAsync(&d->rp_touched, 0, 2 * sizeof(uint32_t), s));
    with_bool(pen_on, [&](auto on) {
      hipLaunchKernelGGL(planner_touched_kernel<decltype(on)::value>, dim3(blocks), dim3(kPlanBlock), 0, s, old, c->d_valid_old.p, c->d_valid.p,
                         pen_old, pen_new, W, H, &d->rp_T);
    });
    KC_HIP(hipGetLastError());
    KC_HIP(plan_fetch_words(c, &PlanWords::rp_T, 2));
    KC_HIP(hipStreamSynchronize(s));
    T = c->h_word.p->w.rp_T;
    touched = c->h_word.p->w.rp_touched;
    if (T != kPlanInf) {
      const unsigned ntiles = c->tiles_x * c->tiles_y;
      KC_TRY(c->d_tile_on.reserve(ntiles));
      KC_TRY(c->d_tile_list.reserve(ntiles));
      KC_HIP(hipMemsetAsync(c->d_tile_on.p, 0, ntiles, s));
      hipLaunchKernelGGL(planner_rollback_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, old, c->d_field[0].p, c->d_field[1].p, c->d_valid.p, W,
                         H, plan_cell_index(c, goal_cell), T, static_cast<int>(c->tiles_x), static_cast<int>(c->tiles_y), c->d_tile_on.p);
      hipLaunchKernelGGL(planner_compact_kernel, dim3(plan_blocks_for(ntiles)), dim3(kPlanBlock), 0, s, c->d_tile_on.p, ntiles,
                         c->d_tile_list.p, &d->rp_listed);
      KC_HIP(hipMemsetAsync(d, 0, kPlanSolveWords * sizeof(uint32_t), s));
      KC_HIP(hipGetLastError());
      KC_HIP(plan_fetch_words(c, &PlanWords::rp_listed, 1));
      KC_HIP(hipStreamSynchronize(s));
      listed = c->h_word.p->w.rp_listed;
      if (listed > ntiles) KC_FAIL(KC_ERR_STATE, "%u tiles listed of %u", listed, ntiles);
      c->final_buf = 0;  // both buffers hold the rollback state, so pass 1 reads either
      if (listed) KC_TRY(planner_relax(c, disc_pass(c, c->d_tile_list.p, listed), n, "cost", &c->final_buf, &passes));
    }
  }
  KC_TRY(planner_finish(c, start_cell, goal_cell, c->d_field[c->final_buf].p, c->d_valid.p, 0xFFu, 0xFFu, true, status_out, cost_out));
  if (passes_out) *passes_out = static_cast<int>(passes);
  c->rp_kept = true;
  c->rp_T = T;
  c->rp_touched = touched;
  c->rp_tiles = listed;
  return KC_OK;
}

int kc_planner_replan_info(kc_planner *c, int *replanned_out, uint32_t *threshold_out, uint32_t *touched_out, uint32_t *active_tiles_out) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (replanned_out) *replanned_out = c->rp_kept ? 1 : 0;
  if (threshold_out) *threshold_out = c->rp_T;
  if (touched_out) *touched_out = c->rp_touched;
  if (active_tiles_out) *active_tiles_out = c->rp_tiles;
  return KC_OK;
}

int kc_planner_get_field(kc_planner *c, uint32_t *field_out, uint8_t *valid_out, size_t cap) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (!c->solved) KC_FAIL(KC_ERR_STATE, "kc_planner_get_field before kc_planner_solve");
  if (c->or_solve) KC_FAIL(KC_ERR_STATE, "kc_planner_get_field after an oriented solve: kc_planner_get_oriented_field");
  if (c->car_solve) KC_FAIL(KC_ERR_STATE, "kc_planner_get_field after a car solve: kc_planner_get_car_field");
  const size_t n = static_cast<size_t>(c->W) * static_cast<size_t>(c->H);
  if (n > cap) KC_FAIL(KC_ERR_RANGE, "%zu cells do not fit the output capacity %zu", n, cap);
  KC_HIP(hipSetDevice(c->device));
  if (field_out)
    KC_HIP(hipMemcpyAsync(field_out, c->d_field[c->final_buf].p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (valid_out) KC_HIP(hipMemcpyAsync(valid_out, c->d_valid.p, n, hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  return KC_OK;
}

int kc_planner_field_device(kc_planner *c, const uint32_t **field_out, int *width_out, int *height_out, void **stream_out) {
  if (!c || !field_out || !width_out || !height_out || !stream_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *field_out = nullptr;
  *width_out = *height_out = 0;
  *stream_out = nullptr;
  PlannerFieldView v{};
  KC_TRY(kc::planner_field_view(c, &v));
  *field_out = v.field;
  *width_out = v.W;
  *height_out = v.H;
  *stream_out = v.stream;
  return KC_OK;
}

int kc_planner_get_path(kc_planner *c, int32_t *cells_ij_out, size_t cap_points, size_t *count_out) {
  if (!c || !count_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *count_out = 0;
  if (!c->solved) KC_FAIL(KC_ERR_STATE, "kc_planner_get_path before kc_planner_solve");
  if (c->explored) KC_FAIL(KC_ERR_STATE, "kc_planner_get_path after kc_planner_explore: kc_planner_get_frontier_path");
  if (c->status != KC_PLAN_FOUND) return KC_OK;  // no path: zero points
  KC_TRY(planner_walk(c));
  *count_out = c->path.size();
  if (!cells_ij_out) return KC_OK;  // the count alone
  if (c->path.size() > cap_points) KC_FAIL(KC_ERR_RANGE, "%zu path cells do not fit the output capacity %zu", c->path.size(), cap_points);
  for (size_t k = 0; k < c->path.size(); ++k) {
    cells_ij_out[2 * k] = c->path[k] % c->W;
    cells_ij_out[2 * k + 1] = c->path[k] / c->W;
  }
  return KC_OK;
}

int kc_planner_set_clearance_cost(kc_planner *c, uint32_t c2, const uint32_t *pen_by_d2, size_t n) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  const bool on = c2 > 0 && pen_by_d2 != nullptr;
  if (on && c->or_a2 > 0) KC_FAIL(KC_ERR_STATE, "a clearance cost cannot be set while the oriented footprint is on (rule 18)");
  if (on && c->car_turn > 0) KC_FAIL(KC_ERR_STATE, "a clearance cost cannot be set while car motion is on (rule 35)");
  if (on) {
    if (c2 > static_cast<uint32_t>(KC_PLANNER_MAX_RADIUS_CELLS) * KC_PLANNER_MAX_RADIUS_CELLS)
      KC_FAIL(KC_ERR_RANGE, "a clearance reach of C2 = %u is wider than %d cells", c2, KC_PLANNER_MAX_RADIUS_CELLS);
    if (n != static_cast<size_t>(c2) + 1) KC_FAIL(KC_ERR_INVALID, "the penalty table of C2 = %u has %u entries, not %zu", c2, c2 + 1u, n);
    KC_HIP(hipSetDevice(c->device));
    KC_TRY(c->d_pen_by_d2.reserve(n));
    // pageable memory: the copy has left the caller's table when the call returns
    KC_HIP(hipMemcpyAsync(c->d_pen_by_d2.p, pen_by_d2, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    KC_HIP(hipStreamSynchronize(c->stream));
    c->clear_max_pen = *std::max_element(pen_by_d2, pen_by_d2 + n);
  }
  c->clear_c2 = on ? c2 : 0u;
  forget_maps(c, true, false);  // clear2 and the penalty come with the validity pass
  return KC_OK;
}

int kc_planner_get_clearance(kc_planner *c, uint16_t *clear2_out, uint32_t *penalty_out, size_t cap) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (!c->solved) KC_FAIL(KC_ERR_STATE, "kc_planner_get_clearance before kc_planner_solve");
  if (c->clear_c2 == 0) KC_FAIL(KC_ERR_STATE, "kc_planner_get_clearance with the clearance cost off");
  const size_t n = static_cast<size_t>(c->W) * static_cast<size_t>(c->H);
  if (n > cap) KC_FAIL(KC_ERR_RANGE, "%zu cells do not fit the output capacity %zu", n, cap);
  KC_HIP(hipSetDevice(c->device));
  if (clear2_out) KC_HIP(hipMemcpyAsync(clear2_out, c->d_clear2.p, n * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
  if (penalty_out) KC_HIP(hipMemcpyAsync(penalty_out, c->d_pen.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  return KC_OK;
}

int kc_planner_path_clearance(kc_planner *c, uint32_t *min_clear2_out) {
  if (!c || !min_clear2_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (!c->solved || c->explored || c->status != KC_PLAN_FOUND) KC_FAIL(KC_ERR_STATE, "kc_planner_path_clearance without a path");
  if (c->clear_c2 == 0) KC_FAIL(KC_ERR_STATE, "kc_planner_path_clearance with the clearance cost off");
  KC_TRY(planner_walk(c));
  *min_clear2_out = c->path_clear2;
  return KC_OK;
}

int kc_planner_shortcut(kc_planner *c, int max_span, size_t *count_out, uint32_t *min_clear2_out) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (count_out) *count_out = 0;
  if (!c->solved || c->explored || c->status != KC_PLAN_FOUND) KC_FAIL(KC_ERR_STATE, "kc_planner_shortcut without a path");
  if (c->or_solve) KC_FAIL(KC_ERR_STATE, "no any-angle path in oriented mode: a segment at an arbitrary angle has no class (rule 18)");
  if (c->car_solve) KC_FAIL(KC_ERR_STATE, "no any-angle path with car motion: a segment at an arbitrary angle is no primitive (rule 35)");
  if (max_span < 1 || max_span > KC_PLANNER_MAX_SPAN)
    KC_FAIL(KC_ERR_RANGE, "max_span %d is outside 1 .. %d", max_span, KC_PLANNER_MAX_SPAN);
  KC_TRY(planner_shortcut(c, max_span));
  if (count_out) *count_out = c->short_idx.size();
  if (min_clear2_out) *min_clear2_out = c->short_clear2;
  return KC_OK;
}

int kc_planner_get_shortcut(kc_planner *c, int32_t *cells_ij_out, int32_t *index_out, size_t cap, size_t *count_out) {
  if (!c || !count_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *count_out = 0;
  if (!c->solved || c->explored || c->status != KC_PLAN_FOUND || !c->have_path || !c->have_short)
    KC_FAIL(KC_ERR_STATE, "kc_planner_get_shortcut before kc_planner_shortcut");
  const size_t n = c->short_idx.size();
  *count_out = n;
  if (!cells_ij_out && !index_out) return KC_OK;  // the count alone
  if (n > cap) KC_FAIL(KC_ERR_RANGE, "%zu kept cells do not fit the output capacity %zu", n, cap);
  for (size_t k = 0; k < n; ++k) {
    const int32_t cell = c->path[static_cast<size_t>(c->short_idx[k])];
    if (cells_ij_out) {
      cells_ij_out[2 * k] = cell % c->W;
      cells_ij_out[2 * k + 1] = cell / c->W;
    }
    if (index_out) index_out[k] = c->short_idx[k];
  }
  return KC_OK;
}

int kc_planner_set_oriented(kc_planner *c, uint32_t a2, uint32_t b2, uint32_t turn10) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (a2 == 0) {
    c->or_a2 = c->or_b2 = c->or_turn10 = 0;
    forget_maps(c, false, true);
    return KC_OK;
  }
  if (c->clear_c2 > 0) KC_FAIL(KC_ERR_STATE, "the oriented footprint cannot be set while a clearance cost is on (rule 18)");
  if (c->car_turn > 0) KC_FAIL(KC_ERR_STATE, "the oriented mode cannot be set while car motion is on: kc_planner_set_car takes the box (rule 35)");
  if (turn10 < 1u || turn10 > 10000u) KC_FAIL(KC_ERR_RANGE, "turn10 = %u is outside 1 .. 10000", turn10);
  KC_TRY(check_box(a2, b2, "turning disc of T2"));
  const bool new_box = c->or_a2 != a2 || c->or_b2 != b2;
  if (new_box) KC_TRY(planner_upload_box(c, a2, b2));
  c->or_a2 = a2;
  c->or_b2 = b2;
  c->or_turn10 = turn10;
  forget_maps(c, false, new_box);  // an unchanged box keeps its masks; the oriented solve shares final_buf with the kept field
  return KC_OK;
}

int kc_planner_solve_oriented(kc_planner *c, const int start_cell[2], int start_class, const int goal_cell[2], int allow_unknown,
                              int *status_out, uint32_t *cost_out, int *passes_out) {
  if (!c || !start_cell || !goal_cell || !status_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (!c->have_grid) KC_FAIL(KC_ERR_STATE, "kc_planner_solve_oriented before a grid was set");
  if (c->car_turn > 0) KC_FAIL(KC_ERR_STATE, "kc_planner_solve_oriented with car motion on: kc_planner_solve_car");
  if (c->or_a2 == 0) KC_FAIL(KC_ERR_STATE, "kc_planner_solve_oriented before kc_planner_set_oriented");
  if (start_class < 0 || start_class > 3) KC_FAIL(KC_ERR_INVALID, "start class %d is outside 0 .. 3", start_class);
  const long long n = static_cast<long long>(c->W) * c->H;
  // field <= max(14, turn10) * (4 * cells - 1): the sums of the relaxation stay below the 0xFFFFFFFF of "nothing arrives"
  if (static_cast<unsigned long long>(std::max<uint32_t>(14u, c->or_turn10)) * 4ull * static_cast<unsigned long long>(n) > 0xFFFFFFFEull)
    KC_FAIL(KC_ERR_RANGE, "a turn cost of %u over 4 x %lld states does not fit the 32-bit field", c->or_turn10, n);
  KC_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int W = c->W, H = c->H;
  forget_solve(c, cost_out, passes_out);  // no kept field to lose: kc_planner_set_oriented dropped it
  c->or_solve = true;
  const int unknown_blocks = allow_unknown ? 0 : 1;
  KC_TRY(planner_oriented_validity(c, c->or_a2, c->or_b2, unknown_blocks));
  const long long goal = plan_cell_index(c, goal_cell);
  KC_TRY(planner_start_pair(c, c->d_field4, 4 * static_cast<size_t>(n), [&](uint32_t *a, uint32_t *b) {
    hipLaunchKernelGGL(planner_init4_kernel, dim3(plan_blocks_for(n)), dim3(kPlanBlock), 0, s, a, b, c->d_valid4.p, n, goal);
  }));
  uint32_t passes = 0;
  if (goal >= 0) {
    const auto pass4 = [&](uint32_t pass, int b) {
      hipLaunchKernelGGL(planner_relax4_kernel, dim3(c->tiles_x * c->tiles_y), dim3(kPlanThreads), 0, s, c->d_field4[b].p, c->d_field4[b ^ 1].p,
                         c->d_valid4.p, W, H, static_cast<size_t>(n), c->tiles_x, c->or_turn10, &c->d_word.p->changed, pass);
    };
    KC_TRY(planner_relax(c, pass4, 4ull * n, "state", &c->final_buf, &passes));
  }
  c->start_class = start_class;
  // the start needs its own class, the goal any (rule 16); the state field is not kept (rule 20)
  KC_TRY(planner_finish(c, start_cell, goal_cell, c->d_field4[c->final_buf].p + static_cast<size_t>(start_class) * static_cast<size_t>(n),
                        c->d_valid4.p, 1u << start_class, 15u, false, status_out, cost_out));
  if (passes_out) *passes_out = static_cast<int>(passes);
  return KC_OK;
}

int kc_planner_get_oriented_field(kc_planner *c, uint32_t *field4_out, uint8_t *valid4_out, uint8_t *turn_valid_out, size_t cap) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (!c->solved || !c->or_solve) KC_FAIL(KC_ERR_STATE, "kc_planner_get_oriented_field before kc_planner_solve_oriented");
  const size_t n = static_cast<size_t>(c->W) * static_cast<size_t>(c->H);
  if (n > cap) KC_FAIL(KC_ERR_RANGE, "%zu cells do not fit the output capacity %zu", n, cap);
  KC_HIP(hipSetDevice(c->device));
  if (field4_out)
    KC_HIP(hipMemcpyAsync(field4_out, c->d_field4[c->final_buf].p, 4 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (valid4_out) KC_HIP(hipMemcpyAsync(valid4_out, c->d_valid4.p, n, hipMemcpyDeviceToHost, c->stream));
  if (turn_valid_out) KC_HIP(hipMemcpyAsync(turn_valid_out, c->d_turn.p, n, hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  if (valid4_out)
    for (size_t i = 0; i < n; ++i) valid4_out[i] &= 15u;  // the device byte carries the turn bit beside the four classes
  return KC_OK;
}

int kc_planner_get_oriented_path(kc_planner *c, int32_t *states_ijk_out, size_t cap, size_t *count_out) {
  if (!c || !count_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *count_out = 0;
  if (!c->solved || !c->or_solve) KC_FAIL(KC_ERR_STATE, "kc_planner_get_oriented_path before kc_planner_solve_oriented");
  if (c->status != KC_PLAN_FOUND) return KC_OK;  // no path: zero states
  KC_TRY(planner_walk(c));
  *count_out = c->states.size();
  if (!states_ijk_out) return KC_OK;  // the count alone
  if (c->states.size() > cap) KC_FAIL(KC_ERR_RANGE, "%zu states do not fit the output capacity %zu", c->states.size(), cap);
  for (size_t k = 0; k < c->states.size(); ++k) {
    const int32_t cell = c->states[k] / 4;
    states_ijk_out[3 * k] = cell % c->W;
    states_ijk_out[3 * k + 1] = cell / c->W;
    states_ijk_out[3 * k + 2] = c->states[k] % 4;
  }
  return KC_OK;
}

int kc_planner_set_car(kc_planner *c, int turn_cells, uint32_t reverse_weight, uint32_t a2, uint32_t b2) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (turn_cells == 0) {
    if (c->car_turn == 0) return KC_OK;  // off already: nothing of another mode's is touched
    const bool had_box = c->car_a2 > 0;
    c->car_turn = 0;
    c->car_rw = c->car_a2 = c->car_b2 = 0;
    forget_maps(c, false, had_box);  // the box's masks leave with it; the disc's map is the disc solve's own
    return KC_OK;
  }
  if (turn_cells < 0 || turn_cells > KC_PLANNER_MAX_TURN_CELLS)
    KC_FAIL(KC_ERR_RANGE, "a turn of %d cells is outside 1 .. %d", turn_cells, KC_PLANNER_MAX_TURN_CELLS);
  if (reverse_weight > static_cast<uint32_t>(KC_PLANNER_MAX_REVERSE_WEIGHT))
    KC_FAIL(KC_ERR_RANGE, "a reverse weight of %u is outside 0 .. %d", reverse_weight, KC_PLANNER_MAX_REVERSE_WEIGHT);
  if (c->clear_c2 > 0) KC_FAIL(KC_ERR_STATE, "car motion cannot be set while a clearance cost is on (rule 35)");
  if (c->or_a2 > 0) KC_FAIL(KC_ERR_STATE, "car motion cannot be set while the oriented mode is on: hand the box to kc_planner_set_car (rule 35)");
  if (a2 == 0 && b2 != 0) KC_FAIL(KC_ERR_INVALID, "a box footprint needs a2 > 0 (a2 = b2 = 0 is the disc)");
  KC_TRY(check_box(a2, b2, "box of A2 + B2"));
  const bool new_box = c->car_turn == 0 || c->car_a2 != a2 || c->car_b2 != b2;
  if (new_box && a2 > 0) KC_TRY(planner_upload_box(c, a2, b2));
  c->car_turn = turn_cells;
  c->car_rw = reverse_weight;
  c->car_a2 = a2;
  c->car_b2 = b2;
  forget_maps(c, false, new_box);  // rule 30's bytes go in any case
  return KC_OK;
}

int kc_planner_solve_car(kc_planner *c, const int start_cell[2], int start_heading, const int goal_cell[2], int goal_heading, uint32_t r2,
                         int allow_unknown, int *status_out, uint32_t *cost_out, int *passes_out) {
  if (!c || !start_cell || !goal_cell || !status_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (!c->have_grid) KC_FAIL(KC_ERR_STATE, "kc_planner_solve_car before a grid was set");
  if (c->car_turn == 0) KC_FAIL(KC_ERR_STATE, "kc_planner_solve_car before kc_planner_set_car");
  if (start_heading < 0 || start_heading > 7) KC_FAIL(KC_ERR_INVALID, "start heading %d is outside 0 .. 7", start_heading);
  if (goal_heading < -1 || goal_heading > 7) KC_FAIL(KC_ERR_INVALID, "goal heading %d is outside -1 .. 7", goal_heading);
  const bool box = c->car_a2 > 0;
  if (!box) KC_TRY(check_radius(r2));
  const long long n = static_cast<long long>(c->W) * c->H;
  // field <= 24 n max(rw, 1) * (8 * cells - 1): the sums of the relaxation stay below the 0xFFFFFFFF of "nothing arrives",
  // and 8 * cells below the bit the walk keeps its primitive in
  if (24ull * static_cast<unsigned long long>(c->car_turn) * std::max<uint32_t>(c->car_rw, 1u) * 8ull * static_cast<unsigned long long>(n) > 0xFFFFFFFEull)
    KC_FAIL(KC_ERR_RANGE, "arcs of %d cells at reverse weight %u over 8 x %lld states do not fit the 32-bit field", c->car_turn, c->car_rw, n);
  KC_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int W = c->W, H = c->H;
  forget_solve(c, cost_out, passes_out);  // the disc's kept field goes as with any other solve
  c->car_solve = true;
  c->car_ms[0] = c->car_ms[1] = c->car_ms[2] = 0.0f;
  PlanClock clock;
  const unsigned blocks = plan_blocks_for(n);
  const int unknown_blocks = allow_unknown ? 0 : 1;
  // rule 28: the maps of the footprint in use, made by the kernels of rules 2 and 14 as they are
  if (box) {
    if (!c->or_have_valid || c->or_valid_unknown != unknown_blocks) c->car_have_moves = false;
    KC_TRY(planner_oriented_validity(c, c->car_a2, c->car_b2, unknown_blocks));
  } else if (!c->have_valid || c->valid_r2 != r2 || c->valid_unknown != unknown_blocks) {
    c->car_have_moves = false;
    KC_TRY(planner_validity(c, r2, unknown_blocks));
  }
  const uint8_t *vmap = box ? c->d_valid4.p : c->d_valid.p;
  if (!c->car_have_moves) {
    KC_TRY(c->d_steps.reserve(static_cast<size_t>(n)));
    KC_TRY(c->d_moves.reserve(8 * static_cast<size_t>(n)));
    with_bool(box, [&](auto on) {
      hipLaunchKernelGGL(planner_car_steps_kernel<decltype(on)::value>, dim3(blocks), dim3(kPlanBlock), 0, s, vmap, c->d_steps.p, W, H);
    });
    hipLaunchKernelGGL(planner_car_moves_kernel, dim3(plan_blocks_for(8 * n)), dim3(kPlanBlock), 0, s, c->d_steps.p, c->d_moves.p, W, H,
                       c->car_turn, c->car_rw > 0 ? 1 : 0);
    KC_HIP(hipGetLastError());
    c->car_have_moves = true;
  }
  const long long goal = plan_cell_index(c, goal_cell);
  KC_TRY(planner_start_pair(c, c->d_field8, 8 * static_cast<size_t>(n), [&](uint32_t *a, uint32_t *b) {
    with_bool(box, [&](auto on) {
      hipLaunchKernelGGL(planner_init8_kernel<decltype(on)::value>, dim3(blocks), dim3(kPlanBlock), 0, s, a, b, vmap, n, goal, goal_heading);
    });
  }));
  KC_HIP(hipStreamSynchronize(s));  // the maps and the moves end here, inside the first phase's clock
  c->car_ms[0] = clock.lap();
  uint32_t passes = 0;
  if (goal >= 0) {
    const auto pass8 = [&](uint32_t pass, int b) {
      hipLaunchKernelGGL(planner_relax8_kernel, dim3(8u * c->tiles_x * c->tiles_y), dim3(kPlanThreads), 0, s, c->d_field8[b].p, c->d_field8[b ^ 1].p,
                         c->d_moves.p, W, H, static_cast<size_t>(n), c->tiles_x, c->car_turn, c->car_rw, &c->d_word.p->changed, pass);
    };
    KC_TRY(planner_relax(c, pass8, 8ull * n, "car", &c->final_buf, &passes));
  }
  c->start_heading = start_heading;
  // the start needs its own heading, the goal the asked one or any (rule 32); the state field is not kept (rule 35)
  const uint32_t start_mask = box ? 1u << (start_heading & 3) : 0xFFu;
  const uint32_t goal_mask = !box ? 0xFFu : (goal_heading < 0 ? 15u : 1u << (goal_heading & 3));
  KC_TRY(planner_finish(c, start_cell, goal_cell, c->d_field8[c->final_buf].p + static_cast<size_t>(start_heading) * static_cast<size_t>(n), vmap,
                        start_mask, goal_mask, false, status_out, cost_out));
  c->car_ms[1] = clock.lap();
  if (passes_out) *passes_out = static_cast<int>(passes);
  return KC_OK;
}

int kc_planner_get_car_field(kc_planner *c, uint32_t *field8_out, uint8_t *moves8_out, uint8_t *valid_out, size_t cap) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (!c->solved || !c->car_solve) KC_FAIL(KC_ERR_STATE, "kc_planner_get_car_field before kc_planner_solve_car");
  const size_t n = static_cast<size_t>(c->W) * static_cast<size_t>(c->H);
  if (n > cap) KC_FAIL(KC_ERR_RANGE, "%zu cells do not fit the output capacity %zu", n, cap);
  KC_HIP(hipSetDevice(c->device));
  const bool box = c->car_a2 > 0;
  if (field8_out) KC_HIP(hipMemcpyAsync(field8_out, c->d_field8[c->final_buf].p, 8 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (moves8_out) KC_HIP(hipMemcpyAsync(moves8_out, c->d_moves.p, 8 * n, hipMemcpyDeviceToHost, c->stream));
  if (valid_out) KC_HIP(hipMemcpyAsync(valid_out, box ? c->d_valid4.p : c->d_valid.p, n, hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  if (valid_out)  // bit h of a cell's byte: heading h is valid there
    for (size_t i = 0; i < n; ++i) valid_out[i] = box ? static_cast<uint8_t>((valid_out[i] & 15u) * 17u) : static_cast<uint8_t>(valid_out[i] ? 0xFFu : 0u);
  return KC_OK;
}

int kc_planner_get_car_path(kc_planner *c, int32_t *states_ijh_out, int32_t *moves_out, size_t cap, size_t *count_out) {
  if (!c || !count_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *count_out = 0;
  if (!c->solved || !c->car_solve) KC_FAIL(KC_ERR_STATE, "kc_planner_get_car_path before kc_planner_solve_car");
  if (c->status != KC_PLAN_FOUND) return KC_OK;  // no path: zero states
  KC_TRY(planner_walk(c));
  const size_t m = c->car_states.size();
  *count_out = m;
  if (!states_ijh_out && !moves_out) return KC_OK;  // the count alone
  if (m > cap) KC_FAIL(KC_ERR_RANGE, "%zu states do not fit the output capacity %zu", m, cap);
  for (size_t k = 0; k < m; ++k) {
    const int32_t cell = c->car_states[k] / 8;
    if (states_ijh_out) {
      states_ijh_out[3 * k] = cell % c->W;
      states_ijh_out[3 * k + 1] = cell / c->W;
      states_ijh_out[3 * k + 2] = c->car_states[k] % 8;
    }
    if (moves_out && k + 1 < m) moves_out[k] = c->car_moves[k];
  }
  return KC_OK;
}

int kc_planner_car_info(kc_planner *c, int *turn_cells_out, uint32_t *reverse_weight_out, float phase_ms_out[3]) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (turn_cells_out) *turn_cells_out = c->car_turn;
  if (reverse_weight_out) *reverse_weight_out = c->car_rw;
  if (phase_ms_out) std::copy(c->car_ms, c->car_ms + 3, phase_ms_out);
  return KC_OK;
}

int kc_planner_explore(kc_planner *c, const int robot_cell[2], uint32_t r2, uint32_t min_cost, uint32_t min_size, int *status_out,
                       uint32_t *components_out, size_t *count_out, int *passes_out, int *label_passes_out) {
  if (!c || !robot_cell || !status_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (components_out) *components_out = 0;
  if (count_out) *count_out = 0;
  if (label_passes_out) *label_passes_out = 0;
  KC_TRY(check_radius(r2));
  if (min_size == 0) KC_FAIL(KC_ERR_RANGE, "min_size must be at least 1");
  if (!c->have_grid) KC_FAIL(KC_ERR_STATE, "kc_planner_explore before a grid was set");
  if (c->or_a2 > 0) KC_FAIL(KC_ERR_STATE, "kc_planner_explore with the oriented footprint on (rule 22)");
  if (c->clear_c2 > 0) KC_FAIL(KC_ERR_STATE, "kc_planner_explore with a clearance cost set (rule 22)");
  if (c->car_turn > 0) KC_FAIL(KC_ERR_STATE, "kc_planner_explore with car motion on (rule 35)");
  KC_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int W = c->W, H = c->H;
  const long long n = static_cast<long long>(W) * H;
  const unsigned blocks = plan_blocks_for(n), ntiles = c->tiles_x * c->tiles_y;
  PlanWords *d = c->d_word.p;
  forget_solve(c, nullptr, passes_out);
  c->ex_components = c->ex_tiles = 0;
  PlanClock clock;
  // rule 21.  d_valid then describes no (r2, unknown) of a solve: the cache says so, and forget_solve dropped the kept field
  KC_TRY(planner_validity(c, r2, 0));
  c->have_valid = false;
  hipLaunchKernelGGL(planner_known_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, c->d_cls.p, c->d_valid.p, n);
  // rule 22: rule 3's field with the robot's cell as its root
  const long long robot = plan_cell_index(c, robot_cell);
  KC_TRY(planner_start_pair(c, c->d_field, static_cast<size_t>(n), [&](uint32_t *a, uint32_t *b) {
    hipLaunchKernelGGL(planner_init_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, a, b, c->d_valid.p, n, robot);
  }));
  uint32_t passes = 0, label_passes = 0;
  if (robot >= 0) KC_TRY(planner_relax(c, disc_pass(c, nullptr, ntiles), n, "cost", &c->final_buf, &passes));
  PlanPinned *h = c->h_word.p;
  h->start_valid = 0;
  if (robot >= 0) KC_HIP(hipMemcpyAsync(&h->start_valid, c->d_valid.p + robot, 1, hipMemcpyDeviceToHost, s));
  KC_HIP(hipStreamSynchronize(s));
  c->ex_ms[0] = clock.lap();
  // rule 23, and the tiles that hold a frontier cell.  With the robot outside the grid or on a cell that is not
  // explore-valid the field is INF everywhere and nothing is marked.
  const uint32_t *field = c->d_field[c->final_buf].p;
  KC_TRY(c->d_front.reserve(static_cast<size_t>(n)));
  KC_TRY(c->d_label[0].reserve(static_cast<size_t>(n)));
  KC_TRY(c->d_label[1].reserve(static_cast<size_t>(n)));
  KC_TRY(c->d_tile_on.reserve(ntiles));
  KC_TRY(c->d_tile_list.reserve(ntiles));
  KC_HIP(hipMemsetAsync(c->d_tile_on.p, 0, ntiles, s));
  KC_HIP(hipMemsetAsync(&d->ex_listed, 0, 4 * sizeof(uint32_t), s));  // ex_listed .. ex_slots
  hipLaunchKernelGGL(planner_frontier_mark_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, c->d_cls.p, c->d_valid.p, field, min_cost, W, H,
                     static_cast<int>(c->tiles_x), c->d_front.p, c->d_label[0].p, c->d_label[1].p, c->d_tile_on.p);
  hipLaunchKernelGGL(planner_compact_kernel, dim3(plan_blocks_for(ntiles)), dim3(kPlanBlock), 0, s, c->d_tile_on.p, ntiles, c->d_tile_list.p,
                     &d->ex_listed);
  KC_HIP(hipMemsetAsync(&d->changed, 0, sizeof(uint32_t), s));
  KC_HIP(hipGetLastError());
  KC_HIP(plan_fetch_words(c, &PlanWords::ex_listed, 1));
  KC_HIP(hipStreamSynchronize(s));  // whatever is listed: the mark kernel has ended here, inside the second phase's clock
  const uint32_t listed = h->w.ex_listed;
  if (listed > ntiles) KC_FAIL(KC_ERR_STATE, "%u tiles listed of %u", listed, ntiles);
  c->label_buf = 0;  // both planes hold the initial labels
  if (listed) {
    // rule 24 over the listed tiles, to the fixed point
    const auto label_pass = [&](uint32_t pass, int b) {
      hipLaunchKernelGGL(planner_label_kernel, dim3(listed), dim3(kPlanThreads), 0, s, c->d_label[b].p, c->d_label[b ^ 1].p, W, H, c->tiles_x,
                         c->d_tile_list.p, &d->changed, pass);
    };
    KC_TRY(planner_relax(c, label_pass, n, "label", &c->label_buf, &label_passes));
  }
  c->ex_ms[1] = clock.lap();
  uint32_t components = 0, kept = 0;
  if (listed) {
    // rule 24's sizes at the roots, in the plane the labels no longer need (both hold the fixed point), then the two counts
    const uint32_t *label = c->d_label[c->label_buf].p;
    uint32_t *size = c->d_label[c->label_buf ^ 1].p;
    KC_HIP(hipMemsetAsync(size, 0, static_cast<size_t>(n) * sizeof(uint32_t), s));
    hipLaunchKernelGGL(planner_frontier_size_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, label, size, n);
    hipLaunchKernelGGL(planner_frontier_count_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, label, size, n, min_size, &d->ex_components);
    KC_HIP(hipGetLastError());
    KC_HIP(plan_fetch_words(c, &PlanWords::ex_components, 2));
    KC_HIP(hipStreamSynchronize(s));
    components = h->w.ex_components;
    kept = h->w.ex_kept;
    if (kept > components || components > static_cast<unsigned long long>(n)) KC_FAIL(KC_ERR_STATE, "%u of %u components kept on %lld cells", kept, components, n);
    if (kept) {
      // rule 25: as many records as are kept, not one a cell
      KC_TRY(c->d_rec.reserve(kept));
      KC_TRY(c->h_rec.reserve(kept));
      hipLaunchKernelGGL(planner_frontier_slot_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, label, size, n, min_size, c->d_rec.p, &d->ex_slots);
      hipLaunchKernelGGL(planner_frontier_record_kernel, dim3(blocks), dim3(kPlanBlock), 0, s, label, size, field, W, n, c->d_rec.p);
      KC_HIP(hipGetLastError());
      KC_HIP(hipMemcpyAsync(c->h_rec.p, c->d_rec.p, kept * sizeof(PlanFrontierRec), hipMemcpyDeviceToHost, s));
      KC_HIP(hipStreamSynchronize(s));
      std::sort(c->h_rec.p, c->h_rec.p + kept, [](const PlanFrontierRec &a, const PlanFrontierRec &b) { return a.key < b.key; });
      c->frontiers.reserve(kept);
      for (uint32_t k = 0; k < kept; ++k) {
        const PlanFrontierRec &r = c->h_rec.p[k];
        const uint32_t entry = static_cast<uint32_t>(r.key & 0xFFFFFFFFull);
        kc_planner_frontier f = {};
        f.sum_i = r.sum_i;
        f.sum_j = r.sum_j;
        f.size = r.size;
        f.root = r.root;
        f.cost = static_cast<uint32_t>(r.key >> 32);
        f.entry_i = static_cast<int32_t>(entry % static_cast<uint32_t>(W));
        f.entry_j = static_cast<int32_t>(entry / static_cast<uint32_t>(W));
        c->frontiers.push_back(f);
      }
    }
  }
  c->ex_ms[2] = clock.lap();
  int st = kept ? KC_PLAN_FOUND : KC_PLAN_NO_FRONTIER;
  if (robot < 0) st = KC_PLAN_START_OUTSIDE;
  else if (!h->start_valid) st = KC_PLAN_START_INVALID;
  c->solved = c->explored = true;
  c->start[0] = robot_cell[0];
  c->start[1] = robot_cell[1];
  c->status = st;
  c->ex_components = components;
  c->ex_tiles = listed;
  *status_out = st;
  if (components_out) *components_out = components;
  if (count_out) *count_out = kept;
  if (passes_out) *passes_out = static_cast<int>(passes);
  if (label_passes_out) *label_passes_out = static_cast<int>(label_passes);
  return KC_OK;
}

int kc_planner_explore_info(kc_planner *c, uint32_t *listed_tiles_out, uint32_t *tiles_out, float phase_ms_out[3]) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (!c->explored) KC_FAIL(KC_ERR_STATE, "kc_planner_explore_info unless the last solve-type call was kc_planner_explore");
  if (listed_tiles_out) *listed_tiles_out = c->ex_tiles;
  if (tiles_out) *tiles_out = c->tiles_x * c->tiles_y;
  if (phase_ms_out) std::copy(c->ex_ms, c->ex_ms + 3, phase_ms_out);
  return KC_OK;
}

int kc_planner_get_frontiers(kc_planner *c, kc_planner_frontier *out, size_t cap, size_t *count_out) {
  if (!c || !count_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *count_out = 0;
  if (!c->explored) KC_FAIL(KC_ERR_STATE, "kc_planner_get_frontiers unless the last solve-type call was kc_planner_explore");
  *count_out = c->frontiers.size();
  if (!out) return KC_OK;  // the count alone
  if (c->frontiers.size() > cap) KC_FAIL(KC_ERR_RANGE, "%zu frontiers do not fit the output capacity %zu", c->frontiers.size(), cap);
  std::copy(c->frontiers.begin(), c->frontiers.end(), out);
  return KC_OK;
}

int kc_planner_get_frontier_path(kc_planner *c, size_t k, int32_t *cells_ij_out, size_t cap, size_t *count_out) {
  if (!c || !count_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *count_out = 0;
  if (!c->explored) KC_FAIL(KC_ERR_STATE, "kc_planner_get_frontier_path unless the last solve-type call was kc_planner_explore");
  if (k >= c->frontiers.size()) KC_FAIL(KC_ERR_RANGE, "frontier %zu of %zu", k, c->frontiers.size());
  const kc_planner_frontier &f = c->frontiers[k];
  // rule 26: every step of the walk lowers the field by its own 10 or 14
  const size_t cells = static_cast<size_t>(f.cost / 10u) + 2;
  KC_HIP(hipSetDevice(c->device));
  KC_TRY(c->d_path.reserve(cells));
  KC_TRY(c->h_path.reserve(cells));
  hipLaunchKernelGGL((planner_walk_kernel<false, true>), dim3(1), dim3(64), 0, c->stream, c->d_field[c->final_buf].p, c->d_valid.p, nullptr, nullptr,
                     c->W, c->H, f.entry_i, f.entry_j, c->d_path.p, static_cast<uint32_t>(cells), &c->d_word.p->walk_count);
  uint32_t count = 0;
  KC_TRY(planner_walk_fetch(c, cells, false, "frontier", "cells", &count));
  *count_out = count;
  if (!cells_ij_out) return KC_OK;  // the count alone
  if (count > cap) KC_FAIL(KC_ERR_RANGE, "%u path cells do not fit the output capacity %zu", count, cap);
  for (uint32_t q = 0; q < count; ++q) {  // the walk ends at the robot's cell: handed out reversed
    const int32_t cell = c->h_path.p[count - 1 - q];
    cells_ij_out[2 * q] = cell % c->W;
    cells_ij_out[2 * q + 1] = cell / c->W;
  }
  return KC_OK;
}

int kc_planner_get_frontier_labels(kc_planner *c, uint32_t *labels_out, size_t cap) {
  if (!c || !labels_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (!c->explored) KC_FAIL(KC_ERR_STATE, "kc_planner_get_frontier_labels unless the last solve-type call was kc_planner_explore");
  const size_t n = static_cast<size_t>(c->W) * static_cast<size_t>(c->H);
  if (n > cap) KC_FAIL(KC_ERR_RANGE, "%zu cells do not fit the output capacity %zu", n, cap);
  KC_HIP(hipSetDevice(c->device));
  KC_HIP(hipMemcpyAsync(labels_out, c->d_label[c->label_buf].p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  return KC_OK;
}

}  // extern "C"
