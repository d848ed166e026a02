// World map on gfx950: a world-frame occupancy map that stays on the device, fused from the LocalMapper's
// egocentric grids.  Integer work only; the one place a float is read is the pose quantisation
// on the host, once per update.
//
// The reference has no counterpart: it leaves this layer to its ROS side.  The yardstick is the numpy statement
// of the rule in tests/worldmap_ref.py, bit for bit.
//
//  (a) state.  Two dense int8 planes of W x H cells, cell (I, J) at I + J * W: `evidence` (-128 = never observed,
//      else e_min .. e_max) and `cls` (KC_UNEXPLORED / KC_EMPTY / KC_OCCUPIED), the plane the planner reads in place.
//  (b) update.  worldmap_update_kernel is a gather over the clipped bounding box of the rotated local window: one
//      lane a world cell, 64 lanes along I (one wavefront is 64 consecutive bytes of a row), four rows a workgroup.
//      A lane maps its cell into the local grid by rules 3 and 4, reads at most one local cell and, for an
//      observation of 0 or 100, stores its own two bytes.  BYTE STORES, on purpose: W need not be a multiple of 4,
//      so the dword that holds a row's last cells can hold the next row's first ones, and a box as wide as the map
//      would have two lanes write one dword.  A lane that stores only its own bytes cannot meet another.
//      The box is a launch bound, not part of the rule: every lane runs the full test of rule 4.
//  (c) result record.  A wavefront counts its class changes by ballot + popcount and adds them with one atomic;
//      lanes that changed their class fold their cell into the box by atomic min / max (the wavefront's extremes,
//      one lane each).  Two records alternate (FlipRecord, kc_internal.h): update n accumulates into record n & 1 and puts record (n + 1) & 1
//      back to its start values, which no lane of this launch reads, so an update is one launch plus the read-back
//      of five words.
//  (d) prior / clear.  worldmap_prior_kernel owns dwords by flat index (the planes start at an allocation, so cells
//      4 t .. 4 t + 3 are one aligned dword, whatever W is); the cells behind the last whole dword go as bytes.
//
//  (e) match (rules 9 to 15).  Four launches on the context's stream and one read-back, the map untouched:
//      worldmap_weight_kernel turns the nine cls bytes around every cell of a square scratch plane into one weight
//      byte (rule 12), zeroes the score table and the point counter; worldmap_points_kernel compacts the occupied
//      local cells into packed (a, b) pairs; worldmap_score_kernel is one workgroup per (rotation, share of the point
//      chunks) that keeps its candidates' sums in registers and adds them into the table with one uint32 atomic per
//      candidate; worldmap_pick_kernel folds the table under rule 14 into the record.
//      The plane is centred on (TX >> 16, TY >> 16) and is NOT clipped to the map: cells outside hold 0, so the
//      score loop has no bounds test.  Its half side only has to be large enough (wm_match_half has the argument);
//      every weight is computed from the cls plane with the map's own bounds, so the box never decides one.
//      uint32 adds commute: the table does not depend on the order the workgroups arrive in.
//
//  (f) obstacle list (rules 16 to 19).  worldmap_window_points_kernel (the match's worldmap_points_kernel has the
//      shorter name already) runs over the bounding box of the disc clipped to the map, in the update kernel's
//      layout: 64 lanes along I, so a wavefront loads consecutive bytes of one cls row, four rows a workgroup.
//      Compaction as grid_points_kernel does it (kc_sensor_kernels.h): ballot + popcount in the wavefront, hits and
//      the four index bounds gathered in LDS, one slot range and four bound atomics per workgroup that holds a hit,
//      the five counters a 64-byte line each.  Counts and min / max commute: only the list's order depends on the
//      order of arrival, and rule 19 leaves that open.  The launcher (kc_internal.h) queues it on a caller's stream
//      into a caller's buffers, which is how the controller's translation unit reaches it.
//
//  (h) distance plane (rules 42 and 43; off by default).  dist2, a uint16 a cell: the squared distance in cells to the
//      nearest blocking cell within `reach`.  Kept lazily behind a dirty box on the host: prior / clear mark the whole
//      map, an update merges the changed box of the record it reads back anyway.  A refresh recomputes the box grown
//      by reach: worldmap_dist_tile_kernel up to reach 63 (a workgroup a 64 x 64 tile; the tile and its halo once into
//      LDS as blocking bytes, row distances and the column pass out of LDS, a uint16 store a lane), above it
//      worldmap_dist_rows_kernel + worldmap_dist_cols_kernel over a uint8 scratch plane, in the planner's manner.
//
//  (i) rolling window (rules 46 to 49).  worldmap_shift_kernel moves both planes by whole cells into two scratch planes
//      the context keeps from its first shift on: a lane a destination cell in the update kernel's layout, a byte load
//      (or the never-observed pair where the source cell lies outside the map) and a byte store a plane.  NOT in place: a
//      workgroup must never read a cell another has already overwritten.  Two device-to-device copies on the context's
//      stream bring the planes back to where they were, so every pointer handed out stays valid.  The origin is never
//      summed from shift to shift: it is ox0 + (double)OI * (double)res whenever it is asked for.
//
//  (j) scan integration (rules 52 to 57).  The one way into the map that does not go through a local grid: a measured
//      scan's beams are walked through the world by rule 23 and leave MISS / HIT bits in a mark plane of a byte a cell
//      (worldmap_mark_kernel: consecutive beams on consecutive lanes, a beam's walk shared among lanes in segments that
//      are entered by a closed form, an atomic OR on the aligned dword); worldmap_integrate_apply_kernel then runs over the walk's box in the update kernel's
//      layout, turns a mark byte into one observation (a hit beats a miss), puts the byte back to zero and applies
//      rule 5 with the update's record.  OR commutes and a cell is applied once: no thread order takes part.
//
//  (k) movers (rules 64 to 70).  The map read and never written: worldmap_movers_flag_kernel (a lane a beam) forms rule
//      44's endpoint and tests rule 66 against the cls and dist2 planes; worldmap_movers_cluster_kernel (one workgroup of
//      1024 lanes, consecutive beams a lane) compacts the dynamic beams, runs rule 67's head test and numbers runs and
//      kept clusters by prefix counts, then a wavefront a returned cluster sums its endpoints.  Integer sums, minima and
//      maxima: no thread order takes part.  Record, clusters and labels leave in one copy.
//
// Plain vector loads and stores only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "kc_internal.h"
#include "kompass_hip.h"
#include "kc_worldmap_walk.h"

namespace kc {

constexpr int kWmLanes = 64;               // cells along I per workgroup: one wavefront a row segment
constexpr int kWmRows = 4;                 // rows per workgroup
constexpr int kWmBlock = 256;
constexpr int kWmMaxBlocks = 2048;
constexpr int8_t kWmNever = -128;
constexpr int kWmMaxSide = 32768;
constexpr int kWmRecWords = 5;             // changed, i_min, j_min, i_max, j_max

struct WmModel {
  int hit, miss, e_min, e_max, occ_thr;
};

struct WmUpdateArgs {
  const int32_t *local;   // [gh x gw] column-major: (i, j) at i + j * gh
  int8_t *evidence, *cls;
  int *rec, *rec_next;    // this update's record, and the one to put back for the next
  long long tx, ty;
  int cq, sq;
  int W;
  int gh, gw, c0, c1;
  int i_lo, j_lo, i_hi, j_hi;  // the launch box, inclusive, inside the map
  WmModel m;
};

__device__ __forceinline__ int8_t wm_class(int e, int occ_thr) {
  return static_cast<int8_t>(e >= occ_thr ? KC_OCCUPIED : KC_EMPTY);
}

__global__ __launch_bounds__(kWmBlock) void worldmap_update_kernel(WmUpdateArgs a) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) {
    a.rec_next[0] = 0;
    a.rec_next[1] = INT_MAX;
    a.rec_next[2] = INT_MAX;
    a.rec_next[3] = -1;
    a.rec_next[4] = -1;
  }
  const int I = a.i_lo + static_cast<int>(blockIdx.x) * kWmLanes + static_cast<int>(threadIdx.x);
  const int J = a.j_lo + static_cast<int>(blockIdx.y) * kWmRows + static_cast<int>(threadIdx.y);
  bool changed = false;
  if (I <= a.i_hi && J <= a.j_hi) {
    const long long dx = (static_cast<long long>(I) << 16) - a.tx;
    const long long dy = (static_cast<long long>(J) << 16) - a.ty;
    const long long cq = a.cq, sq = a.sq;
    const long long li = a.c0 + ((cq * dx + sq * dy + (1ll << 31)) >> 32);
    const long long lj = a.c1 + ((cq * dy - sq * dx + (1ll << 31)) >> 32);
    if (li >= 0 && li < a.gh && lj >= 0 && lj < a.gw) {
      const int obs = a.local[li + lj * a.gh];
      if (obs == KC_OCCUPIED || obs == KC_EMPTY) {
        const size_t cell = static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(a.W);
        const int old = a.evidence[cell];
        const int base = old == kWmNever ? 0 : old;
        const int e = obs == KC_OCCUPIED ? min(base + a.m.hit, a.m.e_max) : max(base - a.m.miss, a.m.e_min);
        const int8_t k = wm_class(e, a.m.occ_thr);
        changed = a.cls[cell] != k;
        if (e != old) a.evidence[cell] = static_cast<int8_t>(e);
        if (changed) a.cls[cell] = k;
      }
    }
  }
  // one wavefront is one row segment (blockDim.x == 64): J is uniform in it
  const unsigned long long mask = __ballot(changed);
  if (mask == 0) return;
  const int lane = static_cast<int>(threadIdx.x);
  const int first = __ffsll(mask) - 1, last = 63 - __clzll(mask);
  if (lane == first) {
    atomicAdd(reinterpret_cast<unsigned int *>(&a.rec[0]), static_cast<unsigned int>(__popcll(mask)));
    atomicMin(&a.rec[1], I);
    atomicMin(&a.rec[2], J);
    atomicMax(&a.rec[4], J);
  }
  if (lane == last) atomicMax(&a.rec[3], I);
}

// grid == nullptr: clear.  Otherwise rule 8: 100 -> e_max, 0 -> e_min, anything else never observed.
template <typename T>
__device__ __forceinline__ void wm_prior_cell(const T *grid, long long k, WmModel m, int *e_out, int *c_out) {
  int e = kWmNever, c = KC_UNEXPLORED;
  if (grid) {
    const int v = static_cast<int>(grid[k]);
    if (v == KC_OCCUPIED) e = m.e_max;
    else if (v == KC_EMPTY) e = m.e_min;
    if (e != kWmNever) c = wm_class(e, m.occ_thr);
  }
  *e_out = e;
  *c_out = c;
}

template <typename T>
__global__ __launch_bounds__(kWmBlock) void worldmap_prior_kernel(const T *grid, int8_t *evidence, int8_t *cls, long long n,
                                                                  WmModel m) {
  const long long quads = n / 4, stride = static_cast<long long>(gridDim.x) * kWmBlock;
  const long long t0 = static_cast<long long>(blockIdx.x) * kWmBlock + threadIdx.x;
  for (long long q = t0; q < quads; q += stride) {
    unsigned int ew = 0, cw = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      int e, c;
      wm_prior_cell(grid, 4 * q + b, m, &e, &c);
      ew |= static_cast<unsigned int>(e & 0xFF) << (8 * b);
      cw |= static_cast<unsigned int>(c & 0xFF) << (8 * b);
    }
    reinterpret_cast<unsigned int *>(evidence)[q] = ew;
    reinterpret_cast<unsigned int *>(cls)[q] = cw;
  }
  const long long k = 4 * quads + t0;  // the up to three cells behind the last whole dword
  if (k < n) {
    int e, c;
    wm_prior_cell(grid, k, m, &e, &c);
    evidence[k] = static_cast<int8_t>(e);
    cls[k] = static_cast<int8_t>(c);
  }
}

// ---- rolling window (rules 46 to 49) -----------------------------------------------------------------------------
constexpr int kWmMaxShift = 1 << 30;  // rule 46's cap on |OI| and |OJ|

struct WmShiftArgs {
  const int8_t *evidence, *cls;
  int8_t *evidence_out, *cls_out;  // the scratch planes: never the planes read
  int W, H;
  int di, dj;                      // |di| < W and |dj| < H: the host turns anything larger into a clear
};

// rule 47: P'[I, J] = P[I + di, J + dj] where that cell lies inside the map, never observed elsewhere
__global__ __launch_bounds__(kWmBlock) void worldmap_shift_kernel(WmShiftArgs a) {
  const int I = static_cast<int>(blockIdx.x) * kWmLanes + static_cast<int>(threadIdx.x);
  const int J = static_cast<int>(blockIdx.y) * kWmRows + static_cast<int>(threadIdx.y);
  if (I >= a.W || J >= a.H) return;
  const int si = I + a.di, sj = J + a.dj;
  int8_t e = kWmNever, k = static_cast<int8_t>(KC_UNEXPLORED);
  if (si >= 0 && si < a.W && sj >= 0 && sj < a.H) {
    const size_t src = static_cast<size_t>(si) + static_cast<size_t>(sj) * static_cast<size_t>(a.W);
    e = a.evidence[src];
    k = a.cls[src];
  }
  const size_t cell = static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(a.W);
  a.evidence_out[cell] = e;
  a.cls_out[cell] = k;
}

// ---- match (rules 9 to 15) ---------------------------------------------------------------------------------------
constexpr int kWmMatchMaxYaw = KC_WORLDMAP_MATCH_MAX_YAW, kWmMatchMaxReach = KC_WORLDMAP_MATCH_MAX_REACH;
constexpr int kWmMatchMaxSide = KC_WORLDMAP_MATCH_MAX_SIDE;
constexpr int kWmMatchRot = 2 * kWmMatchMaxYaw + 1;
constexpr int kWmChunk = 256;        // points formed into LDS at a time: one a lane
constexpr int kWmCandPerLane = 16;   // ceil(63 * 63 / 256)
constexpr int kWmChunkBlocks = 32;   // workgroups that share one rotation's chunks
constexpr int kWmPickBlock = 1024;
constexpr int kWmMatchRecWords = 6;  // k, u, v, score, score_guess, n_points

struct WmWeightArgs {
  const int8_t *cls;
  uint8_t *plane;
  uint32_t *table;
  uint32_t *n_points;
  long long plane_cells, table_cells;
  int W, H;
  int i0, j0;  // the world cell of plane cell (0, 0)
  int P;       // the plane's side
};

__device__ __forceinline__ bool wm_occ(const int8_t *cls, int W, int H, int I, int J) {
  return I >= 0 && I < W && J >= 0 && J < H && cls[static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(W)] == KC_OCCUPIED;
}

// rule 12, one lane a plane cell; the same lanes zero the table of the match that follows
__global__ __launch_bounds__(kWmBlock) void worldmap_weight_kernel(WmWeightArgs a) {
  const long long stride = static_cast<long long>(gridDim.x) * kWmBlock;
  const long long t0 = static_cast<long long>(blockIdx.x) * kWmBlock + threadIdx.x;
  if (t0 == 0) *a.n_points = 0;
  for (long long t = t0; t < a.table_cells; t += stride) a.table[t] = 0;
  for (long long t = t0; t < a.plane_cells; t += stride) {
    const int I = a.i0 + static_cast<int>(t % a.P), J = a.j0 + static_cast<int>(t / a.P);
    int w = 0;
    if (I >= 0 && I < a.W && J >= 0 && J < a.H) {  // a cell outside the map has weight 0
      if (wm_occ(a.cls, a.W, a.H, I, J)) w = 3;
      else if (wm_occ(a.cls, a.W, a.H, I - 1, J) || wm_occ(a.cls, a.W, a.H, I + 1, J) || wm_occ(a.cls, a.W, a.H, I, J - 1) ||
               wm_occ(a.cls, a.W, a.H, I, J + 1))
        w = 2;
      else if (wm_occ(a.cls, a.W, a.H, I - 1, J - 1) || wm_occ(a.cls, a.W, a.H, I + 1, J - 1) ||
               wm_occ(a.cls, a.W, a.H, I - 1, J + 1) || wm_occ(a.cls, a.W, a.H, I + 1, J + 1))
        w = 1;
    }
    a.plane[t] = static_cast<uint8_t>(w);
  }
}

// rule 9: the occupied local cells as (a & 0xFFFF) | (b << 16), in any order.  A wavefront reserves its slots with one
// atomic; points[] holds gh * gw words, so no count can overrun it.
__global__ __launch_bounds__(kWmBlock) void worldmap_points_kernel(const int32_t *local, long long cells, int gh, int c0, int c1,
                                                                   uint32_t *points, uint32_t *n_points) {
  const long long stride = static_cast<long long>(gridDim.x) * kWmBlock;
  const long long rounds = (cells + stride - 1) / stride;  // every lane of a wavefront makes every round: the ballot is whole
  long long t = static_cast<long long>(blockIdx.x) * kWmBlock + threadIdx.x;
  const int lane = static_cast<int>(threadIdx.x) & 63;
  for (long long r = 0; r < rounds; ++r, t += stride) {
    const bool occ = t < cells && local[t] == KC_OCCUPIED;
    const unsigned long long mask = __ballot(occ);
    if (mask == 0) continue;
    const int leader = __ffsll(mask) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(n_points, static_cast<uint32_t>(__popcll(mask)));
    base = __shfl(base, leader);
    if (occ) {
      const int pa = static_cast<int>(t % gh) - c0, pb = static_cast<int>(t / gh) - c1;
      points[base + __popcll(mask & ((1ull << lane) - 1ull))] =
          (static_cast<uint32_t>(pa) & 0xFFFFu) | (static_cast<uint32_t>(pb) << 16);
    }
  }
}

struct WmScoreArgs {
  const uint8_t *plane;
  const uint32_t *points, *n_points;
  uint32_t *table;
  long long tx, ty;
  int i0, j0, P;  // the plane: world cell of its cell (0, 0), side
  int S, T, ncand;
  kc_worldmap_rotation rot[kWmMatchRot];
};

// rules 11 and 13.  blockIdx.y: the rotation; blockIdx.x: which of the chunks of kWmChunk points.  Candidate q = (v + S)
// T + (u + S) belongs to lane q % 256, so consecutive lanes read consecutive bytes of a patch row.  M: candidates a lane.
template <int M>
__global__ __launch_bounds__(kWmBlock) void worldmap_score_kernel(WmScoreArgs a) {
  __shared__ int s_base[kWmChunk];
  const int lane = static_cast<int>(threadIdx.x);
  const long long n = *a.n_points;
  const long long cq = a.rot[blockIdx.y].cq, sq = a.rot[blockIdx.y].sq;
  int off[M];
  uint32_t acc[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int q = lane + m * kWmBlock;
    off[m] = q < a.ncand ? (q % a.T) + (q / a.T) * a.P : 0;  // a lane's spare slots read the patch's corner and are dropped
    acc[m] = 0;
  }
  for (long long first = static_cast<long long>(blockIdx.x) * kWmChunk; first < n; first += static_cast<long long>(gridDim.x) * kWmChunk) {
    const int count = static_cast<int>(min(static_cast<long long>(kWmChunk), n - first));
    if (lane < count) {
      const uint32_t w = a.points[first + lane];
      const long long pa = static_cast<int16_t>(w & 0xFFFFu), pb = static_cast<int16_t>(w >> 16);
      const long long X = a.tx + cq * pa - sq * pb, Y = a.ty + sq * pa + cq * pb;
      const int I0 = static_cast<int>((X + (1ll << 15)) >> 16), J0 = static_cast<int>((Y + (1ll << 15)) >> 16);
      s_base[lane] = (I0 - a.S - a.i0) + (J0 - a.S - a.j0) * a.P;  // the patch's corner (u, v) = (-S, -S) in the plane
    }
    __syncthreads();
    for (int p = 0; p < count; ++p) {
      const uint8_t *row = a.plane + s_base[p];
#pragma unroll
      for (int m = 0; m < M; ++m) acc[m] += row[off[m]];
    }
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const int q = lane + m * kWmBlock;
    if (q < a.ncand && acc[m] != 0) atomicAdd(&a.table[static_cast<size_t>(blockIdx.y) * a.ncand + q], acc[m]);
  }
}

// rule 14 as one 64-bit max: score above 29 bits of (2^29 - 1 - tie), tie = (u u + v v, rank of k, v + S, u + S) in
// 11 + 6 + 6 + 6 bits, rank 0, 1, 2, 3, 4 .. for k = 0, -1, 1, -2, 2 .. (that is the order (|k|, k)).
__global__ __launch_bounds__(kWmPickBlock) void worldmap_pick_kernel(const uint32_t *table, const uint32_t *n_points, int K, int S,
                                                                      int *rec) {
  __shared__ unsigned long long s_key[kWmPickBlock];
  const int T = 2 * S + 1, ncand = T * T, total = (2 * K + 1) * ncand;
  unsigned long long best = 0;
  for (int e = static_cast<int>(threadIdx.x); e < total; e += kWmPickBlock) {
    const int k = e / ncand - K, q = e % ncand, v = q / T - S, u = q % T - S;
    const unsigned rank = k < 0 ? static_cast<unsigned>(-2 * k - 1) : static_cast<unsigned>(2 * k);
    const unsigned tie = (((static_cast<unsigned>(u * u + v * v) << 6 | rank) << 6 | static_cast<unsigned>(v + S)) << 6) |
                         static_cast<unsigned>(u + S);
    const unsigned long long key = (static_cast<unsigned long long>(table[e]) << 29) | (0x1FFFFFFFu - tie);
    best = key > best ? key : best;
  }
  s_key[threadIdx.x] = best;
  __syncthreads();
  for (int h = kWmPickBlock / 2; h > 0; h >>= 1) {
    if (static_cast<int>(threadIdx.x) < h && s_key[threadIdx.x + h] > s_key[threadIdx.x]) s_key[threadIdx.x] = s_key[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const unsigned tie = 0x1FFFFFFFu - static_cast<unsigned>(s_key[0] & 0x1FFFFFFFull);
    const unsigned rank = (tie >> 12) & 63u;
    rec[0] = rank & 1u ? -static_cast<int>((rank + 1) / 2) : static_cast<int>(rank / 2);
    rec[1] = static_cast<int>(tie & 63u) - S;
    rec[2] = static_cast<int>((tie >> 6) & 63u) - S;
    rec[3] = static_cast<int>(static_cast<uint32_t>(s_key[0] >> 29));
    rec[4] = static_cast<int>(table[static_cast<size_t>(K) * ncand + S * T + S]);
    rec[5] = static_cast<int>(*n_points);
  }
}

// ---- obstacle list (rules 16 to 19) ------------------------------------------------------------------------------
constexpr int kWmPtsStride = 16;           // words between two counters: one 64-byte line each (kGridCntStride)
constexpr int kWmPtsMaxRadius = 2048;      // rule 16's cap on Rc

struct WmWindowArgs {
  const int8_t *cls;
  float *xyz;            // [n][3]; nullptr: count and bounds only
  unsigned int *cnt;     // count, then (as int) i_min, i_max, j_min, j_max at kWmPtsStride words each
  unsigned int *rearm;   // a second counter block to put back to its start values, or nullptr
  int W;
  int i_lo, j_lo, i_hi, j_hi;  // the launch box, inclusive, inside the map
  int ic, jc;
  long long r2;
  double res, ox, oy;
};

__global__ __launch_bounds__(kWmBlock) void worldmap_window_points_kernel(WmWindowArgs a) {
  __shared__ unsigned int s_hits, s_base;
  __shared__ int s_lo_i, s_hi_i, s_lo_j, s_hi_j;
  const bool first_thread = threadIdx.x == 0 && threadIdx.y == 0;
  if (first_thread) {
    s_hits = 0u;
    s_lo_i = INT_MAX;
    s_hi_i = INT_MIN;
    s_lo_j = INT_MAX;
    s_hi_j = INT_MIN;
    if (a.rearm && blockIdx.x == 0 && blockIdx.y == 0) {  // no lane of this launch reads it
      int *r = reinterpret_cast<int *>(a.rearm);
      a.rearm[0] = 0u;
      r[1 * kWmPtsStride] = INT_MAX;
      r[2 * kWmPtsStride] = INT_MIN;
      r[3 * kWmPtsStride] = INT_MAX;
      r[4 * kWmPtsStride] = INT_MIN;
    }
  }
  __syncthreads();
  const int I = a.i_lo + static_cast<int>(blockIdx.x) * kWmLanes + static_cast<int>(threadIdx.x);
  const int J = a.j_lo + static_cast<int>(blockIdx.y) * kWmRows + static_cast<int>(threadIdx.y);
  bool hit = false;
  if (I <= a.i_hi && J <= a.j_hi) {  // the box is a launch bound inside the map; rule 17's disc is tested in full
    const long long di = static_cast<long long>(I) - a.ic, dj = static_cast<long long>(J) - a.jc;
    if (di * di + dj * dj <= a.r2)
      hit = a.cls[static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(a.W)] == KC_OCCUPIED;
  }
  // one wavefront is one row segment (blockDim.x == 64): J is uniform in it, I ascends with the lane
  const unsigned long long mask = __ballot(hit);
  const int lane = static_cast<int>(threadIdx.x);
  unsigned int rank = 0;
  if (mask != 0ull) {
    const int first = __ffsll(mask) - 1, last = 63 - __clzll(mask);
    unsigned int wbase = 0;
    if (lane == first) {
      wbase = atomicAdd(&s_hits, static_cast<unsigned int>(__popcll(mask)));
      atomicMin(&s_lo_i, I);
      atomicMin(&s_lo_j, J);
      atomicMax(&s_hi_j, J);
    }
    if (lane == last) atomicMax(&s_hi_i, I);
    wbase = __shfl(wbase, first, 64);
    rank = wbase + static_cast<unsigned int>(__popcll(mask & ((1ull << lane) - 1ull)));
  }
  __syncthreads();
  if (s_hits == 0u) return;
  if (first_thread) {
    s_base = atomicAdd(&a.cnt[0], s_hits);
    int *b = reinterpret_cast<int *>(a.cnt);
    atomicMin(&b[1 * kWmPtsStride], s_lo_i);
    atomicMax(&b[2 * kWmPtsStride], s_hi_i);
    atomicMin(&b[3 * kWmPtsStride], s_lo_j);
    atomicMax(&b[4 * kWmPtsStride], s_hi_j);
  }
  __syncthreads();
  if (hit && a.xyz) {
    const size_t slot = static_cast<size_t>(s_base) + rank;
    a.xyz[3 * slot] = worldmap_cell_coord(a.ox, I, a.res);
    a.xyz[3 * slot + 1] = worldmap_cell_coord(a.oy, J, a.res);
    a.xyz[3 * slot + 2] = 0.0f;
  }
}

// ---- virtual laser scan (rules 20 to 27) -------------------------------------------------------------------------
constexpr int kWmScanBlock = 256;          // beams a workgroup
constexpr size_t kWmScanMaxBeams = 65536;
constexpr size_t kWmScanMaxRays = size_t{1} << 22;

struct WmScanArgs {
  const int8_t *cls;
  const int2 *table;              // rule 21: (ac, as) a beam
  const kc_worldmap_pose *poses;  // a batch on the device; nullptr: pose
  kc_worldmap_pose pose;
  const double *real;             // rule 27, or nullptr
  double *ranges;
  int32_t *cells;                 // or nullptr
  int W, H, B, rc, unknown_blocks;
  double res, range_max;
};

// rule 24: e * 16384 is exact (e < 2^28), then one division and one product
__device__ __forceinline__ double wm_scan_range(int e, int a, double res) {
  return (static_cast<double>(e) * 16384.0 / static_cast<double>(a)) * res;
}

// blockIdx.x: the pose; blockIdx.y * 256 + threadIdx.x: the beam.  The walk is wm_walk (kc_worldmap_walk.h), which the
// Monte-Carlo localiser shares; it is given up between rounds once the last step's own r is above range_max: r never
// decreases along a walk (rule 24), so no later cell could count, and the output is that of the full box.
__global__ __launch_bounds__(kWmScanBlock) void worldmap_scan_kernel(WmScanArgs a) {
  const int k = static_cast<int>(blockIdx.y) * kWmScanBlock + static_cast<int>(threadIdx.x);
  if (k >= a.B) return;
  const kc_worldmap_pose p = a.poses ? a.poses[blockIdx.x] : a.pose;
  WmWalkHit h{0, 1, 0, 0};
  const bool blocked = wm_walk(a.cls, a.W, a.H, a.rc, a.unknown_blocks, p, a.table[k],
                               [&](int e, int ax) { return wm_scan_range(e, ax, a.res) > a.range_max; }, &h);
  bool hit = false;
  double r = 0.0;
  if (blocked) {  // the first blocking cell decides, and counts iff r <= range_max
    r = wm_scan_range(h.e, h.a, a.res);
    hit = r <= a.range_max;
  }
  const int hit_i = h.i, hit_j = h.j;
  double out = hit ? r : a.range_max;
  if (a.real) {  // rule 27: a NaN compares false, an infinity is left out by name
    const double q = a.real[k];
    if (isfinite(q) && q < out) out = q;
  }
  const size_t slot = static_cast<size_t>(blockIdx.x) * static_cast<size_t>(a.B) + static_cast<size_t>(k);
  a.ranges[slot] = out;
  if (a.cells) a.cells[slot] = hit ? hit_i + hit_j * a.W : -1;
}

// ---- (h) the distance plane (rules 42 and 43) ----
constexpr int kWmDistTile = 64;        // output cells a side of one workgroup's tile
constexpr int kWmDistTiledReach = 63;  // above it the halo no longer fits: the two global passes below
constexpr uint8_t kWmDistNone = 255;   // a row distance: no blocking cell within reach

struct WmDistArgs {
  const int8_t *cls;
  uint16_t *dist2;
  uint8_t *rowd;  // the fallback's scratch plane only
  int W, H;
  int x0, y0, x1, y1;  // the inclusive box to recompute, inside the map
  int R, unknown_blocks;
  unsigned R2;
};

// LDS bytes of a tile at reach R: the blocking bytes of (64 + 2 R)^2 cells, then 64 row distances for 64 + 2 R rows
__host__ __device__ inline size_t wm_dist_lds(int R) {
  const size_t side = static_cast<size_t>(kWmDistTile + 2 * R);
  return side * side + static_cast<size_t>(kWmDistTile) * side;
}

// One workgroup a tile of at most 64 x 64 cells of the box.  Every cls byte of the tile and its halo is read from
// global memory once, as a blocking byte into LDS (cells outside the map: 0, tested before the load); the row
// distances of the tile's columns are formed in LDS for the tile's rows and the halo rows, the column pass runs out of
// LDS, and a lane stores its own uint16.
__global__ __launch_bounds__(kWmBlock) void worldmap_dist_tile_kernel(WmDistArgs a) {
  extern __shared__ uint8_t wm_dist_smem[];
  const int R = a.R;
  const int tx0 = a.x0 + static_cast<int>(blockIdx.x) * kWmDistTile, ty0 = a.y0 + static_cast<int>(blockIdx.y) * kWmDistTile;
  const int tw = min(kWmDistTile, a.x1 - tx0 + 1), th = min(kWmDistTile, a.y1 - ty0 + 1);
  const int sw = tw + 2 * R, sh = th + 2 * R;  // the region with its halo
  uint8_t *blk = wm_dist_smem;                 // [sh][sw]
  uint8_t *rowd = wm_dist_smem + static_cast<size_t>(kWmDistTile + 2 * R) * static_cast<size_t>(kWmDistTile + 2 * R);  // [sh][64]
  for (int k = threadIdx.x; k < sw * sh; k += kWmBlock) {
    const int r = k / sw, c = k - r * sw;
    const int I = tx0 - R + c, J = ty0 - R + r;
    uint8_t b = 0;
    if (I >= 0 && I < a.W && J >= 0 && J < a.H)
      b = wm_blocks(a.cls[static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(a.W)], a.unknown_blocks) ? 1 : 0;
    blk[k] = b;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < tw * sh; k += kWmBlock) {
    const int r = k / tw, c = k - r * tw;
    const uint8_t *row = blk + r * sw + c + R;  // the cell itself
    int found = kWmDistNone;
    for (int d = 0; d <= R; ++d)
      if (row[-d] | row[d]) {
        found = d;
        break;
      }
    rowd[r * kWmDistTile + c] = static_cast<uint8_t>(found);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < tw * th; k += kWmBlock) {
    const int r = k / tw, c = k - r * tw;
    const uint8_t *col = rowd + (r + R) * kWmDistTile + c;
    unsigned best = 0xFFFFFFFFu;
    for (int dy = -R; dy <= R; ++dy) {
      const unsigned d = col[dy * kWmDistTile];
      if (d != kWmDistNone) best = min(best, d * d + static_cast<unsigned>(dy * dy));
    }
    a.dist2[static_cast<size_t>(tx0 + c) + static_cast<size_t>(ty0 + r) * static_cast<size_t>(a.W)] =
        best <= a.R2 ? static_cast<uint16_t>(best) : static_cast<uint16_t>(KC_WORLDMAP_DIST_FAR);
  }
}

// reach above kWmDistTiledReach, in the planner's manner: the row distances of the box's columns over the box's rows
// grown by R (clipped to the map) into a scratch plane, then the column pass.  blockIdx.y: the row of the pass.
__global__ __launch_bounds__(kWmBlock) void worldmap_dist_rows_kernel(WmDistArgs a) {
  const int J = max(a.y0 - a.R, 0) + static_cast<int>(blockIdx.y);
  const int8_t *row = a.cls + static_cast<size_t>(J) * static_cast<size_t>(a.W);
  for (int I = a.x0 + static_cast<int>(blockIdx.x * kWmBlock + threadIdx.x); I <= a.x1; I += static_cast<int>(gridDim.x) * kWmBlock) {
    int found = kWmDistNone;
    for (int d = 0; d <= a.R; ++d) {
      const bool l = I - d >= 0 && wm_blocks(row[I - d], a.unknown_blocks);
      const bool r = I + d < a.W && wm_blocks(row[I + d], a.unknown_blocks);
      if (l || r) {
        found = d;
        break;
      }
    }
    a.rowd[static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(a.W)] = static_cast<uint8_t>(found);
  }
}

__global__ __launch_bounds__(kWmBlock) void worldmap_dist_cols_kernel(WmDistArgs a) {
  const int J = a.y0 + static_cast<int>(blockIdx.y);
  const int lo = max(-a.R, -J), hi = min(a.R, a.H - 1 - J);
  for (int I = a.x0 + static_cast<int>(blockIdx.x * kWmBlock + threadIdx.x); I <= a.x1; I += static_cast<int>(gridDim.x) * kWmBlock) {
    const size_t cell = static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(a.W);
    unsigned best = 0xFFFFFFFFu;
    for (int dy = lo; dy <= hi; ++dy) {
      const unsigned d = a.rowd[static_cast<long long>(cell) + static_cast<long long>(dy) * a.W];
      if (d != kWmDistNone) best = min(best, d * d + static_cast<unsigned>(dy * dy));
    }
    a.dist2[cell] = best <= a.R2 ? static_cast<uint16_t>(best) : static_cast<uint16_t>(KC_WORLDMAP_DIST_FAR);
  }
}

// ---- (j) scan integration (rules 52 to 57) ----
constexpr unsigned kWmMarkMiss = 1u, kWmMarkHit = 2u;  // the bits of a mark byte

struct WmMarkArgs {
  uint8_t *marks;        // a byte a world cell, the plane rounded up to whole dwords; all zero between calls
  const int2 *table;     // rule 21: (ac, as) a beam
  const int32_t *zq;     // rule 52
  kc_worldmap_pose pose;
  long long zmax;
  int W, H, B, rc;
  int clear_no_return, precheck;
};

// The OR of `bit` into the byte of cell (I, J): an atomic without a return value on the aligned dword that holds it, which
// lies inside the plane whatever W is (the plane's size is a multiple of 4).  Two things in front of it:
//  - a lane whose lower neighbour marks the same bit of the same cell in this step leaves the mark to it.  Near the sensor
//    neighbouring beams stand in the same cell step after step; every lane still in the loop comes through here once a
//    step, so the ballot names the lanes whose `code` the shuffle may read.  Kept: it is the faster kernel at every
//    beam count measured.
//  - `precheck`: a plain byte load that skips the atomic where the bit stands already (a stale byte only costs the atomic
//    it would have saved, and OR is idempotent).  Measured and OFF by default: the walk then waits for a load every step,
//    where the atomic alone is sent and forgotten.  The switch stays for the timing tool.
__device__ __forceinline__ void wm_mark_cell(const WmMarkArgs &a, int I, int J, unsigned bit) {
  const bool inside = I >= 0 && I < a.W && J >= 0 && J < a.H;  // rule 54: outside, walked and never marked
  const size_t cell = inside ? static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(a.W) : size_t{0};
  const unsigned code = inside ? static_cast<unsigned>(cell) * 4u + bit : 0u;  // bit is 1 or 2, cells <= 2^28: 0 is no mark
  const unsigned long long live = __ballot(1);
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const unsigned below = __shfl_up(code, 1);
  if (lane > 0 && ((live >> (lane - 1)) & 1ull) && below == code) return;
  if (!inside) return;
  if (a.precheck && (a.marks[cell] & bit)) return;
  atomicOr(reinterpret_cast<unsigned int *>(a.marks) + (cell >> 2), bit << (8u * static_cast<unsigned>(cell & 3)));
}

constexpr int kWmMarkChunk = 8;  // steps along a beam's dominant axis that one lane walks

// Rule 23's walk with nothing loaded that decides it, so no rounds: a step is the axis choice (D = ex |dy| - ey |dx| kept by
// addition as in wm_walk), the crossing test of rule 53 for the step AHEAD, and the mark of the cell the beam stands in:
// MISS while the step ahead is crossed, else this is the beam's last crossed cell, HIT for a return.  The test e 2^30 < (z +
// 1) a is kept as a remainder per axis, r = (z + 1) a - e 2^30 > 0, that a step lowers by 2^46.  The step that leaves rule
// 23's box is never crossed (rule 53), so the box is not tested; the count only bounds the loop.
//
// blockIdx.x * 256 + threadIdx.x: the beam, consecutive beams on consecutive lanes.  blockIdx.y: the segment of the walk
// this lane makes.  A walk of a few hundred dependent steps leaves a lane alone with its latency, whatever the beam count
// (DESIGN.md 4.11 has the figures), and the walk can be entered in the middle: it merges the x steps m = 0, 1, .. at
// EX_m = ex + m 2^16 and the y steps n at EY_n = ey + n 2^16, x step m before y step n iff EX_m |dy| <= EY_n |dx| (rule 23's
// comparison: the tie goes to x).  With x the dominant axis (|dx| >= |dy|), segment g > 0 starts in front of x step m0 = 8 g
// with every y step before it made: n0 = #{n : EY_n |dx| < EX_m0 |dy|} = ceil(T / (2^16 |dx|)) for T = EX_m0 |dy| - ey |dx| >
// 0, else 0.  With y dominant it starts in front of y step n0 = 8 g with m0 = #{m : EX_m |dy| <= EY_n0 |dx|} = floor(T /
// (2^16 |dy|)) + 1 for T = EY_n0 |dx| - ex |dy| >= 0, else 0 (and 0 for dx == 0, where no step goes along x).  One 64-bit
// division a lane; every product stays below 2^59.  The walk reaches that state iff the steps in front of it are crossed,
// and since q never decreases (rule 53) that is: x step m0 - 1 and y step n0 - 1 are, where they exist.  A lane ends in
// front of the next segment's first step, whose cell that segment marks.  Segment 0 starts in the start cell.
__global__ __launch_bounds__(kWmBlock) void worldmap_mark_kernel(WmMarkArgs a) {
  const int k = static_cast<int>(blockIdx.x) * kWmBlock + static_cast<int>(threadIdx.x);
  if (k >= a.B) return;
  const long long z = a.zq[k];
  if (z < 0) return;  // rule 54: the beam says nothing
  const bool ret = z < a.zmax;
  if (!ret && !a.clear_no_return) return;
  const int2 t = a.table[k];
  const long long cq = a.pose.cq, sq = a.pose.sq;
  const int dx = static_cast<int>(q16_turn_x(cq, sq, t.x, t.y)), dy = static_cast<int>(q16_turn_y(cq, sq, t.x, t.y));
  const long long X0 = a.pose.tx + (1ll << 15), Y0 = a.pose.ty + (1ll << 15);
  int I = static_cast<int>(X0 >> 16), J = static_cast<int>(Y0 >> 16);
  const int fx = static_cast<int>(X0 & 0xFFFF), fy = static_cast<int>(Y0 & 0xFFFF);
  const int sx = dx > 0 ? 1 : -1, sy = dy > 0 ? 1 : -1;
  const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
  const long long ex = dx > 0 ? 65536 - fx : fx, ey = dy > 0 ? 65536 - fy : fy;
  const long long step_x = 65536ll * ady, step_y = 65536ll * adx;
  const bool x_dom = adx >= ady;
  long long m0 = 0, n0 = 0;  // the x and y steps made in front of this segment
  if (blockIdx.y > 0) {
    const long long first = static_cast<long long>(blockIdx.y) * kWmMarkChunk;
    if (x_dom) {
      m0 = first;
      const long long T = (ex + (m0 << 16)) * ady - ey * adx;
      n0 = T > 0 ? (T + step_y - 1) / step_y : 0;
    } else {
      n0 = first;
      const long long T = (ey + (n0 << 16)) * adx - ex * ady;
      m0 = (dx != 0 && T >= 0) ? T / step_x + 1 : 0;
    }
    // the state is on the beam's crossed prefix iff the steps in front of it are crossed
    if (m0 > 0 && !(((ex + ((m0 - 1) << 16)) << 30) < (z + 1) * adx)) return;
    if (n0 > 0 && !(((ey + ((n0 - 1) << 16)) << 30) < (z + 1) * ady)) return;
  }
  const long long EX = ex + (m0 << 16), EY = ey + (n0 << 16);
  I += sx * static_cast<int>(m0);
  J += sy * static_cast<int>(n0);
  // dy == 0: D = -EY |dx| <= 0 and stays (step_x = 0), every step goes along x.  dx == 0: D = EX |dy| may be 0, which would
  // send a step along x, so it is put to 1, and stays (step_y = 0)
  long long D = dx == 0 ? 1 : EX * ady - EY * adx;
  long long rx = (z + 1) * adx - (EX << 30), ry = (z + 1) * ady - (EY << 30);  // all below 2^59 in magnitude
  int dominant = 0;  // steps this lane has made along the dominant axis
  // between two steps along the dominant axis lies at most one along the other (a tie included), and one may come first
  for (int s = 0; s < 2 * kWmMarkChunk + 2; ++s) {
    const bool along_x = D <= 0;
    if (along_x == x_dom && dominant == kWmMarkChunk) return;  // the next segment's first step: its lane marks this cell
    const bool last = (along_x ? rx : ry) <= 0;  // the step ahead is not crossed: this cell is the beam's last
    wm_mark_cell(a, I, J, last && ret ? kWmMarkHit : kWmMarkMiss);
    if (last) return;
    dominant += along_x == x_dom ? 1 : 0;
    if (along_x) {
      I += sx;
      rx -= 1ll << 46;
      D += step_x;
    } else {
      J += sy;
      ry -= 1ll << 46;
      D -= step_y;
    }
  }
}

struct WmApplyArgs {
  uint8_t *marks;
  int8_t *evidence, *cls;
  int *rec, *rec_next;    // as the update's
  int W;
  int i_lo, j_lo, i_hi, j_hi;  // the launch box, inclusive, inside the map
  WmModel m;
};

// worldmap_update_kernel's geometry and record over the walk's box; the observation is the cell's mark byte (rule 55: a
// hit beats a miss), which the lane that read it puts back to zero.  Byte loads and stores, for the update's reason.
__global__ __launch_bounds__(kWmBlock) void worldmap_integrate_apply_kernel(WmApplyArgs a) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) {
    a.rec_next[0] = 0;
    a.rec_next[1] = INT_MAX;
    a.rec_next[2] = INT_MAX;
    a.rec_next[3] = -1;
    a.rec_next[4] = -1;
  }
  const int I = a.i_lo + static_cast<int>(blockIdx.x) * kWmLanes + static_cast<int>(threadIdx.x);
  const int J = a.j_lo + static_cast<int>(blockIdx.y) * kWmRows + static_cast<int>(threadIdx.y);
  bool changed = false;
  if (I <= a.i_hi && J <= a.j_hi) {
    const size_t cell = static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(a.W);
    const unsigned mark = a.marks[cell];
    if (mark != 0u) {
      a.marks[cell] = 0;
      const int old = a.evidence[cell];
      const int base = old == kWmNever ? 0 : old;
      const int e = (mark & kWmMarkHit) ? min(base + a.m.hit, a.m.e_max) : max(base - a.m.miss, a.m.e_min);
      const int8_t k = wm_class(e, a.m.occ_thr);
      changed = a.cls[cell] != k;
      if (e != old) a.evidence[cell] = static_cast<int8_t>(e);
      if (changed) a.cls[cell] = k;
    }
  }
  // one wavefront is one row segment (blockDim.x == 64): J is uniform in it
  const unsigned long long mask = __ballot(changed);
  if (mask == 0) return;
  const int lane = static_cast<int>(threadIdx.x);
  const int first = __ffsll(mask) - 1, last = 63 - __clzll(mask);
  if (lane == first) {
    atomicAdd(reinterpret_cast<unsigned int *>(&a.rec[0]), static_cast<unsigned int>(__popcll(mask)));
    atomicMin(&a.rec[1], I);
    atomicMin(&a.rec[2], J);
    atomicMax(&a.rec[4], J);
  }
  if (lane == last) atomicMax(&a.rec[3], I);
}

// ---- (k) movers in a scan (rules 64 to 70) ----
constexpr int kWmMvBlock = 1024;               // the cluster kernel's one workgroup
constexpr int kWmMvWaves = kWmMvBlock / 64;
constexpr size_t kWmMvRecBytes = 64;           // the record's share of the output block, a cache line
static_assert(sizeof(kc_worldmap_cluster) == 64, "rule 68's record is 64 bytes");
static_assert(sizeof(kc_worldmap_movers_record) <= kWmMvRecBytes, "the record fits its line");

struct WmMoversArgs {
  const int8_t *cls;
  const uint16_t *dist2;
  const int2 *table;     // rule 21
  const int32_t *zq;     // rule 52
  kc_worldmap_pose pose;
  long long zmax;
  unsigned long long join_q;
  unsigned m2;
  int W, H, B, gap, min_beams;
  // scratch the context keeps, B entries each (run_start: B + 1)
  long long *ex, *ey;    // rule 65's endpoint; 0 where a beam has none
  uint8_t *flag;         // rule 66
  int *comp;             // the dynamic beams in scan order
  int *run_of;           // the run of a compacted beam
  int *run_start;        // a run's first compacted index; [n_runs] = n_dynamic
  int *run_kept;         // a run's kept number, or -2
  // the output block
  kc_worldmap_movers_record *rec;
  kc_worldmap_cluster *clusters;
  int32_t *label;
};

// A lane a beam.  The bounds test stands in front of both loads, and neither load waits for the other.
__global__ __launch_bounds__(kWmBlock) void worldmap_movers_flag_kernel(WmMoversArgs a) {
  const int k = static_cast<int>(blockIdx.x) * kWmBlock + static_cast<int>(threadIdx.x);
  if (k >= a.B) return;
  const long long z = a.zq[k];
  long long EX = 0, EY = 0;
  bool dyn = false;
  if (z >= 0 && z < a.zmax) {  // rule 65
    const int2 t = a.table[k];
    const long long dx = q16_turn_x(a.pose.cq, a.pose.sq, t.x, t.y), dy = q16_turn_y(a.pose.cq, a.pose.sq, t.x, t.y);
    EX = a.pose.tx + (1ll << 15) + ((z * dx + (1ll << 29)) >> 30);
    EY = a.pose.ty + (1ll << 15) + ((z * dy + (1ll << 29)) >> 30);
    const long long I = EX >> 16, J = EY >> 16;
    if (I >= 0 && I < a.W && J >= 0 && J < a.H) {  // rule 66
      const size_t cell = static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(a.W);
      const int8_t c = a.cls[cell];
      const unsigned d = a.dist2[cell];
      dyn = c == KC_EMPTY && d > a.m2;
    }
  }
  a.ex[k] = EX;
  a.ey[k] = EY;
  a.flag[k] = dyn ? 1 : 0;
}

// The exclusive prefix of v over the workgroup's 1024 lanes in lane order, and the total: a shuffle scan in the
// wavefront, the 16 wavefront sums through `part`.  Every lane calls it; `part` is free again on return.
__device__ __forceinline__ int wm_mv_exscan(int v, int *part, int *total) {
  const int lane = static_cast<int>(threadIdx.x) & 63, w = static_cast<int>(threadIdx.x) >> 6;
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(inc, d);
    if (lane >= d) inc += u;
  }
  if (lane == 63) part[w] = inc;
  __syncthreads();
  int before = 0, all = 0;
  for (int i = 0; i < kWmMvWaves; ++i) {
    const int p = part[i];
    all += p;
    before += i < w ? p : 0;
  }
  __syncthreads();
  *total = all;
  return before + inc - v;
}

__device__ __forceinline__ long long wm_mv_shfl_xor(long long v, int m) {
  const int lo = __shfl_xor(static_cast<int>(v & 0xFFFFFFFFll), m), hi = __shfl_xor(static_cast<int>(v >> 32), m);
  return (static_cast<long long>(hi) << 32) | static_cast<long long>(static_cast<unsigned>(lo));
}

// One workgroup.  Lane t owns the beams [t C, (t + 1) C), C = ceil(B / 1024) <= 64, so lane order is scan order and a
// prefix count over the lanes numbers things in scan order.  Five steps, a barrier between them; what one step leaves
// for the next goes through global scratch (the workgroup's own writes, visible behind the barrier).
//  A  compaction: a lane counts its dynamic beams, the prefix gives its first compacted index, it writes its beams.
//  B  rule 67's head test of a compacted beam against the one in front of it; the prefix count of heads numbers the runs.
//  C  rule 68: a run's size is the distance of two run starts; the prefix count of kept runs numbers the clusters.
//  D  a wavefront a returned cluster: sums, minima and maxima by shuffles, in int64.
//  E  rule 69's labels, a lane over its own beams again.
__global__ __launch_bounds__(kWmMvBlock) void worldmap_movers_cluster_kernel(WmMoversArgs a) {
  __shared__ int s_part[kWmMvWaves];
  __shared__ int s_kept_run[KC_WORLDMAP_MAX_CLUSTERS];
  const int t = static_cast<int>(threadIdx.x);
  const int C = (a.B + kWmMvBlock - 1) / kWmMvBlock;
  const int k0 = min(t * C, a.B), k1 = min(k0 + C, a.B);
  // A
  int cnt = 0;
  for (int k = k0; k < k1; ++k) cnt += a.flag[k];
  int n_dyn = 0;
  const int base = wm_mv_exscan(cnt, s_part, &n_dyn);
  {
    int idx = base;
    for (int k = k0; k < k1; ++k)
      if (a.flag[k]) a.comp[idx++] = k;
  }
  __syncthreads();
  // B: bit j of hm, the head test of compacted beam base + j (cnt <= C <= 64)
  unsigned long long hm = 0;
  for (int j = 0; j < cnt; ++j) {
    const int idx = base + j;
    bool head = idx == 0;
    if (!head) {
      const int k = a.comp[idx], p = a.comp[idx - 1];
      const long long ddx = (a.ex[k] - a.ex[p]) >> 8, ddy = (a.ey[k] - a.ey[p]) >> 8;  // below 2^30 in magnitude
      head = k - p > a.gap + 1 || static_cast<unsigned long long>(ddx * ddx + ddy * ddy) > a.join_q;
    }
    hm |= static_cast<unsigned long long>(head) << j;
  }
  int n_runs = 0;
  const int rbase = wm_mv_exscan(__popcll(hm), s_part, &n_runs);
  {
    int r = rbase - 1;  // the run of the compacted beam in front of this lane's first
    for (int j = 0; j < cnt; ++j) {
      if ((hm >> j) & 1ull) a.run_start[++r] = base + j;
      a.run_of[base + j] = r;
    }
  }
  if (t == 0) a.run_start[n_runs] = n_dyn;
  __syncthreads();
  // C: the runs in chunks of consecutive runs a lane
  const int RC = (n_runs + kWmMvBlock - 1) / kWmMvBlock;
  const int r0 = min(t * RC, n_runs), r1 = min(r0 + RC, n_runs);
  int kept = 0;
  for (int r = r0; r < r1; ++r) kept += a.run_start[r + 1] - a.run_start[r] >= a.min_beams ? 1 : 0;
  int n_kept = 0;
  const int kbase = wm_mv_exscan(kept, s_part, &n_kept);
  {
    int id = kbase;
    for (int r = r0; r < r1; ++r) {
      const bool keep = a.run_start[r + 1] - a.run_start[r] >= a.min_beams;
      a.run_kept[r] = keep ? id : -2;
      if (keep && id < KC_WORLDMAP_MAX_CLUSTERS) s_kept_run[id] = r;
      id += keep ? 1 : 0;
    }
  }
  __syncthreads();
  // D
  const int n_ret = min(n_kept, KC_WORLDMAP_MAX_CLUSTERS);
  const int lane = t & 63;
  for (int id = t >> 6; id < n_ret; id += kWmMvWaves) {
    const int r = s_kept_run[id];
    const int s = a.run_start[r], e = a.run_start[r + 1];
    long long sx = 0, sy = 0, lo_x = LLONG_MAX, hi_x = LLONG_MIN, lo_y = LLONG_MAX, hi_y = LLONG_MIN;
    for (int i = s + lane; i < e; i += 64) {
      const int k = a.comp[i];
      const long long x = a.ex[k], y = a.ey[k];
      sx += x;
      sy += y;
      lo_x = min(lo_x, x);
      hi_x = max(hi_x, x);
      lo_y = min(lo_y, y);
      hi_y = max(hi_y, y);
    }
    for (int m = 32; m > 0; m >>= 1) {
      sx += wm_mv_shfl_xor(sx, m);
      sy += wm_mv_shfl_xor(sy, m);
      lo_x = min(lo_x, wm_mv_shfl_xor(lo_x, m));
      hi_x = max(hi_x, wm_mv_shfl_xor(hi_x, m));
      lo_y = min(lo_y, wm_mv_shfl_xor(lo_y, m));
      hi_y = max(hi_y, wm_mv_shfl_xor(hi_y, m));
    }
    if (lane == 0) {
      kc_worldmap_cluster c;
      c.k_first = a.comp[s];
      c.k_last = a.comp[e - 1];
      c.n = e - s;
      c.reserved = 0;
      c.sx = sx;
      c.sy = sy;
      c.min_x = lo_x;
      c.max_x = hi_x;
      c.min_y = lo_y;
      c.max_y = hi_y;
      a.clusters[id] = c;
    }
  }
  // E
  {
    int idx = base;
    for (int k = k0; k < k1; ++k) a.label[k] = a.flag[k] ? a.run_kept[a.run_of[idx++]] : -1;
  }
  if (t == 0) {
    a.rec->n_dynamic = static_cast<uint32_t>(n_dyn);
    a.rec->n_runs = static_cast<uint32_t>(n_runs);
    a.rec->n_kept = static_cast<uint32_t>(n_kept);
    a.rec->n_returned = static_cast<uint32_t>(n_ret);
  }
}

}  // namespace kc

using namespace kc;

struct kc_worldmap {
  int device = 0;
  hipStream_t stream = nullptr;
  OrderEvent grid_ready;  // a mapper's scan, for the grids read where the mapper left them
  int W = 0, H = 0;
  float res = 0.0f;
  double ox0 = 0.0, oy0 = 0.0;  // the origin given at creation
  int OI = 0, OJ = 0;           // rule 46: the window's offset in cells
  WmModel m = {3, 1, -8, 14, 1};
  DevBuf<int8_t> d_evidence, d_cls;
  DevBuf<int8_t> d_shift_e, d_shift_c;  // the shift's scratch planes, kept from the first shift on
  DevBuf<int32_t> d_stage;   // a host grid (local, or an int32 prior) on its way to a kernel
  FlipRecord rec;            // the update's: kWmRecWords a block
  // match: scratch grown on demand and kept
  DevBuf<uint8_t> d_weight;    // rule 12 over the scratch plane
  DevBuf<uint32_t> d_points;   // packed (a, b), at most one a local cell
  DevBuf<uint32_t> d_scores;   // the table, behind it the point counter
  DevBuf<int> d_mrec;
  PinBuf<int> h_mrec;
  int match_K = -1, match_S = -1;  // the window of the table d_scores holds; -1: none
  Timing match_time;               // weight, points, score, pick
  // obstacle list (rules 16 to 19): scratch grown on demand and kept
  DevBuf<float> d_pts;             // the list of the last kc_worldmap_points
  FlipRecord pts_rec;              // the list's counters: 5 lines of kWmPtsStride words a block
  // virtual scan (rules 20 to 27): the table of the last angle array, scratch grown on demand and kept
  ScanTable scan_table;
  DevBuf<kc_worldmap_pose> d_poses;
  PinBuf<kc_worldmap_pose> h_poses;
  DevBuf<double> d_scan;           // the ranges, behind them the cells as int32: one read-back
  PinBuf<double> h_scan;
  // distance plane (rules 42 and 43): off while dist_reach is 0
  int dist_reach = 0;
  unsigned dist_flags = 0;
  DevBuf<uint16_t> d_dist2;
  DevBuf<uint8_t> d_rowd;          // the scratch of a reach above kWmDistTiledReach, grown on demand
  int dirty[4] = {0, 0, -1, -1};   // (i_min, j_min, i_max, j_max), empty while i_max < i_min
  int dist_last[4] = {-1, -1, -1, -1};
  bool dist_last_full = false;
  // scan integration (rules 52 to 57): the mark plane from the first call on, all zero between calls
  DevBuf<uint8_t> d_marks;
  bool marks_zero = false;         // the plane has been zeroed once and every call since has left it so
  DevBuf<int32_t> d_zq;
  PinBuf<int32_t> h_zq;
  bool mark_precheck = false;      // the byte load in front of the atomic: measured and off (on: for the timing tool)
  Timing integ_time;               // mark, apply
  // movers (rules 64 to 70): scratch and the output block, grown on demand and kept
  DevBuf<long long> d_mv_xy;       // EX, behind it EY
  DevBuf<uint8_t> d_mv_flag;
  DevBuf<int> d_mv_idx;            // comp, run_of, run_kept, run_start (B + 1)
  DevBuf<uint8_t> d_mv_out;        // the record's line, the clusters, the labels: one read-back
  PinBuf<uint8_t> h_mv_out;
  Timing mv_time;                  // flag, cluster

  // rule 46: one product and one sum in double, never accumulated
  double ox() const { return ox0 + static_cast<double>(OI) * static_cast<double>(res); }
  double oy() const { return oy0 + static_cast<double>(OJ) * static_cast<double>(res); }
  void dirty_all() {
    if (dist_reach == 0) return;
    dirty[0] = dirty[1] = 0;
    dirty[2] = W - 1;
    dirty[3] = H - 1;
  }
  void dirty_merge(int i0, int j0, int i1, int j1) {
    if (dist_reach == 0) return;
    if (dirty[2] < dirty[0]) {
      dirty[0] = i0, dirty[1] = j0, dirty[2] = i1, dirty[3] = j1;
      return;
    }
    dirty[0] = std::min(dirty[0], i0);
    dirty[1] = std::min(dirty[1], j0);
    dirty[2] = std::max(dirty[2], i1);
    dirty[3] = std::max(dirty[3], j1);
  }
};

namespace {

// A local grid, [gh x gw] column-major; from wm_resolve, p is on the device and complete in the stream's order
struct LocalGrid {
  const int32_t *p;
  int gh, gw, c0, c1;
  float res;
};

// Where a call's local grid comes from: the caller's description with p on the host or the device, or a mapper's view
struct GridSource {
  enum Kind { Host, Device, Mapper } kind;
  LocalGrid grid;
  kc_mapper *mapper;
};

int wm_check_model(int hit, int miss, int e_min, int e_max, int occ_thr) {
  if (hit < 1 || hit > 127 || miss < 1 || miss > 127)
    KC_FAIL(KC_ERR_INVALID, "hit and miss must be in 1 .. 127, got %d and %d", hit, miss);
  if (e_min < -127 || e_min > 0) KC_FAIL(KC_ERR_INVALID, "e_min must be in -127 .. 0, got %d", e_min);
  if (e_max < 0 || e_max > 127) KC_FAIL(KC_ERR_INVALID, "e_max must be in 0 .. 127, got %d", e_max);
  if (!(e_min < occ_thr && occ_thr <= e_max))
    KC_FAIL(KC_ERR_INVALID, "occ_thr must satisfy e_min < occ_thr <= e_max, got %d for %d .. %d", occ_thr, e_min, e_max);
  return KC_OK;
}

int wm_check_shape(int W, int H, float res) {
  if (W <= 0 || H <= 0 || !(res > 0.0f) || !std::isfinite(res))
    KC_FAIL(KC_ERR_INVALID, "the map's width, height and resolution must be positive, got %d x %d at %g", W, H, static_cast<double>(res));
  if (W > kWmMaxSide || H > kWmMaxSide ||
      static_cast<unsigned long long>(W) * static_cast<unsigned long long>(H) > KC_PLANNER_MAX_CELLS)
    KC_FAIL(KC_ERR_RANGE, "a %d x %d map is above the cap of %d cells a side and %u cells", W, H, kWmMaxSide,
            static_cast<unsigned>(KC_PLANNER_MAX_CELLS));
  return KC_OK;
}

int wm_check_grid(float world_res, int gh, int gw, int c0, int c1, float res) {
  if (gh <= 0 || gw <= 0) KC_FAIL(KC_ERR_INVALID, "the local grid's height and width must be positive, got %d x %d", gh, gw);
  if (static_cast<unsigned long long>(gh) * static_cast<unsigned long long>(gw) > 0x3FFFFFFFull)
    KC_FAIL(KC_ERR_RANGE, "a %d x %d local grid is too large", gh, gw);
  if (c0 < -(1 << 30) || c0 > (1 << 30) || c1 < -(1 << 30) || c1 > (1 << 30))
    KC_FAIL(KC_ERR_RANGE, "central cell (%d, %d) not within 2^30 cells", c0, c1);
  if (std::memcmp(&world_res, &res, sizeof(float)) != 0)
    KC_FAIL(KC_ERR_INVALID, "the local grid's resolution %.9g is not the map's %.9g: resampling is out of scope",
            static_cast<double>(res), static_cast<double>(world_res));
  return KC_OK;
}

int wm_check_pose(const kc_worldmap_pose *p) {
  if (!p) KC_FAIL(KC_ERR_INVALID, "null pose");
  if (p->cq < -65536 || p->cq > 65536 || p->sq < -65536 || p->sq > 65536)
    KC_FAIL(KC_ERR_INVALID, "pose (cq, sq) = (%d, %d) is outside -65536 .. 65536", p->cq, p->sq);
  if (p->tx < -kQ16MaxOffset || p->tx > kQ16MaxOffset || p->ty < -kQ16MaxOffset || p->ty > kQ16MaxOffset)
    KC_FAIL(KC_ERR_RANGE, "the pose lies more than 2^20 cells from the map's origin");
  return KC_OK;
}

unsigned wm_blocks_for(long long work) {
  return static_cast<unsigned>(std::max<long long>(1, std::min<long long>(kWmMaxBlocks, (work + kWmBlock - 1) / kWmBlock)));
}

// The launch of one lane a cell over an inclusive box of cells: kWmLanes cells along I and kWmRows rows a workgroup
dim3 wm_box_grid(const int box[4]) { return dim3((box[2] - box[0]) / kWmLanes + 1, (box[3] - box[1]) / kWmRows + 1); }

// `host` (nbytes of a local grid or a prior) into d_stage, in the order of the context's stream
int wm_stage(kc_worldmap *c, const void *host, size_t nbytes) {
  KC_TRY(c->d_stage.reserve((nbytes + 3) / 4));
  KC_HIP(hipMemcpyAsync(c->d_stage.p, host, nbytes, hipMemcpyHostToDevice, c->stream));
  return KC_OK;
}

// dev: the prior on the context's device (nullptr: clear), complete in the order of the context's stream
int wm_take_prior(kc_worldmap *c, const void *dev, int elem_bytes) {
  const long long n = static_cast<long long>(c->W) * c->H;
  const dim3 grid(wm_blocks_for((n + 3) / 4)), block(kWmBlock);
  if (elem_bytes == 4)
    hipLaunchKernelGGL(worldmap_prior_kernel<int32_t>, grid, block, 0, c->stream, static_cast<const int32_t *>(dev),
                       c->d_evidence.p, c->d_cls.p, n, c->m);
  else
    hipLaunchKernelGGL(worldmap_prior_kernel<int8_t>, grid, block, 0, c->stream, static_cast<const int8_t *>(dev),
                       c->d_evidence.p, c->d_cls.p, n, c->m);
  KC_HIP(hipGetLastError());
  c->dirty_all();  // rule 43: every class may have changed
  KC_HIP(hipStreamSynchronize(c->stream));  // the caller's grid is not read after the call returns
  return KC_OK;
}

int wm_check_prior(const kc_worldmap *c, const void *grid, int elem_bytes, int W, int H) {
  if (!c || !grid) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (elem_bytes != 1 && elem_bytes != 4) KC_FAIL(KC_ERR_INVALID, "prior cells are int8 (1) or int32 (4) bytes, got %d", elem_bytes);
  if (W != c->W || H != c->H) KC_FAIL(KC_ERR_INVALID, "a %d x %d prior does not fit the %d x %d map", W, H, c->W, c->H);
  return KC_OK;
}

// The inclusive box of world cells that rule 4 can map into the local grid, clipped to the map; false when empty.
// The local window is a in [-c0 - 1/2, gh - c0 - 1/2), b likewise; rule 4 rounds M (p - t) with M = [[C, S], [-S, C]],
// C = cq / 2^16, S = sq / 2^16, whose exact inverse is M^T / (C^2 + S^2).  C^2 + S^2 is within 2^-15 of 1, so the
// corners' images under M^T, widened by 2 cells and by 2^-13 of the window's reach, hold every such cell.
bool wm_box(const kc_worldmap *c, const kc_worldmap_pose *p, int gh, int gw, int c0, int c1, int box[4]) {
  const double C = p->cq / 65536.0, S = p->sq / 65536.0;
  const double tx = static_cast<double>(p->tx) / 65536.0, ty = static_cast<double>(p->ty) / 65536.0;
  const double a0 = -static_cast<double>(c0) - 0.5, a1 = static_cast<double>(gh) - c0 - 0.5;
  const double b0 = -static_cast<double>(c1) - 0.5, b1 = static_cast<double>(gw) - c1 - 0.5;
  double x_lo = INFINITY, x_hi = -INFINITY, y_lo = INFINITY, y_hi = -INFINITY;
  for (int k = 0; k < 4; ++k) {
    const double a = k & 1 ? a1 : a0, b = k & 2 ? b1 : b0;
    const double x = C * a - S * b, y = S * a + C * b;
    x_lo = std::min(x_lo, x);
    x_hi = std::max(x_hi, x);
    y_lo = std::min(y_lo, y);
    y_hi = std::max(y_hi, y);
  }
  const double reach = std::max(std::max(std::fabs(a0), std::fabs(a1)), std::max(std::fabs(b0), std::fabs(b1)));
  const double pad = 2.0 + 2.0 * reach / 16384.0;
  const double lo_i = std::floor(tx + x_lo - pad), hi_i = std::ceil(tx + x_hi + pad);
  const double lo_j = std::floor(ty + y_lo - pad), hi_j = std::ceil(ty + y_hi + pad);
  if (hi_i < 0.0 || hi_j < 0.0 || lo_i > c->W - 1.0 || lo_j > c->H - 1.0) return false;
  box[0] = static_cast<int>(std::max(lo_i, 0.0));
  box[1] = static_cast<int>(std::max(lo_j, 0.0));
  box[2] = static_cast<int>(std::min(hi_i, c->W - 1.0));
  box[3] = static_cast<int>(std::min(hi_j, c->H - 1.0));
  return true;
}

// The one way a local grid reaches a kernel.  Host work first: a mapper's view (and that it lives on this device), then
// check(grid), the operation's own refusals; only then the device: a host grid is staged, a device grid must lie inside
// one allocation, a mapper's grid is read where it lies once the context's stream has waited for the scan.
template <typename Check>
int wm_resolve(kc_worldmap *c, const GridSource &s, Check check, LocalGrid *g) {
  MapperView v{};
  *g = s.grid;
  if (s.kind == GridSource::Mapper) {
    KC_TRY(mapper_view(s.mapper, &v));
    if (v.device != c->device) KC_FAIL(KC_ERR_INVALID, "mapper on device %d, world map on device %d", v.device, c->device);
    *g = LocalGrid{v.grid, v.H, v.W, v.c0, v.c1, v.res};
  }
  KC_TRY(check(*g));
  KC_HIP(hipSetDevice(c->device));
  const size_t nbytes = static_cast<size_t>(g->gh) * static_cast<size_t>(g->gw) * sizeof(int32_t);
  if (s.kind == GridSource::Mapper) return stream_wait_through(c->grid_ready, c->stream, v.stream);  // the host does not wait
  if (s.kind == GridSource::Device)
    return check_device_range(c->device, g->p, 0, static_cast<long long>(nbytes), sizeof(int32_t), "grid");
  KC_TRY(wm_stage(c, g->p, nbytes));
  g->p = c->d_stage.p;
  return KC_OK;
}

// Check order: the grid, the pose, then the device
int wm_update(kc_worldmap *c, const GridSource &s, const kc_worldmap_pose *p, kc_worldmap_result *out) {
  LocalGrid g{};
  KC_TRY(wm_resolve(c, s, [&](const LocalGrid &l) {
    KC_TRY(wm_check_grid(c->res, l.gh, l.gw, l.c0, l.c1, l.res));
    return wm_check_pose(p);
  }, &g));
  *out = kc_worldmap_result{0, -1, -1, -1, -1};
  int box[4];
  if (!wm_box(c, p, g.gh, g.gw, g.c0, g.c1, box)) {
    KC_HIP(hipStreamSynchronize(c->stream));  // nothing to do, but the grid is not read after the call returns
    return KC_OK;
  }
  WmUpdateArgs a{};
  KC_TRY(c->rec.begin(c->stream, &a.rec_next));
  a.rec = c->rec.cur;
  a.local = g.p;
  a.evidence = c->d_evidence.p;
  a.cls = c->d_cls.p;
  a.tx = p->tx;
  a.ty = p->ty;
  a.cq = p->cq;
  a.sq = p->sq;
  a.W = c->W;
  a.gh = g.gh;
  a.gw = g.gw;
  a.c0 = g.c0;
  a.c1 = g.c1;
  a.i_lo = box[0];
  a.j_lo = box[1];
  a.i_hi = box[2];
  a.j_hi = box[3];
  a.m = c->m;
  hipLaunchKernelGGL(worldmap_update_kernel, wm_box_grid(box), dim3(kWmLanes, kWmRows), 0, c->stream, a);
  KC_HIP(hipGetLastError());
  KC_TRY(c->rec.commit(c->stream));
  const int *r = c->rec.h.p;
  out->changed = static_cast<uint32_t>(r[0]);
  if (r[0] != 0) {
    out->i_min = r[1];
    out->j_min = r[2];
    out->i_max = r[3];
    out->j_max = r[4];
    c->dirty_merge(r[1], r[2], r[3], r[4]);  // rule 43: from the read-back the update makes anyway
  }
  return KC_OK;
}

// rule 43's refresh, queued on the context's stream; the plane is on
int wm_dist_refresh(kc_worldmap *c) {
  c->dist_last[0] = c->dist_last[1] = c->dist_last[2] = c->dist_last[3] = -1;
  c->dist_last_full = false;
  if (c->dirty[2] < c->dirty[0]) return KC_OK;
  const int R = c->dist_reach;
  WmDistArgs a{};
  a.cls = c->d_cls.p;
  a.dist2 = c->d_dist2.p;
  a.W = c->W;
  a.H = c->H;
  a.x0 = std::max(c->dirty[0] - R, 0);
  a.y0 = std::max(c->dirty[1] - R, 0);
  a.x1 = std::min(c->dirty[2] + R, c->W - 1);
  a.y1 = std::min(c->dirty[3] + R, c->H - 1);
  a.R = R;
  a.R2 = static_cast<unsigned>(R) * static_cast<unsigned>(R);
  a.unknown_blocks = (c->dist_flags & KC_WORLDMAP_DIST_UNKNOWN_BLOCKS) ? 1 : 0;
  const int bw = a.x1 - a.x0 + 1, bh = a.y1 - a.y0 + 1;
  KC_HIP(hipSetDevice(c->device));
  if (R <= kWmDistTiledReach) {
    const dim3 grid((bw + kWmDistTile - 1) / kWmDistTile, (bh + kWmDistTile - 1) / kWmDistTile);
    hipLaunchKernelGGL(worldmap_dist_tile_kernel, grid, dim3(kWmBlock), wm_dist_lds(R), c->stream, a);
    KC_HIP(hipGetLastError());
  } else {
    KC_TRY(c->d_rowd.reserve(static_cast<size_t>(c->W) * static_cast<size_t>(c->H)));
    a.rowd = c->d_rowd.p;
    const unsigned gx = static_cast<unsigned>((bw + kWmBlock - 1) / kWmBlock);
    const int r0 = std::max(a.y0 - R, 0), r1 = std::min(a.y1 + R, c->H - 1);
    hipLaunchKernelGGL(worldmap_dist_rows_kernel, dim3(gx, r1 - r0 + 1), dim3(kWmBlock), 0, c->stream, a);
    KC_HIP(hipGetLastError());
    hipLaunchKernelGGL(worldmap_dist_cols_kernel, dim3(gx, bh), dim3(kWmBlock), 0, c->stream, a);
    KC_HIP(hipGetLastError());
  }
  c->dist_last[0] = a.x0, c->dist_last[1] = a.y0, c->dist_last[2] = a.x1, c->dist_last[3] = a.y1;
  c->dist_last_full = bw == c->W && bh == c->H;
  c->dirty[0] = c->dirty[1] = 0;
  c->dirty[2] = c->dirty[3] = -1;
  return KC_OK;
}

int wm_check_window(int n_yaw, double yaw_step, int reach) {
  if (n_yaw < 0 || n_yaw > kWmMatchMaxYaw) KC_FAIL(KC_ERR_INVALID, "n_yaw must be in 0 .. %d, got %d", kWmMatchMaxYaw, n_yaw);
  if (reach < 0 || reach > kWmMatchMaxReach) KC_FAIL(KC_ERR_INVALID, "reach must be in 0 .. %d, got %d", kWmMatchMaxReach, reach);
  if (!std::isfinite(yaw_step) || !(yaw_step >= 0.0)) KC_FAIL(KC_ERR_INVALID, "yaw_step must be finite and >= 0, got %g", yaw_step);
  return KC_OK;
}

// rule 9's checks: an update's, the cap on the sides, and every cell within that cap of the central cell (a point's
// (a, b) then fits 16 bits each, and the scratch plane is bounded)
int wm_check_match_grid(float world_res, int gh, int gw, int c0, int c1, float res) {
  KC_TRY(wm_check_grid(world_res, gh, gw, c0, c1, res));
  if (gh > kWmMatchMaxSide || gw > kWmMatchMaxSide)
    KC_FAIL(KC_ERR_RANGE, "a %d x %d local grid is above the match's cap of %d cells a side", gh, gw, kWmMatchMaxSide);
  if (c0 < -kWmMatchMaxSide || c0 - (gh - 1) > kWmMatchMaxSide || c1 < -kWmMatchMaxSide || c1 - (gw - 1) > kWmMatchMaxSide ||
      c0 > kWmMatchMaxSide || (gh - 1) - c0 > kWmMatchMaxSide || c1 > kWmMatchMaxSide || (gw - 1) - c1 > kWmMatchMaxSide)
    KC_FAIL(KC_ERR_RANGE, "central cell (%d, %d) is more than %d cells from a cell of the %d x %d local grid", c0, c1,
            kWmMatchMaxSide, gh, gw);
  return KC_OK;
}

int wm_check_match_args(const kc_worldmap_pose *guess, const kc_worldmap_rotation *rot, int K, int S) {
  KC_TRY(wm_check_window(K, 0.0, S));
  KC_TRY(wm_check_pose(guess));
  if (!rot) KC_FAIL(KC_ERR_INVALID, "null rotation table");
  // (the scratch plane's size rests on this: wm_match_half)
  for (int r = 0; r <= 2 * K; ++r) {
    const long long cq = rot[r].cq, sq = rot[r].sq;
    if (cq < -65536 || cq > 65536 || sq < -65536 || sq > 65536 || cq * cq + sq * sq > 65537ll * 65537ll)
      KC_FAIL(KC_ERR_INVALID, "rotation %d (cq, sq) = (%d, %d) is no unit vector in 16 fraction bits", r - K, rot[r].cq, rot[r].sq);
  }
  return KC_OK;
}

// The plane's half side.  A point (a, b) lands, before translation, at I0 = floor((TX + d + 2^15) / 2^16) with
// |d| = |Cq a - Sq b| <= sqrt(Cq^2 + Sq^2) hypot(a, b) <= 2^16 (1 + 2^-15) r (wm_check_match_args holds the table to that), r the hypot of the farthest cell; with
// TX = 2^16 cx + f, 0 <= f < 2^16, that is cx + floor((f + d) / 2^16 + 1/2), within ceil(r (1 + 2^-15)) + 1 of cx.
// r <= 8192 sqrt 2 makes r 2^-15 < 1, the translation adds S: ceil(r) + S + 3 holds every landing cell, J alike.
int wm_match_half(int gh, int gw, int c0, int c1, int S) {
  const double a = std::max(std::abs(c0), std::abs(gh - 1 - c0)), b = std::max(std::abs(c1), std::abs(gw - 1 - c1));
  return static_cast<int>(std::ceil(std::hypot(a, b))) + S + 3;
}

template <int M>
void wm_launch_score(kc_worldmap *c, const WmScoreArgs &a, dim3 grid) {
  hipLaunchKernelGGL(worldmap_score_kernel<M>, grid, dim3(kWmBlock), 0, c->stream, a);
}

// Check order: the window, the guess and the rotation table, the grid, then the device
int wm_match(kc_worldmap *c, const GridSource &src, const kc_worldmap_pose *g, const kc_worldmap_rotation *rot, int K, int S,
             kc_worldmap_match_result *out) {
  KC_TRY(wm_check_match_args(g, rot, K, S));
  LocalGrid l{};
  KC_TRY(wm_resolve(c, src, [&](const LocalGrid &m) { return wm_check_match_grid(c->res, m.gh, m.gw, m.c0, m.c1, m.res); }, &l));
  const int32_t *dev = l.p;
  const int gh = l.gh, gw = l.gw, c0 = l.c0, c1 = l.c1;
  const int T = 2 * S + 1, ncand = T * T, nrot = 2 * K + 1;
  const size_t table_cells = static_cast<size_t>(nrot) * ncand, cells = static_cast<size_t>(gh) * static_cast<size_t>(gw);
  const int half = wm_match_half(gh, gw, c0, c1, S), P = 2 * half + 1;
  const size_t plane_cells = static_cast<size_t>(P) * static_cast<size_t>(P);
  c->match_K = c->match_S = -1;
  KC_TRY(c->d_weight.reserve(plane_cells));
  KC_TRY(c->d_points.reserve(cells));
  KC_TRY(c->d_scores.reserve(static_cast<size_t>(kWmMatchRot) * kWmMatchRot * kWmMatchRot + 1));
  KC_TRY(c->d_mrec.reserve(kWmMatchRecWords));
  KC_TRY(c->h_mrec.reserve(kWmMatchRecWords));
  uint32_t *n_points = c->d_scores.p + table_cells;

  WmWeightArgs w{};
  w.cls = c->d_cls.p;
  w.plane = c->d_weight.p;
  w.table = c->d_scores.p;
  w.n_points = n_points;
  w.plane_cells = static_cast<long long>(plane_cells);
  w.table_cells = static_cast<long long>(table_cells);
  w.W = c->W;
  w.H = c->H;
  w.i0 = static_cast<int>(g->tx >> 16) - half;
  w.j0 = static_cast<int>(g->ty >> 16) - half;
  w.P = P;
  c->match_time.begin_cycle();
  KC_TRY(c->match_time.start("weight", c->stream));
  hipLaunchKernelGGL(worldmap_weight_kernel, dim3(wm_blocks_for(static_cast<long long>(std::max(plane_cells, table_cells)))),
                     dim3(kWmBlock), 0, c->stream, w);
  KC_HIP(hipGetLastError());
  KC_TRY(c->match_time.stop(c->stream));

  KC_TRY(c->match_time.start("points", c->stream));
  hipLaunchKernelGGL(worldmap_points_kernel, dim3(wm_blocks_for(static_cast<long long>(cells))), dim3(kWmBlock), 0, c->stream, dev,
                     static_cast<long long>(cells), gh, c0, c1, c->d_points.p, n_points);
  KC_HIP(hipGetLastError());
  KC_TRY(c->match_time.stop(c->stream));

  WmScoreArgs s{};
  s.plane = c->d_weight.p;
  s.points = c->d_points.p;
  s.n_points = n_points;
  s.table = c->d_scores.p;
  s.tx = g->tx;
  s.ty = g->ty;
  s.i0 = w.i0;
  s.j0 = w.j0;
  s.P = P;
  s.S = S;
  s.T = T;
  s.ncand = ncand;
  std::memcpy(s.rot, rot, sizeof(kc_worldmap_rotation) * static_cast<size_t>(nrot));
  const unsigned chunks = static_cast<unsigned>(std::min<size_t>((cells + kWmChunk - 1) / kWmChunk, kWmChunkBlocks));
  const dim3 sgrid(chunks, static_cast<unsigned>(nrot));
  const int per_lane = (ncand + kWmBlock - 1) / kWmBlock;
  KC_TRY(c->match_time.start("score", c->stream));
  if (per_lane <= 1) wm_launch_score<1>(c, s, sgrid);
  else if (per_lane <= 2) wm_launch_score<2>(c, s, sgrid);
  else if (per_lane <= 4) wm_launch_score<4>(c, s, sgrid);
  else if (per_lane <= 8) wm_launch_score<8>(c, s, sgrid);
  else wm_launch_score<kWmCandPerLane>(c, s, sgrid);
  KC_HIP(hipGetLastError());
  KC_TRY(c->match_time.stop(c->stream));

  KC_TRY(c->match_time.start("pick", c->stream));
  hipLaunchKernelGGL(worldmap_pick_kernel, dim3(1), dim3(kWmPickBlock), 0, c->stream, c->d_scores.p, n_points, K, S, c->d_mrec.p);
  KC_HIP(hipGetLastError());
  KC_TRY(c->match_time.stop(c->stream));
  KC_HIP(hipMemcpyAsync(c->h_mrec.p, c->d_mrec.p, kWmMatchRecWords * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  c->match_K = K;
  c->match_S = S;
  const int *r = c->h_mrec.p;
  out->k = r[0];
  out->u = r[1];
  out->v = r[2];
  out->score = static_cast<uint32_t>(r[3]);
  out->score_guess = static_cast<uint32_t>(r[4]);
  out->n_points = static_cast<uint32_t>(r[5]);
  if (out->k < -K || out->k > K || out->u < -S || out->u > S || out->v < -S || out->v > S)
    KC_FAIL(KC_ERR_HIP, "the match's record (%d, %d, %d) lies outside its window", out->k, out->u, out->v);
  out->pose.cq = rot[out->k + K].cq;
  out->pose.sq = rot[out->k + K].sq;
  out->pose.tx = g->tx + static_cast<int64_t>(out->u) * 65536;
  out->pose.ty = g->ty + static_cast<int64_t>(out->v) * 65536;
  return KC_OK;
}

// rule 16: the window's centre cell and radius in cells
int wm_window(float res, double ox, double oy, double x, double y, float max_range, int *ic, int *jc, int *rc) {
  if (!std::isfinite(max_range) || !(max_range > 0.0f))
    KC_FAIL(KC_ERR_INVALID, "max_sensor_range must be a finite float > 0, got %g", static_cast<double>(max_range));
  kc_worldmap_pose p;
  KC_TRY(kc_worldmap_quantise_pose(res, ox, oy, x, y, 0.0, &p));
  const double cells = std::ceil(static_cast<double>(max_range) / static_cast<double>(res));
  if (!(cells <= static_cast<double>(kWmPtsMaxRadius)))
    KC_FAIL(KC_ERR_RANGE, "a sensor range of %g m is %g cells at %g m, above the cap of %d", static_cast<double>(max_range), cells,
            static_cast<double>(res), kWmPtsMaxRadius);
  *ic = static_cast<int>((p.tx + (1ll << 15)) >> 16);
  *jc = static_cast<int>((p.ty + (1ll << 15)) >> 16);
  *rc = static_cast<int>(cells);
  return KC_OK;
}

// The disc's bounding box clipped to the map, inclusive; false when empty.  |ic|, |jc| <= 2^20 + 1 and rc <= 2048: no sum
// here leaves int.
bool wm_window_box(int W, int H, int ic, int jc, int rc, int box[4]) {
  box[0] = std::max(ic - rc, 0);
  box[1] = std::max(jc - rc, 0);
  box[2] = std::min(ic + rc, W - 1);
  box[3] = std::min(jc + rc, H - 1);
  return box[0] <= box[2] && box[1] <= box[3];
}

// rule 49 for one axis: size S, the robot's cell c
int wm_recentre_axis(int S, int c, int margin, int stride) {
  if (c >= margin && c <= S - 1 - margin) return 0;
  const long long d = static_cast<long long>(c) - S / 2;
  return static_cast<int>((d / stride) * stride);  // C's truncating division; |d| is far below 2^31
}

int wm_recentre_plan(int W, int H, int ic, int jc, int margin, int stride, int *di, int *dj) {
  if (W <= 0 || H <= 0) KC_FAIL(KC_ERR_INVALID, "the map's width and height must be positive, got %d x %d", W, H);
  if (margin < 0 || stride < 1 || 2ll * margin >= std::min(W, H))
    KC_FAIL(KC_ERR_INVALID, "recentring needs margin >= 0, stride >= 1 and 2 margin < min(W, H), got margin %d, stride %d on %d x %d",
            margin, stride, W, H);
  *di = wm_recentre_axis(W, ic, margin, stride);
  *dj = wm_recentre_axis(H, jc, margin, stride);
  return KC_OK;
}

// rule 46's cap, before any device use
int wm_check_shift(int OI, int OJ, int di, int dj) {
  const long long oi = static_cast<long long>(OI) + di, oj = static_cast<long long>(OJ) + dj;
  if (oi < -kWmMaxShift || oi > kWmMaxShift || oj < -kWmMaxShift || oj > kWmMaxShift)
    KC_FAIL(KC_ERR_RANGE, "a shift by (%d, %d) takes the offset (%d, %d) above 2^30 cells", di, dj, OI, OJ);
  return KC_OK;
}

// rules 47 and 48; the arguments are checked
int wm_shift(kc_worldmap *c, int di, int dj) {
  if (di == 0 && dj == 0) return KC_OK;  // launches nothing
  KC_HIP(hipSetDevice(c->device));
  const bool clear = di <= -c->W || di >= c->W || dj <= -c->H || dj >= c->H;
  if (clear) {
    KC_TRY(wm_take_prior(c, nullptr, 1));  // no source cell lies inside the map
  } else {
    const size_t n = static_cast<size_t>(c->W) * static_cast<size_t>(c->H);
    KC_TRY(c->d_shift_e.reserve(n));
    KC_TRY(c->d_shift_c.reserve(n));
    WmShiftArgs a{};
    a.evidence = c->d_evidence.p;
    a.cls = c->d_cls.p;
    a.evidence_out = c->d_shift_e.p;
    a.cls_out = c->d_shift_c.p;
    a.W = c->W;
    a.H = c->H;
    a.di = di;
    a.dj = dj;
    const int box[4] = {0, 0, c->W - 1, c->H - 1};
    hipLaunchKernelGGL(worldmap_shift_kernel, wm_box_grid(box), dim3(kWmLanes, kWmRows), 0, c->stream, a);
    KC_HIP(hipGetLastError());
    // back to where the planes were: the pointers handed out stay valid (rule 48)
    KC_HIP(hipMemcpyAsync(c->d_evidence.p, c->d_shift_e.p, n, hipMemcpyDeviceToDevice, c->stream));
    KC_HIP(hipMemcpyAsync(c->d_cls.p, c->d_shift_c.p, n, hipMemcpyDeviceToDevice, c->stream));
    c->dirty_all();  // rule 48: the accepted first version
    KC_HIP(hipStreamSynchronize(c->stream));
  }
  c->OI += di;
  c->OJ += dj;
  return KC_OK;
}

// rule 52's refusals in its order: counts, range_max (and Rc), flags, zq (nullptr: not looked at)
int wm_integrate_check(float res, size_t n_beams, float range_max, unsigned flags, const int32_t *zq, int *rc_out, long long *zmax_out) {
  int rc = 0;
  KC_TRY(worldmap_scan_check(res, 1, n_beams, range_max, 0u, &rc));
  if (flags & ~static_cast<unsigned>(KC_INTEGRATE_CLEAR_NO_RETURN)) KC_FAIL(KC_ERR_INVALID, "unknown integration flag bits 0x%x", flags);
  const long long zmax = std::llrint(static_cast<double>(range_max) / static_cast<double>(res) * 65536.0);
  if (zq)
    for (size_t k = 0; k < n_beams; ++k)
      if (zq[k] < -1 || zq[k] > zmax) KC_FAIL(KC_ERR_INVALID, "quantised range %zu is %d, outside -1 .. %lld", k, zq[k], zmax);
  if (rc_out) *rc_out = rc;
  if (zmax_out) *zmax_out = zmax;
  return KC_OK;
}

// The walk's box [I0 - Rc - 1, I0 + Rc + 1] x [J0 - Rc - 1, J0 + Rc + 1] clipped to the map, inclusive; false when empty
bool wm_integrate_box(const kc_worldmap *c, const kc_worldmap_pose *p, int rc, int box[4]) {
  const long long i0 = (p->tx + (1ll << 15)) >> 16, j0 = (p->ty + (1ll << 15)) >> 16;  // within 2^20 + 1 cells
  const long long lo_i = i0 - rc - 1, hi_i = i0 + rc + 1, lo_j = j0 - rc - 1, hi_j = j0 + rc + 1;
  if (hi_i < 0 || hi_j < 0 || lo_i > c->W - 1 || lo_j > c->H - 1) return false;
  box[0] = static_cast<int>(std::max<long long>(lo_i, 0));
  box[1] = static_cast<int>(std::max<long long>(lo_j, 0));
  box[2] = static_cast<int>(std::min<long long>(hi_i, c->W - 1));
  box[3] = static_cast<int>(std::min<long long>(hi_j, c->H - 1));
  return true;
}

// Rules 52 to 57.  marks_out == nullptr: the mark launch, the apply launch and the record's read-back.  Otherwise the mark
// launch alone, the plane copied into marks_out and zeroed again, the map untouched.  Check order: counts, range_max,
// flags, zq, the angles, the pose, then the device; a refused call queues nothing.
int wm_integrate(kc_worldmap *c, const kc_worldmap_pose *p, const double *angles, size_t n, const int32_t *zq, float range_max,
                 unsigned flags, kc_worldmap_result *out, uint8_t *marks_out) {
  int rc = 0;
  long long zmax = 0;
  KC_TRY(wm_integrate_check(c->res, n, range_max, flags, zq, &rc, &zmax));
  for (size_t k = 0; k < n; ++k)
    if (!std::isfinite(angles[k])) KC_FAIL(KC_ERR_INVALID, "beam angle %zu is not finite", k);
  KC_TRY(wm_check_pose(p));
  if (out) *out = kc_worldmap_result{0, -1, -1, -1, -1};
  const size_t cells = static_cast<size_t>(c->W) * static_cast<size_t>(c->H);
  int box[4];
  const bool inside = wm_integrate_box(c, p, rc, box);
  if (!inside && !marks_out) return KC_OK;  // rule 54: no crossed cell lies inside the map; nothing is launched
  KC_HIP(hipSetDevice(c->device));
  const size_t plane = (cells + 3) / 4 * 4;
  if (!c->marks_zero) {
    KC_TRY(c->d_marks.reserve(plane));
    KC_HIP(hipMemsetAsync(c->d_marks.p, 0, plane, c->stream));
  }
  c->marks_zero = false;  // until this call has put the plane back
  if (inside) {
    KC_TRY(c->d_zq.reserve(n));
    KC_TRY(c->h_zq.reserve(n));
    KC_TRY(c->scan_table.ensure(angles, n, c->stream));
    std::memcpy(c->h_zq.p, zq, n * sizeof(int32_t));
    KC_HIP(hipMemcpyAsync(c->d_zq.p, c->h_zq.p, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    WmMarkArgs m{};
    m.marks = c->d_marks.p;
    m.table = reinterpret_cast<const int2 *>(c->scan_table.d.p);
    m.zq = c->d_zq.p;
    m.pose = *p;
    m.zmax = zmax;
    m.W = c->W;
    m.H = c->H;
    m.B = static_cast<int>(n);
    m.rc = rc;
    m.clear_no_return = (flags & KC_INTEGRATE_CLEAR_NO_RETURN) ? 1 : 0;
    m.precheck = c->mark_precheck ? 1 : 0;
    c->integ_time.begin_cycle();
    KC_TRY(c->integ_time.start("mark", c->stream));
    // a crossed step stays inside rule 23's box (rule 53): at most Rc + 1 of them along one axis
    const dim3 mgrid(static_cast<unsigned>((n + kWmBlock - 1) / kWmBlock), static_cast<unsigned>((rc + 2) / kWmMarkChunk + 1));
    hipLaunchKernelGGL(worldmap_mark_kernel, mgrid, dim3(kWmBlock), 0, c->stream, m);
    KC_HIP(hipGetLastError());
    KC_TRY(c->integ_time.stop(c->stream));
  }
  if (marks_out) {
    KC_HIP(hipMemcpyAsync(marks_out, c->d_marks.p, cells, hipMemcpyDeviceToHost, c->stream));
    if (inside) KC_HIP(hipMemsetAsync(c->d_marks.p, 0, plane, c->stream));
    KC_HIP(hipStreamSynchronize(c->stream));
    c->marks_zero = true;
    return KC_OK;
  }
  WmApplyArgs a{};
  KC_TRY(c->rec.begin(c->stream, &a.rec_next));
  a.rec = c->rec.cur;
  a.marks = c->d_marks.p;
  a.evidence = c->d_evidence.p;
  a.cls = c->d_cls.p;
  a.W = c->W;
  a.i_lo = box[0];
  a.j_lo = box[1];
  a.i_hi = box[2];
  a.j_hi = box[3];
  a.m = c->m;
  KC_TRY(c->integ_time.start("apply", c->stream));
  hipLaunchKernelGGL(worldmap_integrate_apply_kernel, wm_box_grid(box), dim3(kWmLanes, kWmRows), 0, c->stream, a);
  KC_HIP(hipGetLastError());
  KC_TRY(c->integ_time.stop(c->stream));
  KC_TRY(c->rec.commit(c->stream));
  c->marks_zero = true;  // every marked cell lies in the box, and its lane has put the byte back
  const int *r = c->rec.h.p;
  out->changed = static_cast<uint32_t>(r[0]);
  if (r[0] != 0) {
    out->i_min = r[1];
    out->j_min = r[2];
    out->i_max = r[3];
    out->j_max = r[4];
    c->dirty_merge(r[1], r[2], r[3], r[4]);  // rule 57: exactly as an update's (rule 43)
  }
  return KC_OK;
}

// rule 70's refusals in its order: rule 52's without flags, then m2, gap, join_q, min_beams
int wm_movers_check(float res, size_t n_beams, float range_max, const int32_t *zq, uint32_t m2, uint32_t gap, uint64_t join_q,
                    uint32_t min_beams, long long *zmax_out) {
  KC_TRY(wm_integrate_check(res, n_beams, range_max, 0u, zq, nullptr, zmax_out));
  if (m2 == 0) KC_FAIL(KC_ERR_INVALID, "m2 must be at least 1");
  if (gap > 64u) KC_FAIL(KC_ERR_RANGE, "gap %u is above 64 beams", gap);
  if (join_q > (1ull << 40)) KC_FAIL(KC_ERR_RANGE, "join_q %llu is above 2^40", static_cast<unsigned long long>(join_q));
  if (min_beams == 0) KC_FAIL(KC_ERR_INVALID, "min_beams must be at least 1");
  if (min_beams > 65536u) KC_FAIL(KC_ERR_RANGE, "min_beams %u is above 65536", min_beams);
  return KC_OK;
}

// Rules 64 to 69.  Check order: rule 70, the angles, the pose, the plane's state; a refused call queues nothing.
int wm_movers(kc_worldmap *c, const kc_worldmap_pose *p, const double *angles, size_t n, const int32_t *zq, float range_max,
              uint32_t m2, uint32_t gap, uint64_t join_q, uint32_t min_beams, int32_t *label_out, kc_worldmap_cluster *clusters_out,
              size_t cap, kc_worldmap_movers_record *out) {
  long long zmax = 0;
  KC_TRY(wm_movers_check(c->res, n, range_max, zq, m2, gap, join_q, min_beams, &zmax));
  for (size_t k = 0; k < n; ++k)
    if (!std::isfinite(angles[k])) KC_FAIL(KC_ERR_INVALID, "beam angle %zu is not finite", k);
  KC_TRY(wm_check_pose(p));
  if (c->dist_reach == 0) KC_FAIL(KC_ERR_STATE, "finding movers needs the map's distance plane: kc_worldmap_set_distance");
  if (m2 > static_cast<uint32_t>(c->dist_reach * c->dist_reach))
    KC_FAIL(KC_ERR_STATE, "m2 = %u is above the plane's reach^2 = %d", m2, c->dist_reach * c->dist_reach);
  KC_HIP(hipSetDevice(c->device));
  const size_t labels_at = kWmMvRecBytes + KC_WORLDMAP_MAX_CLUSTERS * sizeof(kc_worldmap_cluster);
  const size_t out_bytes = labels_at + n * sizeof(int32_t);
  KC_TRY(c->d_mv_xy.reserve(2 * n));
  KC_TRY(c->d_mv_flag.reserve(n));
  KC_TRY(c->d_mv_idx.reserve(4 * n + 1));
  KC_TRY(c->d_mv_out.reserve(out_bytes));
  KC_TRY(c->h_mv_out.reserve(out_bytes));
  KC_TRY(c->d_zq.reserve(n));
  KC_TRY(c->h_zq.reserve(n));
  KC_TRY(wm_dist_refresh(c));  // rule 43
  KC_TRY(c->scan_table.ensure(angles, n, c->stream));
  std::memcpy(c->h_zq.p, zq, n * sizeof(int32_t));
  KC_HIP(hipMemcpyAsync(c->d_zq.p, c->h_zq.p, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  WmMoversArgs a{};
  a.cls = c->d_cls.p;
  a.dist2 = c->d_dist2.p;
  a.table = reinterpret_cast<const int2 *>(c->scan_table.d.p);
  a.zq = c->d_zq.p;
  a.pose = *p;
  a.zmax = zmax;
  a.join_q = join_q;
  a.m2 = m2;
  a.W = c->W;
  a.H = c->H;
  a.B = static_cast<int>(n);
  a.gap = static_cast<int>(gap);
  a.min_beams = static_cast<int>(min_beams);
  a.ex = c->d_mv_xy.p;
  a.ey = c->d_mv_xy.p + n;
  a.flag = c->d_mv_flag.p;
  a.comp = c->d_mv_idx.p;
  a.run_of = c->d_mv_idx.p + n;
  a.run_kept = c->d_mv_idx.p + 2 * n;
  a.run_start = c->d_mv_idx.p + 3 * n;
  a.rec = reinterpret_cast<kc_worldmap_movers_record *>(c->d_mv_out.p);
  a.clusters = reinterpret_cast<kc_worldmap_cluster *>(c->d_mv_out.p + kWmMvRecBytes);
  a.label = reinterpret_cast<int32_t *>(c->d_mv_out.p + labels_at);
  c->mv_time.begin_cycle();
  KC_TRY(c->mv_time.start("flag", c->stream));
  hipLaunchKernelGGL(worldmap_movers_flag_kernel, dim3(static_cast<unsigned>((n + kWmBlock - 1) / kWmBlock)), dim3(kWmBlock), 0,
                     c->stream, a);
  KC_HIP(hipGetLastError());
  KC_TRY(c->mv_time.stop(c->stream));
  KC_TRY(c->mv_time.start("cluster", c->stream));
  hipLaunchKernelGGL(worldmap_movers_cluster_kernel, dim3(1), dim3(kWmMvBlock), 0, c->stream, a);
  KC_HIP(hipGetLastError());
  KC_TRY(c->mv_time.stop(c->stream));
  KC_HIP(hipMemcpyAsync(c->h_mv_out.p, c->d_mv_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  std::memcpy(out, c->h_mv_out.p, sizeof(*out));
  const size_t n_copy = std::min<size_t>(out->n_returned, cap);
  if (n_copy > 0) std::memcpy(clusters_out, c->h_mv_out.p + kWmMvRecBytes, n_copy * sizeof(kc_worldmap_cluster));
  if (label_out) std::memcpy(label_out, c->h_mv_out.p + labels_at, n * sizeof(int32_t));
  return KC_OK;
}

void wm_clear_match_result(const kc_worldmap_pose *g, kc_worldmap_match_result *out) {
  *out = kc_worldmap_match_result{};
  if (g) out->pose = *g;
}

}  // namespace

namespace kc {

int worldmap_view(kc_worldmap *m, WorldMapView *out) {
  if (!m || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *out = WorldMapView{m->d_cls.p, m->W, m->H, m->res, m->ox(), m->oy(), m->stream, m->device, m->OI, m->OJ};
  return KC_OK;
}

int worldmap_distance_state(kc_worldmap *m, WorldMapDistance *out) {
  if (!m || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *out = WorldMapDistance{m->dist_reach ? m->d_dist2.p : nullptr, m->dist_reach};
  return KC_OK;
}

int worldmap_distance_refresh(kc_worldmap *m) {
  if (!m) KC_FAIL(KC_ERR_INVALID, "null context");
  if (m->dist_reach == 0) KC_FAIL(KC_ERR_STATE, "the map's distance plane is off");
  return wm_dist_refresh(m);
}

int worldmap_window(const WorldMapView &v, double x, double y, float max_range, WorldMapWindow *out) {
  *out = WorldMapWindow{};
  KC_TRY(wm_window(v.res, v.ox, v.oy, x, y, max_range, &out->ic, &out->jc, &out->rc));
  int box[4];
  if (!wm_window_box(v.W, v.H, out->ic, out->jc, out->rc, box)) return KC_OK;
  // rule 17's cells inside the map, row by row: what the list can hold at most
  const long long r2 = static_cast<long long>(out->rc) * out->rc;
  size_t cells = 0;
  for (int J = box[1]; J <= box[3]; ++J) {
    const long long dj = static_cast<long long>(J) - out->jc, rest = r2 - dj * dj;
    long long h = static_cast<long long>(std::sqrt(static_cast<double>(rest)));
    while (h * h > rest) --h;
    while ((h + 1) * (h + 1) <= rest) ++h;
    const long long lo = std::max<long long>(out->ic - h, 0), hi = std::min<long long>(out->ic + h, v.W - 1);
    if (lo <= hi) cells += static_cast<size_t>(hi - lo + 1);
  }
  out->max_points = cells;
  return KC_OK;
}

int worldmap_queue_points(const WorldMapView &v, const WorldMapWindow &w, float *xyz, unsigned int *cnt, unsigned int *rearm,
                          hipStream_t stream) {
  int box[4];
  if (!wm_window_box(v.W, v.H, w.ic, w.jc, w.rc, box)) KC_FAIL(KC_ERR_STATE, "an empty window has no launch");
  WmWindowArgs a{};
  a.cls = v.cls;
  a.xyz = xyz;
  a.cnt = cnt;
  a.rearm = rearm;
  a.W = v.W;
  a.i_lo = box[0];
  a.j_lo = box[1];
  a.i_hi = box[2];
  a.j_hi = box[3];
  a.ic = w.ic;
  a.jc = w.jc;
  a.r2 = static_cast<long long>(w.rc) * w.rc;
  a.res = static_cast<double>(v.res);
  a.ox = v.ox;
  a.oy = v.oy;
  hipLaunchKernelGGL(worldmap_window_points_kernel, wm_box_grid(box), dim3(kWmLanes, kWmRows), 0, stream, a);
  KC_HIP(hipGetLastError());
  return KC_OK;
}

// ---- virtual scan (rules 20 to 27) ----
int worldmap_scan_table(const double *angles, size_t n, int32_t *out) {
  for (size_t k = 0; k < n; ++k)
    if (!std::isfinite(angles[k])) KC_FAIL(KC_ERR_INVALID, "beam angle %zu is not finite", k);
  for (size_t k = 0; k < n; ++k) {
    out[2 * k] = static_cast<int32_t>(std::lrint(host_cos(angles[k]) * 1073741824.0));
    out[2 * k + 1] = static_cast<int32_t>(std::lrint(host_sin(angles[k]) * 1073741824.0));
  }
  return KC_OK;
}

int worldmap_scan_check(float res, size_t n_poses, size_t n_beams, float range_max, unsigned flags, int *rc_out) {
  if (!(res > 0.0f) || !std::isfinite(res)) KC_FAIL(KC_ERR_INVALID, "the resolution must be positive");
  if (n_poses == 0 || n_beams == 0) KC_FAIL(KC_ERR_INVALID, "a scan needs at least one pose and one beam, got %zu x %zu", n_poses, n_beams);
  if (n_beams > kWmScanMaxBeams) KC_FAIL(KC_ERR_RANGE, "%zu beams are above the cap of %zu", n_beams, kWmScanMaxBeams);
  if (n_poses > kWmScanMaxRays || n_poses * n_beams > kWmScanMaxRays)
    KC_FAIL(KC_ERR_RANGE, "%zu poses x %zu beams are above the cap of %zu rays", n_poses, n_beams, kWmScanMaxRays);
  if (!std::isfinite(range_max) || !(range_max > 0.0f))
    KC_FAIL(KC_ERR_INVALID, "range_max must be a finite float > 0, got %g", static_cast<double>(range_max));
  const double cells = std::ceil(static_cast<double>(range_max) / static_cast<double>(res));
  if (!(cells <= static_cast<double>(kWmPtsMaxRadius)))
    KC_FAIL(KC_ERR_RANGE, "a range of %g m is %g cells at %g m, above the cap of %d", static_cast<double>(range_max), cells,
            static_cast<double>(res), kWmPtsMaxRadius);
  if (flags & ~static_cast<unsigned>(KC_SCAN_UNKNOWN_BLOCKS)) KC_FAIL(KC_ERR_INVALID, "unknown scan flag bits 0x%x", flags);
  if (rc_out) *rc_out = static_cast<int>(cells);
  return KC_OK;
}

int worldmap_check_pose(const kc_worldmap_pose *p) { return wm_check_pose(p); }

int ScanTable::ensure(const double *a, size_t n, hipStream_t s) {
  if (valid && angles.size() == n && std::memcmp(angles.data(), a, n * sizeof(double)) == 0) return KC_OK;
  valid = false;
  KC_HIP(hipStreamSynchronize(s));  // an upload of the pinned copy that a failed call left queued
  KC_TRY(h.reserve(2 * n));
  KC_TRY(d.reserve(2 * n));
  KC_TRY(worldmap_scan_table(a, n, h.p));
  KC_HIP(hipMemcpyAsync(d.p, h.p, 2 * n * sizeof(int32_t), hipMemcpyHostToDevice, s));
  angles.assign(a, a + n);
  valid = true;
  return KC_OK;
}

int worldmap_queue_scan(const WorldMapView &v, const WorldMapScan &s, hipStream_t stream) {
  WmScanArgs a{};
  a.cls = v.cls;
  a.table = reinterpret_cast<const int2 *>(s.table);
  a.poses = s.dev_poses;
  a.pose = s.pose;
  a.real = s.real;
  a.ranges = s.ranges;
  a.cells = s.cells;
  a.W = v.W;
  a.H = v.H;
  a.B = static_cast<int>(s.n_beams);
  a.rc = s.rc;
  a.unknown_blocks = (s.flags & KC_SCAN_UNKNOWN_BLOCKS) ? 1 : 0;
  a.res = static_cast<double>(v.res);
  a.range_max = static_cast<double>(s.range_max);
  const dim3 grid(static_cast<unsigned>(s.n_poses), static_cast<unsigned>((s.n_beams + kWmScanBlock - 1) / kWmScanBlock));
  hipLaunchKernelGGL(worldmap_scan_kernel, grid, dim3(kWmScanBlock), 0, stream, a);
  KC_HIP(hipGetLastError());
  return KC_OK;
}

}  // namespace kc

extern "C" {

int kc_worldmap_window(float resolution, double origin_x, double origin_y, double x, double y, float max_sensor_range,
                       int32_t *ic_out, int32_t *jc_out, int32_t *rc_out) {
  if (!ic_out || !jc_out || !rc_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *ic_out = *jc_out = *rc_out = 0;
  return wm_window(resolution, origin_x, origin_y, x, y, max_sensor_range, ic_out, jc_out, rc_out);  // (writes on success only)
}

int kc_worldmap_points(kc_worldmap *c, double x, double y, float max_sensor_range, float *xyz_out, size_t cap, size_t *count_out,
                       int32_t bounds_out[4]) {
  if (!c || !count_out || !bounds_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *count_out = 0;
  bounds_out[0] = bounds_out[1] = bounds_out[2] = bounds_out[3] = -1;
  WorldMapView v{};
  KC_TRY(worldmap_view(c, &v));
  WorldMapWindow w{};
  KC_TRY(worldmap_window(v, x, y, max_sensor_range, &w));
  if (w.max_points == 0) return KC_OK;  // the window misses the map: rule 17
  KC_HIP(hipSetDevice(c->device));
  if (xyz_out) KC_TRY(c->d_pts.reserve(3 * w.max_points));
  int *rearm = nullptr;
  KC_TRY(c->pts_rec.begin(c->stream, &rearm));
  KC_TRY(worldmap_queue_points(v, w, xyz_out ? c->d_pts.p : nullptr, reinterpret_cast<unsigned int *>(c->pts_rec.cur),
                               reinterpret_cast<unsigned int *>(rearm), c->stream));
  KC_TRY(c->pts_rec.commit(c->stream));
  const int *r = c->pts_rec.h.p;
  const size_t n = static_cast<size_t>(static_cast<unsigned int>(r[0]));
  if (n > w.max_points) KC_FAIL(KC_ERR_HIP, "the window's count %zu is above its %zu cells", n, w.max_points);
  *count_out = n;
  if (n == 0) return KC_OK;
  bounds_out[0] = r[1 * kWmPtsStride];
  bounds_out[1] = r[2 * kWmPtsStride];
  bounds_out[2] = r[3 * kWmPtsStride];
  bounds_out[3] = r[4 * kWmPtsStride];
  if (!xyz_out) return KC_OK;
  if (cap < n) KC_FAIL(KC_ERR_RANGE, "%zu points do not fit the output capacity %zu", n, cap);
  KC_HIP(hipMemcpyAsync(xyz_out, c->d_pts.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  return KC_OK;
}

int kc_worldmap_scan_table(const double *angles, size_t n, int32_t *ac_as_out) {
  if (!angles || !ac_as_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  return worldmap_scan_table(angles, n, ac_as_out);
}

int kc_worldmap_scan_check(float resolution, size_t n_poses, size_t n_beams, float range_max, unsigned int flags, int32_t *rc_out) {
  if (rc_out) *rc_out = 0;
  int rc = 0;
  KC_TRY(worldmap_scan_check(resolution, n_poses, n_beams, range_max, flags, &rc));
  if (rc_out) *rc_out = rc;
  return KC_OK;
}

// Check order: null arguments; counts, angles, range_max and flags, the poses; then the device
int kc_worldmap_scan(kc_worldmap *c, const kc_worldmap_pose *poses, size_t n_poses, const double *angles, size_t n_beams,
                     float range_max, unsigned int flags, double *ranges_out, int32_t *cells_or_null) {
  if (!c || !poses || !angles || !ranges_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  WorldMapScan s{};
  KC_TRY(worldmap_scan_check(c->res, n_poses, n_beams, range_max, flags, &s.rc));
  for (size_t k = 0; k < n_beams; ++k)
    if (!std::isfinite(angles[k])) KC_FAIL(KC_ERR_INVALID, "beam angle %zu is not finite", k);
  for (size_t p = 0; p < n_poses; ++p) KC_TRY(wm_check_pose(&poses[p]));
  WorldMapView v{};
  KC_TRY(worldmap_view(c, &v));
  KC_HIP(hipSetDevice(c->device));
  const size_t rays = n_poses * n_beams, words = rays + (cells_or_null ? (rays + 1) / 2 : 0);
  KC_TRY(c->d_scan.reserve(words));
  KC_TRY(c->h_scan.reserve(words));
  KC_TRY(c->scan_table.ensure(angles, n_beams, c->stream));
  if (n_poses > 1) {
    KC_TRY(c->d_poses.reserve(n_poses));
    KC_TRY(c->h_poses.reserve(n_poses));
    std::memcpy(c->h_poses.p, poses, n_poses * sizeof(kc_worldmap_pose));
    KC_HIP(hipMemcpyAsync(c->d_poses.p, c->h_poses.p, n_poses * sizeof(kc_worldmap_pose), hipMemcpyHostToDevice, c->stream));
    s.dev_poses = c->d_poses.p;
  }
  s.table = c->scan_table.d.p;
  s.pose = poses[0];
  s.n_poses = n_poses;
  s.n_beams = n_beams;
  s.range_max = range_max;
  s.flags = flags;
  s.ranges = c->d_scan.p;
  s.cells = cells_or_null ? reinterpret_cast<int32_t *>(c->d_scan.p + rays) : nullptr;
  KC_TRY(worldmap_queue_scan(v, s, c->stream));
  KC_HIP(hipMemcpyAsync(c->h_scan.p, c->d_scan.p, words * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  std::memcpy(ranges_out, c->h_scan.p, rays * sizeof(double));
  if (cells_or_null) std::memcpy(cells_or_null, c->h_scan.p + rays, rays * sizeof(int32_t));
  return KC_OK;
}

int kc_worldmap_check_model(int hit, int miss, int e_min, int e_max, int occ_thr) {
  return wm_check_model(hit, miss, e_min, e_max, occ_thr);
}

int kc_worldmap_check_grid(float world_resolution, int grid_height, int grid_width, int central_i, int central_j,
                           float resolution) {
  return wm_check_grid(world_resolution, grid_height, grid_width, central_i, central_j, resolution);
}

int kc_worldmap_quantise_pose(float resolution, double origin_x, double origin_y, double px, double py, double yaw,
                              kc_worldmap_pose *out) {
  if (!out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *out = kc_worldmap_pose{0, 0, 0, 0};
  if (!(resolution > 0.0f) || !std::isfinite(resolution)) KC_FAIL(KC_ERR_INVALID, "the resolution must be positive");
  if (!std::isfinite(origin_x) || !std::isfinite(origin_y) || !std::isfinite(px) || !std::isfinite(py) || !std::isfinite(yaw))
    KC_FAIL(KC_ERR_INVALID, "the pose and the origin must be finite");
  const double R = static_cast<double>(resolution);
  const double fx = (px - origin_x) / R * 65536.0, fy = (py - origin_y) / R * 65536.0;
  const double cap = static_cast<double>(kQ16MaxOffset);
  if (!(std::fabs(fx) <= cap + 0.5) || !(std::fabs(fy) <= cap + 0.5))
    KC_FAIL(KC_ERR_RANGE, "the pose lies more than 2^20 cells from the map's origin");
  kc_worldmap_pose p;
  p.cq = static_cast<int32_t>(std::lrint(std::cos(yaw) * 65536.0));
  p.sq = static_cast<int32_t>(std::lrint(std::sin(yaw) * 65536.0));
  p.tx = static_cast<int64_t>(std::llrint(fx));
  p.ty = static_cast<int64_t>(std::llrint(fy));
  KC_TRY(wm_check_pose(&p));
  *out = p;
  return KC_OK;
}

int kc_worldmap_create(int device, int width, int height, float resolution, double origin_x, double origin_y,
                       kc_worldmap **out) {
  if (!out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *out = nullptr;
  KC_TRY(wm_check_shape(width, height, resolution));
  if (!std::isfinite(origin_x) || !std::isfinite(origin_y)) KC_FAIL(KC_ERR_INVALID, "the map's origin must be finite");
  hipStream_t stream = nullptr;
  KC_TRY(open_device_stream(device, &stream));
  auto *c = new kc_worldmap();
  c->device = device;
  c->stream = stream;
  c->W = width;
  c->H = height;
  c->res = resolution;
  c->ox0 = origin_x;
  c->oy0 = origin_y;
  const int rec_start[kWmRecWords] = {0, INT_MAX, INT_MAX, -1, -1};  // what worldmap_update_kernel puts back
  c->rec.start.assign(rec_start, rec_start + kWmRecWords);
  std::vector<int> &pts_start = c->pts_rec.start;  // ... and worldmap_window_points_kernel
  pts_start.assign(5 * kWmPtsStride, 0);
  pts_start[1 * kWmPtsStride] = pts_start[3 * kWmPtsStride] = INT_MAX;
  pts_start[2 * kWmPtsStride] = pts_start[4 * kWmPtsStride] = INT_MIN;
  const size_t n = static_cast<size_t>(width) * static_cast<size_t>(height);
  int rc;
  if ((rc = c->d_evidence.reserve(n)) || (rc = c->d_cls.reserve(n)) || (rc = c->rec.arm(c->stream)) ||
      (rc = wm_take_prior(c, nullptr, 1))) {
    kc_worldmap_destroy(c);
    return rc;
  }
  *out = c;
  return KC_OK;
}

void kc_worldmap_destroy(kc_worldmap *c) {
  if (!c) return;
  close_device_stream(c->device, &c->stream);
  delete c;  // (the device is current: the buffers and the event go with the context)
}

int kc_worldmap_info(kc_worldmap *c, int *width_out, int *height_out, float *resolution_out, double *origin_x_out,
                     double *origin_y_out) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (width_out) *width_out = c->W;
  if (height_out) *height_out = c->H;
  if (resolution_out) *resolution_out = c->res;
  if (origin_x_out) *origin_x_out = c->ox();  // rule 46
  if (origin_y_out) *origin_y_out = c->oy();
  return KC_OK;
}

int kc_worldmap_set_model(kc_worldmap *c, int hit, int miss, int e_min, int e_max, int occ_thr) {
  KC_TRY(wm_check_model(hit, miss, e_min, e_max, occ_thr));
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  KC_HIP(hipSetDevice(c->device));
  c->m = WmModel{hit, miss, e_min, e_max, occ_thr};
  return wm_take_prior(c, nullptr, 1);  // evidence counted by another model means nothing under this one
}

int kc_worldmap_clear(kc_worldmap *c) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  KC_HIP(hipSetDevice(c->device));
  return wm_take_prior(c, nullptr, 1);
}

int kc_worldmap_set_prior_host(kc_worldmap *c, const void *grid, int elem_bytes, int width, int height) {
  KC_TRY(wm_check_prior(c, grid, elem_bytes, width, height));
  KC_HIP(hipSetDevice(c->device));
  const size_t nbytes = static_cast<size_t>(width) * static_cast<size_t>(height) * static_cast<size_t>(elem_bytes);
  KC_TRY(wm_stage(c, grid, nbytes));
  return wm_take_prior(c, c->d_stage.p, elem_bytes);
}

int kc_worldmap_set_prior_device(kc_worldmap *c, const void *dev_grid, int elem_bytes, int width, int height) {
  KC_TRY(wm_check_prior(c, dev_grid, elem_bytes, width, height));
  KC_HIP(hipSetDevice(c->device));
  const size_t nbytes = static_cast<size_t>(width) * static_cast<size_t>(height) * static_cast<size_t>(elem_bytes);
  KC_TRY(check_device_range(c->device, dev_grid, 0, static_cast<long long>(nbytes), static_cast<size_t>(elem_bytes), "prior"));
  return wm_take_prior(c, dev_grid, elem_bytes);
}

int kc_worldmap_after_stream(kc_worldmap *c, void *stream) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  return stream_wait_for(c->device, c->stream, stream);
}

int kc_worldmap_update_device(kc_worldmap *c, const int32_t *dev_grid, int grid_height, int grid_width, int central_i,
                              int central_j, float resolution, const kc_worldmap_pose *pose, kc_worldmap_result *out) {
  if (!c || !dev_grid || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  const GridSource src{GridSource::Device, {dev_grid, grid_height, grid_width, central_i, central_j, resolution}, nullptr};
  return wm_update(c, src, pose, out);
}

int kc_worldmap_update_host(kc_worldmap *c, const int32_t *grid, int grid_height, int grid_width, int central_i,
                            int central_j, float resolution, const kc_worldmap_pose *pose, kc_worldmap_result *out) {
  if (!c || !grid || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  const GridSource src{GridSource::Host, {grid, grid_height, grid_width, central_i, central_j, resolution}, nullptr};
  return wm_update(c, src, pose, out);
}

int kc_worldmap_update_from_mapper(kc_worldmap *c, kc_mapper *mapper, const kc_worldmap_pose *pose, kc_worldmap_result *out) {
  if (!c || !mapper || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  return wm_update(c, GridSource{GridSource::Mapper, {}, mapper}, pose, out);
}

int kc_worldmap_offset(kc_worldmap *c, int32_t *oi_out, int32_t *oj_out) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (oi_out) *oi_out = c->OI;
  if (oj_out) *oj_out = c->OJ;
  return KC_OK;
}

// Check order: the context, the offset cap, then the device
int kc_worldmap_shift(kc_worldmap *c, int di, int dj) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  KC_TRY(wm_check_shift(c->OI, c->OJ, di, dj));
  return wm_shift(c, di, dj);
}

int kc_worldmap_check_shift(int32_t oi, int32_t oj, int di, int dj) { return wm_check_shift(oi, oj, di, dj); }

int kc_worldmap_recentre_plan(int width, int height, int ic, int jc, int margin, int stride, int32_t *di_out, int32_t *dj_out) {
  if (!di_out || !dj_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *di_out = *dj_out = 0;
  int di = 0, dj = 0;
  KC_TRY(wm_recentre_plan(width, height, ic, jc, margin, stride, &di, &dj));
  *di_out = di;
  *dj_out = dj;
  return KC_OK;
}

// Check order: null arguments, the policy, the position (rule 16 at the current origin), the offset cap, then the device
int kc_worldmap_recentre(kc_worldmap *c, double x, double y, int margin, int stride, int32_t *di_out, int32_t *dj_out) {
  if (!c || !di_out || !dj_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *di_out = *dj_out = 0;
  int di = 0, dj = 0;
  KC_TRY(wm_recentre_plan(c->W, c->H, 0, 0, margin, stride, &di, &dj));  // the policy alone
  kc_worldmap_pose p;
  KC_TRY(kc_worldmap_quantise_pose(c->res, c->ox(), c->oy(), x, y, 0.0, &p));
  const int ic = static_cast<int>((p.tx + (1ll << 15)) >> 16), jc = static_cast<int>((p.ty + (1ll << 15)) >> 16);
  KC_TRY(wm_recentre_plan(c->W, c->H, ic, jc, margin, stride, &di, &dj));
  KC_TRY(wm_check_shift(c->OI, c->OJ, di, dj));
  KC_TRY(wm_shift(c, di, dj));
  *di_out = di;
  *dj_out = dj;
  return KC_OK;
}

int kc_worldmap_integrate_check(float resolution, size_t n_beams, float range_max, unsigned int flags, const int32_t *zq_or_null,
                                int32_t *rc_out, int64_t *zmax_out) {
  if (rc_out) *rc_out = 0;
  if (zmax_out) *zmax_out = 0;
  int rc = 0;
  long long zmax = 0;
  KC_TRY(wm_integrate_check(resolution, n_beams, range_max, flags, zq_or_null, &rc, &zmax));
  if (rc_out) *rc_out = rc;
  if (zmax_out) *zmax_out = zmax;
  return KC_OK;
}

// rule 52, a beam a turn of the loop; the comparisons are written so that a NaN falls into the first
int kc_worldmap_quantise_ranges(float resolution, const double *ranges, size_t n, float range_max, float range_min, int32_t *zq_out) {
  if (!ranges || !zq_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  long long zmax = 0;
  KC_TRY(wm_integrate_check(resolution, n, range_max, 0u, nullptr, nullptr, &zmax));
  if (!std::isfinite(range_min) || range_min < 0.0f) KC_FAIL(KC_ERR_INVALID, "range_min must be a finite float >= 0, got %g", static_cast<double>(range_min));
  const double r = static_cast<double>(resolution), lo = static_cast<double>(range_min), hi = static_cast<double>(range_max);
  for (size_t k = 0; k < n; ++k) {
    const double z = ranges[k];
    if (!(z >= 0.0) || z < lo) zq_out[k] = -1;  // a NaN, a negative range (-0.0 is not one), a range below range_min
    else if (z >= hi) zq_out[k] = static_cast<int32_t>(zmax);  // +inf included
    else zq_out[k] = static_cast<int32_t>(std::llrint(z / r * 65536.0));
  }
  return KC_OK;
}

int kc_worldmap_integrate(kc_worldmap *c, const kc_worldmap_pose *pose, const double *angles, size_t n_beams, const int32_t *zq,
                          float range_max, unsigned int flags, kc_worldmap_result *out) {
  if (!c || !pose || !angles || !zq || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  return wm_integrate(c, pose, angles, n_beams, zq, range_max, flags, out, nullptr);
}

int kc_worldmap_integrate_marks(kc_worldmap *c, const kc_worldmap_pose *pose, const double *angles, size_t n_beams,
                                const int32_t *zq, float range_max, unsigned int flags, uint8_t *marks_out, size_t cap) {
  if (!c || !pose || !angles || !zq || !marks_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  const size_t cells = static_cast<size_t>(c->W) * static_cast<size_t>(c->H);
  if (cells > cap) KC_FAIL(KC_ERR_RANGE, "%zu cells do not fit the output capacity %zu", cells, cap);
  return wm_integrate(c, pose, angles, n_beams, zq, range_max, flags, nullptr, marks_out);
}

int kc_worldmap_integrate_set_precheck(kc_worldmap *c, int enable) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  c->mark_precheck = enable != 0;
  return KC_OK;
}

int kc_worldmap_integrate_set_timing(kc_worldmap *c, int enable) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  c->integ_time.enabled = enable != 0;
  c->integ_time.begin_cycle();
  return KC_OK;
}

int kc_worldmap_integrate_times(kc_worldmap *c, float ms_out[2]) {
  if (!c || !ms_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (!c->integ_time.enabled || c->integ_time.used != 2) KC_FAIL(KC_ERR_STATE, "no integration has been timed on this map");
  KC_HIP(hipSetDevice(c->device));
  size_t n = 0;
  return c->integ_time.get(nullptr, ms_out, 2, &n);
}

int kc_worldmap_movers_check(float resolution, size_t n_beams, float range_max, const int32_t *zq_or_null, uint32_t m2, uint32_t gap,
                             uint64_t join_q, uint32_t min_beams, int64_t *zmax_out) {
  if (zmax_out) *zmax_out = 0;
  long long zmax = 0;
  KC_TRY(wm_movers_check(resolution, n_beams, range_max, zq_or_null, m2, gap, join_q, min_beams, &zmax));
  if (zmax_out) *zmax_out = zmax;
  return KC_OK;
}

int kc_worldmap_movers(kc_worldmap *c, const kc_worldmap_pose *pose, const double *angles, size_t n_beams, const int32_t *zq,
                       float range_max, uint32_t m2, uint32_t gap, uint64_t join_q, uint32_t min_beams, int32_t *label_out_or_null,
                       kc_worldmap_cluster *clusters_out, size_t cap, kc_worldmap_movers_record *record_out) {
  if (record_out) *record_out = kc_worldmap_movers_record{};
  if (!c || !pose || !angles || !zq || !record_out || (!clusters_out && cap > 0)) KC_FAIL(KC_ERR_INVALID, "null argument");
  return wm_movers(c, pose, angles, n_beams, zq, range_max, m2, gap, join_q, min_beams, label_out_or_null, clusters_out, cap,
                   record_out);
}

int kc_worldmap_movers_set_timing(kc_worldmap *c, int enable) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  c->mv_time.enabled = enable != 0;
  c->mv_time.begin_cycle();
  return KC_OK;
}

int kc_worldmap_movers_times(kc_worldmap *c, float ms_out[2]) {
  if (!c || !ms_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (!c->mv_time.enabled || c->mv_time.used != 2) KC_FAIL(KC_ERR_STATE, "no detection has been timed on this map");
  KC_HIP(hipSetDevice(c->device));
  size_t n = 0;
  return c->mv_time.get(nullptr, ms_out, 2, &n);
}

int kc_worldmap_grid_device(kc_worldmap *c, void **dev_cls_int8) {
  if (!c || !dev_cls_int8) KC_FAIL(KC_ERR_INVALID, "null argument");
  *dev_cls_int8 = c->d_cls.p;
  return KC_OK;
}

int kc_worldmap_get(kc_worldmap *c, int8_t *cls_out, int8_t *evidence_out, size_t cap) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  const size_t n = static_cast<size_t>(c->W) * static_cast<size_t>(c->H);
  if (n > cap) KC_FAIL(KC_ERR_RANGE, "%zu cells do not fit the output capacity %zu", n, cap);
  KC_HIP(hipSetDevice(c->device));
  if (cls_out) KC_HIP(hipMemcpyAsync(cls_out, c->d_cls.p, n, hipMemcpyDeviceToHost, c->stream));
  if (evidence_out) KC_HIP(hipMemcpyAsync(evidence_out, c->d_evidence.p, n, hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  return KC_OK;
}

int kc_worldmap_set_distance(kc_worldmap *c, int reach, unsigned int flags) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (reach < 0 || reach > KC_WORLDMAP_DIST_MAX_REACH)
    KC_FAIL(KC_ERR_RANGE, "reach must be in 0 .. %d cells, got %d", KC_WORLDMAP_DIST_MAX_REACH, reach);
  if ((flags & ~static_cast<unsigned>(KC_WORLDMAP_DIST_UNKNOWN_BLOCKS)) || (reach == 0 && flags))
    KC_FAIL(KC_ERR_INVALID, "unknown distance flag bits 0x%x", flags);
  KC_HIP(hipSetDevice(c->device));
  KC_HIP(hipStreamSynchronize(c->stream));  // a refresh in flight still writes the plane
  c->dist_reach = 0;
  c->dist_flags = 0;
  c->dist_last[0] = c->dist_last[1] = c->dist_last[2] = c->dist_last[3] = -1;
  c->dist_last_full = false;
  if (reach == 0) {
    c->d_dist2.release();
    c->d_rowd.release();
    return KC_OK;
  }
  KC_TRY(c->d_dist2.reserve(static_cast<size_t>(c->W) * static_cast<size_t>(c->H)));
  c->dist_reach = reach;
  c->dist_flags = flags;
  c->dirty_all();
  return KC_OK;
}

int kc_worldmap_distance_info(kc_worldmap *c, int *reach_out, unsigned int *flags_out, int last_box[4], int *last_full_out) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (reach_out) *reach_out = c->dist_reach;
  if (flags_out) *flags_out = c->dist_flags;
  if (last_box) std::memcpy(last_box, c->dist_last, sizeof(c->dist_last));
  if (last_full_out) *last_full_out = c->dist_last_full ? 1 : 0;
  return KC_OK;
}

int kc_worldmap_distance_refresh(kc_worldmap *c) { return worldmap_distance_refresh(c); }

int kc_worldmap_get_distance(kc_worldmap *c, uint16_t *out, size_t cap) {
  if (!c || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (c->dist_reach == 0) KC_FAIL(KC_ERR_STATE, "the map's distance plane is off");
  const size_t n = static_cast<size_t>(c->W) * static_cast<size_t>(c->H);
  if (n > cap) KC_FAIL(KC_ERR_RANGE, "%zu cells do not fit the output capacity %zu", n, cap);
  KC_TRY(wm_dist_refresh(c));
  KC_HIP(hipMemcpyAsync(out, c->d_dist2.p, n * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  return KC_OK;
}

int kc_worldmap_distance_device(kc_worldmap *c, void **ptr) {
  if (!c || !ptr) KC_FAIL(KC_ERR_INVALID, "null argument");
  *ptr = nullptr;
  if (c->dist_reach == 0) KC_FAIL(KC_ERR_STATE, "the map's distance plane is off");
  KC_TRY(wm_dist_refresh(c));
  KC_HIP(hipStreamSynchronize(c->stream));
  *ptr = c->d_dist2.p;
  return KC_OK;
}

int kc_worldmap_match_check_window(int n_yaw, double yaw_step, int reach) { return wm_check_window(n_yaw, yaw_step, reach); }

int kc_worldmap_match_check_grid(float world_resolution, int grid_height, int grid_width, int central_i, int central_j,
                                 float resolution) {
  return wm_check_match_grid(world_resolution, grid_height, grid_width, central_i, central_j, resolution);
}

int kc_worldmap_match_rotations(double yaw, int n_yaw, double yaw_step, kc_worldmap_rotation *out, size_t cap) {
  KC_TRY(wm_check_window(n_yaw, yaw_step, 0));
  if (!out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (!std::isfinite(yaw)) KC_FAIL(KC_ERR_INVALID, "the yaw must be finite");
  if (cap < static_cast<size_t>(2 * n_yaw + 1)) KC_FAIL(KC_ERR_RANGE, "%d rotations do not fit the output capacity %zu", 2 * n_yaw + 1, cap);
  for (int k = -n_yaw; k <= n_yaw; ++k) {
    const double yk = yaw + static_cast<double>(k) * yaw_step;
    out[k + n_yaw].cq = static_cast<int32_t>(std::lrint(std::cos(yk) * 65536.0));
    out[k + n_yaw].sq = static_cast<int32_t>(std::lrint(std::sin(yk) * 65536.0));
  }
  return KC_OK;
}

int kc_worldmap_match_device(kc_worldmap *c, const int32_t *dev_grid, int grid_height, int grid_width, int central_i,
                             int central_j, float resolution, const kc_worldmap_pose *guess, const kc_worldmap_rotation *rotations,
                             int n_yaw, int reach, kc_worldmap_match_result *out) {
  if (!c || !dev_grid || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  wm_clear_match_result(guess, out);
  const GridSource src{GridSource::Device, {dev_grid, grid_height, grid_width, central_i, central_j, resolution}, nullptr};
  return wm_match(c, src, guess, rotations, n_yaw, reach, out);
}

int kc_worldmap_match_host(kc_worldmap *c, const int32_t *grid, int grid_height, int grid_width, int central_i, int central_j,
                           float resolution, const kc_worldmap_pose *guess, const kc_worldmap_rotation *rotations, int n_yaw,
                           int reach, kc_worldmap_match_result *out) {
  if (!c || !grid || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  wm_clear_match_result(guess, out);
  const GridSource src{GridSource::Host, {grid, grid_height, grid_width, central_i, central_j, resolution}, nullptr};
  return wm_match(c, src, guess, rotations, n_yaw, reach, out);
}

int kc_worldmap_match_from_mapper(kc_worldmap *c, kc_mapper *mapper, const kc_worldmap_pose *guess,
                                  const kc_worldmap_rotation *rotations, int n_yaw, int reach, kc_worldmap_match_result *out) {
  if (!c || !mapper || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  wm_clear_match_result(guess, out);
  return wm_match(c, GridSource{GridSource::Mapper, {}, mapper}, guess, rotations, n_yaw, reach, out);
}

int kc_worldmap_match_scores(kc_worldmap *c, uint32_t *out, size_t cap) {
  if (!c || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (c->match_K < 0) KC_FAIL(KC_ERR_STATE, "no match has been made on this map");
  const int T = 2 * c->match_S + 1;
  const size_t n = static_cast<size_t>(2 * c->match_K + 1) * T * T;
  if (n > cap) KC_FAIL(KC_ERR_RANGE, "%zu scores do not fit the output capacity %zu", n, cap);
  KC_HIP(hipSetDevice(c->device));
  KC_HIP(hipMemcpyAsync(out, c->d_scores.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  return KC_OK;
}

int kc_worldmap_match_set_timing(kc_worldmap *c, int enable) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  c->match_time.enabled = enable != 0;
  c->match_time.begin_cycle();
  return KC_OK;
}

int kc_worldmap_match_times(kc_worldmap *c, float ms_out[4]) {
  if (!c || !ms_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (!c->match_time.enabled || c->match_time.used != 4) KC_FAIL(KC_ERR_STATE, "no match has been timed on this map");
  KC_HIP(hipSetDevice(c->device));
  size_t n = 0;
  return c->match_time.get(nullptr, ms_out, 4, &n);
}

}  // extern "C"
