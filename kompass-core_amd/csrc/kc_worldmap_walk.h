// The world map's ray walk (DESIGN.md 4.11 rules 20 to 23 and 25) as one __device__ function: worldmap_scan_kernel
// (kc_worldmap.hip) turns its result into a double range, mcl_walk_kernel (kc_mcl.hip) into an integer one.  With it
// the one blocking predicate of the map's readers and the distance plane's lookup (kc_mcl.hip, kc_mppi.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kc_q16.h"
#include "kompass_hip.h"

namespace kc {

constexpr int kWmScanS = 8;    // steps of the walk a round: their byte loads are in flight together
constexpr int kWmScanEnd = 1;  // a step outside rule 23's box; no cls byte has this value

// a class byte that ends a beam and seeds the distance plane
__device__ __forceinline__ bool wm_blocks(int v, int unknown_blocks) {
  return v == KC_OCCUPIED || (unknown_blocks && v == KC_UNEXPLORED);
}

// rules 42 to 45: the distance plane at cell (I, J), KC_WORLDMAP_DIST_FAR outside the map and for a lane with nothing to
// look up (live false: an MPPI sample that has hit); one 2-byte load behind one chain of tests (a test of `live` around
// the call instead changed the roll-out's instructions).  Then the penalty of that entry from a table of c2 + 1
__device__ __forceinline__ unsigned wm_dist2_at(const unsigned short *dist2, int W, int H, long long I, long long J, bool live = true) {
  unsigned d2 = KC_WORLDMAP_DIST_FAR;
  if (live && I >= 0 && I < W && J >= 0 && J < H) d2 = dist2[static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(W)];
  return d2;
}
__device__ __forceinline__ unsigned wm_dist2_pen(unsigned d2, int c2, const unsigned short *pen_d2, unsigned pen_far) {
  return d2 <= static_cast<unsigned>(c2) ? pen_d2[d2] : pen_far;
}

// the first blocking cell of a walk: rule 23's candidate (I, J, e, a); a start cell that blocks has e = 0, a = 1
struct WmWalkHit {
  int e, a, i, j;
};

// One beam of table entry t = (ac, as) from pose p over the W x H plane cls, box Rc + 1.  -> true with *h filled when a
// cell blocks, false when the walk leaves the box (or is given up) without one.  The walk's addresses do not depend on the
// bytes it loads, so a round forms kWmScanS steps ahead, loads their bytes together (a step outside the map loads cell 0
// and drops it: no branch around a load), and only then looks for the first one that ends the beam.  D = ex |dy| - ey |dx|
// is kept by addition.  beyond(e, a): between rounds the walk is given up once the last step's own distance is beyond the
// caller's range: the distance never decreases along a walk, so no later cell could count.
template <typename Beyond>
__device__ __forceinline__ bool wm_walk(const int8_t *__restrict__ cls, int W, int H, int rc, int unknown_blocks,
                                        const kc_worldmap_pose &p, int2 t, Beyond beyond, WmWalkHit *h) {
  const long long cq = p.cq, sq = p.sq;
  const int dx = static_cast<int>(q16_turn_x(cq, sq, t.x, t.y)), dy = static_cast<int>(q16_turn_y(cq, sq, t.x, t.y));
  const long long X0 = p.tx + (1ll << 15), Y0 = p.ty + (1ll << 15);
  const int I0 = static_cast<int>(X0 >> 16), J0 = static_cast<int>(Y0 >> 16);
  const int fx = static_cast<int>(X0 & 0xFFFF), fy = static_cast<int>(Y0 & 0xFFFF);
  const int sx = dx > 0 ? 1 : -1, sy = dy > 0 ? 1 : -1;
  const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
  int ex = dx > 0 ? 65536 - fx : fx, ey = dy > 0 ? 65536 - fy : fy;
  long long D = static_cast<long long>(ex) * ady - static_cast<long long>(ey) * adx;
  const long long step_x = 65536ll * ady, step_y = 65536ll * adx;
  const bool only_x = dy == 0, only_y = dx == 0;
  const int box = rc + 1;
  int I = I0, J = J0;
  if (I0 >= 0 && I0 < W && J0 >= 0 && J0 < H &&
      wm_blocks(cls[static_cast<size_t>(I0) + static_cast<size_t>(J0) * static_cast<size_t>(W)], unknown_blocks)) {
    *h = WmWalkHit{0, 1, I0, J0};  // rule 23: e = 0
    return true;
  }
  // every step leaves a cell, so 2 (Rc + 2) steps leave the box along one axis: the count only bounds the loop
  const int max_rounds = (2 * (rc + 2)) / kWmScanS + 2;
  for (int round = 0; round < max_rounds; ++round) {
    const int Is = I, Js = J;
    int es[kWmScanS], v[kWmScanS];
    unsigned xmask = 0u;
#pragma unroll
    for (int s = 0; s < kWmScanS; ++s) {
      if (only_x || (!only_y && D <= 0)) {
        es[s] = ex;
        I += sx;
        ex += 65536;
        D += step_x;
        xmask |= 1u << s;
      } else {
        es[s] = ey;
        J += sy;
        ey += 65536;
        D -= step_y;
      }
      const int di = I - I0, dj = J - J0;
      const bool out = di > box || di < -box || dj > box || dj < -box;
      const bool in = !out && I >= 0 && I < W && J >= 0 && J < H;
      const size_t cell = in ? static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(W) : size_t{0};
      const int byte = cls[cell];
      v[s] = out ? kWmScanEnd : (in ? byte : static_cast<int>(KC_EMPTY));
    }
#pragma unroll
    for (int s = 0; s < kWmScanS; ++s) {
      if (v[s] == kWmScanEnd) return false;
      if (wm_blocks(v[s], unknown_blocks)) {
        const int nx = __popc(xmask & ((2u << s) - 1u));
        *h = WmWalkHit{es[s], (xmask >> s) & 1u ? adx : ady, Is + sx * nx, Js + sy * (s + 1 - nx)};
        return true;
      }
    }
    if (beyond(es[kWmScanS - 1], (xmask >> (kWmScanS - 1)) & 1u ? adx : ady)) return false;
  }
  return false;
}

}  // namespace kc
