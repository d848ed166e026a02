// Monte-Carlo localisation over the world map (kc_mcl_*; DESIGN.md 4.11 rules 28 to 41, 44 and 45, 59 to 62).
//
// Nothing in the reference to restate: it leaves localisation, like the world map, to its ROS side.  N particles
// (TX, TY, h, acc) live on the device; a step advances them by an odometry increment with counter-based integer noise,
// ray-casts the map in place for every particle x beam with the scan's own walk (kc_worldmap_walk.h), sums a table
// penalty per particle, and reduces the weights to one record the host turns into an estimate.  Integers only, exact
// sums: no result depends on thread order, and tests/worldmap_mcl_ref.py states every rule in Python ints.  The scalar
// rules (clamp, mix64, draw, noise, motion step, weight entry) are kc_q16.h's, the plane lookup kc_worldmap_walk.h's, the
// heading table, the table checks and uploads kc_internal.h's (kc_common.hip): kc_mppi.hip uses the same ones.
//
// Launches: a step is mcl_walk_kernel + mcl_weigh_kernel and the read-back of the record; a resample is
// mcl_prefix_kernel + mcl_select_kernel without a read-back.
//  (a) mcl_walk_kernel: ray r = particle r / B, beam r % B, so consecutive beams of consecutive particles sit on
//      consecutive lanes and every lane but the last workgroup's tail has a ray, whatever B is.  Each ray recomputes its
//      particle's predict step (six mix64, a few products: nothing next to a walk) from the OLD state buffer; beam 0
//      stores it into the NEW one, so no ray reads what another writes.  pen lies in LDS.  A wavefront reduces the
//      penalties of equal particles by a segmented shuffle-down (the segments are contiguous), each segment's first lane
//      adds its sum to cost[p] with one uint32 atomic: integer adds only, exact in any order.
//  (a') mcl_field_kernel (rules 44 and 45, after kc_mcl_set_field_model) in its place: the same lane order, predict step
//      (mcl_predict) and segmented sum (mcl_segment_add); a ray looks its endpoint's cell up in the map's distance plane,
//      one 2-byte load behind the bounds test, pen_d2 in LDS.
//  (b) mcl_weigh_kernel: one workgroup of 1024.  Pass 1 forms acc and the packed minimum (acc << 32 | p: the lowest
//      index among equals), pass 2 the weights and the record's sums.  w (x - x_best) can reach 2^57 and 65536 of them
//      2^73: each product is split into its low 32 bits and the rest, both summed in 64 bits and joined once at the end.
//      It leaves cost at 0 for the next step and amin in the state word rule 35 calls min_prev.  Pass 1 also reduces
//      rule 59's fit from the costs it reads anyway (their sum, their minimum, the best particle's), in the exchange of
//      the packed minimum; the fit is written behind the record and read back with it.  Each pass has ONE exchange
//      through LDS (three values, then the eight sums) and thread 0 alone adds the partials up: with every thread
//      adding all of them up eight times the kernel spilled registers to scratch.
//  (c) mcl_prefix_kernel: one workgroup; a lane sums a contiguous chunk, the 1024 partials are scanned in LDS.
//  (d) mcl_select_kernel: a lane a slot, a binary search over the prefix; reads the current state buffer and writes the
//      other one.
//  (e) global init: row counts of KC_EMPTY (a workgroup a row), the prefix over rows on the host, then a wavefront a
//      particle: a binary search for the row and a ballot walk along it.
//  (f) mcl_shift_kernel (rule 50): the map's window moved by whole cells since the particles were last touched; a lane a
//      particle takes the difference out of (TX, TY) in place, clamped as every state is.  Applied lazily by the entries
//      that read or write particles.
//  (g) injecting resample (rule 62): (e)'s row counts, mcl_row_prefix_kernel (one workgroup, the exclusive prefix over the
//      rows, chunked as (c) is), then (c) and (d) over all N slots, then mcl_inject_kernel: a wavefront an injected slot
//      reads n_free on the device and overwrites the slot by (e)'s search and ballot walk.  No read-back, but the call
//      waits for the stream: its kernels read the map's plane, which the map's next writer must not find half read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kc_internal.h"
#include "kc_worldmap_walk.h"
#include "kompass_hip.h"

namespace kc {

constexpr int kMclBlock = 256;
constexpr int kMclOne = 1024;  // the single-workgroup kernels
constexpr unsigned kMclAccCap = 1u << 30;

struct MclState {  // one of the two state buffers
  long long *tx, *ty;
  unsigned *h;
};

// what rule 31 needs, shared by both sensor models' kernels
struct MclPredictArgs {
  const int2 *heading;  // rule 29: (Cq, Sq) a heading
  MclState in, out;
  unsigned long long key;
  long long d_f, d_l;
  int d_h, s_f, s_l, s_h;
};

// rule 31 for particle p from the OLD state buffer, the heading before the step; the ray of beam 0 stores it into the
// NEW one, so no ray reads what another writes
__device__ __forceinline__ kc_worldmap_pose mcl_predict(const MclPredictArgs &a, int p, bool store) {
  const unsigned h0 = a.in.h[p];
  const int2 cs0 = a.heading[h0];
  const long long C = cs0.x, S = cs0.y;
  const long long F = a.d_f + q16_noise(q16_draw(a.key, p, 0), a.s_f);
  const long long L = a.d_l + q16_noise(q16_draw(a.key, p, 1), a.s_l);
  kc_worldmap_pose pose;
  pose.tx = q16_move_x(a.in.tx[p], C, S, F, L);
  pose.ty = q16_move_y(a.in.ty[p], C, S, F, L);
  const unsigned h1 =
      static_cast<unsigned>((static_cast<long long>(h0) + a.d_h + q16_noise(q16_draw(a.key, p, 2), a.s_h)) & 0xFFFF);
  const int2 cs1 = a.heading[h1];
  pose.cq = cs1.x;
  pose.sq = cs1.y;
  if (store) {
    a.out.tx[p] = pose.tx;
    a.out.ty[p] = pose.ty;
    a.out.h[p] = h1;
  }
  return pose;
}

// The penalties c of the rays of equal particles p (contiguous lanes; -1: no ray) summed over the wavefront by a
// segmented shuffle-down; each segment's first lane adds its sum to cost[p] with one uint32 atomic.  Every lane of the
// wavefront calls it.
__device__ __forceinline__ void mcl_segment_add(unsigned *cost, int p, unsigned c, bool live) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned c2 = __shfl_down(c, off);
    const int p2 = __shfl_down(p, off);
    if (lane + off < 64 && p2 == p) c += c2;
  }
  const int before = __shfl_up(p, 1);
  if (live && (lane == 0 || before != p)) atomicAdd(&cost[p], c);
}

// rule 50: TX' = clamp(TX - (di << 16)), TY alike; sx = di << 16 and sy = dj << 16 formed on the host
__global__ __launch_bounds__(kMclBlock) void mcl_shift_kernel(MclState st, long long sx, long long sy, int N) {
  const int p = static_cast<int>(blockIdx.x) * kMclBlock + static_cast<int>(threadIdx.x);
  if (p >= N) return;
  st.tx[p] = q16_clamp(st.tx[p] - sx);
  st.ty[p] = q16_clamp(st.ty[p] - sy);
}

struct MclWalkArgs {
  MclPredictArgs pre;
  const int8_t *cls;
  const int2 *table;    // rule 21: (ac, as) a beam
  const int *zq;        // rule 33
  const unsigned short *pen;
  unsigned *cost;
  long long zmax;
  int W, H, N, B, rc, unknown_blocks, E, err_shift;
};

__global__ __launch_bounds__(kMclBlock) void mcl_walk_kernel(MclWalkArgs a) {
  __shared__ unsigned short s_pen[KC_MCL_MAX_TABLE];
  for (int i = threadIdx.x; i < a.E; i += kMclBlock) s_pen[i] = a.pen[i];
  __syncthreads();
  const unsigned ray = blockIdx.x * kMclBlock + threadIdx.x;  // N B <= 2^22
  const bool live = ray < static_cast<unsigned>(a.N) * static_cast<unsigned>(a.B);
  int p = -1;
  unsigned c = 0;
  if (live) {
    p = static_cast<int>(ray / static_cast<unsigned>(a.B));
    const int k = static_cast<int>(ray - static_cast<unsigned>(p) * static_cast<unsigned>(a.B));
    const kc_worldmap_pose pose = mcl_predict(a.pre, p, k == 0);
    const long long zq = a.zq[k];
    if (zq >= 0) {  // rule 33: -1 contributes nothing
      // rule 32: q > ZMAX iff e 2^30 >= (ZMAX + 1) a; both sides below 2^59
      const long long over = a.zmax + 1;
      WmWalkHit hit{0, 1, 0, 0};
      long long q = a.zmax;
      if (wm_walk(a.cls, a.W, a.H, a.rc, a.unknown_blocks, pose, a.table[k],
                  [&](int e, int ax) { return (static_cast<long long>(e) << 30) >= over * ax; }, &hit)) {
        const unsigned long long num = static_cast<unsigned long long>(hit.e) << 30;
        const unsigned long long qq = num / static_cast<unsigned long long>(hit.a);
        if (qq <= static_cast<unsigned long long>(a.zmax)) q = static_cast<long long>(qq);
      }
      const long long d = q > zq ? q - zq : zq - q;
      const long long bin = d >> a.err_shift;
      c = s_pen[bin < a.E - 1 ? bin : a.E - 1];
    }
  }
  mcl_segment_add(a.cost, p, c, live);
}

struct MclFieldArgs {
  MclPredictArgs pre;
  const unsigned short *dist2;  // rule 42's plane, refreshed
  const int2 *table;
  const int *zq;
  const unsigned short *pen_d2;  // c2 + 1 entries
  unsigned *cost;
  long long zmax;
  int W, H, N, B, c2;
  unsigned pen_far;
};

// rules 44 and 45 in mcl_walk_kernel's lane order: one 2-byte load of the plane a ray, behind its bounds test
__global__ __launch_bounds__(kMclBlock) void mcl_field_kernel(MclFieldArgs a) {
  __shared__ unsigned short s_pen[KC_MCL_MAX_TABLE];
  for (int i = threadIdx.x; i <= a.c2; i += kMclBlock) s_pen[i] = a.pen_d2[i];
  __syncthreads();
  const unsigned ray = blockIdx.x * kMclBlock + threadIdx.x;  // N B <= 2^22
  const bool live = ray < static_cast<unsigned>(a.N) * static_cast<unsigned>(a.B);
  int p = -1;
  unsigned c = 0;
  if (live) {
    p = static_cast<int>(ray / static_cast<unsigned>(a.B));
    const int k = static_cast<int>(ray - static_cast<unsigned>(p) * static_cast<unsigned>(a.B));
    const kc_worldmap_pose pose = mcl_predict(a.pre, p, k == 0);
    const long long zq = a.zq[k];
    if (zq >= 0 && zq < a.zmax) {  // rule 45: a beam without a return says nothing about an endpoint
      const int2 t = a.table[k];
      // rule 22
      const long long dx = q16_turn_x(pose.cq, pose.sq, t.x, t.y), dy = q16_turn_y(pose.cq, pose.sq, t.x, t.y);
      const long long I = (pose.tx + (1ll << 15) + ((zq * dx + (1ll << 29)) >> 30)) >> 16;
      const long long J = (pose.ty + (1ll << 15) + ((zq * dy + (1ll << 29)) >> 30)) >> 16;
      c = wm_dist2_pen(wm_dist2_at(a.dist2, a.W, a.H, I, J), a.c2, s_pen, a.pen_far);
    }
  }
  mcl_segment_add(a.cost, p, c, live);
}

// ---- reductions over one workgroup of kMclOne: wavefront shuffles, then the 16 partials through LDS ----
// The eight sums of pass 2 in one exchange; thread 0 alone needs the totals and alone reads the partials.
__device__ __forceinline__ void mcl_block_sum8(long long (&v)[8], long long (*s)[kMclOne / 64]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_down(v[i], off);
    if ((threadIdx.x & 63) == 0) s[i][threadIdx.x >> 6] = v[i];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    long long t = 0;
#pragma unroll
    for (int w = 0; w < kMclOne / 64; ++w) t += s[i][w];
    v[i] = t;
  }
}
// What pass 1 of the weigh kernel reduces, in one exchange: rule 35's packed minimum, which every thread needs, and rule
// 59's sum and minimum, which thread 0 alone needs and alone reads.
struct MclPass1 {
  unsigned long long key, cost_sum;
  unsigned cost_min;
};
__device__ __forceinline__ MclPass1 mcl_block_pass1(MclPass1 v, unsigned long long *s_key, unsigned long long *s_sum,
                                                    unsigned *s_min) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long k = __shfl_down(v.key, off);
    const unsigned m = __shfl_down(v.cost_min, off);
    v.key = k < v.key ? k : v.key;
    v.cost_sum += __shfl_down(v.cost_sum, off);
    v.cost_min = m < v.cost_min ? m : v.cost_min;
  }
  if ((threadIdx.x & 63) == 0) {
    s_key[threadIdx.x >> 6] = v.key;
    s_sum[threadIdx.x >> 6] = v.cost_sum;
    s_min[threadIdx.x >> 6] = v.cost_min;
  }
  __syncthreads();
  MclPass1 t{s_key[0], 0ull, 0xFFFFFFFFu};
#pragma unroll
  for (int i = 1; i < kMclOne / 64; ++i) t.key = s_key[i] < t.key ? s_key[i] : t.key;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < kMclOne / 64; ++i) {
      t.cost_sum += s_sum[i];
      t.cost_min = s_min[i] < t.cost_min ? s_min[i] : t.cost_min;
    }
  }
  return t;
}

// the record and, next to it, the fit: one read-back
struct MclOut {
  kc_mcl_record rec;
  kc_mcl_fit fit;
};

struct MclWeighArgs {
  MclState st;
  unsigned *acc, *cost, *w, *min_prev;
  const unsigned *wtab;
  const int2 *heading;
  MclOut *out;
  int N, EW, w_shift;
  unsigned step;
};

// a 128-bit sum kept as sum of (t >> 32) and sum of (t & 0xFFFFFFFF): -> (lo, hi)
__device__ __forceinline__ void mcl_join(long long high, long long low, unsigned long long *lo, long long *hi) {
  const unsigned long long base = static_cast<unsigned long long>(high) << 32;
  *lo = base + static_cast<unsigned long long>(low);
  *hi = (high >> 32) + (*lo < base ? 1 : 0);
}

__global__ __launch_bounds__(kMclOne) void mcl_weigh_kernel(MclWeighArgs a) {
  __shared__ long long s_sums[8][kMclOne / 64];
  __shared__ unsigned long long s_key[kMclOne / 64], s_sum[kMclOne / 64];
  __shared__ unsigned s_min[kMclOne / 64];
  const unsigned min_prev = *a.min_prev;
  MclPass1 mine{~0ull, 0ull, 0xFFFFFFFFu};
  unsigned cost_of_key = 0u;  // the step cost of this thread's own best, for rule 59's cost_best
  for (int p = threadIdx.x; p < a.N; p += kMclOne) {  // rules 35 and 59
    const unsigned cost = a.cost[p];
    const unsigned long long sum = static_cast<unsigned long long>(a.acc[p] - min_prev) + cost;
    const unsigned v = sum < kMclAccCap ? static_cast<unsigned>(sum) : kMclAccCap;
    a.acc[p] = v;
    a.cost[p] = 0u;
    const unsigned long long k = (static_cast<unsigned long long>(v) << 32) | static_cast<unsigned>(p);
    if (k < mine.key) {
      mine.key = k;
      cost_of_key = cost;
    }
    mine.cost_sum += cost;
    mine.cost_min = cost < mine.cost_min ? cost : mine.cost_min;
  }
  const MclPass1 all = mcl_block_pass1(mine, s_key, s_sum, s_min);
  const unsigned long long key = all.key;
  // rule 59, written here so that nothing of it stays live across pass 2.  Keys are distinct (p is part of them): one
  // thread holds the winner, and with it the best particle's cost
  if (mine.key == key) a.out->fit.cost_best = cost_of_key;
  if (threadIdx.x == 0) {
    a.out->fit.cost_sum = all.cost_sum;
    a.out->fit.cost_min = all.cost_min;
    a.out->fit.step = a.step;
  }
  const unsigned amin = static_cast<unsigned>(key >> 32), best = static_cast<unsigned>(key & 0xFFFFFFFFull);
  const long long bx = a.st.tx[best], by = a.st.ty[best];
  long long w1 = 0, w2 = 0, sc = 0, ss = 0, sxh = 0, sxl = 0, syh = 0, syl = 0;
  for (int p = threadIdx.x; p < a.N; p += kMclOne) {  // rules 36 and 37
    const long long w = a.wtab[q16_weight_bin(a.acc[p], amin, a.w_shift, a.EW)];
    a.w[p] = static_cast<unsigned>(w);
    const int2 cs = a.heading[a.st.h[p]];
    const long long tx = w * (a.st.tx[p] - bx), ty = w * (a.st.ty[p] - by);
    w1 += w;
    w2 += w * w;
    sc += w * cs.x;
    ss += w * cs.y;
    sxh += tx >> 32;
    sxl += tx & 0xFFFFFFFFll;
    syh += ty >> 32;
    syl += ty & 0xFFFFFFFFll;
  }
  long long sums[8] = {w1, w2, sc, ss, sxh, sxl, syh, syl};
  mcl_block_sum8(sums, s_sums);
  if (threadIdx.x == 0) {
    kc_mcl_record r;
    r.w1 = static_cast<uint64_t>(sums[0]);
    r.w2 = static_cast<uint64_t>(sums[1]);
    unsigned long long lo;
    long long hi;
    mcl_join(sums[4], sums[5], &lo, &hi);
    r.sx_lo = lo;
    r.sx_hi = hi;
    mcl_join(sums[6], sums[7], &lo, &hi);
    r.sy_lo = lo;
    r.sy_hi = hi;
    r.sc = sums[2];
    r.ss = sums[3];
    r.best_tx = bx;
    r.best_ty = by;
    r.best_h = a.st.h[best];
    r.amin = amin;
    r.best = best;
    r.step = a.step;
    a.out->rec = r;
    *a.min_prev = amin;
  }
}

// rule 40: cum_i, the inclusive prefix sum of w in index order
__global__ __launch_bounds__(kMclOne) void mcl_prefix_kernel(const unsigned *w, unsigned long long *cum, int N) {
  __shared__ unsigned long long s[kMclOne];
  const int chunk = (N + kMclOne - 1) / kMclOne;
  const int lo = static_cast<int>(threadIdx.x) * chunk, hi = lo + chunk < N ? lo + chunk : N;
  unsigned long long mine = 0;
  for (int i = lo; i < hi; ++i) mine += w[i];
  s[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 1; off < kMclOne; off <<= 1) {
    const unsigned long long add = static_cast<int>(threadIdx.x) >= off ? s[threadIdx.x - off] : 0ull;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  unsigned long long run = s[threadIdx.x] - mine;  // the chunks before this one
  for (int i = lo; i < hi; ++i) {
    run += w[i];
    cum[i] = run;
  }
}

// rule 40: slot j takes the smallest i with N cum_i > u0 + j W1 (below 2^53 on both sides)
__global__ __launch_bounds__(kMclBlock) void mcl_select_kernel(MclState in, MclState out, unsigned *acc, unsigned *min_prev,
                                                               const unsigned long long *cum, unsigned long long u0,
                                                               unsigned long long w1, int N) {
  const int j = blockIdx.x * kMclBlock + threadIdx.x;
  if (j >= N) return;
  const unsigned long long t = u0 + static_cast<unsigned long long>(j) * w1, n = static_cast<unsigned long long>(N);
  int lo = 0, hi = N - 1;  // N cum_{N-1} = N W1 > t: the answer exists
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (n * cum[mid] > t) hi = mid;
    else lo = mid + 1;
  }
  out.tx[j] = in.tx[lo];
  out.ty[j] = in.ty[lo];
  out.h[j] = in.h[lo];
  acc[j] = 0u;
  if (j == 0) *min_prev = 0u;
}

// rule 41, Gaussian
__global__ __launch_bounds__(kMclBlock) void mcl_init_pose_kernel(MclState out, unsigned *acc, unsigned *cost, unsigned *min_prev,
                                                                  unsigned long long key, long long tx0, long long ty0,
                                                                  unsigned h0, int s_xy, int s_h, int N) {
  const int p = blockIdx.x * kMclBlock + threadIdx.x;
  if (p >= N) return;
  out.tx[p] = q16_clamp(tx0 + q16_noise(q16_draw(key, p, 0), s_xy));
  out.ty[p] = q16_clamp(ty0 + q16_noise(q16_draw(key, p, 1), s_xy));
  out.h[p] = static_cast<unsigned>((static_cast<long long>(h0) + q16_noise(q16_draw(key, p, 2), s_h)) & 0xFFFF);
  acc[p] = 0u;
  cost[p] = 0u;
  if (p == 0) *min_prev = 0u;
}

// rule 41, global: KC_EMPTY cells a row; blockIdx.x: the row
__global__ __launch_bounds__(kMclBlock) void mcl_row_count_kernel(const int8_t *cls, int W, unsigned *rows) {
  __shared__ unsigned s[kMclBlock];
  const int8_t *row = cls + static_cast<size_t>(blockIdx.x) * static_cast<size_t>(W);
  unsigned n = 0;
  for (int i = threadIdx.x; i < W; i += kMclBlock) n += row[i] == KC_EMPTY ? 1u : 0u;
  s[threadIdx.x] = n;
  __syncthreads();
  for (int off = kMclBlock / 2; off > 0; off >>= 1) {
    if (static_cast<int>(threadIdx.x) < off) s[threadIdx.x] += s[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) rows[blockIdx.x] = s[0];
}

// For rule 62, mcl_init_global_kernel's search as a function (the init below keeps its own text: calling this one from
// both measured about a tenth slower there at 65536 particles).
// Rule 41's free cell number `rest` (< before[H]) found by a whole wavefront: a binary search for the row, a ballot walk
// along it.  True on the one lane that stands on the cell, with (I, J); before[J]: the free cells of the rows below J.
__device__ __forceinline__ bool mcl_free_cell(const int8_t *cls, int W, int H, const unsigned long long *before,
                                              unsigned long long rest, int *I, int *J) {
  const int lane = threadIdx.x & 63;
  int lo = 0, hi = H - 1;  // the last row with before[J] <= rest
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (before[mid] <= rest) lo = mid;
    else hi = mid - 1;
  }
  rest -= before[lo];
  const int8_t *row = cls + static_cast<size_t>(lo) * static_cast<size_t>(W);
  for (int i0 = 0; i0 < W; i0 += 64) {
    const int i = i0 + lane;
    const bool free_cell = i < W && row[i] == KC_EMPTY;
    const unsigned long long m = __ballot(free_cell);
    const unsigned long long n = static_cast<unsigned long long>(__popcll(m));
    if (rest < n) {
      *I = i;
      *J = lo;
      return free_cell && static_cast<unsigned long long>(__popcll(m & ((1ull << lane) - 1ull))) == rest;
    }
    rest -= n;
  }
  return false;
}

// rule 41's state in cell (I, J) from the draw v
__device__ __forceinline__ void mcl_seed_in_cell(MclState out, int p, int I, int J, unsigned long long v) {
  out.tx[p] = (static_cast<long long>(I) << 16) + static_cast<long long>(v & 0xFFFF) - (1ll << 15);
  out.ty[p] = (static_cast<long long>(J) << 16) + static_cast<long long>((v >> 16) & 0xFFFF) - (1ll << 15);
  out.h[p] = static_cast<unsigned>((v >> 32) & 0xFFFF);
}

// a wavefront a particle.  before[J]: the free cells of the rows below J, before[H] = n_free
__global__ __launch_bounds__(kMclBlock) void mcl_init_global_kernel(const int8_t *cls, int W, int H, const unsigned long long *before,
                                                                    MclState out, unsigned *acc, unsigned *cost, unsigned *min_prev,
                                                                    unsigned long long key, int N) {
  const int p = static_cast<int>((blockIdx.x * kMclBlock + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  if (p >= N) return;  // the whole wavefront
  unsigned long long rest = q16_draw(key, p, 0) % before[H];
  int lo = 0, hi = H - 1;  // the last row with before[J] <= rest
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (before[mid] <= rest) lo = mid;
    else hi = mid - 1;
  }
  const int J = lo;
  rest -= before[J];
  const int8_t *row = cls + static_cast<size_t>(J) * static_cast<size_t>(W);
  for (int i0 = 0; i0 < W; i0 += 64) {
    const int i = i0 + lane;
    const bool free_cell = i < W && row[i] == KC_EMPTY;
    const unsigned long long m = __ballot(free_cell);
    const unsigned long long n = static_cast<unsigned long long>(__popcll(m));
    if (rest < n) {
      if (free_cell && static_cast<unsigned long long>(__popcll(m & ((1ull << lane) - 1ull))) == rest) {
        const unsigned long long v = q16_draw(key, p, 1);
        out.tx[p] = (static_cast<long long>(i) << 16) + static_cast<long long>(v & 0xFFFF) - (1ll << 15);
        out.ty[p] = (static_cast<long long>(J) << 16) + static_cast<long long>((v >> 16) & 0xFFFF) - (1ll << 15);
        out.h[p] = static_cast<unsigned>((v >> 32) & 0xFFFF);
        acc[p] = 0u;
        cost[p] = 0u;
        if (p == 0) *min_prev = 0u;
      }
      return;
    }
    rest -= n;
  }
}

// rule 62's index: before[J] = the free cells of the rows below J, before[H] = n_free; one workgroup, a lane a
// contiguous chunk of rows as mcl_prefix_kernel has it (H can exceed kMclOne)
__global__ __launch_bounds__(kMclOne) void mcl_row_prefix_kernel(const unsigned *rows, unsigned long long *before, int H) {
  __shared__ unsigned long long s[kMclOne];
  const int chunk = (H + kMclOne - 1) / kMclOne;
  const int lo = static_cast<int>(threadIdx.x) * chunk < H ? static_cast<int>(threadIdx.x) * chunk : H;
  const int hi = lo + chunk < H ? lo + chunk : H;
  unsigned long long mine = 0;
  for (int i = lo; i < hi; ++i) mine += rows[i];
  s[threadIdx.x] = mine;
  __syncthreads();
  for (int off = 1; off < kMclOne; off <<= 1) {
    const unsigned long long add = static_cast<int>(threadIdx.x) >= off ? s[threadIdx.x - off] : 0ull;
    __syncthreads();
    s[threadIdx.x] += add;
    __syncthreads();
  }
  unsigned long long run = s[threadIdx.x] - mine;  // the chunks before this one
  for (int i = lo; i < hi; ++i) {
    before[i] = run;
    run += rows[i];
  }
  if (threadIdx.x == kMclOne - 1) before[H] = s[kMclOne - 1];
}

// rule 62: a wavefront an injected slot, over the buffer the select has filled.  Wavefront i stands for the i-th
// injected slot, j = ceil((i + 1) N / n) - 1; with no free cell the slot keeps rule 40's state.
__global__ __launch_bounds__(kMclBlock) void mcl_inject_kernel(const int8_t *cls, int W, int H, const unsigned long long *before,
                                                               MclState out, unsigned long long key, int N, int n) {
  const int i = static_cast<int>((blockIdx.x * kMclBlock + threadIdx.x) >> 6);
  if (i >= n) return;  // the whole wavefront
  const unsigned long long n_free = before[H];
  if (n_free == 0) return;
  const int j = static_cast<int>(((static_cast<long long>(i) + 1) * N + n - 1) / n) - 1;
  int I = 0, J = 0;
  if (mcl_free_cell(cls, W, H, before, q16_draw(key, j, 16) % n_free, &I, &J)) mcl_seed_in_cell(out, j, I, J, q16_draw(key, j, 17));
}

}  // namespace kc

using namespace kc;

struct kc_mcl {
  kc_worldmap *map = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  OrderEvent map_ready;  // the map's writes, for the walk and the row counts
  size_t N = 0, B = 0;
  float range_max = 0.0f;
  int rc = 0;
  long long zmax = 0;
  unsigned long long seed = 0;
  unsigned step = 0;
  ScanTable table;
  DevBuf<int2> d_heading;
  DevBuf<long long> d_tx[2], d_ty[2];
  DevBuf<unsigned> d_h[2];
  int cur = 0;  // the state buffer that holds the particles
  DevBuf<unsigned> d_acc, d_cost, d_w, d_min_prev;
  DevBuf<unsigned long long> d_cum;
  DevBuf<unsigned short> d_pen;
  DevBuf<unsigned> d_wtab;
  int E = 0, err_shift = 0, EW = 0, w_shift = 0;
  int kind = KC_MCL_MODEL_NONE;  // what a step runs; d_pen holds pen (beam) or pen_d2 (field: E = c2 + 1)
  unsigned pen_far = 0;
  DevBuf<int> d_zq;
  PinBuf<int> h_zq;
  DevBuf<MclOut> d_rec;  // the record and the fit, one read-back
  PinBuf<MclOut> h_rec;
  DevBuf<unsigned> d_rows;  // global init and rule 62: scratch grown on demand and kept
  DevBuf<unsigned long long> d_before;
  bool inited = false, have_weights = false, have_fit = false;
  unsigned long long w1 = 0;  // of the last step
  int OI = 0, OJ = 0;         // rule 50: the map offset the particles are expressed in
  Timing step_time, resample_time, inject_time;

  MclState state(int which) { return MclState{d_tx[which].p, d_ty[which].p, d_h[which].p}; }
};

namespace {

// rule 38, in its order
int mcl_check(float res, size_t N, size_t B, float range_max, const uint16_t *pen, size_t E, int err_shift, const uint32_t *wtab,
              size_t EW, int w_shift, unsigned flags, int *rc_out, long long *zmax_out) {
  if (!(res > 0.0f) || !std::isfinite(res)) KC_FAIL(KC_ERR_INVALID, "the resolution must be positive");
  if (N == 0 || B == 0) KC_FAIL(KC_ERR_INVALID, "a localiser needs at least one particle and one beam, got %zu x %zu", N, B);
  if (N > KC_MCL_MAX_PARTICLES) KC_FAIL(KC_ERR_RANGE, "%zu particles are above the cap of %d", N, KC_MCL_MAX_PARTICLES);
  if (B > KC_MCL_MAX_BEAMS) KC_FAIL(KC_ERR_RANGE, "%zu beams are above the cap of %d", B, KC_MCL_MAX_BEAMS);
  if (N * B > (size_t{1} << 22)) KC_FAIL(KC_ERR_RANGE, "%zu particles x %zu beams are above the cap of 2^22 rays", N, B);
  int rc = 0;
  KC_TRY(worldmap_scan_check(res, N, B, range_max, 0u, &rc));  // range_max, then Rc
  if (pen) {
    if (E == 0) KC_FAIL(KC_ERR_INVALID, "an empty penalty table");
    if (E > KC_MCL_MAX_TABLE) KC_FAIL(KC_ERR_RANGE, "%zu penalty entries are above the cap of %d", E, KC_MCL_MAX_TABLE);
    if (err_shift < 0 || err_shift > 30) KC_FAIL(KC_ERR_INVALID, "err_shift must be in 0 .. 30, got %d", err_shift);
  }
  if (wtab) KC_TRY(check_weight_table(wtab, EW, w_shift, KC_MCL_MAX_TABLE));
  if (flags & ~static_cast<unsigned>(KC_SCAN_UNKNOWN_BLOCKS | KC_MCL_SKIP_NO_RETURN))
    KC_FAIL(KC_ERR_INVALID, "unknown localiser flag bits 0x%x", flags);
  if (rc_out) *rc_out = rc;
  if (zmax_out) *zmax_out = std::llrint(static_cast<double>(range_max) / static_cast<double>(res) * 65536.0);
  return KC_OK;
}

// kc_mcl_field_check's order: rule 38's up to Rc, pen_d2, the reach, wtab, the flags
int mcl_field_check(float res, size_t N, size_t B, float range_max, const uint16_t *pen_d2, size_t n_pen, int reach,
                    const uint32_t *wtab, size_t EW, int w_shift, unsigned flags, int *rc_out, long long *zmax_out) {
  KC_TRY(mcl_check(res, N, B, range_max, nullptr, 0, 0, nullptr, 0, 0, 0u, rc_out, zmax_out));
  if (pen_d2) {
    if (n_pen < 2) KC_FAIL(KC_ERR_INVALID, "a field penalty table needs c2 + 1 >= 2 entries, got %zu", n_pen);
    if (n_pen > KC_MCL_MAX_TABLE) KC_FAIL(KC_ERR_RANGE, "%zu penalty entries are above the cap of %d", n_pen, KC_MCL_MAX_TABLE);
    KC_TRY(check_reach(n_pen, reach));
  }
  KC_TRY(mcl_check(res, N, B, range_max, nullptr, 0, 0, wtab, EW, w_shift, 0u, nullptr, nullptr));
  if (flags & ~static_cast<unsigned>(KC_MCL_SKIP_NO_RETURN))
    KC_FAIL(KC_ERR_INVALID, "a field step takes KC_MCL_SKIP_NO_RETURN alone, got flag bits 0x%x", flags);
  return KC_OK;
}

// rules 34 / 45 and 36's tables onto the device; the particles stay
int mcl_take_tables(kc_mcl *c, int kind, const uint16_t *pen, size_t n_pen, int err_shift, unsigned pen_far, const uint32_t *wtab,
                    size_t n_wtab, int w_shift) {
  KC_HIP(hipSetDevice(c->device));
  c->kind = KC_MCL_MODEL_NONE;
  KC_TRY(upload_tables(c->d_pen, pen, n_pen, c->d_wtab, wtab, n_wtab, c->stream));
  c->E = static_cast<int>(n_pen);
  c->err_shift = err_shift;
  c->pen_far = pen_far;
  c->EW = static_cast<int>(n_wtab);
  c->w_shift = w_shift;
  c->kind = kind;
  c->have_weights = false;  // weights of another table
  c->have_fit = false;      // and a fit in another table's penalties
  return KC_OK;
}

unsigned mcl_blocks(size_t work) { return static_cast<unsigned>((work + kMclBlock - 1) / kMclBlock); }

unsigned long long mcl_key(const kc_mcl *c, unsigned step) { return q16_key(c->seed, step); }

// rule 50, queued on the context's stream (the device is current): the particles into the map's present offset
int mcl_follow(kc_mcl *c, const WorldMapView &v) {
  const long long di = static_cast<long long>(v.OI) - c->OI, dj = static_cast<long long>(v.OJ) - c->OJ;
  if (di == 0 && dj == 0) return KC_OK;
  hipLaunchKernelGGL(mcl_shift_kernel, dim3(mcl_blocks(c->N)), dim3(kMclBlock), 0, c->stream, c->state(c->cur), di * 65536,
                     dj * 65536, static_cast<int>(c->N));
  KC_HIP(hipGetLastError());
  c->OI = v.OI;
  c->OJ = v.OJ;
  return KC_OK;
}

// what either init leaves behind: particles in the map's present offset
void mcl_started(kc_mcl *c, int into, const WorldMapView &v) {
  c->OI = v.OI;
  c->OJ = v.OJ;
  c->cur = into;
  c->step = 0;
  c->inited = true;
  c->have_weights = false;
  c->have_fit = false;
}

}  // namespace

extern "C" {

int kc_mcl_check(float resolution, size_t n_particles, size_t n_beams, float range_max, const uint16_t *pen_or_null, size_t n_pen,
                 int err_shift, const uint32_t *wtab_or_null, size_t n_wtab, int w_shift, unsigned int flags, int32_t *rc_out,
                 int64_t *zmax_out) {
  if (rc_out) *rc_out = 0;
  if (zmax_out) *zmax_out = 0;
  int rc = 0;
  long long zmax = 0;
  KC_TRY(mcl_check(resolution, n_particles, n_beams, range_max, pen_or_null, n_pen, err_shift, wtab_or_null, n_wtab, w_shift, flags,
                   &rc, &zmax));
  if (rc_out) *rc_out = rc;
  if (zmax_out) *zmax_out = zmax;
  return KC_OK;
}

int kc_mcl_heading(uint32_t h, int32_t *cq_out, int32_t *sq_out) {
  if (!cq_out || !sq_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (h > 65535u) KC_FAIL(KC_ERR_RANGE, "heading %u is outside 0 .. 65535", h);
  const int2 v = heading_table()[h];
  *cq_out = v.x;
  *sq_out = v.y;
  return KC_OK;
}

int kc_mcl_create(kc_worldmap *map, size_t n_particles, const double *angles, size_t n_beams, float range_max, uint64_t seed,
                  kc_mcl **out) {
  if (!out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *out = nullptr;
  if (!map || !angles) KC_FAIL(KC_ERR_INVALID, "null argument");
  WorldMapView v{};
  KC_TRY(worldmap_view(map, &v));
  int rc = 0;
  long long zmax = 0;
  KC_TRY(mcl_check(v.res, n_particles, n_beams, range_max, nullptr, 0, 0, nullptr, 0, 0, 0u, &rc, &zmax));
  for (size_t k = 0; k < n_beams; ++k)
    if (!std::isfinite(angles[k])) KC_FAIL(KC_ERR_INVALID, "beam angle %zu is not finite", k);
  hipStream_t stream = nullptr;
  KC_TRY(open_device_stream(v.device, &stream));
  auto *c = new kc_mcl();
  c->map = map;
  c->device = v.device;
  c->stream = stream;
  c->N = n_particles;
  c->B = n_beams;
  c->range_max = range_max;
  c->rc = rc;
  c->zmax = zmax;
  c->seed = seed;
  const size_t N = n_particles;
  int e = KC_OK;
  for (int b = 0; b < 2 && !e; ++b)
    if ((e = c->d_tx[b].reserve(N)) || (e = c->d_ty[b].reserve(N)) || (e = c->d_h[b].reserve(N))) break;
  if (!e && ((e = c->d_acc.reserve(N)) || (e = c->d_cost.reserve(N)) || (e = c->d_w.reserve(N)) || (e = c->d_cum.reserve(N)) ||
             (e = c->d_min_prev.reserve(1)) || (e = c->d_zq.reserve(n_beams)) ||
             (e = c->h_zq.reserve(n_beams)) || (e = c->d_rec.reserve(1)) || (e = c->h_rec.reserve(1)) ||
             (e = c->table.ensure(angles, n_beams, stream)) || (e = upload_heading_table(c->d_heading, stream)))) {
  }
  if (e) {
    kc_mcl_destroy(c);
    return e;
  }
  *out = c;
  return KC_OK;
}

void kc_mcl_destroy(kc_mcl *c) {
  if (!c) return;
  close_device_stream(c->device, &c->stream);
  delete c;  // (the device is current: the buffers and the events go with the context)
}

int kc_mcl_info(kc_mcl *c, size_t *n_particles_out, size_t *n_beams_out, int32_t *rc_out, int64_t *zmax_out, uint32_t *step_out) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (n_particles_out) *n_particles_out = c->N;
  if (n_beams_out) *n_beams_out = c->B;
  if (rc_out) *rc_out = c->rc;
  if (zmax_out) *zmax_out = c->zmax;
  if (step_out) *step_out = c->step;
  return KC_OK;
}

int kc_mcl_set_model(kc_mcl *c, const uint16_t *pen, size_t n_pen, int err_shift, const uint32_t *wtab, size_t n_wtab, int w_shift) {
  if (!c || !pen || !wtab) KC_FAIL(KC_ERR_INVALID, "null argument");
  WorldMapView v{};
  KC_TRY(worldmap_view(c->map, &v));
  KC_TRY(mcl_check(v.res, c->N, c->B, c->range_max, pen, n_pen, err_shift, wtab, n_wtab, w_shift, 0u, nullptr, nullptr));
  return mcl_take_tables(c, KC_MCL_MODEL_BEAM, pen, n_pen, err_shift, 0u, wtab, n_wtab, w_shift);
}

int kc_mcl_field_check(float resolution, size_t n_particles, size_t n_beams, float range_max, const uint16_t *pen_d2_or_null,
                       size_t n_pen, int reach, const uint32_t *wtab_or_null, size_t n_wtab, int w_shift, unsigned int flags,
                       int32_t *rc_out, int64_t *zmax_out) {
  if (rc_out) *rc_out = 0;
  if (zmax_out) *zmax_out = 0;
  int rc = 0;
  long long zmax = 0;
  KC_TRY(mcl_field_check(resolution, n_particles, n_beams, range_max, pen_d2_or_null, n_pen, reach, wtab_or_null, n_wtab, w_shift,
                         flags, &rc, &zmax));
  if (rc_out) *rc_out = rc;
  if (zmax_out) *zmax_out = zmax;
  return KC_OK;
}

int kc_mcl_set_field_model(kc_mcl *c, const uint16_t *pen_d2, size_t n, uint16_t pen_far, const uint32_t *wtab, size_t n_wtab,
                           int w_shift) {
  if (!c || !pen_d2 || !wtab) KC_FAIL(KC_ERR_INVALID, "null argument");
  WorldMapView v{};
  KC_TRY(worldmap_view(c->map, &v));
  KC_TRY(mcl_field_check(v.res, c->N, c->B, c->range_max, pen_d2, n, 0, wtab, n_wtab, w_shift, 0u, nullptr, nullptr));
  return mcl_take_tables(c, KC_MCL_MODEL_FIELD, pen_d2, n, 0, pen_far, wtab, n_wtab, w_shift);
}

int kc_mcl_model_kind(kc_mcl *c, int *kind_out) {
  if (!c || !kind_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *kind_out = c->kind;
  return KC_OK;
}

int kc_mcl_init_pose(kc_mcl *c, int64_t tx0, int64_t ty0, uint32_t h0, int32_t s_xy, int32_t s_h) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (tx0 < -kQ16MaxOffset || tx0 > kQ16MaxOffset || ty0 < -kQ16MaxOffset || ty0 > kQ16MaxOffset)
    KC_FAIL(KC_ERR_RANGE, "the pose lies more than 2^20 cells from the map's origin");
  if (h0 > 65535u) KC_FAIL(KC_ERR_RANGE, "heading %u is outside 0 .. 65535", h0);
  if (s_xy < 0 || s_h < 0) KC_FAIL(KC_ERR_INVALID, "a noise scale is negative");
  WorldMapView v{};
  KC_TRY(worldmap_view(c->map, &v));
  KC_HIP(hipSetDevice(c->device));
  c->inited = c->have_fit = false;
  const int N = static_cast<int>(c->N);
  hipLaunchKernelGGL(mcl_init_pose_kernel, dim3(mcl_blocks(c->N)), dim3(kMclBlock), 0, c->stream, c->state(0), c->d_acc.p,
                     c->d_cost.p, c->d_min_prev.p, mcl_key(c, 0), static_cast<long long>(tx0), static_cast<long long>(ty0), h0, s_xy,
                     s_h, N);
  KC_HIP(hipGetLastError());
  KC_HIP(hipStreamSynchronize(c->stream));
  mcl_started(c, 0, v);
  return KC_OK;
}

int kc_mcl_init_global(kc_mcl *c, size_t *n_free_out) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (n_free_out) *n_free_out = 0;
  WorldMapView v{};
  KC_TRY(worldmap_view(c->map, &v));
  KC_HIP(hipSetDevice(c->device));
  const size_t H = static_cast<size_t>(v.H);
  KC_TRY(c->d_rows.reserve(H));
  KC_TRY(c->d_before.reserve(H + 1));
  KC_TRY(stream_wait_through(c->map_ready, c->stream, v.stream));  // for the map's writes; the host does not wait
  hipLaunchKernelGGL(mcl_row_count_kernel, dim3(static_cast<unsigned>(H)), dim3(kMclBlock), 0, c->stream, v.cls, v.W, c->d_rows.p);
  KC_HIP(hipGetLastError());
  std::vector<unsigned> rows(H);
  KC_HIP(hipMemcpyAsync(rows.data(), c->d_rows.p, H * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  std::vector<unsigned long long> before(H + 1, 0ull);
  for (size_t j = 0; j < H; ++j) before[j + 1] = before[j] + rows[j];
  if (n_free_out) *n_free_out = static_cast<size_t>(before[H]);
  if (before[H] == 0) KC_FAIL(KC_ERR_STATE, "the map has no KC_EMPTY cell to seed a particle in");
  c->inited = c->have_fit = false;  // only now: the refusal above has touched nothing but the row counts' scratch
  KC_HIP(hipMemcpyAsync(c->d_before.p, before.data(), (H + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(mcl_init_global_kernel, dim3(mcl_blocks(c->N * 64)), dim3(kMclBlock), 0, c->stream, v.cls, v.W, v.H,
                     c->d_before.p, c->state(0), c->d_acc.p, c->d_cost.p, c->d_min_prev.p, mcl_key(c, 0), static_cast<int>(c->N));
  KC_HIP(hipGetLastError());
  KC_HIP(hipStreamSynchronize(c->stream));  // `before` is the copy's source
  mcl_started(c, 0, v);
  return KC_OK;
}

// Check order: null arguments; the state (model, init); increments, scales, flags, the ranges; then the device
int kc_mcl_step(kc_mcl *c, int64_t d_f, int64_t d_l, int32_t d_h, int32_t s_f, int32_t s_l, int32_t s_h, const int32_t *zq,
                unsigned int flags, kc_mcl_record *out) {
  if (!c || !zq || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  std::memset(out, 0, sizeof(*out));
  if (c->kind == KC_MCL_MODEL_NONE) KC_FAIL(KC_ERR_STATE, "a step needs kc_mcl_set_model or kc_mcl_set_field_model first");
  const bool field = c->kind == KC_MCL_MODEL_FIELD;
  if (!c->inited) KC_FAIL(KC_ERR_STATE, "a step needs kc_mcl_init_pose or kc_mcl_init_global first");
  if (d_f < -kQ16MaxOffset || d_f > kQ16MaxOffset || d_l < -kQ16MaxOffset || d_l > kQ16MaxOffset)
    KC_FAIL(KC_ERR_RANGE, "the odometry increment is above 2^20 cells");
  if (s_f < 0 || s_l < 0 || s_h < 0) KC_FAIL(KC_ERR_INVALID, "a noise scale is negative");
  if (flags & ~static_cast<unsigned>(KC_SCAN_UNKNOWN_BLOCKS | KC_MCL_SKIP_NO_RETURN))
    KC_FAIL(KC_ERR_INVALID, "unknown localiser flag bits 0x%x", flags);
  if (field && (flags & KC_SCAN_UNKNOWN_BLOCKS))
    KC_FAIL(KC_ERR_INVALID, "a field step takes no KC_SCAN_UNKNOWN_BLOCKS: the distance plane's own flag decides what blocks");
  for (size_t k = 0; k < c->B; ++k)
    if (!((zq[k] >= 0 && zq[k] <= c->zmax) || (zq[k] == -1 && (flags & KC_MCL_SKIP_NO_RETURN))))
      KC_FAIL(KC_ERR_INVALID, "quantised range %zu is %d, outside 0 .. %lld", k, zq[k], c->zmax);
  if (c->step == 0xFFFFFFFFu) KC_FAIL(KC_ERR_STATE, "the step counter is exhausted: init again");
  WorldMapView v{};
  KC_TRY(worldmap_view(c->map, &v));
  WorldMapDistance dist{};
  if (field) {  // rule 45's state, before anything is queued
    KC_TRY(worldmap_distance_state(c->map, &dist));
    if (dist.reach == 0) KC_FAIL(KC_ERR_STATE, "a field step needs the map's distance plane: kc_worldmap_set_distance");
    if (c->E - 1 > dist.reach * dist.reach)
      KC_FAIL(KC_ERR_STATE, "the field model's c2 = %d is above the plane's reach^2 = %d", c->E - 1, dist.reach * dist.reach);
  }
  KC_HIP(hipSetDevice(c->device));
  KC_TRY(mcl_follow(c, v));  // rule 50, ahead of the predict step in the stream's order
  std::memcpy(c->h_zq.p, zq, c->B * sizeof(int32_t));
  KC_HIP(hipMemcpyAsync(c->d_zq.p, c->h_zq.p, c->B * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  if (field) KC_TRY(worldmap_distance_refresh(c->map));  // on the map's stream, a launch only when its dirty box is not empty
  KC_TRY(stream_wait_through(c->map_ready, c->stream, v.stream));  // for the map's writes; the host does not wait
  const unsigned step = c->step + 1;
  MclPredictArgs pre{};
  pre.heading = c->d_heading.p;
  pre.in = c->state(c->cur);
  pre.out = c->state(c->cur ^ 1);
  pre.key = mcl_key(c, step);
  pre.d_f = d_f;
  pre.d_l = d_l;
  pre.d_h = d_h;
  pre.s_f = s_f;
  pre.s_l = s_l;
  pre.s_h = s_h;
  // from here on the particles are the new buffer's, whatever fails: a failed step asks for a new init
  c->inited = false;
  c->have_weights = false;
  c->have_fit = false;
  c->step_time.begin_cycle();
  KC_TRY(c->step_time.start("walk", c->stream));
  if (field) {
    MclFieldArgs a{};
    a.pre = pre;
    a.dist2 = dist.dist2;
    a.table = reinterpret_cast<const int2 *>(c->table.d.p);
    a.zq = c->d_zq.p;
    a.pen_d2 = c->d_pen.p;
    a.cost = c->d_cost.p;
    a.zmax = c->zmax;
    a.W = v.W;
    a.H = v.H;
    a.N = static_cast<int>(c->N);
    a.B = static_cast<int>(c->B);
    a.c2 = c->E - 1;
    a.pen_far = c->pen_far;
    hipLaunchKernelGGL(mcl_field_kernel, dim3(mcl_blocks(c->N * c->B)), dim3(kMclBlock), 0, c->stream, a);
  } else {
    MclWalkArgs a{};
    a.pre = pre;
    a.cls = v.cls;
    a.table = reinterpret_cast<const int2 *>(c->table.d.p);
    a.zq = c->d_zq.p;
    a.pen = c->d_pen.p;
    a.cost = c->d_cost.p;
    a.zmax = c->zmax;
    a.W = v.W;
    a.H = v.H;
    a.N = static_cast<int>(c->N);
    a.B = static_cast<int>(c->B);
    a.rc = c->rc;
    a.unknown_blocks = (flags & KC_SCAN_UNKNOWN_BLOCKS) ? 1 : 0;
    a.E = c->E;
    a.err_shift = c->err_shift;
    hipLaunchKernelGGL(mcl_walk_kernel, dim3(mcl_blocks(c->N * c->B)), dim3(kMclBlock), 0, c->stream, a);
  }
  KC_HIP(hipGetLastError());
  KC_TRY(c->step_time.stop(c->stream));
  MclWeighArgs w{};
  w.st = pre.out;
  w.acc = c->d_acc.p;
  w.cost = c->d_cost.p;
  w.w = c->d_w.p;
  w.min_prev = c->d_min_prev.p;
  w.wtab = c->d_wtab.p;
  w.heading = c->d_heading.p;
  w.out = c->d_rec.p;
  w.N = static_cast<int>(c->N);
  w.EW = c->EW;
  w.w_shift = c->w_shift;
  w.step = step;
  KC_TRY(c->step_time.start("weigh", c->stream));
  hipLaunchKernelGGL(mcl_weigh_kernel, dim3(1), dim3(kMclOne), 0, c->stream, w);
  KC_HIP(hipGetLastError());
  KC_TRY(c->step_time.stop(c->stream));
  KC_HIP(hipMemcpyAsync(c->h_rec.p, c->d_rec.p, sizeof(MclOut), hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  *out = c->h_rec.p->rec;
  if (out->step != step || out->w1 == 0 || c->h_rec.p->fit.step != step) KC_FAIL(KC_ERR_HIP, "the step's record is not this step's");
  c->cur ^= 1;
  c->step = step;
  c->w1 = out->w1;
  c->inited = true;
  c->have_weights = true;
  c->have_fit = true;
  return KC_OK;
}

int kc_mcl_resample(kc_mcl *c) { return kc_mcl_resample_inject(c, 0); }

int kc_mcl_resample_inject(kc_mcl *c, size_t n_inject) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (n_inject > c->N) KC_FAIL(KC_ERR_RANGE, "%zu injected slots are above the %zu particles", n_inject, c->N);
  if (!c->inited || !c->have_weights) KC_FAIL(KC_ERR_STATE, "a resample needs the weights of a step since the last init or resample");
  WorldMapView v{};
  KC_TRY(worldmap_view(c->map, &v));
  KC_HIP(hipSetDevice(c->device));
  const size_t H = static_cast<size_t>(v.H);
  if (n_inject > 0) {
    KC_TRY(c->d_rows.reserve(H));
    KC_TRY(c->d_before.reserve(H + 1));
  }
  KC_TRY(mcl_follow(c, v));  // rule 50: the select copies the moved states
  const int N = static_cast<int>(c->N);
  const unsigned long long key = mcl_key(c, c->step);
  const unsigned long long u0 = q16_draw(key, c->N, 15) % c->w1;
  c->inited = false;
  c->have_weights = false;
  c->inject_time.begin_cycle();
  if (n_inject > 0) {  // rule 62's index of the free cells, as the plane is behind the map's stream; it stays on the device
    KC_TRY(stream_wait_through(c->map_ready, c->stream, v.stream));
    KC_TRY(c->inject_time.start("rows", c->stream));
    hipLaunchKernelGGL(mcl_row_count_kernel, dim3(static_cast<unsigned>(H)), dim3(kMclBlock), 0, c->stream, v.cls, v.W, c->d_rows.p);
    KC_HIP(hipGetLastError());
    KC_TRY(c->inject_time.stop(c->stream));
    KC_TRY(c->inject_time.start("row_prefix", c->stream));
    hipLaunchKernelGGL(mcl_row_prefix_kernel, dim3(1), dim3(kMclOne), 0, c->stream, c->d_rows.p, c->d_before.p, v.H);
    KC_HIP(hipGetLastError());
    KC_TRY(c->inject_time.stop(c->stream));
  }
  c->resample_time.begin_cycle();
  KC_TRY(c->resample_time.start("prefix", c->stream));
  hipLaunchKernelGGL(mcl_prefix_kernel, dim3(1), dim3(kMclOne), 0, c->stream, c->d_w.p, c->d_cum.p, N);
  KC_HIP(hipGetLastError());
  KC_TRY(c->resample_time.stop(c->stream));
  KC_TRY(c->resample_time.start("select", c->stream));
  hipLaunchKernelGGL(mcl_select_kernel, dim3(mcl_blocks(c->N)), dim3(kMclBlock), 0, c->stream, c->state(c->cur), c->state(c->cur ^ 1),
                     c->d_acc.p, c->d_min_prev.p, c->d_cum.p, u0, c->w1, N);
  KC_HIP(hipGetLastError());
  KC_TRY(c->resample_time.stop(c->stream));
  if (n_inject > 0) {  // over the slots the select has just filled
    KC_TRY(c->inject_time.start("inject", c->stream));
    hipLaunchKernelGGL(mcl_inject_kernel, dim3(mcl_blocks(n_inject * 64)), dim3(kMclBlock), 0, c->stream, v.cls, v.W, v.H, c->d_before.p,
                       c->state(c->cur ^ 1), key, N, static_cast<int>(n_inject));
    KC_HIP(hipGetLastError());
    KC_TRY(c->inject_time.stop(c->stream));
    // The row counts and the injection read the map's class plane on this stream, and the map's writers wait for no
    // reader: the call returns only once those reads are over, so that whatever the caller does to the map next (an
    // update, an integration, a shift's two copies) cannot reach into them.  Every other reader of the plane ends in a
    // read-back; this path has none and runs only while the filter is lost.
    KC_HIP(hipStreamSynchronize(c->stream));
  }
  c->cur ^= 1;
  c->inited = true;
  return KC_OK;
}

int kc_mcl_particles(kc_mcl *c, int64_t *tx_out, int64_t *ty_out, uint32_t *h_out, uint32_t *acc_out, size_t cap) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (!c->inited) KC_FAIL(KC_ERR_STATE, "no particles before an init");
  if (cap < c->N) KC_FAIL(KC_ERR_RANGE, "%zu particles do not fit the output capacity %zu", c->N, cap);
  WorldMapView v{};
  KC_TRY(worldmap_view(c->map, &v));
  KC_HIP(hipSetDevice(c->device));
  KC_TRY(mcl_follow(c, v));  // rule 50
  const MclState s = c->state(c->cur);
  if (tx_out) KC_HIP(hipMemcpyAsync(tx_out, s.tx, c->N * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  if (ty_out) KC_HIP(hipMemcpyAsync(ty_out, s.ty, c->N * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  if (h_out) KC_HIP(hipMemcpyAsync(h_out, s.h, c->N * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (acc_out) KC_HIP(hipMemcpyAsync(acc_out, c->d_acc.p, c->N * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  return KC_OK;
}

int kc_mcl_particles_device(kc_mcl *c, void **tx_out, void **ty_out, void **h_out, void **acc_out) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (!c->inited) KC_FAIL(KC_ERR_STATE, "no particles before an init");
  WorldMapView v{};
  KC_TRY(worldmap_view(c->map, &v));
  if (v.OI != c->OI || v.OJ != c->OJ) {  // rule 50; the caller reads on a stream of its own, so the move is finished here
    KC_HIP(hipSetDevice(c->device));
    KC_TRY(mcl_follow(c, v));
    KC_HIP(hipStreamSynchronize(c->stream));
  }
  const MclState s = c->state(c->cur);
  if (tx_out) *tx_out = s.tx;
  if (ty_out) *ty_out = s.ty;
  if (h_out) *h_out = s.h;
  if (acc_out) *acc_out = c->d_acc.p;
  return KC_OK;
}

int kc_mcl_set_timing(kc_mcl *c, int enable) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  c->step_time.enabled = c->resample_time.enabled = c->inject_time.enabled = enable != 0;
  c->step_time.begin_cycle();
  c->resample_time.begin_cycle();
  c->inject_time.begin_cycle();
  return KC_OK;
}

int kc_mcl_inject_times(kc_mcl *c, float ms_out[3]) {
  if (!c || !ms_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  ms_out[0] = ms_out[1] = ms_out[2] = 0.0f;
  if (!c->inject_time.enabled || c->inject_time.used != 3) KC_FAIL(KC_ERR_STATE, "no injecting resample has been timed on this localiser");
  KC_HIP(hipSetDevice(c->device));
  size_t n = 0;
  KC_TRY(c->inject_time.get(nullptr, ms_out, 3, &n));
  return KC_OK;
}

int kc_mcl_last_fit(kc_mcl *c, kc_mcl_fit *out) {
  if (!c || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  std::memset(out, 0, sizeof(*out));
  if (!c->have_fit) KC_FAIL(KC_ERR_STATE, "no fit before a step since the last init or change of model");
  *out = c->h_rec.p->fit;
  return KC_OK;
}

// rules 60 and 61, in the documented order
int kc_mcl_recovery_update(uint64_t cost_sum, size_t n_particles, size_t beams_used, int a_slow, int a_fast, uint32_t max_num,
                           uint32_t max_den, kc_mcl_recovery *state, int64_t *m_out, size_t *n_inject_out) {
  if (m_out) *m_out = -1;
  if (n_inject_out) *n_inject_out = 0;
  if (!state || !n_inject_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  constexpr int64_t kMaxFit = 65535ll * 256;
  if (a_slow < 0 || a_slow > 30) KC_FAIL(KC_ERR_INVALID, "a_slow must be in 0 .. 30, got %d", a_slow);
  if (a_fast < 0 || a_fast > 30) KC_FAIL(KC_ERR_INVALID, "a_fast must be in 0 .. 30, got %d", a_fast);
  if (max_den == 0) KC_FAIL(KC_ERR_INVALID, "max_den is 0");
  if (max_num > max_den) KC_FAIL(KC_ERR_INVALID, "the injected share %u / %u is above 1", max_num, max_den);
  if (n_particles == 0 || n_particles > KC_MCL_MAX_PARTICLES)
    KC_FAIL(KC_ERR_RANGE, "%zu particles are outside 1 .. %d", n_particles, KC_MCL_MAX_PARTICLES);
  if (beams_used > KC_MCL_MAX_BEAMS) KC_FAIL(KC_ERR_RANGE, "%zu beams are above the cap of %d", beams_used, KC_MCL_MAX_BEAMS);
  const uint64_t rays = static_cast<uint64_t>(n_particles) * static_cast<uint64_t>(beams_used);  // <= 2^26
  if (cost_sum > rays * 65535ull) KC_FAIL(KC_ERR_RANGE, "cost_sum is above what %zu x %zu uint16 penalties can sum to", n_particles, beams_used);
  if (state->primed && (state->slow < 0 || state->slow > kMaxFit || state->fast < 0 || state->fast > kMaxFit))
    KC_FAIL(KC_ERR_RANGE, "an average of the state is outside 0 .. 65535 * 256");
  if (beams_used == 0) return KC_OK;  // the step said nothing
  const int64_t m = static_cast<int64_t>(cost_sum * 256ull / rays);  // cost_sum * 256 < 2^50
  if (m_out) *m_out = m;
  if (!state->primed) {
    state->slow = state->fast = m;
    state->primed = 1;
    return KC_OK;
  }
  state->slow += (m - state->slow) >> a_slow;  // arithmetic shifts: they floor
  state->fast += (m - state->fast) >> a_fast;
  if (state->fast <= state->slow) return KC_OK;
  const uint64_t n = static_cast<uint64_t>(n_particles);
  const uint64_t cap = n * max_num / max_den;  // n max_num < 2^49
  const uint64_t want = n * static_cast<uint64_t>(state->fast - state->slow) / static_cast<uint64_t>(state->fast);
  *n_inject_out = static_cast<size_t>(cap < want ? cap : want);
  return KC_OK;
}

int kc_mcl_times(kc_mcl *c, float ms_out[4]) {
  if (!c || !ms_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  ms_out[0] = ms_out[1] = ms_out[2] = ms_out[3] = 0.0f;
  if (!c->step_time.enabled || c->step_time.used != 2) KC_FAIL(KC_ERR_STATE, "no step has been timed on this localiser");
  KC_HIP(hipSetDevice(c->device));
  size_t n = 0;
  KC_TRY(c->step_time.get(nullptr, ms_out, 2, &n));
  if (c->resample_time.used == 2) KC_TRY(c->resample_time.get(nullptr, ms_out + 2, 2, &n));
  return KC_OK;
}

}  // extern "C"
