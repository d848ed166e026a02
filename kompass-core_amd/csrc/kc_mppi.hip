// Model-predictive path-integral control over the world map's distance plane (kc_mppi_*; DESIGN.md 4.12 rules 1 to 36).
//
// Nothing in the reference to restate: its controllers commit to one velocity for the whole look-ahead.  K noisy
// control sequences of T steps are drawn around a nominal one, rolled out from the robot's state in the localiser's
// integers (rules 28 to 31 of 4.11: 16 fraction bits of a cell, the 65536-entry heading table, the counter-based noise),
// costed against the map's distance plane and a window of path points, and blended by rule 36's table weights into the
// next nominal sequence.  Integers only, exact sums: no result depends on thread order, and tests/mppi_ref.py states
// every rule in Python ints.  No kernel modifies the map, and the context keeps no sequence between calls.
//
// A step is two launches and one read-back.
//  (a) mppi_rollout_kernel<TEAM>: TEAM lanes a sample (1, 4 or 8; a team lies inside one wavefront).  pen_d2, the path
//      window and the nominal sequence lie in LDS.  Every lane of a team carries the sample's state; the three noise
//      draws of a step are split over the team's first three lanes and handed round by shuffles, the path search of
//      rule 6 is split by j = lane, lane + TEAM, ... and its packed key (min(q, qcap) << 8 | j) reduced by one 64-bit
//      minimum per shuffle.  The plane costs one 2-byte load a step behind the bounds test.  Control flow is uniform
//      over a wavefront (a sample that has hit goes on masked; the loop ends when every sample of the wavefront has
//      hit), so every shuffle finds its source lane active.  The wavefront reduces S_k << 32 | k to one 64-bit atomic
//      minimum and its hits to one atomic add; both words were put to their start values by the step's upload.
//  (b) mppi_update_kernel: a workgroup a step t.  It draws X_k[t] again from the counter noise (rule 3 depends on U[t],
//      k and t only), forms the weights from S_k and the packed minimum, and reduces three int64 numerators and den
//      exactly.  No K x T x 3 buffer exists.  Workgroup 0 writes the record behind U'.
//
// Moving obstacles (rules 13 to 18) are one more term inside (a): mppi_rollout_kernel<TEAM, true> runs while the context
// holds a list, <TEAM, false> (the code without the term) while it holds none.  The list lies in LDS as seven arrays, 3 KB;
// a team splits it by i = sub, sub + TEAM, ... as it splits the path window, adds its soft sums by shuffles and ORs its
// hits by shuffles.  A mover's place at step t is OX + (t + 1) VX, formed where it is used.  The samples a mover ended
// are one more ballot and one more atomic add a wavefront, into the word of the step's upload that was padding.
//
// The grid planner's cost field (rules 19 to 24) is a mode of (a): mppi_rollout_kernel<TEAM, MOVERS, true> runs while a
// planner is attached (kc_mppi_set_field), the six instantiations with FIELD false (the code from before) while none is.
// Rule 20's term stands in the place of rule 6's path search and rule 21's in the place of rule 7's: no path window and no
// LDS for it, the last field value in a register.  A step asks the planner for its kept field (its two buffers alternate
// between solves), orders its stream behind the planner's and reads the field where it lies: the plane's 2 bytes and the
// field's 4 of a state's cell are loaded together.  f0 and f_nom (rule 22) are written by sample 0's first lane behind the
// record and ride in the step's one read-back.
//
// Acceleration limits (rules 25 to 29) are a mode of (a) too: mppi_rollout_kernel<TEAM, MOVERS, FIELD, true> runs while the
// context holds rates (kc_mppi_set_rates), the twelve instantiations with RATE false (the code from before) while it
// holds none.  Rule 26 (mppi_apply_rates, which kc_mppi_apply_rates calls on the host as well) stands between rule 2's
// clamp and rule 4's move: the applied triple is three ints in registers of every lane, as the state is, and rule 4
// moves by it.  No LDS, no shuffle and no load inside the step loop for it: the rates are kernel arguments, and V0, which
// rides behind U in the step's one upload, is read once in front of the loop.  (b) is not touched: rule 10 blends X.
//
// A box footprint (rules 30 to 36) is one more mode of (a): mppi_rollout_kernel<TEAM, MOVERS, FIELD, RATE, true> runs while
// the context holds a list of disc offsets (kc_mppi_set_footprint), the twenty-four instantiations with BOX false (the code
// from before) while it holds none.  The offsets are eight ints among the kernel arguments: no LDS, no upload.  A team
// splits the discs by i = sub, sub + TEAM, ... as it splits the mover list: a lane picks its offsets once in front of the
// loop, forms its centres by the heading pair of the state's new heading, loads their cells together (a disc off the map,
// past the list or of a frozen sample loads cell 0 and drops it) and the team reduces dm by shuffle-minimum.  That heading
// pair is the next step's rule-4 pair and is carried over: one table load a step, as before.  With movers every lane
// forms all NB centres from the scalar offsets and takes rule 32's minimum inside its share of the list.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "kc_internal.h"
#include "kc_worldmap_walk.h"
#include "kompass_hip.h"

namespace kc {

constexpr int kMppiBlock = 64;   // the roll-out's workgroup: one wavefront, so that few samples still spread over the CUs
constexpr int kMppiUpdate = 256;
constexpr unsigned kMppiCap = 1u << 30;

__host__ __device__ inline long long mppi_within(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct MppiModel {  // rule 2's limits, rule 3's scales
  int f_lo, f_hi, l_hi, h_hi, kq;
  int s[3];
};

// rule 2: the box, then the cone
__host__ __device__ inline void mppi_clamp_u(const MppiModel &m, long long &F, long long &L, long long &H) {
  F = mppi_within(F, m.f_lo, m.f_hi);
  L = mppi_within(L, -static_cast<long long>(m.l_hi), m.l_hi);
  H = mppi_within(H, -static_cast<long long>(m.h_hi), m.h_hi);
  if (m.kq > 0) {
    const long long lim = ((F < 0 ? -F : F) * m.kq) >> 16;
    H = mppi_within(H, -lim, lim);
  }
}

struct MppiRates {  // rule 25: a change a control step, each at least 1
  int f_up, f_dn, l_up, l_dn, h_up, h_dn;
};

// rule 26's lim: up for a rising value, dn for a falling one, signed.  |p|, |x| <= 2^22 and a rate <= 2^23: no int wraps
__host__ __device__ inline int mppi_lim(int p, int x, int up, int dn) {
  if (p < x) return p + up < x ? p + up : x;
  return p - dn > x ? p - dn : x;
}

// rule 26: (AF, AL, AH) holds A[t - 1] on entry and A[t] on return; (F, L, H) is X[t], inside rule 2's bounds.  The
// value behind the cone is the next step's p
__host__ __device__ inline void mppi_apply_rates(const MppiRates &r, int kq, int F, int L, int H, int &AF, int &AL, int &AH) {
  AF = mppi_lim(AF, F, r.f_up, r.f_dn);
  AL = mppi_lim(AL, L, r.l_up, r.l_dn);
  AH = mppi_lim(AH, H, r.h_up, r.h_dn);
  if (kq > 0) {
    const int lim = static_cast<int>(((AF < 0 ? -static_cast<long long>(AF) : static_cast<long long>(AF)) * kq) >> 16);
    AH = AH < -lim ? -lim : (AH > lim ? lim : AH);
  }
}

// rule 3's eps of sample k, step t, channel c
__device__ __forceinline__ long long mppi_eps(const MppiModel &m, unsigned long long key, int k, int t, int c) {
  if (k == 0) return 0;
  return q16_noise(q16_draw(key, k, 3 * t + c), m.s[c]);
}

// What a step uploads in one copy: the nominal sequence and the start values of the two words the roll-out reduces into
struct MppiIn {
  unsigned long long min_key;  // S_k << 32 | k, ~0 at the start
  unsigned n_hit, n_hit_mv;    // both 0 at the start; n_hit_mv: the hits by a mover among n_hit (rule 17)
  int U[KC_MPPI_MAX_HORIZON * 3];
  int V0[3];  // rule 25's start velocity, copied only while rates are set
};
// and what it reads back in one copy
struct MppiOut {
  int U[KC_MPPI_MAX_HORIZON * 3];
  kc_mppi_record rec;
  unsigned f0, f_nom;  // rule 22, written by the field roll-out and copied only while a field is attached
};

// rule 13's list as the device holds it: what kc_mppi_set_movers uploads in one copy
struct MppiMovers {
  long long ox[KC_MPPI_MAX_MOVERS], oy[KC_MPPI_MAX_MOVERS];
  unsigned long long hq[KC_MPPI_MAX_MOVERS], sq[KC_MPPI_MAX_MOVERS], g[KC_MPPI_MAX_MOVERS];
  int vx[KC_MPPI_MAX_MOVERS], vy[KC_MPPI_MAX_MOVERS];
};
constexpr unsigned long long kMppiMoverCap = 1ull << 40;  // rule 14's cap of q

struct MppiRollArgs {
  const int2 *heading;           // rule 29
  const unsigned short *dist2;   // rule 42's plane, refreshed
  const unsigned short *pen_d2;  // c2 + 1 entries
  const long long *px, *py;      // M points
  MppiIn *in;
  unsigned *S;
  MppiModel m;
  unsigned long long key, qcap;
  long long tx, ty;
  unsigned h, r2, pen_far, pen_hit, w_path, w_goal;
  int W, H, K, T, M, c2;
  // rules 13 to 16, read by the MOVERS instantiations alone
  const MppiMovers *movers;
  int N;
  unsigned pen_hit_mv;
  // rules 19 to 22, read by the FIELD instantiations alone
  const unsigned *fld;  // the planner's kept field, W x H as the plane
  MppiOut *out;         // f0 and f_nom go behind the record
  unsigned fcap, w_run, w_term;
  // rules 25 to 27, read by the RATE instantiations alone (V0 is in->V0)
  MppiRates rates;
  // rules 30 to 32, read by the BOX instantiations alone: NB and the offsets, the entries past NB zero
  int nb;
  int off[KC_MPPI_MAX_DISCS];
};

constexpr unsigned kMppiFieldInf = 0xFFFFFFFFu;  // rule 19: no walk reaches the goal

// FIELD: rules 20 and 21 stand in for rules 6 and 7.  No path window, no LDS for it; fl is carried in a register.
// RATE: rule 26 between rule 2's clamp and rule 4's move; the applied triple is carried in three registers
// BOX: rule 31's minimum over the discs in the place of rule 5's one lookup, rule 32's in the place of rule 14's q
template <int TEAM, bool MOVERS, bool FIELD = false, bool RATE = false, bool BOX = false>
__global__ __launch_bounds__(kMppiBlock) void mppi_rollout_kernel(MppiRollArgs a) {
  __shared__ unsigned short s_pen[KC_MPPI_MAX_TABLE];
  __shared__ long long s_px[FIELD ? 1 : KC_MPPI_MAX_PATH], s_py[FIELD ? 1 : KC_MPPI_MAX_PATH];
  __shared__ int s_U[KC_MPPI_MAX_HORIZON * 3];
  for (int i = threadIdx.x; i <= a.c2; i += kMppiBlock) s_pen[i] = a.pen_d2[i];
  if constexpr (!FIELD) {
    for (int i = threadIdx.x; i < a.M; i += kMppiBlock) {
      s_px[i] = a.px[i];
      s_py[i] = a.py[i];
    }
  }
  for (int i = threadIdx.x; i < 3 * a.T; i += kMppiBlock) s_U[i] = a.in->U[i];
  __shared__ long long s_ox[MOVERS ? KC_MPPI_MAX_MOVERS : 1], s_oy[MOVERS ? KC_MPPI_MAX_MOVERS : 1];
  __shared__ unsigned long long s_hq[MOVERS ? KC_MPPI_MAX_MOVERS : 1], s_sq[MOVERS ? KC_MPPI_MAX_MOVERS : 1],
      s_g[MOVERS ? KC_MPPI_MAX_MOVERS : 1];
  __shared__ int s_vx[MOVERS ? KC_MPPI_MAX_MOVERS : 1], s_vy[MOVERS ? KC_MPPI_MAX_MOVERS : 1];
  if constexpr (MOVERS) {
    for (int i = threadIdx.x; i < a.N; i += kMppiBlock) {  // N <= 64: one pass
      s_ox[i] = a.movers->ox[i];
      s_oy[i] = a.movers->oy[i];
      s_hq[i] = a.movers->hq[i];
      s_sq[i] = a.movers->sq[i];
      s_g[i] = a.movers->g[i];
      s_vx[i] = a.movers->vx[i];
      s_vy[i] = a.movers->vy[i];
    }
  }
  __syncthreads();
  const int lane = static_cast<int>(threadIdx.x);
  const int k = (static_cast<int>(blockIdx.x) * kMppiBlock + lane) / TEAM, sub = lane % TEAM;  // K TEAM <= 2^19
  const bool live = k < a.K;  // a whole team, or none of it
  long long tx = a.tx, ty = a.ty;
  unsigned h = a.h;
  bool alive = live, hit = false, hit_mv = false;
  long long total = 0;
  int jm = 0;
  // rules 21 and 22: fv of the pose's own cell, one address for every lane
  unsigned f0 = kMppiFieldInf, fl = 0;
  if constexpr (FIELD) {
    const long long I0 = (a.tx + (1ll << 15)) >> 16, J0 = (a.ty + (1ll << 15)) >> 16;
    if (I0 >= 0 && I0 < a.W && J0 >= 0 && J0 < a.H) f0 = a.fld[static_cast<size_t>(I0) + static_cast<size_t>(J0) * static_cast<size_t>(a.W)];
    fl = f0 < a.fcap ? f0 : a.fcap;
  }
  // rule 26: A[-1] = V0, one address for every lane
  int aF = 0, aL = 0, aH = 0;
  if constexpr (RATE) {
    aF = a.in->V0[0];
    aL = a.in->V0[1];
    aH = a.in->V0[2];
  }
  // rule 31: this lane's discs i = sub + j TEAM and their offsets, picked once (the index differs by lane, so a chain of
  // selects over the eight scalar arguments, not an indexed load); the heading pair of h, carried from step to step
  constexpr int kPer = KC_MPPI_MAX_DISCS / (TEAM < KC_MPPI_MAX_DISCS ? TEAM : KC_MPPI_MAX_DISCS);
  long long my_off[kPer];
  int2 cs_next = make_int2(0, 0);
  if constexpr (BOX) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
      int o = 0;
#pragma unroll
      for (int d = 0; d < KC_MPPI_MAX_DISCS; ++d) o = (sub + j * TEAM == d) ? a.off[d] : o;
      my_off[j] = o;
    }
    cs_next = a.heading[h];
  }
  for (int t = 0; t < a.T; ++t) {
    if (__all(!alive)) break;  // wavefront-uniform
    // rule 3.  Lanes 0 to 2 of a team draw a channel each; with one lane a sample it draws all three
    long long e0, e1, e2;
    if (TEAM == 1) {
      e0 = mppi_eps(a.m, a.key, live ? k : 0, t, 0);
      e1 = mppi_eps(a.m, a.key, live ? k : 0, t, 1);
      e2 = mppi_eps(a.m, a.key, live ? k : 0, t, 2);
    } else {
      const long long mine = mppi_eps(a.m, a.key, live ? k : 0, t, sub < 3 ? sub : 0);
      e0 = __shfl(mine, 0, TEAM);
      e1 = __shfl(mine, 1, TEAM);
      e2 = __shfl(mine, 2, TEAM);
    }
    long long F = s_U[3 * t] + e0, L = s_U[3 * t + 1] + e1, Hc = s_U[3 * t + 2] + e2;
    mppi_clamp_u(a.m, F, L, Hc);
    if constexpr (RATE) {  // rules 26 and 27: the state moves by A, not by X
      mppi_apply_rates(a.rates, a.m.kq, static_cast<int>(F), static_cast<int>(L), static_cast<int>(Hc), aF, aL, aH);
      F = aF;
      L = aL;
      Hc = aH;
    }
    // rule 4, from the heading before the step; a sample that has hit stays where it is
    int2 cs;
    if constexpr (BOX) cs = cs_next;  // loaded behind the last step's turn (in front of the loop for t = 0)
    else cs = a.heading[h];
    const long long C = cs.x, S = cs.y;
    if (alive) {
      tx = q16_move_x(tx, C, S, F, L);
      ty = q16_move_y(ty, C, S, F, L);
      h = static_cast<unsigned>((static_cast<long long>(h) + Hc) & 0xFFFF);
    }
    // rule 5
    const long long I = (tx + (1ll << 15)) >> 16, J = (ty + (1ll << 15)) >> 16;
    unsigned d2, fv = kMppiFieldInf;
    long long DC = 0, DS = 0;  // rule 31's pair, of the heading after the step
    if constexpr (BOX) {
      cs_next = a.heading[h];
      DC = cs_next.x;
      DS = cs_next.y;
      // this lane's share of the discs: every cell's address first, then the loads, then the minimum.  j TEAM < NB is
      // uniform over the wavefront; the field's word of the pose's own cell (rule 33) goes out with them
      size_t cell[kPer];
      bool in[kPer];
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const long long DI = (tx + q16_turn_x(DC, DS, my_off[j], 0) + (1ll << 15)) >> 16;
        const long long DJ = (ty + q16_turn_y(DC, DS, my_off[j], 0) + (1ll << 15)) >> 16;
        in[j] = alive && sub + j * TEAM < a.nb && DI >= 0 && DI < a.W && DJ >= 0 && DJ < a.H;
        cell[j] = in[j] ? static_cast<size_t>(DI) + static_cast<size_t>(DJ) * static_cast<size_t>(a.W) : size_t{0};
      }
      unsigned dv[kPer];
#pragma unroll
      for (int j = 0; j < kPer; ++j) dv[j] = j * TEAM < a.nb ? a.dist2[cell[j]] : 0u;
      if constexpr (FIELD) {
        const bool pin = alive && I >= 0 && I < a.W && J >= 0 && J < a.H;
        const unsigned fw = a.fld[pin ? static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(a.W) : size_t{0}];
        fv = pin ? fw : kMppiFieldInf;
      }
      d2 = static_cast<unsigned>(KC_WORLDMAP_DIST_FAR);
#pragma unroll
      for (int j = 0; j < kPer; ++j) {
        const unsigned dj = in[j] ? dv[j] : static_cast<unsigned>(KC_WORLDMAP_DIST_FAR);
        d2 = dj < d2 ? dj : d2;
      }
#pragma unroll
      for (int off = TEAM / 2; off > 0; off >>= 1) {
        const unsigned other = __shfl_xor(d2, off, TEAM);
        d2 = other < d2 ? other : d2;
      }
    } else if constexpr (FIELD) {
      // the plane's 2 bytes and the field's 4 of one cell, issued together: neither address waits for the other's
      // data, and a state outside the map (or a frozen sample) loads cell 0 and drops it, so no branch stands around them
      const bool in = alive && I >= 0 && I < a.W && J >= 0 && J < a.H;
      const size_t cell = in ? static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(a.W) : size_t{0};
      const unsigned dv = a.dist2[cell], fw = a.fld[cell];
      d2 = in ? dv : static_cast<unsigned>(KC_WORLDMAP_DIST_FAR);
      fv = in ? fw : kMppiFieldInf;
    } else {
      d2 = wm_dist2_at(a.dist2, a.W, a.H, I, J, alive);
    }
    if (alive && d2 <= a.r2) {
      total += static_cast<long long>(a.pen_hit) * (a.T - t);
      hit = true;
      alive = false;
    }
    // rules 14 to 16, behind rule 5's test (a static hit wins) and before its penalty: this lane's share of the list,
    // then the team's sum and its OR.  A frozen sample goes through it masked, like rule 6 below
    if constexpr (MOVERS) {
      long long soft = 0;  // at most 64 tops of 2^20
      int struck = 0;
      for (int i = sub; i < a.N; i += TEAM) {
        const long long mx = s_ox[i] + static_cast<long long>(t + 1) * s_vx[i], my = s_oy[i] + static_cast<long long>(t + 1) * s_vy[i];
        unsigned long long q;
        if constexpr (BOX) {  // rule 32: the least over the discs, the centres from the scalar offsets; d < NB is uniform
          q = kMppiMoverCap;
#pragma unroll
          for (int d = 0; d < KC_MPPI_MAX_DISCS; ++d) {
            if (d < a.nb) {
              const long long cx = tx + q16_turn_x(DC, DS, a.off[d], 0), cy = ty + q16_turn_y(DC, DS, a.off[d], 0);
              const long long dx = static_cast<int>((cx - mx) >> 8), dy = static_cast<int>((cy - my) >> 8);  // |.| < 2^30
              const unsigned long long qd = static_cast<unsigned long long>(dx * dx + dy * dy);
              q = qd < q ? qd : q;
            }
          }
        } else {
          const long long dx = static_cast<int>((tx - mx) >> 8), dy = static_cast<int>((ty - my) >> 8);  // |.| < 2^30
          q = static_cast<unsigned long long>(dx * dx + dy * dy);
          q = q < kMppiMoverCap ? q : kMppiMoverCap;
        }
        const unsigned long long sq = s_sq[i];
        struck |= q <= s_hq[i] ? 1 : 0;
        soft += q < sq ? static_cast<long long>((((sq - q) >> 16) * s_g[i]) >> 16) : 0;  // 2^24 2^32 before the shift
      }
#pragma unroll
      for (int off = TEAM / 2; off > 0; off >>= 1) {
        soft += __shfl_xor(soft, off, TEAM);
        struck |= __shfl_xor(struck, off, TEAM);
      }
      if (alive && struck != 0) {
        total += static_cast<long long>(a.pen_hit_mv) * (a.T - t);
        hit = hit_mv = true;
        alive = false;
      }
      if (alive) total += soft;
    }
    if (alive) total += wm_dist2_pen(d2, a.c2, s_pen, a.pen_far);
    if constexpr (FIELD) {  // rule 20, in place of rule 6
      if (alive) {
        fl = fv < a.fcap ? fv : a.fcap;
        total += static_cast<long long>((static_cast<unsigned long long>(fl) * a.w_run) >> 8);  // 2^24 2^12 before the shift
      }
    } else {
      // rule 6: this lane's share of the window, then the team's minimum of the packed key
      unsigned long long best = ~0ull;
      for (int j = sub; j < a.M; j += TEAM) {
        const long long dx = static_cast<int>((tx - s_px[j]) >> 8), dy = static_cast<int>((ty - s_py[j]) >> 8);  // |.| <= 2^29
        const unsigned long long q = static_cast<unsigned long long>(dx * dx + dy * dy);
        const unsigned long long key = ((q < a.qcap ? q : a.qcap) << 8) | static_cast<unsigned>(j);
        best = key < best ? key : best;
      }
#pragma unroll
      for (int off = TEAM / 2; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(best, off, TEAM);
        best = other < best ? other : best;
      }
      if (alive) {
        total += static_cast<long long>(((best >> 8) * a.w_path) >> 16);  // below 2^56 before the shift
        jm = static_cast<int>(best & 0xFF);
      }
    }
  }
  // rules 7 (21 with a field) and 8
  if constexpr (FIELD) total += static_cast<long long>(a.w_term) * fl;
  else total += static_cast<long long>(a.w_goal) * (a.M - 1 - jm);
  const unsigned Sk = total < static_cast<long long>(kMppiCap) ? static_cast<unsigned>(total) : kMppiCap;
  const bool writer = live && sub == 0;
  if (writer) a.S[k] = Sk;
  unsigned long long key = writer ? (static_cast<unsigned long long>(Sk) << 32) | static_cast<unsigned>(k) : ~0ull;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_xor(key, off);
    key = other < key ? other : key;
  }
  const unsigned long long hits = __ballot(writer && hit);
  if (lane == 0) {
    if (key != ~0ull) atomicMin(&a.in->min_key, key);
    if (hits != 0ull) atomicAdd(&a.in->n_hit, static_cast<unsigned>(__popcll(hits)));
  }
  if constexpr (MOVERS) {
    const unsigned long long hits_mv = __ballot(writer && hit_mv);
    if (lane == 0 && hits_mv != 0ull) atomicAdd(&a.in->n_hit_mv, static_cast<unsigned>(__popcll(hits_mv)));
  }
  if constexpr (FIELD) {  // rule 22: sample 0 is lane 0 of workgroup 0
    if (writer && k == 0) {
      a.out->f0 = f0;
      a.out->f_nom = fl;
    }
  }
}

struct MppiUpdateArgs {
  const MppiIn *in;
  const unsigned *S;
  const unsigned *wtab;
  MppiOut *out;
  MppiModel m;
  unsigned long long key;
  int K, T, EW, w_shift;
  unsigned step;
};

// floor(a / b) for b > 0
__host__ __device__ inline long long mppi_floor_div(long long a, long long b) {
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// rules 9 to 11; blockIdx.x: the step t
__global__ __launch_bounds__(kMppiUpdate) void mppi_update_kernel(MppiUpdateArgs a) {
  __shared__ long long s_part[4][kMppiUpdate / 64];
  const int t = static_cast<int>(blockIdx.x);
  const long long U0 = a.in->U[3 * t], U1 = a.in->U[3 * t + 1], U2 = a.in->U[3 * t + 2];
  const unsigned long long min_key = a.in->min_key;
  const unsigned s_min = static_cast<unsigned>(min_key >> 32);
  long long sums[4] = {0, 0, 0, 0};  // three numerators (below 2^59) and den
  for (int k = threadIdx.x; k < a.K; k += kMppiUpdate) {
    const long long w = a.wtab[q16_weight_bin(a.S[k], s_min, a.w_shift, a.EW)];
    long long F = U0 + mppi_eps(a.m, a.key, k, t, 0), L = U1 + mppi_eps(a.m, a.key, k, t, 1), H = U2 + mppi_eps(a.m, a.key, k, t, 2);
    mppi_clamp_u(a.m, F, L, H);
    sums[0] += w * (F - U0);
    sums[1] += w * (L - U1);
    sums[2] += w * (H - U2);
    sums[3] += w;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sums[i] += __shfl_down(sums[i], off);
    if ((threadIdx.x & 63) == 0) s_part[i][threadIdx.x >> 6] = sums[i];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    long long v = 0;
#pragma unroll
    for (int w = 0; w < kMppiUpdate / 64; ++w) v += s_part[i][w];
    sums[i] = v;
  }
  const long long den = sums[3];  // >= wtab[0] >= 1: the best sample's weight
  long long F = U0 + mppi_floor_div(2 * sums[0] + den, 2 * den);
  long long L = U1 + mppi_floor_div(2 * sums[1] + den, 2 * den);
  long long H = U2 + mppi_floor_div(2 * sums[2] + den, 2 * den);
  mppi_clamp_u(a.m, F, L, H);
  a.out->U[3 * t] = static_cast<int>(F);
  a.out->U[3 * t + 1] = static_cast<int>(L);
  a.out->U[3 * t + 2] = static_cast<int>(H);
  if (t == 0) {
    kc_mppi_record r;
    r.den = static_cast<uint64_t>(den);
    r.s_min = s_min;
    r.k_best = static_cast<uint32_t>(min_key & 0xFFFFFFFFull);
    r.s_0 = a.S[0];
    r.n_hit = a.in->n_hit;
    r.step = a.step;
    r.n_hit_moving = a.in->n_hit_mv;
    a.out->rec = r;
  }
}

}  // namespace kc

using namespace kc;

struct kc_mppi {
  kc_worldmap *map = nullptr;
  int device = 0;
  hipStream_t stream = nullptr;
  OrderEvent map_ready;  // the map's writes, for the roll-out
  size_t K = 0, T = 0, M = 0;
  unsigned long long seed = 0;
  DevBuf<int2> d_heading;
  DevBuf<unsigned> d_S;
  DevBuf<unsigned short> d_pen;
  DevBuf<unsigned> d_wtab;
  DevBuf<long long> d_px, d_py;
  DevBuf<MppiIn> d_in;
  PinBuf<MppiIn> h_in;
  DevBuf<MppiOut> d_out;
  PinBuf<MppiOut> h_out;
  MppiModel m{};
  bool have_model = false, have_costs = false, have_S = false;
  int c2 = 0, EW = 0, w_shift = 0;
  int team = 8;  // lanes a sample: the fastest of 1, 4 and 8 at both measured shapes
  bool team_set = false;  // kc_mppi_set_team was called: `team` holds in both modes.  Otherwise the field mode takes 4
                          // lanes a sample while no mover is set, the faster there by the same measurement
  unsigned r2 = 0, pen_far = 0, pen_hit = 0, w_path = 0, w_goal = 0;
  unsigned long long qcap = 0;
  DevBuf<MppiMovers> d_movers;  // rule 13's list; N_mv == 0: none, and the roll-out without the term runs
  int N_mv = 0;
  unsigned pen_hit_mv = 0;
  kc_planner *planner = nullptr;  // rules 19 to 24: attached while not null; asked for its field at every step
  OrderEvent fld_ready;           // the planner's writes, for the roll-out
  unsigned fcap = 0, w_run = 0, w_term = 0;
  bool have_fld = false;          // the last step ran with a field: h_out's f0 and f_nom are its
  bool have_rates = false;        // rules 25 to 29: the mode is on while rates are set
  MppiRates rates{};
  int v0[3] = {0, 0, 0};          // rule 25's V0, kept here and sent in the step's upload
  int nb = 0;                     // rules 30 to 36: the mode is on while nb > 0
  int off[KC_MPPI_MAX_DISCS] = {0, 0, 0, 0, 0, 0, 0, 0};  // rule 30's offsets, the entries past nb zero
  Timing time;
};

namespace {

// rule 12, in its order
int mppi_check(size_t K, size_t T, size_t M, const int32_t *limits, const int32_t *s3, uint32_t r2, const uint16_t *pen_d2, size_t n_pen,
               uint32_t pen_hit, uint32_t w_path, uint64_t qcap, uint32_t w_goal, int reach, const uint32_t *wtab, size_t EW,
               int w_shift) {
  if (K == 0 || T == 0 || M == 0)
    KC_FAIL(KC_ERR_INVALID, "a controller needs at least one sample, one step and one path point, got %zu x %zu x %zu", K, T, M);
  if (K > KC_MPPI_MAX_SAMPLES) KC_FAIL(KC_ERR_RANGE, "%zu samples are above the cap of %d", K, KC_MPPI_MAX_SAMPLES);
  if (T > KC_MPPI_MAX_HORIZON) KC_FAIL(KC_ERR_RANGE, "%zu steps are above the cap of %d", T, KC_MPPI_MAX_HORIZON);
  if (M > KC_MPPI_MAX_PATH) KC_FAIL(KC_ERR_RANGE, "%zu path points are above the cap of %d", M, KC_MPPI_MAX_PATH);
  if (limits) {
    const long long f_lo = limits[0], f_hi = limits[1], l_hi = limits[2], h_hi = limits[3], kq = limits[4];
    if (f_lo > f_hi || l_hi < 0 || h_hi < 0 || kq < 0) KC_FAIL(KC_ERR_INVALID, "an empty or negative control limit");
    if (f_lo < -(1ll << 22) || f_lo > (1ll << 22) || f_hi < -(1ll << 22) || f_hi > (1ll << 22) || l_hi > (1ll << 22))
      KC_FAIL(KC_ERR_RANGE, "a displacement limit is above 2^22");
    if (h_hi > 32767) KC_FAIL(KC_ERR_RANGE, "H_hi = %lld is above 32767", h_hi);
    if (kq > (1ll << 24)) KC_FAIL(KC_ERR_RANGE, "kq = %lld is above 2^24", kq);
    if (!s3) KC_FAIL(KC_ERR_INVALID, "null noise scales");
    if (s3[0] < 0 || s3[1] < 0 || s3[2] < 0) KC_FAIL(KC_ERR_INVALID, "a noise scale is negative");
  }
  if (pen_d2) {
    if (n_pen < 2) KC_FAIL(KC_ERR_INVALID, "the penalty table needs c2 + 1 >= 2 entries, got %zu", n_pen);
    if (n_pen > KC_MPPI_MAX_TABLE) KC_FAIL(KC_ERR_RANGE, "%zu penalty entries are above the cap of %d", n_pen, KC_MPPI_MAX_TABLE);
    if (r2 > n_pen - 1) KC_FAIL(KC_ERR_INVALID, "r2 = %u is above c2 = %zu", r2, n_pen - 1);
    if (pen_hit > (1u << 20)) KC_FAIL(KC_ERR_RANGE, "pen_hit = %u is above 2^20", pen_hit);
    if (w_path > (1u << 16)) KC_FAIL(KC_ERR_RANGE, "w_path = %u is above 2^16", w_path);
    if (qcap > (1ull << 40)) KC_FAIL(KC_ERR_RANGE, "qcap is above 2^40");
    if ((qcap >> 16) * w_path > (1ull << 24)) KC_FAIL(KC_ERR_RANGE, "(qcap >> 16) w_path is above 2^24");
    if (w_goal > (1u << 20)) KC_FAIL(KC_ERR_RANGE, "w_goal = %u is above 2^20", w_goal);
    KC_TRY(check_reach(n_pen, reach));
    if (!wtab) KC_FAIL(KC_ERR_INVALID, "null weight table");
    KC_TRY(check_weight_table(wtab, EW, w_shift, KC_MPPI_MAX_TABLE));
  }
  return KC_OK;
}

// rule 18, in its order
int mppi_check_movers(const int64_t *ox, const int64_t *oy, const int32_t *vx, const int32_t *vy, const uint64_t *hq, const uint64_t *sq,
                      const uint64_t *g, size_t n, uint32_t pen_hit_mv) {
  if (n == 0) return KC_OK;  // clears the list, whatever else is given
  if (n > KC_MPPI_MAX_MOVERS) KC_FAIL(KC_ERR_RANGE, "%zu movers are above the cap of %d", n, KC_MPPI_MAX_MOVERS);
  if (!ox || !oy || !vx || !vy || !hq || !sq || !g) KC_FAIL(KC_ERR_INVALID, "a null array with %zu movers", n);
  if (pen_hit_mv > (1u << 20)) KC_FAIL(KC_ERR_RANGE, "pen_hit_mv = %u is above 2^20", pen_hit_mv);
  for (size_t i = 0; i < n; ++i) {
    if (ox[i] < -kQ16MaxOffset || ox[i] > kQ16MaxOffset || oy[i] < -kQ16MaxOffset || oy[i] > kQ16MaxOffset)
      KC_FAIL(KC_ERR_RANGE, "mover %zu: a position beyond 2^36 (2^20 cells from the map's origin)", i);
    if (vx[i] < -(1 << 22) || vx[i] > (1 << 22) || vy[i] < -(1 << 22) || vy[i] > (1 << 22))
      KC_FAIL(KC_ERR_RANGE, "mover %zu: a velocity beyond 2^22 a step", i);
    if (hq[i] > sq[i]) KC_FAIL(KC_ERR_INVALID, "mover %zu: hq above sq", i);
    if (sq[i] > kMppiMoverCap) KC_FAIL(KC_ERR_RANGE, "mover %zu: sq above 2^40", i);
    if (g[i] > (1ull << 32)) KC_FAIL(KC_ERR_RANGE, "mover %zu: g above 2^32", i);
    if (((((sq[i] - hq[i]) >> 16) * g[i]) >> 16) > (1ull << 20)) KC_FAIL(KC_ERR_RANGE, "mover %zu: the ramp's top above 2^20", i);
  }
  return KC_OK;
}

// rule 23, in its order
int mppi_check_field(uint32_t fcap, uint32_t w_run, uint32_t w_term) {
  if (fcap == 0) KC_FAIL(KC_ERR_INVALID, "fcap = 0: a field term needs a cap of at least 1");
  if (fcap > (1u << 24)) KC_FAIL(KC_ERR_RANGE, "fcap = %u is above 2^24", fcap);
  if (w_run > (1u << 12)) KC_FAIL(KC_ERR_RANGE, "w_run = %u is above 2^12", w_run);
  if (w_term > 64u) KC_FAIL(KC_ERR_RANGE, "w_term = %u is above 64", w_term);
  return KC_OK;
}

// rule 29's two halves, each in its order
int mppi_check_rates6(const int32_t *r) {
  for (int i = 0; i < 6; ++i)
    if (r[i] < 1) KC_FAIL(KC_ERR_INVALID, "rate %d = %d is below 1", i, r[i]);
  for (int i = 0; i < 4; ++i)
    if (r[i] > (1 << 23)) KC_FAIL(KC_ERR_RANGE, "rate %d = %d, an F or L rate, is above 2^23", i, r[i]);
  for (int i = 4; i < 6; ++i)
    if (r[i] > 65535) KC_FAIL(KC_ERR_RANGE, "rate %d = %d, an H rate, is above 65535", i, r[i]);
  return KC_OK;
}

int mppi_check_v0(const int32_t *v) {
  for (int i = 0; i < 2; ++i)
    if (v[i] < -(1 << 22) || v[i] > (1 << 22)) KC_FAIL(KC_ERR_RANGE, "V0[%d] = %d is beyond 2^22", i, v[i]);
  if (v[2] < -32767 || v[2] > 32767) KC_FAIL(KC_ERR_RANGE, "H0 = %d is beyond 32767", v[2]);
  return KC_OK;
}

int mppi_check_rates(const int32_t *rates, const int32_t *v0) {
  if (!rates) return KC_OK;  // the mode is off, whatever v0 is
  KC_TRY(mppi_check_rates6(rates));
  if (v0) KC_TRY(mppi_check_v0(v0));
  return KC_OK;
}

// rule 35, in its order
int mppi_check_footprint(const int32_t *offsets, size_t n) {
  if (n == 0) return KC_OK;  // clears the list, whatever else is given
  if (n > KC_MPPI_MAX_DISCS) KC_FAIL(KC_ERR_RANGE, "%zu discs are above the cap of %d", n, KC_MPPI_MAX_DISCS);
  if (!offsets) KC_FAIL(KC_ERR_INVALID, "a null array with %zu discs", n);
  for (size_t i = 0; i < n; ++i)
    if (offsets[i] < -(1 << 22) || offsets[i] > (1 << 22)) KC_FAIL(KC_ERR_RANGE, "offset %zu = %d is beyond 2^22", i, offsets[i]);
  return KC_OK;
}

template <int TEAM, bool RATE, bool BOX>
void mppi_launch_rollout(const kc_mppi *c, const MppiRollArgs &a) {
  const size_t lanes = c->K * static_cast<size_t>(TEAM);
  const dim3 grid(static_cast<unsigned>((lanes + kMppiBlock - 1) / kMppiBlock));
  if (a.fld) {
    if (a.N > 0) hipLaunchKernelGGL((mppi_rollout_kernel<TEAM, true, true, RATE, BOX>), grid, dim3(kMppiBlock), 0, c->stream, a);
    else hipLaunchKernelGGL((mppi_rollout_kernel<TEAM, false, true, RATE, BOX>), grid, dim3(kMppiBlock), 0, c->stream, a);
    return;
  }
  if (a.N > 0) hipLaunchKernelGGL((mppi_rollout_kernel<TEAM, true, false, RATE, BOX>), grid, dim3(kMppiBlock), 0, c->stream, a);
  else hipLaunchKernelGGL((mppi_rollout_kernel<TEAM, false, false, RATE, BOX>), grid, dim3(kMppiBlock), 0, c->stream, a);
}

template <bool RATE, bool BOX>
void mppi_launch_team(const kc_mppi *c, const MppiRollArgs &a, int team) {
  if (team == 8) mppi_launch_rollout<8, RATE, BOX>(c, a);
  else if (team == 4) mppi_launch_rollout<4, RATE, BOX>(c, a);
  else mppi_launch_rollout<1, RATE, BOX>(c, a);
}

}  // namespace

extern "C" {

int kc_mppi_check(size_t n_samples, size_t horizon, size_t n_path, const int32_t *limits_or_null, const int32_t *s_or_null, uint32_t r2,
                  const uint16_t *pen_d2_or_null, size_t n_pen, uint32_t pen_hit, uint32_t w_path, uint64_t qcap, uint32_t w_goal,
                  int reach, const uint32_t *wtab_or_null, size_t n_wtab, int w_shift) {
  return mppi_check(n_samples, horizon, n_path, limits_or_null, s_or_null, r2, pen_d2_or_null, n_pen, pen_hit, w_path, qcap, w_goal, reach,
                    wtab_or_null, n_wtab, w_shift);
}

int kc_mppi_create(kc_worldmap *map, size_t n_samples, size_t horizon, uint64_t seed, kc_mppi **out) {
  if (!out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *out = nullptr;
  if (!map) KC_FAIL(KC_ERR_INVALID, "null argument");
  KC_TRY(mppi_check(n_samples, horizon, 1, nullptr, nullptr, 0, nullptr, 0, 0, 0, 0, 0, 0, nullptr, 0, 0));
  WorldMapView v{};
  KC_TRY(worldmap_view(map, &v));
  hipStream_t stream = nullptr;
  KC_TRY(open_device_stream(v.device, &stream));
  auto *c = new kc_mppi();
  c->map = map;
  c->device = v.device;
  c->stream = stream;
  c->K = n_samples;
  c->T = horizon;
  c->seed = seed;
  int e = KC_OK;
  if ((e = c->d_S.reserve(n_samples)) || (e = c->d_px.reserve(KC_MPPI_MAX_PATH)) || (e = c->d_py.reserve(KC_MPPI_MAX_PATH)) ||
      (e = c->d_in.reserve(1)) || (e = c->h_in.reserve(1)) || (e = c->d_out.reserve(1)) || (e = c->h_out.reserve(1)) ||
      (e = upload_heading_table(c->d_heading, stream))) {
  }
  if (e) {
    kc_mppi_destroy(c);
    return e;
  }
  *out = c;
  return KC_OK;
}

void kc_mppi_destroy(kc_mppi *c) {
  if (!c) return;
  close_device_stream(c->device, &c->stream);
  delete c;  // (the device is current: the buffers and the events go with the context)
}

int kc_mppi_set_model(kc_mppi *c, int32_t f_lo, int32_t f_hi, int32_t l_hi, int32_t h_hi, int32_t kq, const int32_t *s) {
  if (!c || !s) KC_FAIL(KC_ERR_INVALID, "null argument");
  const int32_t limits[5] = {f_lo, f_hi, l_hi, h_hi, kq};
  KC_TRY(mppi_check(c->K, c->T, 1, limits, s, 0, nullptr, 0, 0, 0, 0, 0, 0, nullptr, 0, 0));
  c->m = MppiModel{f_lo, f_hi, l_hi, h_hi, kq, {s[0], s[1], s[2]}};
  c->have_model = true;
  return KC_OK;
}

int kc_mppi_set_costs(kc_mppi *c, uint32_t r2, const uint16_t *pen_d2, size_t n_pen, uint16_t pen_far, uint32_t pen_hit, uint32_t w_path,
                      uint64_t qcap, uint32_t w_goal, const uint32_t *wtab, size_t n_wtab, int w_shift) {
  if (!c || !pen_d2 || !wtab) KC_FAIL(KC_ERR_INVALID, "null argument");
  KC_TRY(mppi_check(c->K, c->T, 1, nullptr, nullptr, r2, pen_d2, n_pen, pen_hit, w_path, qcap, w_goal, 0, wtab, n_wtab, w_shift));
  KC_HIP(hipSetDevice(c->device));
  c->have_costs = false;
  KC_TRY(upload_tables(c->d_pen, pen_d2, n_pen, c->d_wtab, wtab, n_wtab, c->stream));
  c->c2 = static_cast<int>(n_pen) - 1;
  c->r2 = r2;
  c->pen_far = pen_far;
  c->pen_hit = pen_hit;
  c->w_path = w_path;
  c->qcap = qcap;
  c->w_goal = w_goal;
  c->EW = static_cast<int>(n_wtab);
  c->w_shift = w_shift;
  c->have_costs = true;
  return KC_OK;
}

int kc_mppi_set_path(kc_mppi *c, const int64_t *px, const int64_t *py, size_t n) {
  if (!c || !px || !py) KC_FAIL(KC_ERR_INVALID, "null argument");
  KC_TRY(mppi_check(c->K, c->T, n, nullptr, nullptr, 0, nullptr, 0, 0, 0, 0, 0, 0, nullptr, 0, 0));
  for (size_t j = 0; j < n; ++j)
    if (px[j] < -kQ16MaxOffset || px[j] > kQ16MaxOffset || py[j] < -kQ16MaxOffset || py[j] > kQ16MaxOffset)
      KC_FAIL(KC_ERR_RANGE, "path point %zu lies more than 2^20 cells from the map's origin", j);
  KC_HIP(hipSetDevice(c->device));
  c->M = 0;
  KC_HIP(hipMemcpyAsync(c->d_px.p, px, n * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  KC_HIP(hipMemcpyAsync(c->d_py.p, py, n * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  c->M = n;
  return KC_OK;
}

int kc_mppi_check_movers(const int64_t *ox, const int64_t *oy, const int32_t *vx, const int32_t *vy, const uint64_t *hq, const uint64_t *sq,
                         const uint64_t *g, size_t n, uint32_t pen_hit_mv) {
  return mppi_check_movers(ox, oy, vx, vy, hq, sq, g, n, pen_hit_mv);
}

int kc_mppi_set_movers(kc_mppi *c, const int64_t *ox, const int64_t *oy, const int32_t *vx, const int32_t *vy, const uint64_t *hq,
                       const uint64_t *sq, const uint64_t *g, size_t n, uint32_t pen_hit_mv) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  KC_TRY(mppi_check_movers(ox, oy, vx, vy, hq, sq, g, n, pen_hit_mv));
  c->N_mv = 0;
  if (n == 0) return KC_OK;
  MppiMovers list{};
  for (size_t i = 0; i < n; ++i) {
    list.ox[i] = ox[i];
    list.oy[i] = oy[i];
    list.vx[i] = vx[i];
    list.vy[i] = vy[i];
    list.hq[i] = hq[i];
    list.sq[i] = sq[i];
    list.g[i] = g[i];
  }
  KC_HIP(hipSetDevice(c->device));
  KC_TRY(c->d_movers.reserve(1));
  KC_HIP(hipMemcpyAsync(c->d_movers.p, &list, sizeof(list), hipMemcpyHostToDevice, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  c->N_mv = static_cast<int>(n);
  c->pen_hit_mv = pen_hit_mv;
  return KC_OK;
}

int kc_mppi_check_field(uint32_t fcap, uint32_t w_run, uint32_t w_term) { return mppi_check_field(fcap, w_run, w_term); }

int kc_mppi_set_field(kc_mppi *c, kc_planner *planner, uint32_t fcap, uint32_t w_run, uint32_t w_term) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (!planner) {  // detaches, whatever else is given: the steps after this are the path mode's
    c->planner = nullptr;
    return KC_OK;
  }
  KC_TRY(mppi_check_field(fcap, w_run, w_term));
  c->planner = planner;
  c->fcap = fcap;
  c->w_run = w_run;
  c->w_term = w_term;
  return KC_OK;
}

int kc_mppi_last_field(kc_mppi *c, uint32_t *f0_out, uint32_t *f_nom_out) {
  if (!c || !f0_out || !f_nom_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *f0_out = *f_nom_out = kMppiFieldInf;
  if (!c->have_S || !c->have_fld) KC_FAIL(KC_ERR_STATE, "the last step had no field attached, or there was none");
  *f0_out = c->h_out.p->f0;
  *f_nom_out = c->h_out.p->f_nom;
  return KC_OK;
}

int kc_mppi_check_rates(const int32_t *rates_or_null, const int32_t *v0_or_null) { return mppi_check_rates(rates_or_null, v0_or_null); }

int kc_mppi_set_rates(kc_mppi *c, const int32_t *rates_or_null) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (!rates_or_null) {  // the mode is off: the steps after this are those of a context that never had rates
    c->have_rates = false;
    return KC_OK;
  }
  KC_TRY(mppi_check_rates6(rates_or_null));
  const int32_t *r = rates_or_null;
  c->rates = MppiRates{r[0], r[1], r[2], r[3], r[4], r[5]};
  c->have_rates = true;
  return KC_OK;
}

int kc_mppi_set_velocity(kc_mppi *c, const int32_t *v0) {
  if (!c || !v0) KC_FAIL(KC_ERR_INVALID, "null argument");
  KC_TRY(mppi_check_v0(v0));
  for (int i = 0; i < 3; ++i) c->v0[i] = v0[i];
  return KC_OK;
}

int kc_mppi_apply_rates(const int32_t *limits, const int32_t *rates, const int32_t *v0, const int32_t *u, size_t horizon, int32_t *out) {
  if (!limits || !rates || !v0 || !u || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  const int32_t quiet[3] = {0, 0, 0};
  KC_TRY(mppi_check(1, horizon, 1, limits, quiet, 0, nullptr, 0, 0, 0, 0, 0, 0, nullptr, 0, 0));
  KC_TRY(mppi_check_rates(rates, v0));
  for (size_t t = 0; t < horizon; ++t) {
    const long long F = u[3 * t], L = u[3 * t + 1], H = u[3 * t + 2];
    if (F < -(1ll << 22) || F > (1ll << 22) || L < -(1ll << 22) || L > (1ll << 22) || H < -32767 || H > 32767)
      KC_FAIL(KC_ERR_RANGE, "control %zu of the sequence is outside the bounds of the limits", t);
  }
  const MppiRates r{rates[0], rates[1], rates[2], rates[3], rates[4], rates[5]};
  int aF = v0[0], aL = v0[1], aH = v0[2];
  for (size_t t = 0; t < horizon; ++t) {
    mppi_apply_rates(r, limits[4], u[3 * t], u[3 * t + 1], u[3 * t + 2], aF, aL, aH);
    out[3 * t] = aF;
    out[3 * t + 1] = aL;
    out[3 * t + 2] = aH;
  }
  return KC_OK;
}

int kc_mppi_check_footprint(const int32_t *offsets_or_null, size_t n) { return mppi_check_footprint(offsets_or_null, n); }

int kc_mppi_set_footprint(kc_mppi *c, const int32_t *offsets_or_null, size_t n) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  KC_TRY(mppi_check_footprint(offsets_or_null, n));
  c->nb = static_cast<int>(n);  // n == 0: the steps after this are those of a context that never had a footprint
  for (size_t i = 0; i < KC_MPPI_MAX_DISCS; ++i) c->off[i] = i < n ? offsets_or_null[i] : 0;
  return KC_OK;
}

int kc_mppi_set_team(kc_mppi *c, int lanes) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (lanes != 1 && lanes != 4 && lanes != 8) KC_FAIL(KC_ERR_INVALID, "a sample takes 1, 4 or 8 lanes, got %d", lanes);
  c->team = lanes;
  c->team_set = true;
  return KC_OK;
}

// Check order: null arguments; the state (model, costs, path unless a field is attached); the pose, the heading, the
// sequence; the map's plane; the planner's field (rule 23); then the device
int kc_mppi_step(kc_mppi *c, int64_t tx, int64_t ty, uint32_t h, const int32_t *u_in, uint32_t step, int32_t *u_out, kc_mppi_record *rec) {
  if (!c || !u_in || !u_out || !rec) KC_FAIL(KC_ERR_INVALID, "null argument");
  std::memset(rec, 0, sizeof(*rec));
  if (!c->have_model) KC_FAIL(KC_ERR_STATE, "a step needs kc_mppi_set_model first");
  if (!c->have_costs) KC_FAIL(KC_ERR_STATE, "a step needs kc_mppi_set_costs first");
  const bool field = c->planner != nullptr;  // rule 20: no path window then
  if (!field && c->M == 0) KC_FAIL(KC_ERR_STATE, "a step needs kc_mppi_set_path first");
  if (tx < -kQ16MaxOffset || tx > kQ16MaxOffset || ty < -kQ16MaxOffset || ty > kQ16MaxOffset)
    KC_FAIL(KC_ERR_RANGE, "the pose lies more than 2^20 cells from the map's origin");
  if (h > 65535u) KC_FAIL(KC_ERR_RANGE, "heading %u is outside 0 .. 65535", h);
  const size_t T = c->T;
  for (size_t t = 0; t < T; ++t) {
    const long long F = u_in[3 * t], L = u_in[3 * t + 1], H = u_in[3 * t + 2];
    if (F < -(1ll << 22) || F > (1ll << 22) || L < -(1ll << 22) || L > (1ll << 22) || H < -32767 || H > 32767)
      KC_FAIL(KC_ERR_RANGE, "control %zu of the sequence is outside the bounds of the limits", t);
  }
  WorldMapView v{};
  KC_TRY(worldmap_view(c->map, &v));
  WorldMapDistance dist{};
  KC_TRY(worldmap_distance_state(c->map, &dist));
  if (dist.reach == 0) KC_FAIL(KC_ERR_STATE, "a step needs the map's distance plane: kc_worldmap_set_distance");
  if (c->c2 > dist.reach * dist.reach)
    KC_FAIL(KC_ERR_STATE, "the costs' c2 = %d is above the plane's reach^2 = %d", c->c2, dist.reach * dist.reach);
  PlannerFieldView fld{};
  if (field) {  // rule 23; asked at every step: the planner's two buffers alternate between solves
    KC_TRY(planner_field_view(c->planner, &fld));
    if (fld.W != v.W || fld.H != v.H)
      KC_FAIL(KC_ERR_STATE, "the planner's field is %d x %d, the map %d x %d", fld.W, fld.H, v.W, v.H);
    if (fld.device != c->device) KC_FAIL(KC_ERR_INVALID, "the planner is on device %d, the controller on device %d", fld.device, c->device);
  }
  KC_HIP(hipSetDevice(c->device));
  c->have_S = false;
  c->have_fld = false;
  MppiIn *in = c->h_in.p;  // pinned; the last step's copy from it is over (every step ends drained)
  in->min_key = ~0ull;
  in->n_hit = 0;
  in->n_hit_mv = 0;
  std::memcpy(in->U, u_in, T * 3 * sizeof(int32_t));
  const bool rate = c->have_rates;
  for (int i = 0; i < 3; ++i) in->V0[i] = c->v0[i];
  // rule 25: V0 rides behind U in the same copy, and only while rates are set
  KC_HIP(hipMemcpyAsync(c->d_in.p, in, rate ? sizeof(MppiIn) : offsetof(MppiIn, V0), hipMemcpyHostToDevice, c->stream));
  KC_TRY(worldmap_distance_refresh(c->map));  // on the map's stream, a launch only when its dirty box is not empty
  KC_TRY(stream_wait_through(c->map_ready, c->stream, v.stream));  // for the map's writes; the host does not wait
  if (field) KC_TRY(stream_wait_through(c->fld_ready, c->stream, fld.stream));  // and for the planner's
  const unsigned long long key = q16_key(c->seed, step);
  MppiRollArgs a{};
  a.heading = c->d_heading.p;
  a.dist2 = dist.dist2;
  a.pen_d2 = c->d_pen.p;
  a.px = c->d_px.p;
  a.py = c->d_py.p;
  a.in = c->d_in.p;
  a.S = c->d_S.p;
  a.m = c->m;
  a.key = key;
  a.qcap = c->qcap;
  a.tx = tx;
  a.ty = ty;
  a.h = h;
  a.r2 = c->r2;
  a.pen_far = c->pen_far;
  a.pen_hit = c->pen_hit;
  a.w_path = c->w_path;
  a.w_goal = c->w_goal;
  a.W = v.W;
  a.H = v.H;
  a.K = static_cast<int>(c->K);
  a.T = static_cast<int>(T);
  a.M = static_cast<int>(c->M);
  a.c2 = c->c2;
  a.movers = c->d_movers.p;
  a.N = c->N_mv;
  a.pen_hit_mv = c->pen_hit_mv;
  a.fld = field ? fld.field : nullptr;
  a.out = c->d_out.p;
  a.fcap = c->fcap;
  a.w_run = c->w_run;
  a.w_term = c->w_term;
  a.rates = c->rates;
  a.nb = c->nb;
  for (int i = 0; i < KC_MPPI_MAX_DISCS; ++i) a.off[i] = c->off[i];
  c->time.begin_cycle();
  KC_TRY(c->time.start("rollout", c->stream));
  // (with a footprint the field mode's loads are the discs', and 8 lanes a sample measured the faster again: DESIGN.md 4.12)
  const int team = (field && !c->team_set && c->N_mv == 0 && c->nb == 0) ? 4 : c->team;
  if (a.nb > 0) {
    if (rate) mppi_launch_team<true, true>(c, a, team);
    else mppi_launch_team<false, true>(c, a, team);
  } else if (rate) {
    mppi_launch_team<true, false>(c, a, team);
  } else {
    mppi_launch_team<false, false>(c, a, team);
  }
  KC_HIP(hipGetLastError());
  KC_TRY(c->time.stop(c->stream));
  MppiUpdateArgs u{};
  u.in = c->d_in.p;
  u.S = c->d_S.p;
  u.wtab = c->d_wtab.p;
  u.out = c->d_out.p;
  u.m = c->m;
  u.key = key;
  u.K = static_cast<int>(c->K);
  u.T = static_cast<int>(T);
  u.EW = c->EW;
  u.w_shift = c->w_shift;
  u.step = step;
  KC_TRY(c->time.start("update", c->stream));
  hipLaunchKernelGGL(mppi_update_kernel, dim3(static_cast<unsigned>(T)), dim3(kMppiUpdate), 0, c->stream, u);
  KC_HIP(hipGetLastError());
  KC_TRY(c->time.stop(c->stream));
  c->h_out.p->rec.den = 0;  // so that a copy that did not happen cannot pass for a record
  // rule 22: f0 and f_nom ride behind the record in the same copy, and only while a field is attached
  KC_HIP(hipMemcpyAsync(c->h_out.p, c->d_out.p, field ? sizeof(MppiOut) : offsetof(MppiOut, f0), hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  const kc_mppi_record &r = c->h_out.p->rec;
  if (r.step != step || r.den == 0 || r.k_best >= c->K) KC_FAIL(KC_ERR_HIP, "the step's record is not this step's");
  std::memcpy(u_out, c->h_out.p->U, T * 3 * sizeof(int32_t));
  *rec = r;
  c->have_S = true;
  c->have_fld = field;
  return KC_OK;
}

int kc_mppi_costs(kc_mppi *c, uint32_t *s_out, size_t cap) {
  if (!c || !s_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (!c->have_S) KC_FAIL(KC_ERR_STATE, "no costs before a step");
  if (cap < c->K) KC_FAIL(KC_ERR_RANGE, "%zu costs do not fit the output capacity %zu", c->K, cap);
  KC_HIP(hipSetDevice(c->device));
  KC_HIP(hipMemcpyAsync(s_out, c->d_S.p, c->K * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  return KC_OK;
}

int kc_mppi_set_timing(kc_mppi *c, int enable) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  c->time.enabled = enable != 0;
  c->time.begin_cycle();
  return KC_OK;
}

int kc_mppi_times(kc_mppi *c, float ms_out[2]) {
  if (!c || !ms_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  ms_out[0] = ms_out[1] = 0.0f;
  if (!c->time.enabled || c->time.used != 2) KC_FAIL(KC_ERR_STATE, "no step has been timed on this controller");
  KC_HIP(hipSetDevice(c->device));
  size_t n = 0;
  KC_TRY(c->time.get(nullptr, ms_out, 2, &n));
  return KC_OK;
}

}  // extern "C"
