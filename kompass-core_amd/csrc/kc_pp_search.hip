// PurePursuit's avoidance search on gfx950 (reference: controllers/pure_pursuit.cpp:150-212): for a list of
// velocity candidates, roll each one out `horizon` steps with Path::State::update and report the first candidate
// none of whose poses touches an occupied voxel.  ONE launch per call: pp_search_kernel rolls out every candidate,
// tests every pose and reduces to the smallest clear index; the host reads three words back.
//
// Lane layout: a candidate owns a segment of G lanes (G = the power of two >= horizon + 1, at most 64; 64 / G
// candidates per wavefront).  Lane l of a segment takes step index j = chunk + l (poses are j = 1 .. horizon, the
// start is j = 0): it forms yaw_j by the serial additions, cos / sin(yaw_j) (kc_trig_exact.h, or the host table
// of the fallback), the increment of step j, and -- by adding the increments of the lanes in front of it one by one,
// in step order -- x_j / y_j; then it tests pose j.  The running sums are therefore the reference's bit for bit.
#include "kc_dwa_ctx.h"

namespace kc {

struct PpArgs {
  CollDev c;        // planar octree frame (window around the start)
  TiltDev t;        // tilted LaserScan mount
  const double *vx, *vy, *om;  // [n] candidate commands
  const double *tab;           // 440 values of the device sincos (trig == null)
  const double2 *trig;         // fallback: [n][horizon + 1] cos / sin(yaw_j) from the host's libm
  double x0, y0, yaw0, dt;     // dt: the float time step, widened
  int n, H, G;
  int full;                    // cropped tilted scan: every pose is looked at (the reach check needs them all)
  double bx, by, inv_res, crop;  // ... the pose of that scan, 1 / res, kTiltCrop
  unsigned long long *slots;   // [0] smallest clear | [1] trig failure | [2] pose beyond the cropped scan
  unsigned long long epoch;
};

constexpr int kPpBlock = 256;

template <bool kTilt>
__global__ __launch_bounds__(kPpBlock) void pp_search_kernel(PpArgs a) {
  __shared__ double ltab[440];  // the sincos table as four rows of 110 (TabRows: see rollout_collide_kernel)
  if (!a.trig)
    for (int k = threadIdx.x; k < 440; k += kPpBlock) ltab[(k & 3) * 110 + (k >> 2)] = a.tab[k];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int G = a.G;
  const int seg0 = lane & ~(G - 1), l = lane - seg0;
  const int per_wave = 64 / G;
  const unsigned long long segmask = G == 64 ? ~0ull : ((1ull << G) - 1ull) << seg0;
  const int wave = static_cast<int>((blockIdx.x * kPpBlock + threadIdx.x) >> 6);
  const int nwaves = static_cast<int>((gridDim.x * kPpBlock) >> 6);
  const unsigned long long tag = a.epoch << 32;
  const bool box = kTilt ? a.t.shape == KC_BOX : a.c.shape == KC_BOX;
  for (int first = wave * per_wave; first < a.n; first += nwaves * per_wave) {  // (uniform in the wavefront)
    const int i = first + lane / G;
    const bool live = i < a.n;
    // a smaller clear index is known already: nothing this candidate finds can matter
    bool skip = !live;
    if (live && !a.full) {
      const unsigned long long b = __hip_atomic_load(a.slots, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((b >> 32) == a.epoch && static_cast<long long>(0xFFFFFFFFull - (b & 0xFFFFFFFFull)) < i) skip = true;
    }
    if (__all(skip)) continue;
    const double vx = live ? a.vx[i] : 0.0, vy = live ? a.vy[i] : 0.0, om = live ? a.om[i] : 0.0;
    const double w = om * a.dt;
    double px = a.x0, py = a.y0, yaw = a.yaw0;  // the pose at the chunk's first step index
    bool hit = false, fail = false, beyond = false;
    for (int chunk = 0; chunk <= a.H; chunk += G) {
      const int j = chunk + l;
      const bool step = live && j <= a.H;
      //   yaw += omega * dt  (datatypes/path.h:24-30): yaw_j by the serial additions
      double yj = yaw;
      for (int q = 0; q < l; ++q) yj += w;
      double sn = 0.0, cs = 1.0;
      if (a.trig) {
        if (step) {
          const double2 t = a.trig[static_cast<size_t>(i) * (a.H + 1) + j];
          cs = t.x;
          sn = t.y;
        }
      } else if (!trig::sincos_exact(yj, &sn, &cs, trig::TabRows{ltab})) {
        fail = fail || step;  // (the host redoes the call with its own table)
        sn = 0.0;
        cs = 1.0;
      }
      //   x += (vx*cos - vy*sin) * dt;  y += (vx*sin + vy*cos) * dt
      const double ix = (vx * cs - vy * sn) * a.dt;
      const double iy = (vx * sn + vy * cs) * a.dt;
      // x_j = ((x_chunk + inc_chunk) + inc_chunk+1) + ... + inc_j-1
      double xj = px, yp = py;
      for (int t = 0; t + 1 < G; ++t) {
        const double sx = __shfl(ix, seg0 + t, 64), sy = __shfl(iy, seg0 + t, 64);
        if (t < l) {
          xj += sx;
          yp += sy;
        }
      }
      if (step && j >= 1 && !skip) {
        if constexpr (kTilt) {
          if (a.full) {  // kc_dwa_check_poses: every pose within the kept window of the cropped scan
            const double far = hypot(xj - a.bx, yp - a.by);
            if (!((far + a.t.rho) * a.inv_res + 4.0 < a.crop)) beyond = true;
          }
          if (!hit) hit = tilt_hit(a.t, a.t.gbits, xj, yp, box ? cs : 1.0, box ? sn : 0.0);
        } else {
          if (!hit && a.c.enabled) hit = box ? hit_box(a.c, a.c.bits, xj, yp, cs, sn) : hit_round(a.c, a.c.bits, xj, yp);
        }
      }
      // the pose behind the chunk: x_{chunk+G} = x_{chunk+G-1} + inc_{chunk+G-1}
      px = __shfl(xj + ix, seg0 + G - 1, 64);
      py = __shfl(yp + iy, seg0 + G - 1, 64);
      yaw = __shfl(yj + w, seg0 + G - 1, 64);
      if (!a.full && G == 64 && __any(hit)) break;  // (more than one chunk: G = 64, one candidate per wavefront)
    }
    const bool seg_hit = (__ballot(hit) & segmask) != 0;
    if (l == 0 && live && !skip && !seg_hit) atomicMax(&a.slots[0], tag | (0xFFFFFFFFull - static_cast<unsigned>(i)));
    if ((__ballot(fail) & segmask) && l == 0) atomicMax(&a.slots[1], tag | 1ull);
    if ((__ballot(beyond) & segmask) && l == 0) atomicMax(&a.slots[2], tag | 1ull);
  }
}

}  // namespace kc

int kc_dwa_first_clear_command(kc_dwa *c, const kc_state *start, const double *vx, const double *vy,
                               const double *omega, size_t n, int horizon, double dt, int64_t *first_clear_out) {
  if (!c || !start || !first_clear_out || (n && (!vx || !vy || !omega))) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (horizon < 0) KC_FAIL(KC_ERR_RANGE, "horizon %d is negative", horizon);
  if (n > 0x7FFFFFFEul) KC_FAIL(KC_ERR_RANGE, "too many candidates");
  *first_clear_out = -1;
  if (n == 0) return KC_OK;
  const double dtf = static_cast<double>(static_cast<float>(dt));  // Path::State::update takes a float step
  double vmax = 0.0, om_max = 0.0;
  bool finite = std::isfinite(start->x) && std::isfinite(start->y) && std::isfinite(start->yaw) && std::isfinite(dtf);
  for (size_t i = 0; i < n; ++i) {
    finite = finite && std::isfinite(vx[i]) && std::isfinite(vy[i]) && std::isfinite(omega[i]);
    vmax = std::max(vmax, std::fabs(vx[i]) + std::fabs(vy[i]));
    om_max = std::max(om_max, std::fabs(omega[i]));
  }
  if (!finite) KC_FAIL(KC_ERR_INVALID, "start pose, time step and candidates must be finite");
  KC_TRY(use_device(c));
  hipStream_t s = c->stream;
  KC_HIP(hipStreamSynchronize(s));
  // every pose of every candidate lies within this distance of the start
  const double reach = static_cast<double>(horizon) * std::fabs(dtf) * vmax * 1.0001 + 1e-9;
  PpArgs a{};
  bool tilt = false;
  if (c->tilted) {  // (kc_dwa_check_poses: the same tests, the same "no data: nothing is hit")
    if (horizon == 0 || !c->have_sensor || c->vox_kx.empty()) {
      *first_clear_out = 0;
      return KC_OK;
    }
    KC_TRY(tilt_params(c, a.t));
    tilt = true;
    if (c->tilt_cropped) {
      a.full = 1;
      a.bx = c->tilt_body_x;
      a.by = c->tilt_body_y;
      a.inv_res = c->inv_res;
      a.crop = static_cast<double>(kTiltCrop);
    }
  } else {
    if (horizon == 0 || !c->have_sensor) {
      *first_clear_out = 0;
      return KC_OK;
    }
    // (no occupied voxel within reach: the launch still runs -- one per call with sensor data -- and finds every
    // candidate clear without a single shape test)
    KC_TRY(build_window_at(c, start->x, start->y, reach, a.c));
    a.c.lds = 0;
  }
  auto &pp = c->pp;
  KC_TRY(pp.h_cand.reserve(3 * n));
  KC_TRY(pp.d_cand.reserve(3 * n));
  std::memcpy(pp.h_cand.p, vx, n * sizeof(double));
  std::memcpy(pp.h_cand.p + n, vy, n * sizeof(double));
  std::memcpy(pp.h_cand.p + 2 * n, omega, n * sizeof(double));
  KC_HIP(hipMemcpyAsync(pp.d_cand.p, pp.h_cand.p, 3 * n * sizeof(double), hipMemcpyHostToDevice, s));
  KC_TRY(pp.h_slots.reserve(3));
  if (!pp.d_slots.p || pp.epoch == 0xFFFFFFFFu) {  // fresh words (or a wrapped epoch): all below any tag
    KC_TRY(pp.d_slots.reserve(3));
    for (int k = 0; k < 3; ++k) pp.h_slots.p[k] = 0;
    KC_HIP(hipMemcpyAsync(pp.d_slots.p, pp.h_slots.p, 3 * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    KC_HIP(hipStreamSynchronize(s));
    pp.epoch = 0;
  }
  a.vx = pp.d_cand.p;
  a.vy = pp.d_cand.p + n;
  a.om = pp.d_cand.p + 2 * n;
  a.x0 = start->x;
  a.y0 = start->y;
  a.yaw0 = start->yaw;
  a.dt = dtf;
  a.n = static_cast<int>(n);
  a.H = horizon;
  a.G = 1;
  while (a.G < 64 && a.G < horizon + 1) a.G <<= 1;
  a.slots = pp.d_slots.p;
  // Device trig while every yaw_j stays inside the range kc_trig_exact.h covers and the restatement agreed with
  // the installed libm (yaw_reach_ok: the roll-out's rule); otherwise -- and if the kernel reports a failure
  // anyway -- the host's libm fills the table, as the roll-out's fallback does.
  bool dev_trig = c->device_trig && trig_selfcheck_ok() && yaw_reach_ok(start->yaw, om_max, std::fabs(dtf), static_cast<size_t>(horizon));
  if (dev_trig) {
    KC_TRY(ensure_sincostab(c));
    a.tab = c->d_sincostab.p;
  }
  const size_t cands_per_block = static_cast<size_t>(kPpBlock / 64) * (64 / a.G);
  const unsigned blocks = static_cast<unsigned>(std::min<size_t>((n + cands_per_block - 1) / cands_per_block, 4096));
  for (int pass = 0; pass < 2; ++pass) {
    if (!dev_trig) {
      const size_t H1 = static_cast<size_t>(horizon) + 1;
      KC_TRY(pp.h_trig.reserve(n * H1));
      KC_TRY(pp.d_trig.reserve(n * H1));
      for (size_t i = 0; i < n; ++i) {
        double yaw = start->yaw;
        const double w = omega[i] * dtf;
        for (size_t j = 0; j < H1; ++j) {
          pp.h_trig.p[i * H1 + j] = make_double2(std::cos(yaw), std::sin(yaw));
          yaw += w;
        }
      }
      KC_HIP(hipMemcpyAsync(pp.d_trig.p, pp.h_trig.p, n * H1 * sizeof(double2), hipMemcpyHostToDevice, s));
      a.trig = pp.d_trig.p;
      a.tab = nullptr;
    }
    a.epoch = ++pp.epoch;
    c->timing.begin_cycle();
    KC_TRY(c->timing.start("pp_search_kernel", s));
    if (tilt)
      hipLaunchKernelGGL(pp_search_kernel<true>, dim3(blocks), dim3(kPpBlock), 0, s, a);
    else
      hipLaunchKernelGGL(pp_search_kernel<false>, dim3(blocks), dim3(kPpBlock), 0, s, a);
    KC_HIP(hipGetLastError());
    KC_TRY(c->timing.stop(s));
    KC_HIP(hipMemcpyAsync(pp.h_slots.p, pp.d_slots.p, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    KC_HIP(hipStreamSynchronize(s));
    const unsigned long long tag = static_cast<unsigned long long>(pp.epoch) << 32;
    if (dev_trig && (pp.h_slots.p[1] >> 32) == pp.epoch) {
      dev_trig = false;  // a yaw outside the device range after all: the host table
      continue;
    }
    if (tilt && a.full && (pp.h_slots.p[2] >> 32) == pp.epoch)
      KC_FAIL(KC_ERR_UNSUPPORTED, "tilted sensor frame: a pose lies beyond the %d voxel columns kept of a scan that "
                                  "spans more than 8192", kTiltCrop);
    const unsigned long long b = pp.h_slots.p[0];
    *first_clear_out = (b & 0xFFFFFFFF00000000ull) == tag ? static_cast<int64_t>(0xFFFFFFFFull - (b & 0xFFFFFFFFull)) : -1;
    break;
  }
  c->rolled = false;  // (as kc_dwa_check_poses: the window buffers were rewritten)
  c->evaluated = false;
  return KC_OK;
}
