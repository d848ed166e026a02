// Deformable Virtual Zone deformation on gfx950 (reference: kompass_core/algorithms/dvz.py:372-404,
// get_total_deformation, with _get_undeformed_radius :213-245 and _get_deformation_radius :247-266).
//
// The reference walks the scan beam by beam in Python: per beam the undeformed radius of the zone's ellipse at
// the beam angle, the radius the scan leaves of it, and -- for a deformed beam -- two running sums.  Here that is
// ONE launch: one lane per beam computes the reference's expressions (squares as products), and
// the two sums and the deformed-beam count are formed in double in a fixed order -- lane, wavefront (xor
// butterfly), workgroup (wavefronts in index order), then the workgroup partials in index order by the workgroup
// that takes the last arrival ticket.  No float atomics: the same input gives the same bits on every call.
// The zone constants (radii, centre shift, the constant term C) are the host's, in double, passed by value.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "kc_internal.h"
#include "kc_sincostab.h"
#include "kc_trig_exact.h"
#include "kompass_hip.h"

bool trig_selfcheck_ok();  // kc_dwa.hip: kc_trig_exact.h agrees with the installed libm

namespace kc {
namespace {

const double kDvzSincostab[440] = {KC_SINCOSTAB_VALUES};
constexpr double kTwoPi = 2 * M_PI;  // Python's 2 * math.pi
constexpr int kDvzBlock = 256;
constexpr size_t kDvzMaxBeams = size_t{1} << 24;

// kc_trig_exact.h covers |x| < 105414350 (sincos_reduce): beyond, NaN and inf go to the host's libm
bool device_trig_covers(double x) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  return (static_cast<uint32_t>(u >> 32) & 0x7fffffffu) < 0x419921FBu;
}

// The reference takes np.cos / np.sin: the host libm's separate cos and sin, called through pointers (host_cos and
// host_sin, kc_internal.h) so that the compiler cannot fold the pair into one sincos call.  On x86-64, glibc picks
// FMA builds of cos and sin on FMA hardware; those differ from `sincos` -- which kc_trig_exact.h restates and which
// has no FMA build -- by one ulp in about 0.1 % of arguments.  The device trig is therefore used only when the
// restatement also agrees with the separate cos and sin on a fixed argument set; otherwise the host fills the table.
bool dvz_trig_ok() {
  static const bool ok = [] {
    if (!trig_selfcheck_ok()) return false;
    unsigned long long st = 0x2545F4914F6CDD1Dull;
    auto unit = [&st]() {  // xorshift64*
      st ^= st >> 12;
      st ^= st << 25;
      st ^= st >> 27;
      return static_cast<double>((st * 0x2545F4914F6CDD1Dull) >> 11) * 0x1p-53;
    };
    const double ranges[][2] = {{0.0, 1e-7}, {0.0, 0.86}, {0.85, 2.43}, {2.42, 7.0}, {7.0, 13.0}, {13.0, 1.0e4}};
    for (const auto &r : ranges)
      for (int i = 0; i < 4000; ++i) {
        const double x = (i & 1 ? -1.0 : 1.0) * (r[0] + (r[1] - r[0]) * unit());
        double s, c;
        if (!trig::sincos_exact(x, &s, &c, kDvzSincostab)) return false;
        const double hs = host_sin(x), hc = host_cos(x);
        if (std::memcmp(&s, &hs, 8) != 0 || std::memcmp(&c, &hc, 8) != 0) return false;
      }
    return true;
  }();
  return ok;
}

struct DvzArgs {
  const double *angles, *ranges;
  const double2 *trig;  // fallback: (cos, sin) of every beam from the host's libm; null: device sincos
  const double *tab;    // the 440 table values of kc_trig_exact.h
  double minor, major, shift_x, shift_y, ori, minor2, major2, C;
  int n;
  double *radii;         // [n] deformed radius per beam (deformation_plot), or null
  double *partial;       // [3 * gridDim.x] per-workgroup (total, orientation, count)
  unsigned int *ticket;  // zero at launch; the last workgroup clears it
  double *result;        // {total, orientation_sum, n_deformed}
};

__device__ __forceinline__ void wave_sum(double v[3]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] += __shfl_xor(v[k], off, 64);
}

// the workgroup's sums in lane 0: wavefront butterflies, then the four wavefronts in index order
__device__ __forceinline__ void block_sum(double v[3], double (*s)[3]) {
  wave_sum(v);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 3; ++k) s[wave][k] = v[k];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kDvzBlock / 64; ++w)
      for (int k = 0; k < 3; ++k) v[k] += s[w][k];
}

__global__ __launch_bounds__(kDvzBlock) void dvz_deform_kernel(DvzArgs a) {
  __shared__ double ltab[440];  // the sincos table as four rows of 110 (trig::TabRows)
  __shared__ double s_wave[kDvzBlock / 64][3];
  __shared__ int s_last;
  if (!a.trig)
    for (int k = threadIdx.x; k < 440; k += kDvzBlock) ltab[(k & 3) * 110 + (k >> 2)] = a.tab[k];
  __syncthreads();
  const int i = blockIdx.x * kDvzBlock + threadIdx.x;
  double v[3] = {0.0, 0.0, 0.0};  // this beam's deformation, deformation * angle, 1 when deformed
  if (i < a.n) {
    const double angle = a.angles[i];
    double cs, sn;
    if (a.trig) {
      const double2 t = a.trig[i];
      cs = t.x;
      sn = t.y;
    } else {
      trig::sincos_exact(angle - a.ori, &sn, &cs, trig::TabRows{ltab});  // (in range: checked by the host)
    }
    // _get_undeformed_radius: x ** 2 as x * x
    const double mc = a.minor * cs, ms = a.major * sn;
    const double A = mc * mc + ms * ms;
    const double B = 2.0 * (a.shift_x * cs * a.minor2 + a.shift_y * sn * a.major2);
    const double root = dsqrt_rn(B * B - 4.0 * A * a.C);
    const double undeformed = (-B + root) / (2.0 * A);
    // _get_deformation_radius
    const double range = a.ranges[i];
    const double deformed = undeformed > range ? range : undeformed;
    if (a.radii) a.radii[i] = deformed;
    if (deformed < undeformed) {
      v[0] = (undeformed - deformed) / deformed;
      // convert_to_0_2pi: Python's %, i.e. fmod, + 2 pi below zero, +0.0 for a zero remainder
      double m = fmod(angle, kTwoPi);
      if (m < 0.0)
        m += kTwoPi;
      else if (m == 0.0)
        m = 0.0;
      v[1] = v[0] * m;
      v[2] = 1.0;
    }
  }
  block_sum(v, s_wave);
  if (threadIdx.x == 0) {
    for (int k = 0; k < 3; ++k)
      __hip_atomic_store(reinterpret_cast<unsigned long long *>(a.partial) + 3 * blockIdx.x + k,
                         static_cast<unsigned long long>(__double_as_longlong(v[k])), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    s_last = atomicAdd(a.ticket, 1u) == gridDim.x - 1 ? 1 : 0;
  }
  __syncthreads();
  if (!s_last) return;
  // ---- last arriver: every other workgroup's partials are behind its ticket ----
  __threadfence();
  double w[3] = {0.0, 0.0, 0.0};
  for (unsigned g = threadIdx.x; g < gridDim.x; g += kDvzBlock)
    for (int k = 0; k < 3; ++k)
      w[k] += __longlong_as_double(static_cast<long long>(__hip_atomic_load(
          reinterpret_cast<const unsigned long long *>(a.partial) + 3 * g + k, __ATOMIC_RELAXED,
          __HIP_MEMORY_SCOPE_AGENT)));
  __syncthreads();  // s_wave is reused
  block_sum(w, s_wave);
  if (threadIdx.x == 0) {
    for (int k = 0; k < 3; ++k) a.result[k] = w[k];
    *a.ticket = 0u;
  }
}

}  // namespace
}  // namespace kc

using namespace kc;

struct kc_dvz {
  int device = 0;
  hipStream_t stream = nullptr;
  size_t cap = 0;
  DevBuf<double> d_angles, d_ranges, d_radii, d_partial, d_result, d_tab;
  DevBuf<double2> d_trig;
  DevBuf<unsigned int> d_ticket;
  PinBuf<double> h_in;      // staging: [angles | ranges]
  PinBuf<double> h_result;  // the record {total, orientation_sum, n_deformed}
  PinBuf<double> h_radii;   // deformation_plot, on request
  PinBuf<double2> h_trig;   // the host libm's (cos, sin) when the device trig does not apply
  // kc_dvz_deform_worldmap: the map's virtual scan (DESIGN.md 4.11 rules 20 to 27) lands in d_ranges
  OrderEvent map_ready;     // the map's stream, for its writes
  ScanTable scan_table;
  DevBuf<double> d_real;    // rule 27's present scan
  PinBuf<double> h_ranges;  // the ranges the zone was deformed by, on request
};

namespace {

// One deformation but for where the ranges come from: fill() queues them into z->d_ranges on the context's stream, after
// the angles' upload.  ranges_out: a copy of them for the caller, or nullptr.
template <typename Fill>
int dvz_run(kc_dvz *z, const kc_dvz_zone *zone, const double *angles, size_t n, double out[3], double *radii_or_null,
            double *ranges_out, Fill fill) {
  hipStream_t s = z->stream;
  DvzArgs a{};
  a.minor = zone->minor_radius;
  a.major = zone->major_radius;
  a.shift_x = zone->center_shift_x;
  a.shift_y = zone->center_shift_y;
  a.ori = zone->ori_shift;
  // dvz.py:232-236, with the reference's operand order; x ** 2 as x * x
  a.minor2 = a.minor * a.minor;
  a.major2 = a.major * a.major;
  const double cx = a.shift_x * a.minor, cy = a.shift_y * a.major, mm = a.minor * a.major;
  a.C = cx * cx + cy * cy - mm * mm;
  a.n = static_cast<int>(n);
  std::memcpy(z->h_in.p, angles, n * sizeof(double));
  bool dev_trig = dvz_trig_ok();
  for (size_t i = 0; dev_trig && i < n; ++i) dev_trig = device_trig_covers(angles[i] - a.ori);
  KC_HIP(hipMemcpyAsync(z->d_angles.p, z->h_in.p, n * sizeof(double), hipMemcpyHostToDevice, s));
  KC_TRY(fill());
  if (!dev_trig) {  // np.cos / np.sin of the reference: the host libm's cos / sin
    KC_TRY(z->h_trig.reserve(n));
    KC_TRY(z->d_trig.reserve(n));
    for (size_t i = 0; i < n; ++i) {
      const double x = angles[i] - a.ori;
      z->h_trig.p[i] = make_double2(host_cos(x), host_sin(x));
    }
    KC_HIP(hipMemcpyAsync(z->d_trig.p, z->h_trig.p, n * sizeof(double2), hipMemcpyHostToDevice, s));
    a.trig = z->d_trig.p;
  }
  a.angles = z->d_angles.p;
  a.ranges = z->d_ranges.p;
  a.tab = z->d_tab.p;
  a.radii = radii_or_null ? z->d_radii.p : nullptr;
  a.partial = z->d_partial.p;
  a.ticket = z->d_ticket.p;
  a.result = z->d_result.p;
  const unsigned blocks = static_cast<unsigned>((n + kDvzBlock - 1) / kDvzBlock);
  hipLaunchKernelGGL(dvz_deform_kernel, dim3(blocks), dim3(kDvzBlock), 0, s, a);
  KC_HIP(hipGetLastError());
  KC_HIP(hipMemcpyAsync(z->h_result.p, z->d_result.p, 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (radii_or_null) {
    KC_TRY(z->h_radii.reserve(n));
    KC_HIP(hipMemcpyAsync(z->h_radii.p, z->d_radii.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  if (ranges_out) {
    KC_TRY(z->h_ranges.reserve(n));
    KC_HIP(hipMemcpyAsync(z->h_ranges.p, z->d_ranges.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  KC_HIP(hipStreamSynchronize(s));
  std::memcpy(out, z->h_result.p, 3 * sizeof(double));
  if (radii_or_null) std::memcpy(radii_or_null, z->h_radii.p, n * sizeof(double));
  if (ranges_out) std::memcpy(ranges_out, z->h_ranges.p, n * sizeof(double));
  return KC_OK;
}

}  // namespace

extern "C" {

int kc_dvz_create(int device, size_t max_beams, kc_dvz **out) {
  if (!out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *out = nullptr;
  if (max_beams == 0) KC_FAIL(KC_ERR_INVALID, "max_beams must be at least 1");
  if (max_beams > kDvzMaxBeams) KC_FAIL(KC_ERR_RANGE, "max_beams %zu above %zu", max_beams, kDvzMaxBeams);
  hipStream_t stream = nullptr;
  KC_TRY(open_device_stream(device, &stream));
  auto *z = new kc_dvz();
  z->device = device;
  z->stream = stream;
  z->cap = max_beams;
  auto fail = [&](int rc) {
    kc_dvz_destroy(z);
    return rc;
  };
  const size_t blocks = (max_beams + kDvzBlock - 1) / kDvzBlock;
  int rc;
  if ((rc = z->d_angles.reserve(max_beams)) || (rc = z->d_ranges.reserve(max_beams)) ||
      (rc = z->d_radii.reserve(max_beams)) || (rc = z->d_partial.reserve(3 * blocks)) ||
      (rc = z->d_result.reserve(3)) || (rc = z->d_tab.reserve(440)) || (rc = z->d_ticket.reserve(1)) ||
      (rc = z->h_in.reserve(2 * max_beams)) || (rc = z->h_result.reserve(3)))
    return fail(rc);
  // the arrival ticket starts at zero once; every launch's last workgroup clears it again
  if (hipMemset(z->d_ticket.p, 0, sizeof(unsigned int)) != hipSuccess ||
      hipMemcpy(z->d_tab.p, kDvzSincostab, sizeof(kDvzSincostab), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("DVZ context initialisation failed");
    return fail(KC_ERR_HIP);
  }
  *out = z;
  return KC_OK;
}

void kc_dvz_destroy(kc_dvz *z) {
  if (!z) return;
  close_device_stream(z->device, &z->stream);
  delete z;
}

int kc_dvz_deform(kc_dvz *z, const kc_dvz_zone *zone, const double *angles, const double *ranges, size_t n,
                  double out[3], double *radii_or_null) {
  if (!z || !zone || !out || (n && (!angles || !ranges))) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (n > z->cap) KC_FAIL(KC_ERR_RANGE, "%zu beams for a context of %zu", n, z->cap);
  if (!(zone->minor_radius > 0.0) || !(zone->major_radius > 0.0))
    KC_FAIL(KC_ERR_INVALID, "zone radii must be positive (minor %g, major %g)", zone->minor_radius,
            zone->major_radius);
  out[0] = out[1] = out[2] = 0.0;
  if (n == 0) return KC_OK;
  KC_HIP(hipSetDevice(z->device));
  return dvz_run(z, zone, angles, n, out, radii_or_null, nullptr, [&]() -> int {
    std::memcpy(z->h_in.p + n, ranges, n * sizeof(double));
    KC_HIP(hipMemcpyAsync(z->d_ranges.p, z->h_in.p + n, n * sizeof(double), hipMemcpyHostToDevice, z->stream));
    return KC_OK;
  });
}

// Check order: null arguments; the count, the zone, the scan's own refusals, the angles, the pose; the map's device; then
// the device
int kc_dvz_deform_worldmap(kc_dvz *z, const kc_dvz_zone *zone, kc_worldmap *map, const kc_worldmap_pose *pose,
                           const double *angles, size_t n, float range_max, unsigned int flags, const double *real_or_null,
                           double out[3], double *radii_or_null, double *ranges_or_null) {
  if (!z || !zone || !map || !pose || !angles || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (n > z->cap) KC_FAIL(KC_ERR_RANGE, "%zu beams for a context of %zu", n, z->cap);
  if (!(zone->minor_radius > 0.0) || !(zone->major_radius > 0.0))
    KC_FAIL(KC_ERR_INVALID, "zone radii must be positive (minor %g, major %g)", zone->minor_radius,
            zone->major_radius);
  WorldMapView v{};
  KC_TRY(worldmap_view(map, &v));
  WorldMapScan sc{};
  KC_TRY(worldmap_scan_check(v.res, 1, n, range_max, flags, &sc.rc));
  for (size_t k = 0; k < n; ++k)
    if (!std::isfinite(angles[k])) KC_FAIL(KC_ERR_INVALID, "beam angle %zu is not finite", k);
  KC_TRY(worldmap_check_pose(pose));
  if (v.device != z->device) KC_FAIL(KC_ERR_INVALID, "world map on device %d, DVZ context on device %d", v.device, z->device);
  out[0] = out[1] = out[2] = 0.0;
  KC_HIP(hipSetDevice(z->device));
  if (real_or_null) KC_TRY(z->d_real.reserve(n));
  return dvz_run(z, zone, angles, n, out, radii_or_null, ranges_or_null, [&]() -> int {
    hipStream_t s = z->stream;
    KC_TRY(z->scan_table.ensure(angles, n, s));
    if (real_or_null) {
      std::memcpy(z->h_in.p + n, real_or_null, n * sizeof(double));
      KC_HIP(hipMemcpyAsync(z->d_real.p, z->h_in.p + n, n * sizeof(double), hipMemcpyHostToDevice, s));
    }
    KC_TRY(stream_wait_through(z->map_ready, s, v.stream));  // for the map's writes; the host does not wait
    sc.table = z->scan_table.d.p;
    sc.pose = *pose;
    sc.n_poses = 1;
    sc.n_beams = n;
    sc.range_max = range_max;
    sc.flags = flags;
    sc.real = real_or_null ? z->d_real.p : nullptr;
    sc.ranges = z->d_ranges.p;
    return worldmap_queue_scan(v, sc, s);
  });
}

}  // extern "C"
