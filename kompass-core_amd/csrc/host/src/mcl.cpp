// MCL host side: the doubles around kc_mcl_* (no reference counterpart, see the header).
#include "mapping/mcl.h"

#include <cmath>
#include <stdexcept>

namespace Kompass {
namespace Mapping {

namespace {
// libm's separate cos and sin through pointers, so that the compiler cannot fold the pair into one sincos call, whose
// bits can differ from theirs (the scan table's note)
double (*volatile host_cos)(double) = static_cast<double (*)(double)>(std::cos);
double (*volatile host_sin)(double) = static_cast<double (*)(double)>(std::sin);
constexpr double kTwoPi = 2.0 * M_PI;

__int128 wide(uint64_t lo, int64_t hi) { return (static_cast<__int128>(hi) << 64) + static_cast<__int128>(lo); }
int64_t floorDiv(__int128 a, uint64_t b) {
  __int128 q = a / static_cast<__int128>(b);
  if (a % static_cast<__int128>(b) < 0) --q;
  return static_cast<int64_t>(q);
}
}  // namespace

MCL::MCL(const WorldMap &map, size_t n_particles, const std::vector<double> &angles, float range_max, uint64_t seed)
    : map_(map), n_(n_particles), beams_(angles.size()), range_max_(range_max),
      ctx_(hip::make<Handle>(kc_mcl_create, map.hipContext(), n_particles, angles.data(), angles.size(), range_max, seed)) {
  hip::check(kc_mcl_info(ctx_.get(), nullptr, nullptr, nullptr, &zmax_, nullptr));
  setModel(Model{});
}

int32_t MCL::noiseScale(double sigma_units) {
  const double s = std::nearbyint(sigma_units * 65536.0 / std::sqrt((65536.0 * 65536.0 - 1.0) / 3.0));
  if (!(s >= 0.0 && s <= 2147483647.0)) throw std::invalid_argument("sigma out of range");
  return static_cast<int32_t>(s);
}

uint32_t MCL::quantiseHeading(double yaw) {
  if (!std::isfinite(yaw)) throw std::invalid_argument("yaw is not finite");
  return static_cast<uint32_t>(std::llrint(yaw / kTwoPi * 65536.0) & 0xFFFF);
}

std::vector<int32_t> MCL::quantiseRanges(const std::vector<double> &ranges, float resolution, float range_max, unsigned flags) {
  const double r = static_cast<double>(resolution), m = static_cast<double>(range_max);
  const int32_t zmax = static_cast<int32_t>(std::llrint(m / r * 65536.0));
  const int32_t none = (flags & KC_MCL_SKIP_NO_RETURN) ? -1 : zmax;
  std::vector<int32_t> out(ranges.size());
  for (size_t k = 0; k < ranges.size(); ++k) {
    const double z = ranges[k];
    out[k] = (std::isfinite(z) && z >= 0.0 && z < m) ? static_cast<int32_t>(std::llrint(z / r * 65536.0)) : none;
  }
  return out;
}

std::array<int64_t, 3> MCL::odometryIncrement(float resolution, const std::array<double, 3> &a, const std::array<double, 3> &b) {
  const double r = static_cast<double>(resolution);
  const double dx = b[0] - a[0], dy = b[1] - a[1];
  const double c = host_cos(a[2]), s = host_sin(a[2]);
  const double f = (c * dx + s * dy) / r * 65536.0, l = (-s * dx + c * dy) / r * 65536.0;
  const double t = (b[2] - a[2]) / kTwoPi * 65536.0;
  if (!std::isfinite(f) || !std::isfinite(l) || !std::isfinite(t) || std::fabs(t) > 2147483647.0 || std::fabs(f) > 9.0e18 ||
      std::fabs(l) > 9.0e18)
    throw std::invalid_argument("the odometry increment is not finite or out of range");
  return {static_cast<int64_t>(std::llrint(f)), static_cast<int64_t>(std::llrint(l)), static_cast<int64_t>(std::llrint(t))};
}

MCL::Tables MCL::sensorTables(float resolution, const Model &m) {
  if (!(m.sigma_hit > 0.0) || !(m.floor > 0.0 && m.floor < 1.0) || !(m.pen_scale > 0.0) || !(m.temperature > 0.0) || m.n_pen < 1 ||
      m.n_w < 1 || m.err_shift < 0 || m.err_shift > 30 || m.w_shift < 0 || m.w_shift > 30)
    throw std::invalid_argument("sensor model out of range");
  Tables t;
  t.err_shift = m.err_shift;
  t.w_shift = m.w_shift;
  const double sig = m.sigma_hit / static_cast<double>(resolution) * 65536.0;
  for (int i = 0; i < m.n_pen; ++i) {
    const double d = static_cast<double>(static_cast<int64_t>(i) << m.err_shift);
    const double v = std::nearbyint(m.pen_scale * -std::log(m.floor + (1.0 - m.floor) * std::exp(-d * d / (2.0 * sig * sig))));
    t.pen.push_back(static_cast<uint16_t>(v > 65535.0 ? 65535.0 : v));
  }
  for (int i = 0; i < m.n_w; ++i)
    t.wtab.push_back(static_cast<uint32_t>(std::nearbyint(
        static_cast<double>(m.wtab0) * std::exp(-static_cast<double>(static_cast<int64_t>(i) << m.w_shift) / m.temperature))));
  return t;
}

MCL::FieldTables MCL::fieldTables(float resolution, const FieldModel &m) {
  if (!(m.sigma_hit > 0.0) || !(m.floor > 0.0 && m.floor < 1.0) || !(m.pen_scale > 0.0) || !(m.temperature > 0.0) || m.n_w < 1 ||
      m.w_shift < 0 || m.w_shift > 30 || m.reach < 0 || m.reach > 63)
    throw std::invalid_argument("field model out of range");
  FieldTables t;
  const double sig = m.sigma_hit / static_cast<double>(resolution);  // cells
  t.reach = m.reach;
  if (t.reach == 0) {
    const double r = std::ceil(3.0 * sig);
    t.reach = r < 1.0 ? 1 : (r > 63.0 ? 63 : static_cast<int>(r));
  }
  const int c2 = t.reach * t.reach;
  for (int d = 0; d <= c2; ++d) {
    const double v = std::nearbyint(m.pen_scale * -std::log(m.floor + (1.0 - m.floor) * std::exp(-static_cast<double>(d) / (2.0 * sig * sig))));
    t.pen_d2.push_back(static_cast<uint16_t>(v > 65535.0 ? 65535.0 : v));
  }
  const double far = std::nearbyint(m.pen_scale * -std::log(m.floor));
  t.pen_far = static_cast<uint16_t>(far > 65535.0 ? 65535.0 : far);
  Model w;
  w.w_shift = m.w_shift;
  w.n_w = m.n_w;
  w.wtab0 = m.wtab0;
  w.temperature = m.temperature;
  w.n_pen = 1;
  const Tables wt = sensorTables(resolution, w);
  t.wtab = wt.wtab;
  t.w_shift = wt.w_shift;
  return t;
}

MCL::Estimate MCL::estimateOf(const kc_mcl_record &r, float resolution, double origin_x, double origin_y) {
  if (r.w1 == 0) throw std::invalid_argument("a record without weight");
  Estimate e;
  e.record = r;
  e.txe = r.best_tx + floorDiv(wide(r.sx_lo, r.sx_hi), r.w1);
  e.tye = r.best_ty + floorDiv(wide(r.sy_lo, r.sy_hi), r.w1);
  const double res = static_cast<double>(resolution);
  e.x = origin_x + static_cast<double>(e.txe) / 65536.0 * res;
  e.y = origin_y + static_cast<double>(e.tye) / 65536.0 * res;
  e.yaw = std::atan2(static_cast<double>(r.ss), static_cast<double>(r.sc));
  e.n_eff = static_cast<double>(r.w1) * static_cast<double>(r.w1) / static_cast<double>(r.w2);
  e.best_cost = r.amin;
  return e;
}

bool MCL::shouldResample(const kc_mcl_record &r, size_t n, uint32_t num, uint32_t den) {
  const unsigned __int128 lhs = static_cast<unsigned __int128>(r.w1) * r.w1 * den;
  const unsigned __int128 rhs = static_cast<unsigned __int128>(num) * n * r.w2;
  return lhs < rhs;
}

void MCL::setModel(const Model &m) { setTables(sensorTables(map_.resolution(), m)); }

void MCL::setTables(const Tables &t) {
  hip::check(kc_mcl_set_model(ctx_.get(), t.pen.data(), t.pen.size(), t.err_shift, t.wtab.data(), t.wtab.size(), t.w_shift));
  tables_ = t;
  field_ = false;
}

void MCL::setFieldModel(const FieldModel &m) { setFieldTables(fieldTables(map_.resolution(), m)); }

void MCL::setFieldTables(const FieldTables &t) {
  hip::check(kc_mcl_field_check(map_.resolution(), n_, beams_, range_max_, t.pen_d2.data(), t.pen_d2.size(), t.reach, t.wtab.data(),
                                t.wtab.size(), t.w_shift, 0u, nullptr, nullptr));
  hip::check(kc_mcl_set_field_model(ctx_.get(), t.pen_d2.data(), t.pen_d2.size(), t.pen_far, t.wtab.data(), t.wtab.size(), t.w_shift));
  if (map_.distanceReach() < t.reach)
    hip::check(kc_worldmap_set_distance(map_.hipContext(), t.reach, (flags_ & KC_SCAN_UNKNOWN_BLOCKS) ? KC_WORLDMAP_DIST_UNKNOWN_BLOCKS : 0u));
  tables_.wtab = t.wtab;  // what spreadOf reads
  tables_.w_shift = t.w_shift;
  field_ = true;
}

void MCL::setMotionNoise(double sigma_forward, double sigma_lateral, double sigma_yaw) {
  const double cells = 65536.0 / static_cast<double>(map_.resolution());
  s_f_ = noiseScale(sigma_forward * cells);
  s_l_ = noiseScale(sigma_lateral * cells);
  s_h_ = noiseScale(sigma_yaw / kTwoPi * 65536.0);
}

void MCL::setResampleRatio(uint32_t num, uint32_t den) {
  if (den == 0 || den > 65536 || num > den) throw std::invalid_argument("the resample ratio must be num / den <= 1, den in 1 .. 65536");
  r_num_ = num;
  r_den_ = den;
}

void MCL::setFlags(bool unknown_blocks, bool skip_no_return) {
  flags_ = (unknown_blocks ? KC_SCAN_UNKNOWN_BLOCKS : 0u) | (skip_no_return ? KC_MCL_SKIP_NO_RETURN : 0u);
}

void MCL::setRecovery(const Recovery &r) {
  // the library's own refusals, on a state and a step that are fine
  kc_mcl_recovery probe{};
  size_t n = 0;
  hip::check(kc_mcl_recovery_update(0, 1, 0, r.a_slow, r.a_fast, r.max_num, r.max_den, &probe, nullptr, &n));
  recovery_ = r;
  recovery_on_ = true;
}

void MCL::init(double x, double y, double yaw, double sigma_xy, double sigma_yaw) {
  const kc_worldmap_pose p = WorldMap::quantisePose(map_.resolution(), map_.originX(), map_.originY(), x, y, 0.0);
  hip::check(kc_mcl_init_pose(ctx_.get(), p.tx, p.ty, quantiseHeading(yaw),
                              noiseScale(sigma_xy * 65536.0 / static_cast<double>(map_.resolution())),
                              noiseScale(sigma_yaw / kTwoPi * 65536.0)));
  fit_state_ = {};
}

size_t MCL::initGlobal() {
  size_t n_free = 0;
  hip::check(kc_mcl_init_global(ctx_.get(), &n_free));
  fit_state_ = {};
  return n_free;
}

MCL::Estimate MCL::step(const std::array<double, 3> &from, const std::array<double, 3> &to, const std::vector<double> &ranges) {
  if (ranges.size() != beams_) throw std::invalid_argument("one range a beam");
  const auto d = odometryIncrement(map_.resolution(), from, to);
  // the field model's plane has its own flag for what blocks (rule 45)
  const unsigned flags = field_ ? (flags_ & ~static_cast<unsigned>(KC_SCAN_UNKNOWN_BLOCKS)) : flags_;
  return stepQuantised(d[0], d[1], static_cast<int32_t>(d[2]), s_f_, s_l_, s_h_,
                       quantiseRanges(ranges, map_.resolution(), range_max_, flags), flags, true);
}

MCL::Estimate MCL::stepQuantised(int64_t d_f, int64_t d_l, int32_t d_h, int32_t s_f, int32_t s_l, int32_t s_h,
                                 const std::vector<int32_t> &zq, unsigned flags, bool resample_allowed) {
  if (zq.size() != beams_) throw std::invalid_argument("one quantised range a beam");
  kc_mcl_record r{};
  hip::check(kc_mcl_step(ctx_.get(), d_f, d_l, d_h, s_f, s_l, s_h, zq.data(), flags, &r));
  Estimate e = estimateOf(r, map_.resolution(), map_.originX(), map_.originY());
  if (spread_) e.spread = spreadOf(e);
  // rules 59 to 61: the averages run whether or not recovery is on
  kc_mcl_fit fit{};
  hip::check(kc_mcl_last_fit(ctx_.get(), &fit));
  e.cost_min = fit.cost_min;
  e.cost_best = fit.cost_best;
  for (const int32_t z : zq) e.beams_used += field_ ? (z >= 0 && z < zmax_) : (z != -1);
  size_t n_inject = 0;
  hip::check(kc_mcl_recovery_update(fit.cost_sum, n_, e.beams_used, recovery_.a_slow, recovery_.a_fast, recovery_.max_num,
                                    recovery_.max_den, &fit_state_, &e.fit, &n_inject));
  e.fit_slow = fit_state_.slow;
  e.fit_fast = fit_state_.fast;
  if (!recovery_on_ || !resample_allowed) n_inject = 0;
  if (resample_allowed && (n_inject > 0 || shouldResample(r, n_, r_num_, r_den_))) {  // rule 63
    hip::check(kc_mcl_resample_inject(ctx_.get(), n_inject));
    e.injected = n_inject;
    e.resampled = true;
  }
  return e;
}

void MCL::resample() { hip::check(kc_mcl_resample(ctx_.get())); }

MCL::Particles MCL::particles() const {
  Particles p;
  p.tx.resize(n_);
  p.ty.resize(n_);
  p.h.resize(n_);
  p.acc.resize(n_);
  hip::check(kc_mcl_particles(ctx_.get(), p.tx.data(), p.ty.data(), p.h.data(), p.acc.data(), n_));
  return p;
}

// sqrt(sum w ((TX - TXe)^2 + (TY - TYe)^2) / W1) in metres: doubles in index order, the weights by rule 36 from the
// read-back acc
double MCL::spreadOf(const Estimate &e) const {
  const Particles p = particles();
  const uint32_t last = static_cast<uint32_t>(tables_.wtab.size() - 1);
  double sum = 0.0;
  for (size_t i = 0; i < n_; ++i) {
    const uint32_t bin = (p.acc[i] - e.record.amin) >> tables_.w_shift;
    const double w = static_cast<double>(tables_.wtab[bin < last ? bin : last]);
    const double dx = static_cast<double>(p.tx[i] - e.txe), dy = static_cast<double>(p.ty[i] - e.tye);
    sum += w * (dx * dx + dy * dy);
  }
  return std::sqrt(sum / static_cast<double>(e.record.w1)) / 65536.0 * static_cast<double>(map_.resolution());
}

}  // namespace Mapping
}  // namespace Kompass
