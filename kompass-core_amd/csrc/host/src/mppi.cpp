// MPPI host side: the doubles around kc_mppi_* (no reference counterpart, see the header).
#include "controllers/mppi.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <stdexcept>
#include <string>

#include "mapping/mcl.h"

namespace Kompass {
namespace Control {

namespace {
constexpr double kTwoPi = 2.0 * M_PI;

// rule 25: a rate from an acceleration already in rule 2's units a step^2, clamped into 1 .. cap
int32_t quantiseRate(double v, double cap, const char *what) {
  if (!std::isfinite(v) || v < 0.0) throw std::invalid_argument(std::string(what) + " is negative or not finite");
  return static_cast<int32_t>(std::llrint(std::max(1.0, std::min(v, cap))));
}

int32_t quantiseLimit(double v, double cap, const char *what) {
  if (!std::isfinite(v) || v < 0.0) throw std::invalid_argument(std::string(what) + " is negative or not finite");
  return static_cast<int32_t>(std::llrint(std::min(v, cap)));
}
}  // namespace

MPPI::MPPI(ControlType type, const ControlLimitsParams &limits, double time_step, const Config &config)
    : Follower(), cfg_(config), dt_(time_step) {
  if (!(time_step > 0.0) || !std::isfinite(time_step)) throw std::invalid_argument("the control time step must be positive");
  setControlType(type);
  setLinearControlLimits(limits.velXParams, limits.velYParams);
  setAngularControlLimits(limits.omegaParams);
  const Costs c = costsOf(cfg_);  // refuses a bad configuration before a device is looked for
  hip::check(kc_mppi_check(cfg_.samples, cfg_.horizon, cfg_.window, nullptr, nullptr, c.r2, c.pen_d2.data(), c.pen_d2.size(), c.pen_hit,
                           c.w_path, c.qcap, c.w_goal, cfg_.reach, c.wtab.data(), c.wtab.size(), c.w_shift));
  if (!(cfg_.mover_margin >= 0.0) || !(cfg_.mover_margin <= 1024.0) || !(cfg_.mover_weight >= 0.0) || !(cfg_.mover_weight <= 1048576.0) ||
      cfg_.mover_hit_penalty > (1u << 20))
    throw std::invalid_argument("MPPI moving-obstacle configuration out of range");
  hip::check(kc_mppi_check_field(cfg_.field_cap, cfg_.field_run_weight, cfg_.field_goal_weight));
  resetSequence();
}

void MPPI::setCostField(Planning::GridPlanner &planner) { field_ = &planner; }

void MPPI::clearCostField() {
  field_ = nullptr;
  f0_ = f_nom_ = 0xFFFFFFFFu;
}

void MPPI::setBoxFootprint(double length, double width) {
  if (!(length > 0.0) || !(width > 0.0) || !std::isfinite(length) || !std::isfinite(width))
    throw std::invalid_argument("a box footprint needs a positive, finite length and width");
  box_ = true;
  box_len_ = length;
  box_wid_ = width;
}

void MPPI::clearFootprint() { box_ = false; }

MPPI::Footprint MPPI::footprintOf(double length_m, double width_m, float resolution, double margin_cells) {
  const double r = static_cast<double>(resolution);
  if (!(r > 0.0) || !std::isfinite(r)) throw std::invalid_argument("the resolution must be positive");
  if (!(length_m > 0.0) || !(width_m > 0.0) || !std::isfinite(length_m) || !std::isfinite(width_m))
    throw std::invalid_argument("a box footprint needs a positive, finite length and width");
  if (!(margin_cells >= 0.0) || !std::isfinite(margin_cells)) throw std::invalid_argument("the footprint margin is negative or not finite");
  const double a = length_m / (2.0 * r), b = width_m / (2.0 * r);
  const int n = static_cast<int>(std::min(static_cast<double>(KC_MPPI_MAX_DISCS), std::max(1.0, std::ceil(a / b))));
  const double s = 2.0 * a / n;
  Footprint f;
  for (int i = 0; i < n; ++i) {
    const double o = (-a + s / 2.0 + i * s) * 65536.0;
    if (!(std::fabs(o) <= 4194304.0)) throw std::out_of_range("a disc of the footprint lies more than 64 cells from the pose");
    f.offsets.push_back(static_cast<int32_t>(std::llrint(o)));
  }
  f.rho = std::sqrt(b * b + s * s / 4.0);
  const double reach = f.rho + margin_cells;
  if (!(reach * reach <= 4294967295.0)) throw std::out_of_range("the footprint's r2 does not fit 32 bits");
  f.r2 = static_cast<uint32_t>(std::ceil(reach * reach));
  hip::check(kc_mppi_check_footprint(f.offsets.data(), f.offsets.size()));
  return f;
}

void MPPI::setMovingObstacles(std::vector<MovingObstacle> obstacles) { movers_ = std::move(obstacles); }

MovingObstacle MPPI::fromTrackedBox(const TrackedBbox3D &b) {
  return {static_cast<double>(b.box.center.x()), static_cast<double>(b.box.center.y()), static_cast<double>(b.vel.x()),
          static_cast<double>(b.vel.y()), std::hypot(static_cast<double>(b.box.size.x()), static_cast<double>(b.box.size.y())) / 2.0};
}

MPPI::Movers MPPI::moversOf(const std::vector<MovingObstacle> &obstacles, double time_step, float resolution, double ox, double oy,
                            double x, double y, const Config &c, double hit_cells) {
  const double r = static_cast<double>(resolution);
  const double hit_radius = hit_cells >= 0.0 ? hit_cells : c.hit_radius;
  if (!(r > 0.0) || !std::isfinite(r)) throw std::invalid_argument("the resolution must be positive");
  if (!(time_step > 0.0) || !std::isfinite(time_step)) throw std::invalid_argument("the control time step must be positive");
  Movers m;
  m.pen_hit = c.mover_hit_penalty;
  std::vector<size_t> pick(obstacles.size());
  std::iota(pick.begin(), pick.end(), size_t{0});
  if (pick.size() > KC_MPPI_MAX_MOVERS) {  // the nearest to the robot now, the lower index among equals; kept in index order
    std::stable_sort(pick.begin(), pick.end(), [&](size_t a, size_t b) {
      return std::hypot(obstacles[a].x - x, obstacles[a].y - y) < std::hypot(obstacles[b].x - x, obstacles[b].y - y);
    });
    m.dropped = pick.size() - KC_MPPI_MAX_MOVERS;
    pick.resize(KC_MPPI_MAX_MOVERS);
    std::sort(pick.begin(), pick.end());
  }
  for (const size_t i : pick) {
    const MovingObstacle &o = obstacles[i];
    auto refuse = [&](const char *what) { throw std::out_of_range("moving obstacle " + std::to_string(i) + ": " + what); };
    if (!std::isfinite(o.x) || !std::isfinite(o.y) || !std::isfinite(o.vx) || !std::isfinite(o.vy) || !std::isfinite(o.radius) ||
        o.radius < 0.0)
      refuse("a value is not finite or the radius is negative");
    const double fx = (o.x - ox) / r * 65536.0, fy = (o.y - oy) / r * 65536.0;  // as the pose is quantised
    const double pos_cap = 68719476736.0, vel_cap = 4194304.0, q_cap = 1099511627776.0;  // 2^36, 2^22, 2^40
    if (!(std::fabs(fx) <= pos_cap + 0.5) || !(std::fabs(fy) <= pos_cap + 0.5)) refuse("it lies more than 2^20 cells from the map's origin");
    const double vx = o.vx * time_step / r * 65536.0, vy = o.vy * time_step / r * 65536.0;
    if (!(std::fabs(vx) <= vel_cap) || !(std::fabs(vy) <= vel_cap)) refuse("it moves more than 64 cells a control step");
    const double hit = hit_radius + o.radius / r, soft = hit + c.mover_margin;
    const double hq = hit * hit * 65536.0, sq = soft * soft * 65536.0;
    if (!(sq <= q_cap)) refuse("its soft distance is above 4096 cells");
    m.ox.push_back(std::llrint(fx));
    m.oy.push_back(std::llrint(fy));
    m.vx.push_back(static_cast<int32_t>(std::llrint(vx)));
    m.vy.push_back(static_cast<int32_t>(std::llrint(vy)));
    m.hq.push_back(static_cast<uint64_t>(std::llrint(hq)));
    m.sq.push_back(static_cast<uint64_t>(std::llrint(sq)));
    m.g.push_back(static_cast<uint64_t>(std::floor(c.mover_weight * 65536.0 / static_cast<double>(((m.sq.back() - m.hq.back()) >> 16) + 1))));
  }
  // what is left of rule 18 (a rounding at a bound, the gain, the ramp's top) is the library's to refuse
  hip::check(kc_mppi_check_movers(m.ox.data(), m.oy.data(), m.vx.data(), m.vy.data(), m.hq.data(), m.sq.data(), m.g.data(), m.ox.size(),
                                  m.pen_hit));
  return m;
}

void MPPI::resetSequence() {
  u_.assign(cfg_.horizon * 3, 0);
  out_.clear();
  applied_.clear();
  v0_ = {0, 0, 0};
  step_ = 0;
}

MPPI::Quantised MPPI::quantise(ControlType type, const ControlLimitsParams &limits, double time_step, float resolution, const Config &c) {
  const double r = static_cast<double>(resolution);
  if (!(r > 0.0) || !std::isfinite(r)) throw std::invalid_argument("the resolution must be positive");
  Quantised q;
  const double cap = 4194304.0;  // rule 2's 2^22
  q.f_hi = quantiseLimit(limits.velXParams.maxVel * time_step / r * 65536.0, cap, "the forward limit");
  q.f_lo = c.allow_reverse ? -q.f_hi : 0;
  q.l_hi = type == ControlType::OMNI ? quantiseLimit(limits.velYParams.maxVel * time_step / r * 65536.0, cap, "the lateral limit") : 0;
  q.h_hi = quantiseLimit(limits.omegaParams.maxOmega * time_step / kTwoPi * 65536.0, 32767.0, "the turn limit");
  if (type == ControlType::ACKERMANN) {
    if (!(c.min_turning_radius > 0.0)) throw std::invalid_argument("the turning radius must be positive");
    q.kq = quantiseLimit(65536.0 / (kTwoPi * c.min_turning_radius / r), 16777216.0, "the turning cone");
  }
  q.s = {Mapping::MCL::noiseScale(c.sigma_forward * 65536.0),
         type == ControlType::OMNI ? Mapping::MCL::noiseScale(c.sigma_lateral * 65536.0) : 0,
         Mapping::MCL::noiseScale(c.sigma_turn / kTwoPi * 65536.0)};
  // rule 25: a change a control step
  const double lin = time_step * time_step / r * 65536.0, ang = time_step * time_step / kTwoPi * 65536.0;
  const double lin_cap = 8388608.0, ang_cap = 65535.0;  // 2^23
  if (c.acceleration_limits)
    q.rates = {quantiseRate(limits.velXParams.maxAcceleration * lin, lin_cap, "the forward acceleration"),
               quantiseRate(limits.velXParams.maxDeceleration * lin, lin_cap, "the forward deceleration"),
               quantiseRate(limits.velYParams.maxAcceleration * lin, lin_cap, "the lateral acceleration"),
               quantiseRate(limits.velYParams.maxDeceleration * lin, lin_cap, "the lateral deceleration"),
               quantiseRate(limits.omegaParams.maxAcceleration * ang, ang_cap, "the turn acceleration"),
               quantiseRate(limits.omegaParams.maxDeceleration * ang, ang_cap, "the turn deceleration")};
  return q;
}

MPPI::Costs MPPI::costsOf(const Config &c) {
  if (!(c.hit_radius >= 0.0) || !(c.clearance >= 1.0) || !(c.clearance <= 63.0) || !(c.hit_radius <= c.clearance) ||
      !(c.clearance_weight >= 0.0) || !(c.clearance_weight <= 65535.0) || !(c.lambda > 0.0) || c.n_w < 1 || c.w_shift < 0 ||
      c.w_shift > 30 || !(c.path_cap >= 0.0) || !(c.path_cap <= 1024.0))
    throw std::invalid_argument("MPPI configuration out of range");
  Costs t;
  t.r2 = static_cast<uint32_t>(std::llrint(c.hit_radius * c.hit_radius));
  const int c2 = static_cast<int>(std::llrint(c.clearance * c.clearance));
  for (int d = 0; d <= c2; ++d)
    t.pen_d2.push_back(static_cast<uint16_t>(
        std::nearbyint(c.clearance_weight * std::max(0.0, 1.0 - std::sqrt(static_cast<double>(d)) / c.clearance))));
  t.pen_far = c.pen_far;
  t.pen_hit = c.pen_hit;
  t.w_path = c.w_path;
  t.qcap = static_cast<uint64_t>(std::llrint(c.path_cap * c.path_cap)) << 16;
  t.w_goal = c.w_goal;
  t.w_shift = c.w_shift;
  for (int i = 0; i < c.n_w; ++i)
    t.wtab.push_back(static_cast<uint32_t>(
        std::nearbyint(65535.0 * std::exp(-static_cast<double>(static_cast<int64_t>(i) << c.w_shift) / c.lambda))));
  return t;
}

void MPPI::bind(const Mapping::WorldMap &map) {
  const Costs c = costsOf(cfg_);
  const int c2 = static_cast<int>(c.pen_d2.size()) - 1;
  // The map is the caller's: the const reference is a promise not to change its cells, which holds
  const int have = map.distanceReach();
  if (have == 0 || have * have < c2) hip::check(kc_worldmap_set_distance(map.hipContext(), std::max(cfg_.reach, have), 0u));
  if (bound_ == map.hipContext() && ctx_) return;
  ctx_ = hip::make<Handle>(kc_mppi_create, map.hipContext(), cfg_.samples, cfg_.horizon, cfg_.seed);
  movers_on_device_ = false;
  field_on_device_ = false;
  rates_on_device_ = false;
  footprint_on_device_ = false;
  r2_on_device_ = c.r2;
  bound_ = map.hipContext();
  hip::check(kc_mppi_set_costs(ctx_.get(), c.r2, c.pen_d2.data(), c.pen_d2.size(), c.pen_far, c.pen_hit, c.w_path, c.qcap, c.w_goal,
                               c.wtab.data(), c.wtab.size(), c.w_shift));
}

// From the follower's closest point forward at one-cell arc spacing, up to M points; the path's end closes a window that
// reaches it.  Quantised against the map's present origin.
void MPPI::buildWindow(const Mapping::WorldMap &map) {
  in_.px.clear();
  in_.py.clear();
  const Path::Path &p = *on_.path;
  const size_t n = p.getSize();
  size_t i = std::min<size_t>(on_.nearest->index, n - 1);
  const double cell = static_cast<double>(res_);
  auto push = [&](double x, double y) {
    const kc_worldmap_pose q = Mapping::WorldMap::quantisePose(res_, ox_, oy_, x, y, 0.0);
    in_.px.push_back(q.tx);
    in_.py.push_back(q.ty);
  };
  double x = p.getIndex(i).x(), y = p.getIndex(i).y();
  push(x, y);
  double need = cell;  // arc length still to walk to the next point
  while (in_.px.size() < cfg_.window && i + 1 < n) {
    const double nx = p.getIndex(i + 1).x(), ny = p.getIndex(i + 1).y();
    const double d = std::hypot(nx - x, ny - y);
    if (d < need) {
      need -= d;
      x = nx;
      y = ny;
      ++i;
      if (i + 1 == n) push(x, y);  // the end itself
      continue;
    }
    const double f = d > 0.0 ? need / d : 0.0;
    x += (nx - x) * f;
    y += (ny - y) * f;
    push(x, y);
    need = cell;
  }
  (void)map;
}

Controller::Result MPPI::execute(const Mapping::WorldMap &map, const Path::State &state) {
  setCurrentState(state);
  const bool field = field_ != nullptr;
  if (field) {  // rule 20: no path; the goal is the planner's
    double gx = 0.0, gy = 0.0;
    if (!field_->goalWorld(&gx, &gy)) throw std::runtime_error("MPPI: the cost field's planner has no problem set up");
    if (std::hypot(state.x - gx, state.y - gy) <= knob_.goal_radius) {
      command_ = Velocity2D(0.0, 0.0, 0.0);
      return {Result::Status::GOAL_REACHED, command_};
    }
  } else {
    if (!on_.ready || !on_.path || on_.path->getSize() == 0)
      return {(on_.at_goal ? Result::Status::GOAL_REACHED : Result::Status::NO_COMMAND_POSSIBLE), {0.0, 0.0, 0.0}};
    if (isGoalReached()) {
      command_ = Velocity2D(0.0, 0.0, 0.0);
      return {Result::Status::GOAL_REACHED, command_};
    }
  }
  bind(map);
  if (res_ != map.resolution()) v0_ = {0, 0, 0};  // rule 28: the kept triple is in cells of another size
  res_ = map.resolution();
  ox_ = map.originX();
  oy_ = map.originY();
  const Quantised q = quantise(drive_, limits_, dt_, res_, cfg_);
  hip::check(kc_mppi_set_model(ctx_.get(), q.f_lo, q.f_hi, q.l_hi, q.h_hi, q.kq, q.s.data()));
  const bool limited = cfg_.acceleration_limits;
  in_.limited = limited;
  in_.rates = limited ? q.rates : std::array<int32_t, 6>{0, 0, 0, 0, 0, 0};
  in_.v0 = limited ? v0_ : std::array<int32_t, 3>{0, 0, 0};
  if (limited) {
    hip::check(kc_mppi_set_rates(ctx_.get(), q.rates.data()));
    hip::check(kc_mppi_set_velocity(ctx_.get(), v0_.data()));
    rates_on_device_ = true;
  } else if (rates_on_device_) {
    hip::check(kc_mppi_set_rates(ctx_.get(), nullptr));
    rates_on_device_ = false;
  }
  // rules 30 to 36: the offsets in cells of this map; the discs' r2 in the place of hit_radius'
  Footprint fp;
  double mover_hit = -1.0;
  in_.offsets.clear();
  in_.r2 = static_cast<uint32_t>(std::llrint(cfg_.hit_radius * cfg_.hit_radius));  // costsOf's r2, without its tables
  if (box_) {
    fp = footprintOf(box_len_, box_wid_, res_, cfg_.footprint_margin);
    const uint32_t c2 = static_cast<uint32_t>(std::llrint(cfg_.clearance * cfg_.clearance));
    if (fp.r2 > c2)
      throw std::invalid_argument("MPPI: the box footprint's r2 = " + std::to_string(fp.r2) + " is above c2 = " + std::to_string(c2) +
                                  ": raise `clearance` to at least " + std::to_string(std::sqrt(static_cast<double>(fp.r2))) + " cells");
    in_.offsets = fp.offsets;
    in_.r2 = fp.r2;
    mover_hit = fp.rho + cfg_.footprint_margin;
  }
  if (in_.r2 != r2_on_device_) {  // the costs with the other r2: only when a box was set, cleared or the resolution changed
    Costs c = costsOf(cfg_);
    c.r2 = in_.r2;
    hip::check(kc_mppi_set_costs(ctx_.get(), c.r2, c.pen_d2.data(), c.pen_d2.size(), c.pen_far, c.pen_hit, c.w_path, c.qcap, c.w_goal,
                                 c.wtab.data(), c.wtab.size(), c.w_shift));
    r2_on_device_ = c.r2;
  }
  if (box_ || footprint_on_device_) {
    hip::check(kc_mppi_set_footprint(ctx_.get(), in_.offsets.data(), in_.offsets.size()));
    footprint_on_device_ = box_;
  }
  in_.field = field;
  if (field) {
    in_.px.clear();
    in_.py.clear();
    hip::check(kc_mppi_set_field(ctx_.get(), field_->hipContext(), cfg_.field_cap, cfg_.field_run_weight, cfg_.field_goal_weight));
    field_on_device_ = true;
  } else {
    if (field_on_device_) {
      hip::check(kc_mppi_set_field(ctx_.get(), nullptr, 0u, 0u, 0u));
      field_on_device_ = false;
    }
    aimAtTarget();
    on_.segment = on_.target->segment_index;
    on_.along = on_.target->position_in_segment;
    buildWindow(map);
    hip::check(kc_mppi_set_path(ctx_.get(), in_.px.data(), in_.py.data(), in_.px.size()));
  }
  const kc_worldmap_pose pose = Mapping::WorldMap::quantisePose(res_, ox_, oy_, state.x, state.y, state.yaw);
  in_.tx = pose.tx;
  in_.ty = pose.ty;
  in_.h = Mapping::MCL::quantiseHeading(state.yaw);
  in_.step = step_;
  in_.u = u_;
  in_.movers = moversOf(movers_, dt_, res_, ox_, oy_, state.x, state.y, cfg_, mover_hit);
  if (in_.movers.dropped != 0 && !logged_drop_) {
    LOG_WARNING("MPPI takes the ", KC_MPPI_MAX_MOVERS, " moving obstacles nearest to the robot; ", in_.movers.dropped, " more were given");
    logged_drop_ = true;
  }
  if (!in_.movers.ox.empty() || movers_on_device_) {  // an empty list after a full one clears it; none at all costs nothing
    const Movers &mv = in_.movers;
    hip::check(kc_mppi_set_movers(ctx_.get(), mv.ox.data(), mv.oy.data(), mv.vx.data(), mv.vy.data(), mv.hq.data(), mv.sq.data(), mv.g.data(),
                                  mv.ox.size(), mv.pen_hit));
    movers_on_device_ = !mv.ox.empty();
  }
  out_.assign(cfg_.horizon * 3, 0);
  hip::check(kc_mppi_step(ctx_.get(), in_.tx, in_.ty, in_.h, in_.u.data(), in_.step, out_.data(), &rec_));
  ++step_;
  if (field) hip::check(kc_mppi_last_field(ctx_.get(), &f0_, &f_nom_));
  // the warm start: U[t] = U'[t + 1], the last entry repeated
  const size_t T = cfg_.horizon;
  for (size_t t = 0; t + 1 < T; ++t)
    for (int c = 0; c < 3; ++c) u_[3 * t + c] = out_[3 * (t + 1) + c];
  for (int c = 0; c < 3; ++c) u_[3 * (T - 1) + c] = out_[3 * (T - 1) + c];
  applied_.clear();
  if (limited) {  // rule 28: the command is the first applied control of U', and the next step's V0; no doubles in between
    const int32_t box[5] = {q.f_lo, q.f_hi, q.l_hi, q.h_hi, q.kq};
    std::vector<int32_t> applied(T * 3, 0);
    hip::check(kc_mppi_apply_rates(box, q.rates.data(), v0_.data(), out_.data(), T, applied.data()));
    applied_ = std::move(applied);
    v0_ = {applied_[0], applied_[1], applied_[2]};
    const std::array<double, 3> a = controls(1)[0];
    command_ = Velocity2D(a[0], a[1], a[2]);
    return {Result::Status::COMMAND_FOUND, command_};
  }
  const std::array<double, 3> v = controls(1)[0];
  const auto &lx = limits_.velXParams;
  const auto &ly = limits_.velYParams;
  const auto &lw = limits_.omegaParams;
  command_ = Velocity2D(restrictVelocityTolimits(command_.vx(), v[0], lx.maxAcceleration, lx.maxDeceleration, lx.maxVel, dt_),
                        restrictVelocityTolimits(command_.vy(), v[1], ly.maxAcceleration, ly.maxDeceleration, ly.maxVel, dt_),
                        restrictVelocityTolimits(command_.omega(), v[2], lw.maxAcceleration, lw.maxDeceleration, lw.maxOmega, dt_));
  return {Result::Status::COMMAND_FOUND, command_};
}

std::vector<std::array<double, 3>> MPPI::controls(size_t n) const {
  std::vector<std::array<double, 3>> out;
  const double r = static_cast<double>(res_);
  const std::vector<int32_t> &u = shown();
  for (size_t t = 0; t < n && 3 * t + 2 < u.size(); ++t)
    out.push_back({static_cast<double>(u[3 * t]) / 65536.0 * r / dt_, static_cast<double>(u[3 * t + 1]) / 65536.0 * r / dt_,
                   static_cast<double>(u[3 * t + 2]) / 65536.0 * kTwoPi / dt_});
  return out;
}

std::vector<std::array<double, 3>> MPPI::predictedPath() const {
  std::vector<std::array<double, 3>> out;
  int64_t tx = in_.tx, ty = in_.ty;
  uint32_t h = in_.h;
  const int64_t cap = int64_t{1} << 36;
  const double r = static_cast<double>(res_);
  const std::vector<int32_t> &u = shown();
  for (size_t t = 0; 3 * t + 2 < u.size(); ++t) {
    int32_t C = 0, S = 0;
    hip::check(kc_mcl_heading(h, &C, &S));
    const int64_t F = u[3 * t], L = u[3 * t + 1];
    tx = std::max(-cap, std::min(cap, tx + ((C * F - S * L + (int64_t{1} << 15)) >> 16)));
    ty = std::max(-cap, std::min(cap, ty + ((S * F + C * L + (int64_t{1} << 15)) >> 16)));
    h = static_cast<uint32_t>((static_cast<int64_t>(h) + u[3 * t + 2]) & 0xFFFF);
    out.push_back({ox_ + static_cast<double>(tx) / 65536.0 * r, oy_ + static_cast<double>(ty) / 65536.0 * r,
                   static_cast<double>(h) / 65536.0 * kTwoPi});
  }
  return out;
}

std::vector<uint32_t> MPPI::sampleCosts() const {
  if (!ctx_) throw std::runtime_error("no step has run");
  std::vector<uint32_t> s(cfg_.samples);
  hip::check(kc_mppi_costs(ctx_.get(), s.data(), s.size()));
  return s;
}

}  // namespace Control
}  // namespace Kompass
