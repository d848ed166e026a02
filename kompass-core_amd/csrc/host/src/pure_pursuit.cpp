// PurePursuit host logic (reference: src/controllers/pure_pursuit.cpp).  The
// tracking law is serial per-cycle bookkeeping; the avoidance search is one
// kc_dwa_first_clear_command call over the reference's whole candidate list.
#include "controllers/pure_pursuit.h"

#include <cmath>

#include "utils/angles.h"
#include "utils/logger.h"

namespace Kompass {
namespace Control {

PurePursuit::PurePursuit(const ControlType &robotCtrlType, const ControlLimitsParams &ctrlLimits,
                         const CollisionChecker::ShapeType robotShapeType, const std::vector<float> robotDimensions,
                         const Eigen::Vector3f &sensor_position_body, const Eigen::Vector4f &sensor_rotation_body,
                         const double octreeRes, const PurePursuitConfig &cfg)
    : Follower() {
  setParams(cfg);
  setControlType(robotCtrlType);
  limits_ = ctrlLimits;
  collision_checker_ = std::make_unique<CollisionChecker>(robotShapeType, robotDimensions, sensor_position_body,
                                                          Eigen::Quaternionf(sensor_rotation_body), octreeRes);
  wheel_base = cfg.getParameter<double>("wheel_base");
  lookahead_gain_forward = cfg.getParameter<double>("lookahead_gain_forward");
  prediction_horizon = cfg.getParameter<int>("prediction_horizon");
  // :31-39: the candidate count is rounded up to even; offsets +-step * (i + 1) for even i
  const double path_search_step = cfg.getParameter<double>("path_search_step");
  int max_search_candidates = cfg.getParameter<int>("max_search_candidates");
  if (max_search_candidates % 2 != 0) max_search_candidates += 1;
  search_offsets_.resize(static_cast<size_t>(max_search_candidates));
  for (int i = 0; i < max_search_candidates; i = i + 2) {
    search_offsets_[static_cast<size_t>(i)] = static_cast<float>(path_search_step * (i + 1));
    search_offsets_[static_cast<size_t>(i) + 1] = static_cast<float>(-path_search_step * (i + 1));
  }
}

Controller::Result PurePursuit::execute(const double deltaTime) {
  if (!on_.ready)
    return {(on_.at_goal ? Result::Status::GOAL_REACHED : Result::Status::NO_COMMAND_POSSIBLE), {0.0, 0.0, 0.0}};
  // lookahead L = max(lookahead_distance, gain * |v|)
  const double current_v_mag = std::hypot(velocity_.vx(), velocity_.vy());
  const double lookahead_val = std::max(current_v_mag * lookahead_gain_forward, knob_.lookahead);
  const Path::Point target_point = findLookaheadPoint(lookahead_val);
  const double dx = target_point.x() - pose_.x;
  const double dy = target_point.y() - pose_.y;
  const double alpha_world = std::atan2(dy, dx);
  const double alpha_robot = Angle::normalizeToMinusPiPlusPi(alpha_world - pose_.yaw);
  const double dist_to_target = std::hypot(dx, dy);
  // the speed factor reads the nearest-point index as it stands: PurePursuit never moves it
  double cmd_v = limits_.velXParams.maxVel;
  cmd_v *= calculateExponentialSpeedFactor(velocity_.omega());
  Velocity2D cmd;
  if (drive_ == ControlType::OMNI && !(std::abs(alpha_robot) > (M_PI * 0.9))) {
    cmd = Velocity2D(cmd_v * std::cos(alpha_robot), cmd_v * std::sin(alpha_robot), 2.0 * alpha_robot);
  } else {
    // diff drive and Ackermann (wheel_base unused), and an omni robot facing away from the target (:234-266)
    const double safe_dist = std::max(dist_to_target, 0.001);
    const double curvature = 2.0 * std::sin(alpha_robot) / safe_dist;
    cmd = Velocity2D(cmd_v, 0.0, cmd_v * curvature);
  }
  const double v_safe =
      restrictVelocityTolimits(velocity_.vx(), cmd.vx(), limits_.velXParams.maxAcceleration,
                               limits_.velXParams.maxDeceleration, limits_.velXParams.maxVel, deltaTime);
  // keep the curvature when the speed was limited
  if (std::abs(cmd.vx()) > 1e-4) cmd.setOmega(cmd.omega() * (v_safe / cmd.vx()));
  cmd.setVx(v_safe);
  command_ = cmd;
  // :130-139: the goal test follows the command; reaching the goal is sticky
  const Path::Point path_end = on_.path->getEnd();
  const double dist_to_end = std::hypot(path_end.x() - pose_.x, path_end.y() - pose_.y);
  if (dist_to_end < knob_.goal_radius) {
    on_.at_goal = true;
    return {Result::Status::GOAL_REACHED, Velocity2D()};
  }
  return {Result::Status::COMMAND_FOUND, cmd};
}

Controller::Result PurePursuit::execute(const Path::State currentPosition, const double deltaTime) {
  setCurrentState(currentPosition);
  return execute(deltaTime);
}

std::vector<Velocity2D> PurePursuit::searchCandidates(const Velocity2D &nominal) const {
  const bool omni = drive_ == ControlType::OMNI;
  std::vector<Velocity2D> out;
  out.reserve(1 + 2 * search_offsets_.size() * (omni ? 2 : 1));
  out.push_back(nominal);
  // :163-212: forward pass from the nominal command, then the reverse pass from the nominal command with vx
  // negated.  In the omni branch `candidate` keeps the vy shift of the previous offset when the next omega
  // offset is tried.
  for (int pass = 0; pass < 2; ++pass) {
    Velocity2D candidate = nominal;
    if (pass == 1) candidate.setVx(-nominal.vx());
    for (const float off_f : search_offsets_) {
      const double off = off_f;
      candidate.setOmega(nominal.omega() + off);
      out.push_back(candidate);
      if (omni) {
        candidate.setOmega(nominal.omega());
        candidate.setVy(nominal.vy() + off);
        out.push_back(candidate);
      }
    }
  }
  return out;
}

Velocity2D PurePursuit::findSafeCommand(const Velocity2D &nominal, double dt) {
  const std::vector<Velocity2D> cands = searchCandidates(nominal);
  const size_t n = cands.size();
  std::vector<double> vx(n), vy(n), om(n);
  for (size_t i = 0; i < n; ++i) {
    vx[i] = cands[i].vx();
    vy[i] = cands[i].vy();
    om[i] = cands[i].omega();
  }
  const kc_state st{pose_.x, pose_.y, pose_.yaw, pose_.speed};
  int64_t first = -1;
  hip::check(kc_dwa_first_clear_command(collision_checker_->context().get(), &st, vx.data(), vy.data(), om.data(), n,
                                        prediction_horizon, dt, &first));
  if (first > 0) LOG_DEBUG("PurePursuit: obstacle on the nominal path, candidate ", first, " is clear");
  // every candidate collides: stop and wait for the obstacle (:211)
  return first < 0 ? Velocity2D(0.0, 0.0, 0.0) : cands[static_cast<size_t>(first)];
}

Path::Point PurePursuit::findLookaheadPoint(double radius) {
  // :214-272: the LAST segment from last_found_index_ on that the circle cuts (t2 preferred over t1); none: the
  // path end when it lies inside the circle, else the same search with a radius 1.1 times larger
  Path::Point target = on_.path->getEnd();
  bool intersection_found = false;
  for (size_t i = last_found_index_; i < on_.path->getSize() - 1; ++i) {
    const Path::Point p1 = on_.path->getIndex(i);
    const Path::Point p2 = on_.path->getIndex(i + 1);
    const double d_x = p2.x() - p1.x();
    const double d_y = p2.y() - p1.y();
    const double f_x = p1.x() - pose_.x;
    const double f_y = p1.y() - pose_.y;
    const double a = d_x * d_x + d_y * d_y;
    const double b = 2.0 * (f_x * d_x + f_y * d_y);
    const double c = (f_x * f_x + f_y * f_y) - (radius * radius);
    double discriminant = b * b - 4.0 * a * c;
    if (discriminant >= 0.0) {
      discriminant = std::sqrt(discriminant);
      const double t1 = (-b - discriminant) / (2.0 * a);
      const double t2 = (-b + discriminant) / (2.0 * a);
      if (t2 >= 0.0 && t2 <= 1.0) {
        target = Path::Point(p1.x() + t2 * d_x, p1.y() + t2 * d_y, 0.0);
        last_found_index_ = i;
        intersection_found = true;
      } else if (t1 >= 0.0 && t1 <= 1.0) {
        target = Path::Point(p1.x() + t1 * d_x, p1.y() + t1 * d_y, 0.0);
        last_found_index_ = i;
        intersection_found = true;
      }
    }
  }
  if (!intersection_found) {
    const double dist_to_end = std::hypot(on_.path->getEnd().x() - pose_.x, on_.path->getEnd().y() - pose_.y);
    if (dist_to_end < radius) {
      last_found_index_ = on_.path->getSize() - 1;
      return on_.path->getEnd();
    }
    return findLookaheadPoint(1.1 * radius);
  }
  on_.target->movement = Path::State(target.x(), target.y(), 0.0);
  return target;
}

}  // namespace Control
}  // namespace Kompass
