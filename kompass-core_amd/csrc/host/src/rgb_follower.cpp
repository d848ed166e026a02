// RGBFollower (reference: controllers/rgb_follower.cpp), expression by expression: the float / double mix of the
// reference is kept where it decides a value (search-command loop, rotation speed).
#include "controllers/rgb_follower.h"

#include <algorithm>
#include <cmath>

#include "utils/logger.h"

namespace Kompass {
namespace Control {

RGBFollower::RGBFollower(const ControlType robotCtrlType, const ControlLimitsParams robotCtrlLimits,
                         const RGBFollowerConfig config) {
  ctrl_limits_ = robotCtrlLimits;
  config_ = config;
  rotate_in_place_ = (robotCtrlType == ControlType::DIFFERENTIAL_DRIVE || robotCtrlType == ControlType::OMNI);
}

void RGBFollower::resetTarget(const Bbox2D &target) {
  std::queue<SearchCommand> empty;
  std::swap(search_commands_queue_, empty);
  const float size = static_cast<float>(target.size.x() * target.size.y()) /
                     static_cast<float>(target.img_size.x() * target.img_size.y());
  LOG_DEBUG("Setting vision target reference distance to size: ", size);
  config_.set_target_distance(size);
}

void RGBFollower::generateSearchCommands(float total_rotation, float search_radius, float max_rotation_time,
                                         bool enable_pause) {
  const double rotation_sign = (total_rotation < 0.0) ? -1.0 : 1.0;
  float rotation_time = max_rotation_time;
  const int num_pause_steps = static_cast<int>(config_.search_pause() / config_.control_time_step());
  if (enable_pause) {
    // NOTE (reference): steps divided by the time step, kept as written
    rotation_time = max_rotation_time * (1 - num_pause_steps / config_.control_time_step());
  }
  double omega_val = total_rotation / rotation_time;  // a float quotient
  omega_val = std::max(std::min(omega_val, ctrl_limits_.omegaParams.maxOmega), config_.min_vel());
  // NOTE (reference): a float clock advanced by the double time step
  for (float t = 0.0f; t <= max_rotation_time; t = t + config_.control_time_step()) {
    if (rotate_in_place_) {
      search_commands_queue_.push(SearchCommand{0.0, 0.0, rotation_sign * omega_val});
    } else {
      const double omega_ackermann = rotation_sign * ctrl_limits_.velXParams.maxVel / search_radius;
      search_commands_queue_.push(SearchCommand{ctrl_limits_.velXParams.maxVel, 0.0, omega_ackermann});
    }
    if (enable_pause)
      for (int j = 0; j <= num_pause_steps; j++) search_commands_queue_.push(SearchCommand{0.0, 0.0, 0.0});
  }
}

void RGBFollower::getFindTargetCmds(const int last_direction) {
  LOG_DEBUG("Generating new search commands in direction: ", last_direction);
  search_commands_queue_ = std::queue<SearchCommand>();
  const float part = config_.target_search_timeout() / 4;
  generateSearchCommands(last_direction * M_PI, config_.target_search_radius(), part);               // rotate pi
  generateSearchCommands(-2.0 * last_direction * M_PI, config_.target_search_radius(), 2.0 * part);  // go back
  generateSearchCommands(last_direction * M_PI, config_.target_search_radius(), part);               // again
}

bool RGBFollower::run(const std::optional<Bbox2D> target) {
  if (target.has_value()) {
    recorded_wait_time_ = 0.0;
    recorded_search_time_ = 0.0;
    last_tracking_ = std::make_unique<Bbox2D>(target.value());
    trackTarget(target.value());
    return true;
  }
  if (config_.enable_search()) {
    if (recorded_search_time_ < config_.target_search_timeout()) {
      if (search_commands_queue_.empty()) {
        int last_direction = 1;
        if (last_tracking_ != nullptr) {
          const auto c = last_tracking_->getCenter();
          last_direction = ((c.x() - c.y() / 2.0) > 0.0) ? 1 : -1;  // (reference expression)
          last_tracking_ = nullptr;
        }
        getFindTargetCmds(last_direction);
      }
      search_command_ = search_commands_queue_.front();
      search_commands_queue_.pop();
      recorded_search_time_ += config_.control_time_step();
      return true;
    }
    recorded_search_time_ = 0.0;
    return false;
  }
  if (recorded_wait_time_ < config_.target_wait_timeout()) {
    LOG_DEBUG("Target lost, waiting to get tracked target again ...");
    last_tracking_ = nullptr;
    recorded_wait_time_ += config_.control_time_step();
    return true;
  }
  recorded_wait_time_ = 0.0;
  return false;
}

void RGBFollower::trackTarget(const Bbox2D &target) {
  const float current_dist = static_cast<float>(target.size.x() * target.size.y()) /
                             static_cast<float>(target.img_size.x() * target.img_size.y());
  dist_error_ = config_.target_distance() - current_dist;
  const float distance_tolerance = config_.tolerance() * config_.target_distance();
  const float error_y =
      2.0f * (static_cast<float>(target.getCenter().y()) / static_cast<float>(target.img_size.y()) - 0.5f);
  const float error_x =
      2.0f * (static_cast<float>(target.getCenter().x()) / static_cast<float>(target.img_size.x()) - 0.5f);
  orientation_error_ = error_x;
  if (std::abs(dist_error_) < distance_tolerance && std::abs(error_y) < config_.tolerance() &&
      std::abs(error_x) < config_.tolerance()) {
    out_vel_ = TrajectoryVelocities2D(2);
    out_vel_.add(0, 0.0f, 0.0f, 0.0f);
    return;
  }
  const float dist_speed = std::abs(dist_error_) > distance_tolerance
                               ? (dist_error_ / config_.target_distance()) * ctrl_limits_.velXParams.maxVel
                               : 0.0;
  float omega = -config_.K_omega() * error_x * ctrl_limits_.omegaParams.maxOmega;
  float v = config_.K_v() * dist_speed;
  omega = std::abs(omega) >= config_.min_vel() ? omega : 0.0f;
  const float omega_limit = static_cast<float>(ctrl_limits_.omegaParams.maxOmega);
  omega = std::clamp(omega, -omega_limit, omega_limit);
  const float v_limit = static_cast<float>(ctrl_limits_.velXParams.maxVel);
  v = std::abs(v) >= config_.min_vel() ? v : 0.0f;
  v = std::clamp(v, -v_limit, v_limit);
  out_vel_ = TrajectoryVelocities2D(2);
  out_vel_.add(0, v, 0.0f, omega);
}

const TrajectoryVelocities2D RGBFollower::getCtrl() const {
  if (recorded_search_time_ <= 0.0 && recorded_wait_time_ <= 0.0) return out_vel_;
  TrajectoryVelocities2D out(2);
  if (recorded_search_time_ > 0.0)
    out.add(0, static_cast<float>(search_command_[0]), static_cast<float>(search_command_[1]),
            static_cast<float>(search_command_[2]));
  else
    out.add(0, 0.0f, 0.0f, 0.0f);  // waiting
  return out;
}

std::vector<RGBFollower::SearchCommand> RGBFollower::pendingSearchCommands() const {
  std::queue<SearchCommand> q = search_commands_queue_;
  std::vector<SearchCommand> out;
  for (; !q.empty(); q.pop()) out.push_back(q.front());
  return out;
}

}  // namespace Control
}  // namespace Kompass
