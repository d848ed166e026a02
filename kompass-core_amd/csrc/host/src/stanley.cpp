// Stanley host logic (reference: src/controllers/stanley.cpp).
#include "controllers/stanley.h"

#include <algorithm>
#include <cmath>

#include "utils/angles.h"

namespace Kompass {
namespace Control {

Stanley::Stanley() : Follower() {
  cross_track_gain = stanley_config_.getParameter<double>("cross_track_gain");
  heading_gain = stanley_config_.getParameter<double>("heading_gain");
  min_velocity = stanley_config_.getParameter<double>("cross_track_min_linear_vel");
  wheel_base = stanley_config_.getParameter<double>("wheel_base");
}

Stanley::Stanley(const StanleyParameters &config) : Stanley() { setParams(config); }

Controller::Result Stanley::execute(Path::State currentPosition, double deltaTime) {
  setCurrentState(currentPosition);
  return computeVelocityCommand(deltaTime);
}

Controller::Result Stanley::computeVelocityCommand(double timeStep) {
  if (!on_.ready)
    return {(on_.at_goal ? Result::Status::GOAL_REACHED : Result::Status::NO_COMMAND_POSSIBLE), {0.0, 0.0, 0.0}};
  aimAtTarget();
  const Target target = *on_.target;
  const double target_speed = target.reverse ? -limits_.velXParams.maxVel : limits_.velXParams.maxVel;
  // the Stanley law: cross-track term at a speed of at least min_velocity, plus the heading term
  const double control_steering_angle =
      -cross_track_gain * std::atan2(target.crosstrack_error, std::max(std::abs(target_speed), min_velocity)) +
      heading_gain * Angle::normalizeToMinusPiPlusPi(target.heading_error);
  on_.segment = target.segment_index;
  on_.along = target.position_in_segment;
  command_ = computeCommand(command_, target_speed, control_steering_angle, timeStep);
  return {Result::Status::COMMAND_FOUND, command_};
}

void Stanley::setWheelBase(double length) { robotWheelBase = length; }

Velocity2D Stanley::computeCommand(Velocity2D current_velocity, double linear_velocity, double steering_angle,
                                   double time_step) const {
  // the linear command goes through a float, as in the reference
  const float linearCtrl = static_cast<float>(restrictVelocityTolimits(
      current_velocity.vx(), linear_velocity, limits_.velXParams.maxAcceleration,
      limits_.velXParams.maxDeceleration, limits_.velXParams.maxVel, time_step));
  Velocity2D velocity_command{linearCtrl, 0.0, 0.0, 0.0};
  const double max_steering_angle = limits_.omegaParams.maxAngle;
  velocity_command.setSteerAng(std::min(std::max(steering_angle, -max_steering_angle), max_steering_angle));
  const double omega = std::tan(velocity_command.steer_ang()) * std::abs(linearCtrl) / robotWheelBase;
  velocity_command.setOmega(restrictVelocityTolimits(current_velocity.omega(), omega,
                                                     limits_.omegaParams.maxAcceleration,
                                                     limits_.omegaParams.maxDeceleration,
                                                     limits_.omegaParams.maxOmega, time_step));
  return velocity_command;
}

}  // namespace Control
}  // namespace Kompass
