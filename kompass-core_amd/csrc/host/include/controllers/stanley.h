// Stanley path follower (reference: controllers/stanley.{h,cpp}).  Serial per-cycle host logic on top of the
// Follower's closest-point tracking; nothing here is batch work.  The DVZ controller of kompass_core uses it to
// generate its reference commands.
#pragma once

#include "controllers/follower.h"

namespace Kompass {
namespace Control {

class Stanley : public Follower {
 public:
  class StanleyParameters : public Follower::FollowerParameters {
   public:
    StanleyParameters() : Follower::FollowerParameters() {
      addParameter("wheel_base", Parameter(0.3, 0.0001, 100.0));                 // [m]
      addParameter("heading_gain", Parameter(1.0, 0.0, 10.0));                   // heading error gain
      addParameter("cross_track_min_linear_vel", Parameter(0.05, 0.0, 10.0));    // [m/s] floor of the speed
      addParameter("cross_track_gain", Parameter(10.0, 0.0, 50.0));              // cross-track error gain
    }
  };

  Stanley();
  // NOTE (reference quirk, stanley.cpp:19-21): `config` reaches the Follower's parameters only; the four Stanley
  // gains keep the defaults the default constructor read.
  Stanley(const StanleyParameters &config);
  ~Stanley() = default;

  Controller::Result computeVelocityCommand(double timeStep);
  Controller::Result execute(Path::State currentPosition, double deltaTime);
  // the wheel base of the omega = tan(steer) |v| / L step (1.0 until set; `wheel_base` is read, not used)
  void setWheelBase(double length);

 protected:
  StanleyParameters stanley_config_;
  double robotWheelBase{1.0};
  double cross_track_gain{0.0};
  double heading_gain{0.0};
  double min_velocity{0.0};
  double wheel_base{0.0};

  // the target speed and steering angle within the limits (stanley.cpp:78-105)
  Velocity2D computeCommand(Velocity2D current_velocity, double linear_velocity, double steering_angle,
                            double time_step) const;
};

}  // namespace Control
}  // namespace Kompass
