// Control value types of the kompass_cpp surface (reference:
// datatypes/control.h:12, 112-140, 190-247).
#pragma once

#include <cmath>
#include <string>
#include <vector>

#include "kc_linalg.h"

namespace Kompass {
namespace Control {

enum class ControlType { ACKERMANN = 0, DIFFERENTIAL_DRIVE = 1, OMNI = 2 };

class Velocity2D {
 public:
  Velocity2D() = default;
  Velocity2D(double vx, double vy, double omega, double steer_ang = 0.0)
      : v_{vx, vy, omega, steer_ang} {}
  double vx() const { return v_[0]; }
  double vy() const { return v_[1]; }
  double omega() const { return v_[2]; }
  double steer_ang() const { return v_[3]; }
  void setVx(double x) { v_[0] = x; }
  void setVy(double x) { v_[1] = x; }
  void setOmega(double x) { v_[2] = x; }
  void setSteerAng(double x) { v_[3] = x; }
  Velocity2D operator-() const { return Velocity2D(-v_[0], -v_[1], -v_[2]); }

 private:
  double v_[4] = {0.0, 0.0, 0.0, 0.0};
};

// A tracked target's planar pose and velocity (reference: datatypes/control.h:14-188, Pose3D + TrackedPose2D).
// As in the reference the yaw is kept as a float quaternion about z and read back as atan2(R10, R00) of its
// rotation matrix; position in float, velocity in double.
class TrackedPose2D {
 public:
  TrackedPose2D(const float pose_x, const float pose_y, const float pose_yaw, const Velocity2D &vel)
      : vel_(vel) {
    updatePose(pose_x, pose_y, pose_yaw);
  }
  TrackedPose2D(const float pose_x, const float pose_y, const float pose_yaw, const float vx, const float vy,
                const float omega)
      : vel_(vx, vy, omega) {
    updatePose(pose_x, pose_y, pose_yaw);
  }

  float x() const { return position_[0]; }
  float y() const { return position_[1]; }
  float z() const { return position_[2]; }
  float yaw() const {
    // Eigen's toRotationMatrix of (w, 0, 0, qz): R00 = 1 - 2 qz qz, R10 = 2 qz w
    const float tz = 2.0f * qz_;
    return std::atan2(tz * qw_, 1.0f - tz * qz_);
  }
  float v() const {
    const float vx = static_cast<float>(vel_.vx()), vy = static_cast<float>(vel_.vy());
    return std::sqrt(vx * vx + vy * vy);
  }
  float omega() const { return static_cast<float>(vel_.omega()); }
  const Velocity2D &velocity() const { return vel_; }

  void updatePose(const float pose_x, const float pose_y, const float pose_yaw) {
    position_[0] = pose_x;
    position_[1] = pose_y;
    position_[2] = 0.0f;
    setYaw(pose_yaw);
  }

  // constant-velocity step in the target's own frame
  void update(const float timeStep) {
    const double c = std::cos(static_cast<double>(yaw())), s = std::sin(static_cast<double>(yaw()));
    position_[0] += static_cast<float>((vel_.vx() * c - vel_.vy() * s) * timeStep);
    position_[1] += static_cast<float>((vel_.vx() * s + vel_.vy() * c) * timeStep);
    setYaw(static_cast<float>(yaw() + vel_.omega() * timeStep));
  }
  void update(const Velocity2D &vel, const float timeStep) {
    vel_ = vel;
    update(timeStep);
  }

  float distance(const float x, const float y, const float z = 0.0f) const {
    const double dx = position_[0] - x, dy = position_[1] - y, dz = position_[2] - z;
    return static_cast<float>(std::sqrt(dx * dx + dy * dy + dz * dz));
  }

 private:
  void setYaw(const float yaw) {  // AngleAxisf(yaw, UnitZ) with zero pitch and roll
    const float half = 0.5f * yaw;
    qw_ = std::cos(half);
    qz_ = std::sin(half);
  }
  float position_[3] = {0.0f, 0.0f, 0.0f};
  float qw_ = 1.0f, qz_ = 0.0f;
  Velocity2D vel_;
};

struct LinearVelocityControlParams {
  double maxVel, maxAcceleration, maxDeceleration;
  LinearVelocityControlParams(double maxVel = 1.0, double maxAcc = 10.0,
                              double maxDec = 10.0)
      : maxVel(maxVel), maxAcceleration(maxAcc), maxDeceleration(maxDec) {}
};

struct AngularVelocityControlParams {
  double maxAngle, maxOmega, maxAcceleration, maxDeceleration;
  AngularVelocityControlParams(double maxAng = M_PI, double maxOmg = 1.0,
                               double maxAcc = 10.0, double maxDec = 10.0)
      : maxAngle(maxAng), maxOmega(maxOmg), maxAcceleration(maxAcc),
        maxDeceleration(maxDec) {}
};

struct ControlLimitsParams {
  LinearVelocityControlParams velXParams, velYParams;
  AngularVelocityControlParams omegaParams;
  ControlLimitsParams() = default;
  ControlLimitsParams(const LinearVelocityControlParams &x,
                      const LinearVelocityControlParams &y,
                      const AngularVelocityControlParams &w)
      : velXParams(x), velYParams(y), omegaParams(w) {}
};

struct LaserScan {
  std::vector<double> ranges, angles;
  LaserScan(std::vector<double> ranges, std::vector<double> angles)
      : ranges(std::move(ranges)), angles(std::move(angles)) {}
};

// A point cloud the caller already holds as packed (x, y, z) floats -- a numpy (N, 3) float32 array from
// the Python layer: consumed where it lies (the sensor update stores it straight to the device), no
// std::vector<Path::Point> in between.  Same meaning as the vector form (global_frame = true).
struct PointCloudView {
  const float *xyz;
  size_t n;
};

}  // namespace Control
}  // namespace Kompass
