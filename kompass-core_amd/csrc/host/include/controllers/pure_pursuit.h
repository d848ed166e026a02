// Pure Pursuit path follower with a collision-avoiding command search (reference:
// controllers/pure_pursuit.{h,cpp}).  The tracking law is serial per-cycle host
// logic; the avoidance search -- every candidate command rolled out and checked
// against the sensor data -- is ONE call into libkompass_hip.so
// (kc_dwa_first_clear_command) per cycle, whatever the nominal command meets.
#pragma once

#include <memory>
#include <vector>

#include "controllers/follower.h"
#include "utils/collision_check.h"

namespace Kompass {
namespace Control {

class PurePursuit : public Follower {
 public:
  class PurePursuitConfig : public Follower::FollowerParameters {
   public:
    PurePursuitConfig() : Follower::FollowerParameters() {
      addParameter("wheel_base", Parameter(0.34, 0.0, 100.0));
      addParameter("prediction_horizon", Parameter(10, 0, 100));
      addParameter("lookahead_gain_forward",
                   Parameter(0.8, 0.001, 10.0, "Factor to scale lookahead distance by velocity (k * v)"));
      addParameter("path_search_step",
                   Parameter(0.2, 0.001, 1000.0, "Offset step to search for a new path when doing obstacle avoidance"));
      addParameter("max_search_candidates",
                   Parameter(10, 2, 1000, "Number of search candidates to try for obstacle avoidance"));
    }
  };

  PurePursuit(const ControlType &robotCtrlType, const ControlLimitsParams &ctrlLimits,
              const CollisionChecker::ShapeType robotShapeType, const std::vector<float> robotDimensions,
              const Eigen::Vector3f &sensor_position_body, const Eigen::Vector4f &sensor_rotation_body,
              const double octreeRes = 0.1, const PurePursuitConfig &cfg = PurePursuitConfig());
  virtual ~PurePursuit() = default;

  Controller::Result execute(const Path::State currentPosition, const double deltaTime);
  Controller::Result execute(const double deltaTime);

  // LaserScan, std::vector<Path::Point> or PointCloudView (pure_pursuit.h:70-96)
  template <typename T>
  Controller::Result execute(const double deltaTime, const T &sensor_data) {
    collision_checker_->updateState(pose_);
    collision_checker_->updateSensorData(sensor_data);
    auto result = execute(deltaTime);
    if (result.status != Result::Status::COMMAND_FOUND) return result;
    // the nominal command is candidate 0: clear -> returned as it is; else the first clear alternative, or a stop
    // (:95, :211) -- still COMMAND_FOUND
    return {Result::Status::COMMAND_FOUND, findSafeCommand(result.velocity_command, deltaTime)};
  }
  template <typename T>
  Controller::Result execute(const Path::State currentPosition, const double deltaTime, const T &sensor_data) {
    setCurrentState(currentPosition);
    return execute<T>(deltaTime, sensor_data);
  }

  // the reference's candidate order (pure_pursuit.cpp:150-212) with the nominal command in front
  std::vector<Velocity2D> searchCandidates(const Velocity2D &nominal) const;
  const std::vector<float> &searchOffsets() const { return search_offsets_; }

 private:
  double wheel_base{0.0};  // read, unused (as in the reference)
  double lookahead_gain_forward{0.0};
  size_t last_found_index_ = 0;
  int prediction_horizon{0};
  std::vector<float> search_offsets_;  // Eigen::VectorXf in the reference: the offsets are float values
  std::unique_ptr<CollisionChecker> collision_checker_;

  Path::Point findLookaheadPoint(double radius);
  // checkCommandCollisions + findSafeCommand in one device call
  Velocity2D findSafeCommand(const Velocity2D &nominal, double dt);
};

}  // namespace Control
}  // namespace Kompass
