// RGB-D target follower of the kompass_cpp surface (reference:
// controllers/rgbd_follower.{h,cpp}).  2-D detections on an aligned depth
// frame become 3-D boxes through the DepthDetector (one kc_depth_boxes call
// per frame with detections); everything after that -- the
// tracker, its Kalman filter, the pursuit law over the prediction horizon and
// the wait -> search -> give-up pipeline -- is serial host logic over a
// handful of boxes.  Constructing the follower and the whole Bbox3D path touch
// no device; the detector is made by setCameraIntrinsics and opens the device
// on its first frame.
#pragma once

#include <cmath>
#include <cstddef>
#include <memory>
#include <optional>
#include <stdexcept>
#include <vector>

#include "controllers/follower.h"
#include "controllers/rgb_follower.h"
#include "datatypes/control.h"
#include "datatypes/parameter.h"
#include "datatypes/tracking.h"
#include "datatypes/trajectory.h"
#include "utils/collision_check.h"
#include "vision/depth_detector.h"
#include "vision/tracker.h"

namespace Kompass {
namespace Control {

class RGBDFollower : public Follower, public RGBFollower {
 public:
  class RGBDFollowerConfig : public RGBFollower::RGBFollowerConfig {
   public:
    RGBDFollowerConfig() : RGBFollower::RGBFollowerConfig() {
      addParameter("control_horizon", Parameter(2, 1, 1000, "Number of steps for applying the control"));
      addParameter("prediction_horizon", Parameter(10, 1, 1000, "Number of steps for future prediction"));
      addParameter("distance_tolerance", Parameter(0.1, 1e-6, 1e3, "Distance tolerance value (m)"));
      addParameter("angle_tolerance", Parameter(0.1, 1e-6, M_PI, "Angle tolerance value (rad)"));
      addParameter("target_orientation",
                   Parameter(0.0, -M_PI, M_PI, "Bearing angle to maintain with the target (rad)"));
      addParameter("use_local_coordinates", Parameter(true, "Track the item in the local frame of the robot"));
      addParameter("error_pose", Parameter(0.05, 1e-9, 1e9));
      addParameter("error_vel", Parameter(0.05, 1e-9, 1e9));
      addParameter("error_acc", Parameter(0.05, 1e-9, 1e9));
      addParameter("depth_conversion_factor",
                   Parameter(1e-3, 1e-9, 1e9, "Factor to convert depth image values to meters"));
      addParameter("min_depth", Parameter(0.0, 0.0, 1e3, "Range of interest minimum depth value"));
      addParameter("max_depth", Parameter(1e3, 1e-3, 1e9, "Range of interest maximum depth value"));
    }
    int control_horizon() const { return getParameter<int>("control_horizon"); }
    bool enable_vel_tracking() const { return !getParameter<bool>("use_local_coordinates"); }
    int prediction_horizon() const { return getParameter<int>("prediction_horizon"); }
    double dist_tolerance() const { return getParameter<double>("distance_tolerance"); }
    double ang_tolerance() const { return getParameter<double>("angle_tolerance"); }
    double target_orientation() const { return getParameter<double>("target_orientation"); }
    double e_pose() const { return getParameter<double>("error_pose"); }
    double e_vel() const { return getParameter<double>("error_vel"); }
    double e_acc() const { return getParameter<double>("error_acc"); }
    double depth_conversion_factor() const { return getParameter<double>("depth_conversion_factor"); }
    Eigen::Vector2f depth_range() const {
      return Eigen::Vector2f(getParameter<double>("min_depth"), getParameter<double>("max_depth"));
    }
  };

  RGBDFollower(const ControlType &robotCtrlType, const ControlLimitsParams &ctrlLimits,
               const CollisionChecker::ShapeType &robotShapeType, const std::vector<float> &robotDimensions,
               const Eigen::Vector3f &vision_sensor_position_body, const Eigen::Vector4f &vision_sensor_rotation_body,
               const RGBDFollowerConfig &config = RGBDFollowerConfig());
  ~RGBDFollower() override = default;

  void setCameraIntrinsics(const float focal_length_x, const float focal_length_y, const float principal_point_x,
                           const float principal_point_y);

  static double getRobotRadius(const CollisionChecker::ShapeType robot_shape_type,
                               const std::vector<float> &robot_dimensions);

  // one step from 3-D detections (no device)
  TrajSearchResult getTrackingCtrl(const std::vector<Bbox3D> &detected_boxes, const Velocity2D &current_vel);

  // one step from 2-D detections on an aligned depth frame: one kc_depth_boxes call when there are detections,
  // none otherwise; only the boxes with the tracked label go to the device
  TrajSearchResult getTrackingCtrl(const DepthImageView &aligned_depth_img, const std::vector<Bbox2D> &detected_boxes_2d,
                                   const Velocity2D &current_vel);
  TrajSearchResult getTrackingCtrl(const Eigen::MatrixX<unsigned short> &aligned_depth_img,
                                   const std::vector<Bbox2D> &detected_boxes_2d, const Velocity2D &current_vel);

  bool setInitialTracking(const int pose_x_img, const int pose_y_img, const std::vector<Bbox3D> &detected_boxes,
                          const float yaw = 0.0);
  bool setInitialTracking(const int pose_x_img, const int pose_y_img, const DepthImageView &aligned_depth_image,
                          const std::vector<Bbox2D> &detected_boxes_2d, const float yaw = 0.0);
  bool setInitialTracking(const DepthImageView &aligned_depth_image, const Bbox2D &target_box_2d,
                          const float yaw = 0.0);
  bool setInitialTracking(const int pose_x_img, const int pose_y_img,
                          const Eigen::MatrixX<unsigned short> &aligned_depth_image,
                          const std::vector<Bbox2D> &detected_boxes_2d, const float yaw = 0.0);
  bool setInitialTracking(const Eigen::MatrixX<unsigned short> &aligned_depth_image, const Bbox2D &target_box_2d,
                          const float yaw = 0.0);

  Eigen::Vector2f getErrors() const { return Eigen::Vector2f(dist_error_, orientation_error_); }

  // (not in the reference's interface: what the tests and tools read)
  std::optional<Eigen::MatrixXf> getTrackedState() const { return tracker_->getTrackedState(); }
  std::optional<TrackedBbox3D> getRawTracking() const { return tracker_->getRawTracking(); }
  float targetRadius() const { return currentTargetRadius_; }
  double robotRadius() const { return robot_radius_; }
  double goalDistTolerance() const { return knob_.goal_radius; }
  // detector calls so far and the frame bytes the last one uploaded (0 / 0 before setCameraIntrinsics)
  size_t depthCalls() const { return detector_ ? detector_->calls() : 0; }
  size_t depthLastUpload() const { return detector_ ? detector_->lastUpload() : 0; }
  // order the next frame read after a producer's stream (frames already on the device)
  void depthAfterStream(void *stream) {
    requireDetector();
    detector_->afterStream(stream);
  }

 private:
  RGBDFollowerConfig config_;
  std::unique_ptr<FeatureBasedBboxTracker> tracker_;
  std::unique_ptr<DepthDetector> detector_;
  Eigen::Vector3f sensor_position_;
  Eigen::Vector4f sensor_rotation_;  // (x, y, z, w)
  bool track_velocity_;
  double robot_radius_;
  float currentTargetRadius_ = 0.0f;
  // (the reference's latest_velocity_command_ is the Follower's command_: get_vx_cmd & co. read it)

  void requireTracker() const;
  void requireDetector() const;
  // the 3-D boxes of the tracked label among `boxes` (one detector call)
  std::optional<std::vector<Bbox3D>> detect(const DepthImageView &img, const std::vector<Bbox2D> &boxes);
  std::optional<TrackedPose2D> updateFromBoxes(const std::vector<Bbox3D> &boxes);

  void refreshTargetGeometry();
  TrajSearchResult makeHoldResult() const;
  TrajSearchResult popSearchStepResult();
  std::optional<TrajSearchResult> trySearch();
  std::optional<TrajSearchResult> tryWait();
  TrajSearchResult giveUp();
  Trajectory2D getTrackingReferenceSegment(const TrackedPose2D &tracking_pose);
  TrackedPose2D updateLocalTarget(const TrackedPose2D &current_target, const Velocity2D &robot_cmd, double dt);
  Velocity2D getPureTrackingCtrl(const TrackedPose2D &tracking_pose, const bool update_global_error = false);
  TrajSearchResult dispatch(const std::optional<TrackedPose2D> &tracked_pose, const Velocity2D &current_vel);
};

// an Eigen (column-major) depth matrix as a frame view
DepthImageView depthImageView(const Eigen::MatrixX<unsigned short> &img);

}  // namespace Control
}  // namespace Kompass
