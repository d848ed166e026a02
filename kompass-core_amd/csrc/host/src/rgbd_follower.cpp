// RGBDFollower (reference: controllers/rgbd_follower.{h,cpp}).  Host logic; the only device work is the
// DepthDetector's one kc_depth_boxes call per frame with detections.
#include "controllers/rgbd_follower.h"

#include <algorithm>
#include <cmath>

#include "utils/angles.h"
#include "utils/logger.h"

namespace Kompass {
namespace Control {

DepthImageView depthImageView(const Eigen::MatrixX<unsigned short> &img) {
  DepthImageView v;  // column-major, as Eigen's MatrixX
  v.data = img.data();
  v.rows = img.rows();
  v.cols = img.cols();
  v.row_stride = 1;
  v.col_stride = img.rows();
  return v;
}

RGBDFollower::RGBDFollower(const ControlType &robotCtrlType, const ControlLimitsParams &ctrlLimits,
                           const CollisionChecker::ShapeType &robotShapeType, const std::vector<float> &robotDimensions,
                           const Eigen::Vector3f &vision_sensor_position_body,
                           const Eigen::Vector4f &vision_sensor_rotation_body, const RGBDFollowerConfig &config)
    : Follower(), RGBFollower(robotCtrlType, ctrlLimits) {
  ctrl_limits_ = ctrlLimits;
  config_ = config;
  track_velocity_ = config_.enable_vel_tracking();
  // goal_dist_tolerance = error_pose (the reference's DWA-fallback goal radius)
  knob_.goal_radius = config_.e_pose();
  tracker_ = std::make_unique<FeatureBasedBboxTracker>(static_cast<float>(config.control_time_step()),
                                                       static_cast<float>(config.e_pose()),
                                                       static_cast<float>(config.e_vel()),
                                                       static_cast<float>(config.e_acc()));
  sensor_position_ = vision_sensor_position_body;
  sensor_rotation_ = vision_sensor_rotation_body;
  robot_radius_ = getRobotRadius(robotShapeType, robotDimensions);
}

double RGBDFollower::getRobotRadius(const CollisionChecker::ShapeType robot_shape_type,
                                    const std::vector<float> &robot_dimensions) {
  switch (robot_shape_type) {
    case CollisionChecker::ShapeType::CYLINDER:
    case CollisionChecker::ShapeType::SPHERE:
      return robot_dimensions.at(0);
    case CollisionChecker::ShapeType::BOX: {
      // the circumradius, conservative for collisions
      const double a = robot_dimensions.at(0), b = robot_dimensions.at(1);
      return std::sqrt(std::pow(a, 2) + std::pow(b, 2)) / 2;
    }
  }
  throw std::invalid_argument("Invalid robot geometry type");
}

void RGBDFollower::setCameraIntrinsics(const float focal_length_x, const float focal_length_y,
                                       const float principal_point_x, const float principal_point_y) {
  const Eigen::Vector4f &q = sensor_rotation_;
  detector_ = std::make_unique<DepthDetector>(config_.depth_range(), sensor_position_,
                                              Eigen::Quaternionf(q(3), q(0), q(1), q(2)),
                                              Eigen::Vector2f{focal_length_x, focal_length_y},
                                              Eigen::Vector2f{principal_point_x, principal_point_y},
                                              static_cast<float>(config_.depth_conversion_factor()));
}

void RGBDFollower::requireTracker() const {
  if (!tracker_->trackerInitialized())
    throw std::runtime_error(
        "Tracker is not initialized with an initial tracking target. Call 'RGBDFollower::setInitialTracking' first");
}

void RGBDFollower::requireDetector() const {
  if (!detector_)
    throw std::runtime_error(
        "DepthDetector is not initialized with the camera intrinsics. Call 'RGBDFollower::setCameraIntrinsics' "
        "first");
}

std::optional<std::vector<Bbox3D>> RGBDFollower::detect(const DepthImageView &img, const std::vector<Bbox2D> &boxes) {
  if (track_velocity_)
    detector_->updateBoxes(img, boxes, pose_);  // the current state places the boxes in the world
  else
    detector_->updateBoxes(img, boxes);
  return detector_->get3dDetections();
}

std::optional<TrackedPose2D> RGBDFollower::updateFromBoxes(const std::vector<Bbox3D> &boxes) {
  if (!tracker_->updateTracking(boxes)) {
    LOG_WARNING("Tracker failed to update target with the detected boxes");
    return std::nullopt;
  }
  refreshTargetGeometry();
  return tracker_->getFilteredTrackedPose2D();
}

TrajSearchResult RGBDFollower::getTrackingCtrl(const std::vector<Bbox3D> &detected_boxes,
                                               const Velocity2D &current_vel) {
  std::optional<TrackedPose2D> tracked_pose;
  if (!detected_boxes.empty()) {
    requireTracker();
    tracked_pose = updateFromBoxes(detected_boxes);
  }
  return dispatch(tracked_pose, current_vel);
}

TrajSearchResult RGBDFollower::getTrackingCtrl(const DepthImageView &img, const std::vector<Bbox2D> &detected_boxes_2d,
                                               const Velocity2D &current_vel) {
  requireDetector();
  requireTracker();
  std::optional<TrackedPose2D> tracked_pose;
  if (!detected_boxes_2d.empty()) {
    // The tracker drops every other label before association, so only the tracked label is measured (the
    // reference measures them all and logs a different warning).
    std::vector<Bbox2D> same_label;
    for (const auto &b : detected_boxes_2d)
      if (b.label == tracker_->trackedLabel()) same_label.push_back(b);
    auto boxes_3d = detect(img, same_label);
    if (boxes_3d)
      tracked_pose = updateFromBoxes(boxes_3d.value());
    else
      LOG_WARNING("Detector failed to find 3D boxes");
  }
  return dispatch(tracked_pose, current_vel);
}

TrajSearchResult RGBDFollower::getTrackingCtrl(const Eigen::MatrixX<unsigned short> &img,
                                               const std::vector<Bbox2D> &detected_boxes_2d,
                                               const Velocity2D &current_vel) {
  return getTrackingCtrl(depthImageView(img), detected_boxes_2d, current_vel);
}

Velocity2D RGBDFollower::getPureTrackingCtrl(const TrackedPose2D &tracking_pose, const bool update_global_error) {
  float distance, psi, gamma = 0.0f;
  if (track_velocity_) {
    // world frame: bearing from the robot's body
    distance = tracking_pose.distance(pose_.x, pose_.y, 0.0) - robot_radius_ - currentTargetRadius_;
    psi = Angle::normalizeToMinusPiPlusPi(std::atan2(tracking_pose.y() - pose_.y, tracking_pose.x() - pose_.x) -
                                          pose_.yaw);
    gamma = Angle::normalizeToMinusPiPlusPi(tracking_pose.yaw() - pose_.yaw);
  } else {
    distance = tracking_pose.distance(0.0, 0.0, 0.0) - robot_radius_ - currentTargetRadius_;
    psi = Angle::normalizeToMinusPiPlusPi(std::atan2(tracking_pose.y(), tracking_pose.x()));
  }
  constexpr float kMinDistance = 0.001f;  // floor: the omega law divides by it
  distance = std::max(distance, kMinDistance);
  const float distance_error = config_.target_distance() - distance;
  const float angle_error = Angle::normalizeToMinusPiPlusPi(config_.target_orientation() - psi);
  if (update_global_error) {
    dist_error_ = distance_error;
    orientation_error_ = angle_error;
  }
  const float angle_diff = gamma - psi;
  const float sin_diff = std::sin(angle_diff);
  const float cos_diff = std::cos(angle_diff);
  const float tv = track_velocity_ ? 1.0f : 0.0f;
  Velocity2D followingVel;
  // NOTE: std::abs on the float errors (the reference's unqualified abs)
  if (std::abs(distance_error) > config_.dist_tolerance() || std::abs(angle_error) > config_.ang_tolerance()) {
    double v = tv * (tracking_pose.v() * cos_diff) -
               config_.K_v() * ctrl_limits_.velXParams.maxVel * std::tanh(distance_error);
    v = std::clamp(v, -ctrl_limits_.velXParams.maxVel, ctrl_limits_.velXParams.maxVel);
    if (std::abs(v) < config_.min_vel()) v = 0.0;
    followingVel.setVx(v);
    double omega = tv * tracking_pose.v() * sin_diff / distance + v * std::sin(psi) / distance -
                   config_.K_omega() * ctrl_limits_.omegaParams.maxOmega * std::tanh(angle_error);
    omega = std::clamp(omega, -ctrl_limits_.omegaParams.maxOmega, ctrl_limits_.omegaParams.maxOmega);
    if (std::abs(omega) < config_.min_vel()) omega = 0.0;
    followingVel.setOmega(omega);
  }
  return followingVel;
}

bool RGBDFollower::setInitialTracking(const int pose_x_img, const int pose_y_img,
                                      const std::vector<Bbox3D> &detected_boxes, const float yaw) {
  const bool ok = tracker_->setInitialTracking(pose_x_img, pose_y_img, detected_boxes, yaw);
  if (ok) refreshTargetGeometry();
  return ok;
}

bool RGBDFollower::setInitialTracking(const int pose_x_img, const int pose_y_img, const DepthImageView &img,
                                      const std::vector<Bbox2D> &detected_boxes, const float yaw) {
  for (const auto &box : detected_boxes) {  // the first box whose inclusive limits hold the pixel
    const auto lx = box.getXLimits();
    if (pose_x_img >= lx(0) && pose_x_img <= lx(1)) {
      const auto ly = box.getYLimits();
      if (pose_y_img >= ly(0) && pose_y_img <= ly(1)) return setInitialTracking(img, box, yaw);
    }
  }
  LOG_DEBUG("Target point not found in any detected box");
  return false;
}

bool RGBDFollower::setInitialTracking(const DepthImageView &img, const Bbox2D &target_box_2d, const float yaw) {
  requireDetector();
  auto boxes_3d = detect(img, {target_box_2d});
  if (!boxes_3d || boxes_3d->empty()) {
    LOG_DEBUG("Failed to get 3D box from 2D target box");
    return false;
  }
  const bool ok = tracker_->setInitialTracking(boxes_3d.value()[0], yaw);
  if (ok) refreshTargetGeometry();
  return ok;
}

bool RGBDFollower::setInitialTracking(const int pose_x_img, const int pose_y_img,
                                      const Eigen::MatrixX<unsigned short> &img,
                                      const std::vector<Bbox2D> &detected_boxes, const float yaw) {
  return setInitialTracking(pose_x_img, pose_y_img, depthImageView(img), detected_boxes, yaw);
}

bool RGBDFollower::setInitialTracking(const Eigen::MatrixX<unsigned short> &img, const Bbox2D &target_box_2d,
                                      const float yaw) {
  return setInitialTracking(depthImageView(img), target_box_2d, yaw);
}

void RGBDFollower::refreshTargetGeometry() {
  // a miss leaves the previous radius
  if (auto raw = tracker_->getRawTracking())
    currentTargetRadius_ = 0.5f * std::max(raw->box.size.x(), raw->box.size.y());
}

std::optional<TrajSearchResult> RGBDFollower::trySearch() {
  if (!config_.enable_search()) return std::nullopt;
  // a fresh wait if the target is lost again during the search
  recorded_wait_time_ = 0.0;
  if (search_commands_queue_.empty()) {
    const int last_direction = (command_.omega() < 0) ? -1 : 1;
    getFindTargetCmds(last_direction);
  }
  if (recorded_search_time_ >= config_.target_search_timeout()) {
    LOG_DEBUG("Search timeout reached. Giving up.");
    return std::nullopt;
  }
  return popSearchStepResult();
}

std::optional<TrajSearchResult> RGBDFollower::tryWait() {
  if (config_.enable_search()) {
    // hold for one control step before searching (a transient miss should not start a search)
    if (recorded_wait_time_ >= config_.control_time_step()) return std::nullopt;
    std::queue<SearchCommand> empty;
    std::swap(search_commands_queue_, empty);
    recorded_wait_time_ += (config_.control_horizon() - 1) * config_.control_time_step();
    return makeHoldResult();
  }
  if (recorded_wait_time_ >= config_.target_wait_timeout()) return std::nullopt;
  recorded_wait_time_ += (config_.control_horizon() - 1) * config_.control_time_step();
  return makeHoldResult();
}

TrajSearchResult RGBDFollower::giveUp() {
  LOG_WARNING("Target is lost and not recovered from search or wait");
  recorded_wait_time_ = 0.0;
  recorded_search_time_ = 0.0;
  search_commands_queue_ = std::queue<SearchCommand>();
  return TrajSearchResult();
}

TrajSearchResult RGBDFollower::makeHoldResult() const {
  const size_t h = static_cast<size_t>(config_.control_horizon());
  TrajectoryVelocities2D velocities(h);
  TrajectoryPath path(h);
  path.add(0, 0.0f, 0.0f);
  for (size_t i = 0; i + 1 < h; ++i) {
    velocities.add(i, Velocity2D(0.0, 0.0, 0.0));
    path.add(i + 1, 0.0f, 0.0f);
  }
  TrajSearchResult result;
  result.isTrajFound = true;
  result.trajCost = 0.0f;
  result.trajectory = Trajectory2D(velocities, path);
  return result;
}

TrajSearchResult RGBDFollower::popSearchStepResult() {
  const size_t h = static_cast<size_t>(config_.control_horizon());
  TrajectoryVelocities2D velocities(h);
  TrajectoryPath path(h);
  path.add(0, 0.0f, 0.0f);
  for (size_t i = 0; i + 1 < h; ++i) {
    if (search_commands_queue_.empty()) {
      LOG_DEBUG("Search commands queue is empty. Ending Search ");
      return TrajSearchResult();
    }
    const SearchCommand cmd = search_commands_queue_.front();
    search_commands_queue_.pop();
    recorded_search_time_ += config_.control_time_step();
    path.add(i + 1, 0.0f, 0.0f);
    velocities.add(i, Velocity2D(cmd[0], cmd[1], cmd[2]));
  }
  TrajSearchResult result;
  result.isTrajFound = true;
  result.trajCost = 0.0f;
  result.trajectory = Trajectory2D(velocities, path);
  return result;
}

TrackedPose2D RGBDFollower::updateLocalTarget(const TrackedPose2D &current_target, const Velocity2D &robot_cmd,
                                              double dt) {
  // the robot's one-step motion, then the target through its inverse ("pushed back" by the robot's step)
  Path::State step(0.0, 0.0, 0.0);
  step.update(robot_cmd, static_cast<float>(dt));
  const float tx = static_cast<float>(step.x), ty = static_cast<float>(step.y), yaw = static_cast<float>(step.yaw);
  const float c = std::cos(yaw), s = std::sin(yaw);
  const float dx = current_target.x() - tx, dy = current_target.y() - ty;
  return TrackedPose2D(c * dx + s * dy, -s * dx + c * dy, 0.0f, 0.0f, 0.0f, 0.0f);
}

Trajectory2D RGBDFollower::getTrackingReferenceSegment(const TrackedPose2D &tracking_pose) {
  const int ph = config_.prediction_horizon();
  Trajectory2D ref_traj(static_cast<size_t>(ph));
  const Path::State initialState = track_velocity_ ? pose_ : Path::State(0, 0, 0);
  Path::State sim_state = initialState;
  TrackedPose2D sim_target = tracking_pose;
  const double dt = config_.control_time_step();
  for (int step = 0; step < ph; ++step) {
    ref_traj.path.add(static_cast<size_t>(step), static_cast<float>(sim_state.x), static_cast<float>(sim_state.y),
                      0.0f);
    setCurrentState(sim_state);
    const Velocity2D cmd = getPureTrackingCtrl(sim_target, step == 0);  // the errors of step 0 only
    sim_state.update(cmd, static_cast<float>(dt));
    if (track_velocity_)
      sim_target.update(static_cast<float>(dt));
    else
      sim_target = updateLocalTarget(sim_target, cmd, dt);
    if (step < ph - 1) ref_traj.velocities.add(static_cast<size_t>(step), cmd);
  }
  setCurrentState(initialState);  // restored after the segment
  return ref_traj;
}

TrajSearchResult RGBDFollower::dispatch(const std::optional<TrackedPose2D> &tracked_pose, const Velocity2D &) {
  if (tracked_pose) {
    recorded_wait_time_ = 0.0;
    recorded_search_time_ = 0.0;
    TrajSearchResult result;
    result.isTrajFound = true;
    result.trajCost = 0.0f;
    result.trajectory = getTrackingReferenceSegment(tracked_pose.value());
    // (a one-step horizon has no command: the reference reads past the end there)
    if (result.trajectory.velocities.vx.size() > 0)
      command_ = result.trajectory.velocities.getFront();
    return result;
  }
  if (auto r = tryWait()) return *r;
  if (auto r = trySearch()) return *r;
  return giveUp();
}

}  // namespace Control
}  // namespace Kompass
