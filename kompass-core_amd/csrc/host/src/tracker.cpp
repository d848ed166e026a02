// FeatureBasedBboxTracker (reference: vision/tracker.cpp), statement by statement.
#include "vision/tracker.h"

#include <algorithm>
#include <cmath>

#include "utils/logger.h"

namespace Kompass {

FeatureBasedBboxTracker::FeatureBasedBboxTracker(const float &time_step, const float &e_pos, const float &e_vel,
                                                 const float &e_acc) {
  timeStep_ = time_step;
  // constant-acceleration transition on (x, y, yaw, vx, vy, omega, ax, ay, a_yaw); as in the reference's
  // comma initialiser the last diagonal entry (a_yaw) is 0
  const float half_dt2 = static_cast<float>(0.5 * std::pow(time_step, 2));
  Eigen::MatrixXf A(StateSize, StateSize);
  A.fill(0.0f);
  for (int i = 0; i < StateSize - 1; ++i) A(i, i) = 1.0f;
  for (int i = 0; i < 6; ++i) A(i, i + 3) = time_step;
  for (int i = 0; i < 3; ++i) A(i, i + 6) = half_dt2;
  Eigen::MatrixXf B(StateSize, 1);
  B.fill(0.0f);
  Eigen::MatrixXf H(StateSize, StateSize), Err(StateSize, StateSize);
  H.fill(0.0f);
  Err.fill(0.0f);
  for (int i = 0; i < StateSize; ++i) {
    H(i, i) = 1.0f;
    Err(i, i) = i < 3 ? e_pos : (i < 6 ? e_vel : e_acc);
  }
  stateKalmanFilter_ = std::make_unique<LinearSSKalmanFilter>(StateSize, 1);
  stateKalmanFilter_->setup(A, B, Err, H, Err);
}

bool FeatureBasedBboxTracker::setInitialTracking(const TrackedBbox3D &bBox) {
  trackedBox_ = std::make_unique<TrackedBbox3D>(bBox);
  trackedLabel_ = bBox.box.label;
  Eigen::VectorXf s(StateSize);
  s(0) = bBox.box.center[0];
  s(1) = bBox.box.center[1];
  s(2) = bBox.yaw();
  s(3) = bBox.vel[0];
  s(4) = bBox.vel[1];
  s(5) = bBox.omega();
  s(6) = bBox.acc[0];
  s(7) = bBox.acc[1];
  s(8) = bBox.ang_acc();
  stateKalmanFilter_->setInitialState(s);
  return true;
}

bool FeatureBasedBboxTracker::setInitialTracking(const Bbox3D &bBox, const float yaw) {
  LOG_DEBUG("Setting initial tracked box");
  trackedBox_ = std::make_unique<TrackedBbox3D>(bBox);
  trackedLabel_ = bBox.label;
  Eigen::VectorXf s(StateSize);
  s.setZero();
  s(0) = bBox.center.x();
  s(1) = bBox.center.y();
  s(2) = yaw;
  stateKalmanFilter_->setInitialState(s);
  return true;
}

bool FeatureBasedBboxTracker::setInitialTracking(const int &pose_x_img, const int &pose_y_img,
                                                 const std::vector<Bbox3D> &detected_boxes, const float yaw) {
  for (const auto &box : detected_boxes) {  // the first box whose image rectangle holds the point
    const auto lx = box.getXLimitsImg();
    if (pose_x_img >= lx(0) && pose_x_img <= lx(1)) {
      const auto ly = box.getYLimitsImg();
      if (pose_y_img >= ly(0) && pose_y_img <= ly(1)) return setInitialTracking(box, yaw);
    }
  }
  return false;
}

bool FeatureBasedBboxTracker::trackerInitialized() const { return trackedBox_ != nullptr; }

void FeatureBasedBboxTracker::updateTrackedBoxState(const int numberSteps) {
  Eigen::MatrixXf z(StateSize, 1);
  z(0, 0) = trackedBox_->box.center.x();
  z(1, 0) = trackedBox_->box.center.y();
  z(2, 0) = trackedBox_->yaw();
  z(3, 0) = trackedBox_->vel.x();
  z(4, 0) = trackedBox_->vel.y();
  z(5, 0) = trackedBox_->omega();
  z(6, 0) = trackedBox_->acc.x();
  z(7, 0) = trackedBox_->acc.y();
  z(8, 0) = trackedBox_->ang_acc();
  stateKalmanFilter_->estimate(z, numberSteps);
}

bool FeatureBasedBboxTracker::updateTracking(const std::vector<Bbox3D> &detected_boxes) {
  std::vector<const Bbox3D *> label_boxes;
  for (const auto &box : detected_boxes)
    if (box.label == trackedLabel_) label_boxes.push_back(&box);
  if (label_boxes.empty()) {
    LOG_DEBUG("No boxes with label ", trackedLabel_, " found in the detected boxes!");
    return false;
  }
  float max_similarity_score = 0.0f;
  const Bbox3D *found_box = nullptr;
  // dt from the FIRST box of the label
  const float dt = label_boxes[0]->timestamp - trackedBox_->box.timestamp;
  if (label_boxes.size() == 1) {
    max_similarity_score = 1.0f;  // a single candidate is the target, no features needed
    found_box = label_boxes[0];
  } else {
    const FeaturesVector ref = extractFeatures(trackedBox_->predictConstantAcc(dt));
    size_t similar_box_idx = 0;
    for (size_t k = 0; k < label_boxes.size(); ++k) {
      const FeaturesVector f = extractFeatures(*label_boxes[k]);
      float sq = 0.0f;
      for (int i = 0; i < StateSize; ++i) {
        float e = f[i] - ref[i];
        if (std::abs(ref[i]) > 0.0f) e = e / std::abs(ref[i]);
        sq += e * e;
      }
      const float norm = std::sqrt(sq);
      const float similarity_score = std::exp(-std::pow(norm, 2));  // exp in double, then narrowed
      if (similarity_score > max_similarity_score) {
        max_similarity_score = similarity_score;
        similar_box_idx = k;
      }
    }
    found_box = label_boxes[similar_box_idx];
  }
  if (max_similarity_score > minAcceptedSimilarityScore_) {
    const float step_dt = found_box->timestamp - trackedBox_->box.timestamp;
    const int number_steps = std::max(static_cast<int>(step_dt / timeStep_), 1);
    trackedBox_->updateFromNewDetection(*found_box);
    updateTrackedBoxState(number_steps);
    return true;
  }
  LOG_DEBUG("Box not found in the detected boxes! Max similarity score = ", max_similarity_score,
            ", min accepted = ", minAcceptedSimilarityScore_);
  return false;
}

FeatureBasedBboxTracker::FeaturesVector FeatureBasedBboxTracker::extractFeatures(const TrackedBbox3D &b) const {
  return extractFeatures(b.box);
}

FeatureBasedBboxTracker::FeaturesVector FeatureBasedBboxTracker::extractFeatures(const Bbox3D &b) const {
  FeaturesVector f{};
  f[0] = b.center(0);
  f[1] = b.center(1);
  f[2] = b.size(0);
  f[3] = b.size(1);
  f[4] = b.size(2);
  f[5] = static_cast<float>(b.pc_points.size());
  if (f[5] > 0.0f) {
    const Eigen::Vector3f sd = computePointsStdDev(b.pc_points);
    f[6] = sd(0);
    f[7] = sd(1);
    f[8] = sd(2);
  }
  return f;
}

std::optional<TrackedBbox3D> FeatureBasedBboxTracker::getRawTracking() const {
  if (trackedBox_) return *trackedBox_;
  return std::nullopt;
}

std::optional<Eigen::MatrixXf> FeatureBasedBboxTracker::getTrackedState() const {
  if (trackedBox_) return stateKalmanFilter_->getState();
  return std::nullopt;
}

std::optional<Control::TrackedPose2D> FeatureBasedBboxTracker::getFilteredTrackedPose2D() const {
  if (!trackedBox_) return std::nullopt;
  const Eigen::MatrixXf s = stateKalmanFilter_->getState().value();
  return Control::TrackedPose2D(s(0, 0), s(1, 0), s(2, 0), s(3, 0), s(4, 0), s(5, 0));
}

// NOTE (reference): both the mean and the variance are divided by max(n - 1, 1)
Eigen::Vector3f FeatureBasedBboxTracker::computePointsStdDev(const std::vector<Eigen::Vector3f> &pc) const {
  const float size = static_cast<float>(std::max(static_cast<int>(pc.size()) - 1, 1));
  Eigen::Vector3f mean, var, sd;
  for (const auto &p : pc)
    for (int i = 0; i < 3; ++i) mean(i) += p(i);
  for (int i = 0; i < 3; ++i) mean(i) /= size;
  for (const auto &p : pc)
    for (int i = 0; i < 3; ++i) {
      const float d = p(i) - mean(i);
      var(i) += d * d;
    }
  for (int i = 0; i < 3; ++i) sd(i) = std::sqrt(var(i) / size);
  return sd;
}

}  // namespace Kompass
