// DepthDetector (reference: vision/depth_detector.cpp).  The constructor
// validates and keeps the parameters (kc_depth_create); every update is one
// kc_depth_boxes call, and the kept boxes get the Bbox2D-derived fields here.
#include "vision/depth_detector.h"

#include "utils/logger.h"

namespace Kompass {

DepthDetector::DepthDetector(const Eigen::Vector2f &depth_range, const Eigen::Vector3f &camera_in_body_translation,
                             const Eigen::Quaternionf &camera_in_body_rotation, const Eigen::Vector2f &focal_length,
                             const Eigen::Vector2f &principal_point, const float depth_conversion_factor) {
  const float rot[4] = {camera_in_body_rotation.x(), camera_in_body_rotation.y(), camera_in_body_rotation.z(),
                        camera_in_body_rotation.w()};
  ctx_ = hip::make<hip::DepthHandle>(kc_depth_create, depth_range.data(), camera_in_body_translation.data(), rot,
                                     focal_length.data(), principal_point.data(), depth_conversion_factor, 0);
}

std::optional<std::vector<Bbox3D>> DepthDetector::get3dDetections() const {
  if (boxes_) return *boxes_;
  return std::nullopt;
}

size_t DepthDetector::lastUpload() const {
  size_t bytes = 0;
  hip::check(kc_depth_last_upload(ctx_.get(), &bytes));
  return bytes;
}

void DepthDetector::afterStream(void *stream) { hip::check(kc_depth_after_stream(ctx_.get(), stream)); }

void DepthDetector::updateBoxes(const DepthImageView &img, const std::vector<Bbox2D> &detections,
                                const std::optional<Path::State> &robot_state) {
  const size_t n = detections.size();
  std::vector<int32_t> boxes(4 * n);
  for (size_t i = 0; i < n; ++i) {
    boxes[4 * i] = detections[i].top_corner.x();
    boxes[4 * i + 1] = detections[i].top_corner.y();
    boxes[4 * i + 2] = detections[i].size.x();
    boxes[4 * i + 3] = detections[i].size.y();
  }
  double state[3] = {0.0, 0.0, 0.0};
  if (robot_state) {
    state[0] = robot_state->x;
    state[1] = robot_state->y;
    state[2] = robot_state->yaw;
  }
  std::vector<float> out(6 * std::max<size_t>(n, 1));
  std::vector<int32_t> kept(std::max<size_t>(n, 1));
  size_t m = 0;
  boxes_ = std::make_unique<std::vector<Bbox3D>>();
  ++calls_;
  hip::check(kc_depth_boxes(ctx_.get(), img.data, img.on_device ? 1 : 0, img.rows, img.cols, img.row_stride,
                            img.col_stride, boxes.data(), n, robot_state ? state : nullptr, out.data(),
                            kept.data(), kept.size(), &m));
  size_t next = 0;
  for (size_t j = 0; j < m; ++j) {
    for (; next < static_cast<size_t>(kept[j]); ++next)
      LOG_WARNING("Could not get any depth values for 2D bounding box at ", detections[next].top_corner.x(), ", ",
                  detections[next].top_corner.y());
    ++next;
    Bbox3D b(detections[static_cast<size_t>(kept[j])]);
    b.center = Eigen::Vector3f(out[6 * j], out[6 * j + 1], out[6 * j + 2]);
    b.size = Eigen::Vector3f(out[6 * j + 3], out[6 * j + 4], out[6 * j + 5]);
    boxes_->push_back(b);
  }
  for (; next < n; ++next)
    LOG_WARNING("Could not get any depth values for 2D bounding box at ", detections[next].top_corner.x(), ", ",
                detections[next].top_corner.y());
}

void DepthDetector::updateBoxes(const Eigen::MatrixX<unsigned short> &img, const std::vector<Bbox2D> &detections,
                                const std::optional<Path::State> &robot_state) {
  DepthImageView v;  // column-major, as Eigen's MatrixX
  v.data = img.data();
  v.rows = img.rows();
  v.cols = img.cols();
  v.row_stride = 1;
  v.col_stride = img.rows();
  updateBoxes(v, detections, robot_state);
}

void DepthDetector::updatePOIs(const Eigen::MatrixX<unsigned short> &img, const PointsOfInterest &poi,
                               const std::optional<Path::State> &robot_state) {
  updateBoxes(img, std::vector<Bbox2D>{Bbox2D(poi)}, robot_state);
}

}  // namespace Kompass
