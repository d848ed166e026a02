// DepthDetector of the kompass_cpp surface (reference: vision/depth_detector.{h,cpp}):
// 2-D detections on an aligned depth frame -> 3-D boxes in the world frame.
// The per-pixel work -- every depth of every box, median, MAD and the band's
// min / max -- is ONE call into libkompass_hip.so (kc_depth_boxes) per frame;
// the frame is read where it lies, in any memory order.
#pragma once

#include <cstdint>
#include <memory>
#include <optional>
#include <vector>

#include "datatypes/path.h"
#include "datatypes/tracking.h"
#include "kc_linalg.h"
#include "utils/hip_backend.h"

namespace Kompass {

// a uint16 depth frame: element (r, c) at data[r * row_stride + c * col_stride]; on_device: a device address
struct DepthImageView {
  const uint16_t *data = nullptr;
  int64_t rows = 0, cols = 0, row_stride = 0, col_stride = 0;
  bool on_device = false;
};

class DepthDetector {
 public:
  DepthDetector(const Eigen::Vector2f &depth_range, const Eigen::Vector3f &camera_in_body_translation,
                const Eigen::Quaternionf &camera_in_body_rotation, const Eigen::Vector2f &focal_length,
                const Eigen::Vector2f &principal_point, const float depth_conversion_factor = 1e-3);

  void updateBoxes(const Eigen::MatrixX<unsigned short> &aligned_depth_img, const std::vector<Bbox2D> &detections,
                   const std::optional<Path::State> &robot_state = std::nullopt);
  void updatePOIs(const Eigen::MatrixX<unsigned short> &aligned_depth_img, const PointsOfInterest &pois,
                  const std::optional<Path::State> &robot_state = std::nullopt);
  // the same on a frame view (no copy of the frame on the host)
  void updateBoxes(const DepthImageView &aligned_depth_img, const std::vector<Bbox2D> &detections,
                   const std::optional<Path::State> &robot_state = std::nullopt);

  std::optional<std::vector<Bbox3D>> get3dDetections() const;

  // (not in the reference's interface) kc_depth_boxes calls so far, and the frame bytes the last one uploaded
  size_t calls() const { return calls_; }
  size_t lastUpload() const;
  // the next frame read waits for the work queued so far on `stream` (a hipStream_t; NULL: the legacy default)
  void afterStream(void *stream);

 private:
  size_t calls_ = 0;
  hip::DepthHandle ctx_;
  std::unique_ptr<std::vector<Bbox3D>> boxes_;
};

}  // namespace Kompass
