// Vision datatypes of the kompass_cpp surface (reference: datatypes/tracking.h):
// PointsOfInterest, Bbox2D and Bbox3D with the reference's constructors and
// validation (std::invalid_argument), and TrackedBbox3D, the box the
// bounding-box tracker follows.
#pragma once

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "datatypes/control.h"
#include "kc_linalg.h"
#include "utils/logger.h"

namespace Kompass {

struct PointsOfInterest {
  std::vector<Eigen::Vector2i> Points2D = {};  // 2D points in the image frame
  float timestamp = 0.0;                       // seconds
  std::string label = "";
  Eigen::Vector2i img_size = {640, 480};
  Eigen::Vector2i vel = {};  // average points velocity in the image frame

  PointsOfInterest() {}

  PointsOfInterest(const std::vector<Eigen::Vector2i> &points, const Eigen::Vector2i &img_size = {640, 480},
                   const float timestamp = 0.0, const std::string &label = "")
      : Points2D(points), timestamp(timestamp), label(label), img_size(img_size) {
    if (img_size.x() <= 0 || img_size.y() <= 0) throw std::invalid_argument("Invalid image size");
    for (const auto &point : Points2D) {
      if (point.x() < 0 || point.x() >= img_size.x() || point.y() < 0 || point.y() >= img_size.y())
        throw std::invalid_argument("Point " + std::to_string(point.x()) + "," + std::to_string(point.y()) +
                                    " is out of image bounds");
    }
  }

  void setImgSize(const Eigen::Vector2i &size) {
    if (size.x() <= 0 || size.y() <= 0) throw std::invalid_argument("Invalid image size");
    img_size = size;
  }

  void setVel(const Eigen::Vector2i &v) { vel = v; }
};

struct Bbox2D {
  Eigen::Vector2i top_corner = {0, 0};
  Eigen::Vector2i size = {0, 0};
  float timestamp = 0.0;  // seconds
  std::string label = "";
  Eigen::Vector2i img_size = {640, 480};
  Eigen::Vector3f vel = {0.0f, 0.0f, 0.0f};

  Bbox2D() {}

  Bbox2D(const Eigen::Vector2i top_corner, const Eigen::Vector2i size, const float timestamp = 0.0,
         const std::string &label = "", const Eigen::Vector2i img_size = {640, 480})
      : top_corner(top_corner), size(size), timestamp(timestamp), label(label), img_size(img_size) {
    if (size.x() <= 0 || size.y() <= 0) throw std::invalid_argument("Invalid bounding box size");
    if (img_size.x() <= 0 || img_size.y() <= 0) throw std::invalid_argument("Invalid image size");
  }

  // the box spans mad_scale * MAD around the median of the points, at least 5 px, clamped to the image
  Bbox2D(const PointsOfInterest &poi, const float mad_scale = 2.0f)
      : timestamp(poi.timestamp), label(poi.label), img_size(poi.img_size) {
    if (poi.Points2D.empty()) throw std::invalid_argument("PointsOfInterest has no points");
    const size_t n = poi.Points2D.size();
    std::vector<int> xs(n), ys(n);
    for (size_t i = 0; i < n; ++i) {
      xs[i] = poi.Points2D[i].x();
      ys[i] = poi.Points2D[i].y();
    }
    std::sort(xs.begin(), xs.end());
    std::sort(ys.begin(), ys.end());
    const int median_x = xs[n / 2], median_y = ys[n / 2];
    std::vector<int> dx(n), dy(n);
    for (size_t i = 0; i < n; ++i) {
      dx[i] = std::abs(xs[i] - median_x);
      dy[i] = std::abs(ys[i] - median_y);
    }
    std::sort(dx.begin(), dx.end());
    std::sort(dy.begin(), dy.end());
    const int half_w = std::max(static_cast<int>(mad_scale * dx[n / 2]), 5);
    const int half_h = std::max(static_cast<int>(mad_scale * dy[n / 2]), 5);
    const int x0 = std::max(0, median_x - half_w), y0 = std::max(0, median_y - half_h);
    const int x1 = std::min(poi.img_size.x() - 1, median_x + half_w);
    const int y1 = std::min(poi.img_size.y() - 1, median_y + half_h);
    top_corner = {x0, y0};
    size = {x1 - x0, y1 - y0};
  }

  Eigen::Vector2i getXLimits() const { return {top_corner.x(), top_corner.x() + size.x()}; }
  Eigen::Vector2i getYLimits() const { return {top_corner.y(), top_corner.y() + size.y()}; }
  Eigen::Vector2i getCenter() const { return {top_corner.x() + size.x() / 2, top_corner.y() + size.y() / 2}; }

  void setImgSize(const Eigen::Vector2i &s) {
    if (s.x() <= 0 || s.y() <= 0) throw std::invalid_argument("Invalid image size");
    img_size = s;
  }

  void setVel(const Eigen::Vector3f &v) { vel = v; }
};

struct Bbox3D {
  Eigen::Vector3f center = {0.0f, 0.0f, 0.0f};
  Eigen::Vector3f size = {0.0f, 0.0f, 0.0f};
  Eigen::Vector2i center_img_frame = {0, 0};
  Eigen::Vector2i size_img_frame = {0, 0};
  std::vector<Eigen::Vector3f> pc_points = {};
  float timestamp = 0.0;  // seconds
  std::string label = "";

  Bbox3D() {}

  Bbox3D(const Eigen::Vector3f &center, const Eigen::Vector3f &size, const Eigen::Vector2i center_img_frame,
         const Eigen::Vector2i size_img_frame, const float timestamp = 0.0, const std::string &label = "",
         const std::vector<Eigen::Vector3f> pc_points = {})
      : center(center), size(size), center_img_frame(center_img_frame), size_img_frame(size_img_frame),
        pc_points(pc_points), timestamp(timestamp), label(label) {}

  // center_img_frame = top + size / 2 (integer division)
  explicit Bbox3D(const Bbox2D &box2d)
      : center_img_frame(box2d.getCenter()), size_img_frame(box2d.size), timestamp(box2d.timestamp),
        label(box2d.label) {}

  // image-frame limits (float, integer halves as in the reference)
  Eigen::Vector2f getXLimitsImg() const {
    return {static_cast<float>(center_img_frame.x() - size_img_frame.x() / 2),
            static_cast<float>(center_img_frame.x() + size_img_frame.x() / 2)};
  }
  Eigen::Vector2f getYLimitsImg() const {
    return {static_cast<float>(center_img_frame.y() - size_img_frame.y() / 2),
            static_cast<float>(center_img_frame.y() + size_img_frame.y() / 2)};
  }
};

// A box with the velocity and acceleration of its centre (reference: datatypes/tracking.h:207-283)
struct TrackedBbox3D {
  Bbox3D box;
  Eigen::Vector3f vel = {0.0f, 0.0f, 0.0f};
  Eigen::Vector3f acc = {0.0f, 0.0f, 0.0f};
  int unique_id = 0;

  TrackedBbox3D(const Bbox3D &box) : box(box) {}

  void setSize(const Eigen::Vector3f &size) { box.size = size; }
  void setfromBox(const Bbox3D &b) { box = b; }

  // finite differences over the timestamps; a step <= 0 (the usual case: Bbox2D.timestamp defaults to 0) resets
  // velocity and acceleration
  void updateFromNewDetection(const Bbox3D &new_box) {
    if (new_box.label != box.label) {
      LOG_ERROR("Box label mismatch, cannot update tracking.");
      return;
    }
    const float time_step = new_box.timestamp - box.timestamp;
    if (time_step <= 0.0f) {
      LOG_DEBUG("Box updated with invalid time step, Velocity wil be reset to zero.");
      vel = {0.0f, 0.0f, 0.0f};
      acc = {0.0f, 0.0f, 0.0f};
    } else {
      Eigen::Vector3f new_vel;
      for (int i = 0; i < 3; ++i) new_vel(i) = (new_box.center(i) - box.center(i)) / time_step;
      for (int i = 0; i < 3; ++i) acc(i) = (new_vel(i) - vel(i)) / time_step;
      vel = new_vel;
    }
    setfromBox(new_box);
  }

  TrackedBbox3D predictConstantVel(const float dt) const {
    TrackedBbox3D p(*this);
    for (int i = 0; i < 3; ++i) p.box.center(i) += p.vel(i) * dt;
    p.acc = {0.0f, 0.0f, 0.0f};
    p.box.timestamp += dt;
    return p;
  }

  TrackedBbox3D predictConstantAcc(const float dt) const {
    TrackedBbox3D p(*this);
    for (int i = 0; i < 3; ++i) p.vel(i) += acc(i) * dt;
    for (int i = 0; i < 3; ++i) p.box.center(i) += p.vel(i) * dt;
    p.box.timestamp += dt;
    return p;
  }

  float v() const { return std::sqrt(vel.x() * vel.x() + vel.y() * vel.y()); }
  float x() const { return box.center.x(); }
  float y() const { return box.center.y(); }
  float yaw() const { return std::atan2(vel(1), vel(0)); }
  float omega() const { return 0.0f; }
  float ang_acc() const { return 0.0f; }
  float timestamp() const { return box.timestamp; }

  void update(const float timeStep) {
    box.center(0) += vel.x() * timeStep;
    box.center(1) += vel.y() * timeStep;
    box.timestamp += timeStep;
  }

  float distance(const float x, const float y, const float z = 0.0f) const {
    const double dx = box.center.x() - x, dy = box.center.y() - y, dz = box.center.z() - z;
    return static_cast<float>(std::sqrt(dx * dx + dy * dy + dz * dz));
  }

  Control::TrackedPose2D getTrackedPose() const {
    return Control::TrackedPose2D(box.center.x(), box.center.y(), yaw(), vel.x(), vel.y(), 0.0f);
  }
};

}  // namespace Kompass
