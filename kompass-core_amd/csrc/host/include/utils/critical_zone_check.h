// CriticalZoneChecker of the kompass_cpp surface (reference:
// utils/critical_zone_check.{h,cpp}; critical_zone_check_gpu.{h,cpp} for the
// device-named variant).  Preset and checks go through the C ABI (kc_zone_*);
// the results are those of the reference's CPU loop.
#pragma once

#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <vector>

#include "kc_linalg.h"
#include "mapping/world_map.h"
#include "utils/collision_check.h"
#include "utils/hip_backend.h"

namespace Kompass {

enum class PointFieldType { INT8 = 1, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64 };

class CriticalZoneChecker {
 public:
  enum class InputType { LASERSCAN, POINTCLOUD };

  CriticalZoneChecker(InputType input_type, const CollisionChecker::ShapeType robot_shape_type,
                      const std::vector<float> &robot_dimensions,
                      const Eigen::Vector3f &sensor_position_body,
                      const Eigen::Vector4f &sensor_rotation_body, const float critical_angle,
                      const float critical_distance, const float slowdown_distance,
                      const std::vector<double> &angles, const float min_height,
                      const float max_height, const float range_max)
      : input_type_(input_type) {
    const float pos[3] = {sensor_position_body(0), sensor_position_body(1), sensor_position_body(2)};
    const float rot[4] = {sensor_rotation_body(0), sensor_rotation_body(1), sensor_rotation_body(2),
                          sensor_rotation_body(3)};
    ctx_ = hip::make<hip::ZoneHandle>(kc_zone_create, static_cast<int>(robot_shape_type), robot_dimensions.data(),
                                      static_cast<int>(robot_dimensions.size()), pos, rot, critical_angle,
                                      critical_distance, slowdown_distance, angles.data(), angles.size(),
                                      min_height, max_height, range_max, 0);
    for (int k = 0; k < 3; ++k) sensor_pos_[k] = pos[k];
    for (int k = 0; k < 4; ++k) sensor_rot_[k] = rot[k];
    n_angles_ = angles.size();
  }
  virtual ~CriticalZoneChecker() = default;

  // The check on a WorldMap's virtual scan (not in the reference; DESIGN.md 4.11 rules 20 to 27): the robot's pose (x, y,
  // yaw) in the world composed with the planar part of the sensor mount is the scan frame, the preset angles and
  // range_max are the beams; the ranges stay on the device.  The overload with `ranges` merges the present scan by a
  // per-beam minimum (rule 27).  std::invalid_argument for a mount whose rotation is not about z alone.
  float check(const Mapping::WorldMap &map, double x, double y, double yaw, const bool forward) {
    return checkMap(map, x, y, yaw, nullptr, forward);
  }
  float check(const Mapping::WorldMap &map, double x, double y, double yaw, const bool forward,
              const std::vector<double> &ranges) {
    return checkMap(map, x, y, yaw, &ranges, forward);
  }

  float check(const std::vector<double> &ranges, const bool forward) {
    float f = 1.0f;
    hip::check(kc_zone_check(ctx_.get(), ranges.data(), ranges.size(), forward ? 1 : 0, &f));
    return f;
  }
  float check(const std::vector<int8_t> &data, int point_step, int row_step, int height, int width,
              int x_offset, int y_offset, int z_offset, const bool forward) {
    float f = 1.0f;
    hip::check(kc_zone_check_cloud_typed(ctx_.get(), data.data(), data.size(), point_step, row_step, height,
                                         width, x_offset, y_offset, z_offset, static_cast<int>(field_type_),
                                         forward ? 1 : 0, &f));
    return f;
  }

 protected:
  PointFieldType field_type_ = PointFieldType::FLOAT32;
  InputType input_type_;
  hip::ZoneHandle ctx_;
  double sensor_pos_[3] = {0.0, 0.0, 0.0}, sensor_rot_[4] = {0.0, 0.0, 0.0, 1.0};  // the mount: position, (x, y, z, w)
  size_t n_angles_ = 0;

  float checkMap(const Mapping::WorldMap &map, double x, double y, double yaw, const std::vector<double> *ranges,
                 const bool forward) {
    if (sensor_rot_[0] != 0.0 || sensor_rot_[1] != 0.0 || (sensor_rot_[2] == 0.0 && sensor_rot_[3] == 0.0))
      throw std::invalid_argument("CriticalZoneChecker: a scan from the map needs a sensor mount rotated about z alone");
    if (ranges && ranges->size() < n_angles_)
      throw std::out_of_range("CriticalZoneChecker: fewer present ranges than preset angles");
    const double mount_yaw = 2.0 * std::atan2(sensor_rot_[2], sensor_rot_[3]);
    const double c = std::cos(yaw), s = std::sin(yaw);
    const kc_worldmap_pose p = Mapping::WorldMap::quantisePose(map.resolution(), map.originX(), map.originY(),
                                                               x + c * sensor_pos_[0] - s * sensor_pos_[1],
                                                               y + s * sensor_pos_[0] + c * sensor_pos_[1], yaw + mount_yaw);
    float f = 1.0f;
    hip::check(kc_zone_check_worldmap(ctx_.get(), map.hipContext(), &p, 0u, ranges ? ranges->data() : nullptr,
                                      forward ? 1 : 0, &f));
    return f;
  }
};

// critical_zone_check_gpu.h:36-53: same surface plus the datatype of the cloud's x / y / z fields, decoded as
// load_and_cast_val does (utils/pointcloud.h:49-87)
class CriticalZoneCheckerGPU : public CriticalZoneChecker {
 public:
  CriticalZoneCheckerGPU(InputType input_type, const CollisionChecker::ShapeType robot_shape_type,
                         const std::vector<float> &robot_dimensions,
                         const Eigen::Vector3f &sensor_position_body,
                         const Eigen::Vector4f &sensor_rotation_body, const float critical_angle,
                         const float critical_distance, const float slowdown_distance,
                         const std::vector<double> &angles, const float min_height,
                         const float max_height, const float range_max,
                         const PointFieldType cloud_field_type = PointFieldType::FLOAT32)
      : CriticalZoneChecker(input_type, robot_shape_type, robot_dimensions, sensor_position_body,
                            sensor_rotation_body, critical_angle, critical_distance,
                            slowdown_distance, angles, min_height, max_height, range_max) {
    field_type_ = cloud_field_type;
  }
};

}  // namespace Kompass
