// Raw point cloud -> laserscan of the kompass_cpp surface (reference:
// utils/pointcloud.h:116-177, 205-259).  Same signatures; the binning runs on
// the device through the C ABI (kc_cloud_to_laserscan) and returns the same
// doubles as the reference's CPU loop.  Below them the PCD reader (:286-437,
// plain host code) and the PCD -> occupancy grid (:468-540: both loops over the
// points run on the device, kc_cloud_grid_extent / kc_cloud_grid_fill).
#pragma once

#include <array>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <mutex>
#include <optional>
#include <string>
#include <string_view>
#include <utility>
#include <vector>

#include "kc_linalg.h"
#include "utils/hip_backend.h"

namespace Kompass {

namespace detail {
inline kc_cloud *sharedCloud() {
  static hip::CloudHandle ctx = hip::make<hip::CloudHandle>(kc_cloud_create, 1 << 20, 4096, 0);
  return ctx.get();
}
// Calls on one kc_cloud context are serial (kompass_hip.h), and the grid is a protocol of several calls whose
// state lives in the context: every user of the shared context holds this lock from its first call to its last.
inline std::mutex &sharedCloudMutex() {
  static std::mutex m;
  return m;
}
}  // namespace detail

// angle_step overload (pointcloud.h:116-177)
inline void pointCloudToLaserScanFromRaw(
    const std::vector<int8_t> &data, const int point_step, const int row_step,
    const int height, const int width, const int x_offset, const int y_offset,
    const int z_offset, const double max_range, const double min_z,
    const double max_z, const double angle_step,
    std::vector<double> &ranges_out, std::vector<double> &angles_out) {
  const int num_bins = static_cast<int>(std::ceil(2.0 * M_PI / angle_step));
  if (!(angle_step > 0.0) || num_bins <= 0)
    throw std::invalid_argument("pointCloudToLaserScanFromRaw: angle_step must be positive");
  ranges_out.resize(num_bins);
  angles_out.resize(num_bins);
  size_t bins = 0;
  const std::lock_guard<std::mutex> lock(detail::sharedCloudMutex());
  hip::check(kc_cloud_to_laserscan(detail::sharedCloud(), data.data(), data.size(), 0, point_step,
                                   row_step, height, width, x_offset, y_offset, z_offset, max_range,
                                   min_z, max_z, angle_step, 0, ranges_out.data(), angles_out.data(),
                                   ranges_out.size(), &bins));
}

// num_bins overload (pointcloud.h:205-259)
inline void pointCloudToLaserScanFromRaw(
    const std::vector<int8_t> &data, const int point_step, const int row_step,
    const int height, const int width, const int x_offset, const int y_offset,
    const int z_offset, const double max_range, const double min_z,
    const double max_z, const int num_bins, std::vector<double> &ranges_out) {
  if (num_bins <= 0) {  // ranges_out.assign(num_bins, max_range) of the reference
    ranges_out.clear();
    return;
  }
  ranges_out.resize(num_bins);
  size_t bins = 0;
  const std::lock_guard<std::mutex> lock(detail::sharedCloudMutex());
  hip::check(kc_cloud_to_laserscan(detail::sharedCloud(), data.data(), data.size(), 0, point_step,
                                   row_step, height, width, x_offset, y_offset, z_offset, max_range,
                                   min_z, max_z, 0.0, num_bins, ranges_out.data(), nullptr,
                                   ranges_out.size(), &bins));
}

// readPCD (pointcloud.h:286-437): the x, y, z of every point of an ascii or binary PCD file; std::nullopt
// (and a line on stderr) when the file cannot be opened or is malformed.  Where the reference is wrong or
// undefined this reader defines the case:
//  - ascii: a point is one token for each name of FIELDS, and x / y / z are taken by their field index (the
//    reference reads the first three tokens of a running stream whatever FIELDS says);
//  - header lines may end in '\r' or blanks, and blanks may repeat between tokens (the reference compares the
//    raw rest of the DATA line);
//  - x / y / z must be 4-byte fields, every COUNT 1, DATA ascii or binary, POINTS present and covered by the
//    data: std::nullopt otherwise, never a read past the buffer.
inline std::optional<std::vector<std::array<float, 3>>> readPCD(const std::string &filename) {
  auto fail = [&](const std::string &why) {
    std::cerr << "Error: " << why << " (" << filename << ")" << std::endl;
    return std::nullopt;
  };
  std::ifstream file(filename, std::ios::binary);
  if (!file.is_open()) return fail("Could not open file");

  auto blank = [](char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '\f' || c == '\v'; };
  auto tokens = [&](std::string_view rest) {
    std::vector<std::string_view> out;
    size_t pos = 0;
    while (pos < rest.size()) {
      while (pos < rest.size() && blank(rest[pos])) ++pos;
      size_t end = pos;
      while (end < rest.size() && !blank(rest[end])) ++end;
      if (end > pos) out.push_back(rest.substr(pos, end - pos));
      pos = end;
    }
    return out;
  };
  auto number = [](std::string_view t, size_t &value) {
    auto [ptr, ec] = std::from_chars(t.data(), t.data() + t.size(), value);
    return ec == std::errc() && ptr == t.data() + t.size();
  };

  std::vector<std::string> fields;
  std::vector<size_t> sizes;
  int x_idx = -1, y_idx = -1, z_idx = -1;
  size_t num_points = 0;
  bool have_points = false, have_size = false;
  std::string format, line;
  while (std::getline(file, line)) {  // :304-359
    if (line.empty() || line[0] == '#') continue;
    const std::string_view sv(line);
    const auto first_space = sv.find(' ');
    if (first_space == std::string_view::npos) continue;
    const std::string_view keyword = sv.substr(0, first_space);
    const auto rest = tokens(sv.substr(first_space + 1));
    if (keyword == "FIELDS") {
      fields.clear();
      x_idx = y_idx = z_idx = -1;
      for (const auto &f : rest) {
        if (f == "x") x_idx = static_cast<int>(fields.size());
        if (f == "y") y_idx = static_cast<int>(fields.size());
        if (f == "z") z_idx = static_cast<int>(fields.size());
        fields.emplace_back(f);
      }
    } else if (keyword == "SIZE") {
      sizes.clear();
      have_size = true;
      for (const auto &t : rest) {
        size_t v = 0;
        if (!number(t, v) || v == 0 || v > 8) return fail("Bad SIZE entry");
        sizes.push_back(v);
      }
    } else if (keyword == "COUNT") {
      for (const auto &t : rest) {
        size_t v = 0;
        if (!number(t, v) || v != 1) return fail("Only COUNT 1 fields are supported");
      }
    } else if (keyword == "POINTS") {
      if (rest.size() != 1 || !number(rest[0], num_points)) return fail("Failed to parse POINTS value.");
      have_points = true;
    } else if (keyword == "DATA") {
      if (!rest.empty()) format = std::string(rest[0]);
      break;
    }
  }
  if (x_idx == -1 || y_idx == -1 || z_idx == -1) return fail("PCD file must contain 'x', 'y', and 'z' fields.");
  if (!have_points) return fail("PCD file has no POINTS line");
  if (format != "ascii" && format != "binary") return fail("Unsupported DATA format '" + format + "'.");
  if (have_size || format == "binary") {
    if (fields.size() != sizes.size()) return fail("FIELDS and SIZE do not match.");
    if (sizes[x_idx] != 4 || sizes[y_idx] != 4 || sizes[z_idx] != 4) return fail("x, y and z must be 4-byte fields");
  }

  // the rest of the file, once
  const std::string block((std::istreambuf_iterator<char>(file)), std::istreambuf_iterator<char>());
  std::vector<std::array<float, 3>> points;
  if (format == "ascii") {  // :388-409
    // a point is at least one character and a separator for each field
    if (num_points > block.size() / fields.size() + 1) return fail("POINTS is larger than the data");
    points.resize(num_points);
    const char *ptr = block.data(), *const end = block.data() + block.size();
    for (size_t i = 0; i < num_points; ++i) {
      std::array<float, 3> p{0.0f, 0.0f, 0.0f};
      for (int f = 0; f < static_cast<int>(fields.size()); ++f) {
        while (ptr < end && blank(*ptr)) ++ptr;
        const char *start = ptr;
        while (ptr < end && !blank(*ptr)) ++ptr;
        if (start == ptr) return fail("POINTS is larger than the data");
        // from_chars takes the longest numeric prefix of the token, as in the reference ("1.5abc" is 1.5); a token
        // without one, or whose number is out of float's range, leaves 0
        float v = 0.0f;
        std::from_chars(start, ptr, v);
        if (f == x_idx) p[0] = v;
        if (f == y_idx) p[1] = v;
        if (f == z_idx) p[2] = v;
      }
      points[i] = p;
    }
  } else {  // :410-429
    size_t stride = 0, off[3] = {0, 0, 0};
    for (size_t i = 0; i < sizes.size(); ++i) {
      if (static_cast<int>(i) < x_idx) off[0] += sizes[i];
      if (static_cast<int>(i) < y_idx) off[1] += sizes[i];
      if (static_cast<int>(i) < z_idx) off[2] += sizes[i];
      stride += sizes[i];
    }
    if (num_points > block.size() / stride) return fail("Failed to read expected amount of binary data.");
    points.resize(num_points);
    for (size_t i = 0; i < num_points; ++i) {
      const char *rec = block.data() + i * stride;
      for (int k = 0; k < 3; ++k) std::memcpy(&points[i][k], rec + off[k], sizeof(float));
    }
  }
  return points;
}

using OccupancyGridI8 = Eigen::MatrixX<int8_t>;

// The two loops of readPCDToOccupancyGrid (:486-536) over `n_points` records of a cloud on the host or
// (data_on_device) on the device: kc_cloud_grid_extent + kc_cloud_grid_fill on the shared context, under its lock
// from the first call to the last, so that concurrent callers (the Python bindings release the GIL) cannot
// interleave on the context's state.  after_stream: order the reads of a device cloud after the work queued so
// far on `stream` (kc_cloud_after_stream; nullptr = the legacy default stream).
inline std::pair<OccupancyGridI8, std::array<float, 3>> pointsToOccupancyGrid(
    const int8_t *data, size_t nbytes, bool data_on_device, int point_step, size_t n_points, int x_offset,
    int y_offset, int z_offset, float grid_resolution, float z_ground_limit, float robot_height,
    bool after_stream = false, void *stream = nullptr) {
  std::array<float, 3> origin{0.0f, 0.0f, 0.0f};
  int cx = 0, cy = 0;
  const std::lock_guard<std::mutex> lock(detail::sharedCloudMutex());
  kc_cloud *ctx = detail::sharedCloud();
  if (after_stream && data_on_device && n_points) hip::check(kc_cloud_after_stream(ctx, stream));
  hip::check(kc_cloud_grid_extent(ctx, data, nbytes, data_on_device ? 1 : 0, point_step, n_points, x_offset, y_offset,
                                  z_offset, grid_resolution, origin.data(), &cx, &cy));
  OccupancyGridI8 grid(cx, cy);
  hip::check(kc_cloud_grid_fill(ctx, z_ground_limit, robot_height, grid.data(), static_cast<size_t>(grid.size())));
  return {std::move(grid), origin};
}

// readPCDToOccupancyGrid (:468-540): (int8 grid [cells_x x cells_y], {min_x, min_y, 0})
inline std::pair<OccupancyGridI8, std::array<float, 3>> readPCDToOccupancyGrid(const std::string &filename,
                                                                              const float grid_resolution,
                                                                              const float z_ground_limit,
                                                                              const float robot_height) {
  const auto pts = readPCD(filename);
  if (!pts) throw std::runtime_error("Failed to read PCD file: " + filename);
  return pointsToOccupancyGrid(reinterpret_cast<const int8_t *>(pts->data()), pts->size() * 12, false, 12, pts->size(),
                               0, 4, 8, grid_resolution, z_ground_limit, robot_height);
}

}  // namespace Kompass
