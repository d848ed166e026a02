// Deterministic grid planner of the kompass_cpp surface: occupancy grid -> collision-free Path::Path on the
// device (kc_planner_*, csrc/kc_planner.hip).
//
// The reference's planning submodule is an OMPL wrapper (planning/ompl.h:18-89) and stays out of scope; this
// class keeps the method names of that surface where the meaning is the same (setSpaceBoundsFromMap,
// setupProblem, solve, getPath, getCost) and is not a restatement of it: an exact 8-connected shortest path on
// the grid, the robot a disc of its circumscribed horizontal radius (yaw-free, conservative).
#pragma once

#include <cstdint>
#include <memory>
#include <optional>
#include <vector>

#include "datatypes/path.h"
#include "mapping/local_mapper.h"
#include "utils/collision_check.h"
#include "utils/hip_backend.h"

namespace Kompass {
namespace Planning {

class GridPlanner {
 public:
  // margin: metres added to the footprint radius before it is turned into cells
  GridPlanner(const CollisionChecker::ShapeType &robot_shape_type, const std::vector<float> &robot_dimensions,
              bool allow_unknown = true, float margin = 0.0f);

  // The map's frame: cell (i, j) of a width x height grid sits at (origin_x + i * resolution, origin_y + j *
  // resolution) -- the mapper's gridToLocal / localToGrid pair (mapping/local_mapper.h:198-222) with the central
  // point at the origin.  width counts the cells along x (the grid's first, fast index).
  void setSpaceBoundsFromMap(float origin_x, float origin_y, int width, int height, float resolution);

  // The grid, width x height as set above, cell (i, j) at i + j * width; elem_bytes 4 (int32, the mapper's
  // cells) or 1 (int8, the PCD grid's).  The device overload reads a finished grid in place.
  void setGrid(const void *host_grid, int elem_bytes);
  void setGridOnDevice(const void *dev_grid, int elem_bytes);
  // orders the next device grid's read after the work queued so far on a producer's stream (no host wait)
  void waitForStream(void *stream);
  // throws unless a grid of this shape is what set_space_bounds_from_map announced
  void setSpaceBoundsCheck(int width, int height) const;
  // the last grid of a LocalMapper where it lies (scanToGrid / scanToGridOnDevice); sets the bounds from the
  // mapper as well: origin = -(central cell) * resolution
  void setGridFromMapper(Mapping::LocalMapper &mapper);

  void setupProblem(double start_x, double start_y, double start_yaw, double goal_x, double goal_y, double goal_yaw);
  // false (and no path) when the start or the goal is outside the grid or invalid, or the goal out of reach
  bool solve();
  std::optional<Path::Path> getPath(bool simplify = false);
  // the cells of that path, (i, j) pairs
  std::vector<int32_t> getPathCells(bool simplify = false);
  float getCost() const;
  // the last solve's cost field and validity map, width x height as the grid (cap: cells either output holds)
  void getField(uint32_t *field_out, uint8_t *valid_out, size_t cap);
  int width() const { return width_; }
  int height() const { return height_; }

  int status() const { return status_; }
  int passes() const { return passes_; }
  uint32_t footprintR2() const;
  float footprintRadius() const { return radius_; }
  void cells(int start_out[2], int goal_out[2]) const;
  kc_planner *hipContext() const { return ctx_.get(); }

  // (int)((x - origin) / resolution) in float, as localToGrid; false for what no int holds
  static bool worldToCell(float x, float origin, float resolution, int *cell);
  static float cellToWorld(int cell, float origin, float resolution) { return origin + static_cast<float>(cell) * resolution; }
  // floor((radius / resolution)^2 * (1 + 2^-20)) in double
  static uint32_t radiusToR2(double radius, float resolution);

 private:
  struct Deleter {
    void operator()(kc_planner *p) const { kc_planner_destroy(p); }
  };
  std::unique_ptr<kc_planner, Deleter> ctx_;
  double radius_ = 0.0;
  bool allow_unknown_ = true;
  float ox_ = 0.0f, oy_ = 0.0f, res_ = 0.0f;
  int width_ = 0, height_ = 0;
  bool have_bounds_ = false, have_grid_ = false, have_problem_ = false;
  int start_[2] = {-1, -1}, goal_[2] = {-1, -1};
  int status_ = -1, passes_ = 0;
  uint32_t cost_ = 0xFFFFFFFFu;
  void needBounds() const;
  void forgetSolve();
};

}  // namespace Planning
}  // namespace Kompass
