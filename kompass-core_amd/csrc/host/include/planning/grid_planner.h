// Deterministic grid planner of the kompass_cpp surface: occupancy grid -> collision-free Path::Path on the
// device (kc_planner_*, csrc/kc_planner.hip).
//
// The reference's planning submodule is an OMPL wrapper (planning/ompl.h:18-89) and stays out of scope; this
// class keeps the method names of that surface where the meaning is the same (setSpaceBoundsFromMap,
// setupProblem, solve, getPath, getCost) and is not a restatement of it: an exact 8-connected shortest path on
// the grid, the robot a disc of its circumscribed horizontal radius (yaw-free, conservative).  setClearanceCost
// adds a surcharge per cell that falls with the distance to the nearest blocking cell (rules 6 to 8): the path
// then trades length for clearance, as deterministically as before.  getAnyAngle* hand out the any-angle path over
// the same walk (rules 9 to 12): far fewer waypoints, straight where there is line of sight, and with a clearance
// cost no closer to a blocking cell than the walk already came.  setOrientedFootprint (BOX robots, rules 13 to 18)
// plans over (cell, heading class) with the box's own oriented footprint instead of the disc: the robot moves along
// its length axis wherever the box fits and turns in place only where the turning disc fits.  explore (rules 21 to 26)
// asks the map instead of the caller for a goal: the frontiers of the known map that the robot can reach, nearest
// first, and the path to each.  setCarMotion (rules 27 to 36) plans for a car: the state is (cell, one of eight directed
// headings), the transitions one straight step and 45-degree arcs whose legs follow from the minimum turning radius,
// reverse at a price or not at all, no turn in place, and the goal's heading honoured.
#pragma once

#include <cstdint>
#include <memory>
#include <optional>
#include <stdexcept>
#include <vector>

#include "datatypes/path.h"
#include "mapping/local_mapper.h"
#include "mapping/world_map.h"
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
  // The class plane of a WorldMap where it lies on the device, with the map's metadata read again (DESIGN.md 4.11 rule
  // 51): when the origin, shape or resolution differ from the bounds held -- the map's window has been shifted -- the
  // bounds are set again and the start and goal of the last setupProblem are taken into the new bounds' cells.
  // Returns whether the bounds moved.  The bounds are floats, as everywhere in this class: the comparison is theirs.
  bool setGridFromWorldMap(const Mapping::WorldMap &map);

  void setupProblem(double start_x, double start_y, double start_yaw, double goal_x, double goal_y, double goal_yaw);
  // false (and no path) when the start or the goal is outside the grid or invalid, or the goal out of reach
  bool solve();
  // solve() from the field the context kept (rules 19 and 20): the same contract and the same outputs bit for bit.
  // For a robot that follows its plan: after setGrid* with the map's next state and / or setupProblem with the
  // same goal and a new start.  The passes run only over what the new grid changed, none when only the start
  // moved.  A full solve, silently, when there is no kept field, the goal, the footprint or the clearance cost
  // changed, or the oriented footprint is on (replanned() then says false).
  bool replan();
  // setGridFromWorldMap(map), then replan() -- or, when the bounds moved, a full solve() with replanned() false: the
  // kept field is one of the old window's cells and is not carried across a shift (rule 51)
  bool replan(const Mapping::WorldMap &map);
  // the last replan() kept a field / its rollback threshold in field units (0xFFFFFFFF: nothing was rolled back)
  bool replanned() const { return replanned_; }
  uint32_t replanThreshold() const { return replan_threshold_; }
  std::optional<Path::Path> getPath(bool simplify = false);
  // the cells of that path, (i, j) pairs
  std::vector<int32_t> getPathCells(bool simplify = false);
  // field[start] * resolution / 10: the steps, and with a clearance cost the penalties of the cells left
  float getCost() const;
  // the steps of the path alone, summed from its cells: metres along the 8-connected path
  float getPathLength();

  // The any-angle path (rules 9 to 12): from each kept cell the farthest of the next max_span cells of the walk whose
  // segment touches only valid cells (and, with a clearance cost, no cell closer to a blocking one than the walk's
  // closest).  nullopt / empty / +inf without a path; std::out_of_range for max_span outside 1 ..
  // KC_PLANNER_MAX_SPAN.  getCost, getPathLength and getPathMinClearance keep describing the walk.
  std::optional<Path::Path> getAnyAnglePath(int max_span = 128);
  // (i, j) pairs of its cells; indices_out (optional): their indices into getPathCells(false)
  std::vector<int32_t> getAnyAngleCells(int max_span = 128, std::vector<int32_t> *indices_out = nullptr);
  // resolution * sum of sqrt(dx^2 + dy^2) over consecutive kept cells, in double, in path order, cast to float
  float getAnyAngleLength(int max_span = 128);
  // sqrt(smallest clear2 the kept segments touch) * resolution; +inf with the clearance cost off or nothing in reach
  float getAnyAngleMinClearance(int max_span = 128);

  // The clearance cost.  reach: metres beyond the footprint radius plus margin over which a cell is surcharged, C2
  // = radiusToR2(radius + margin + reach, resolution), evaluated with the bounds and again when they change.
  // weight: the surcharge at the footprint's edge in straight-cell lengths, Wt = lround(weight * 10); the table is
  // clearanceTable(Wt, R2, C2).  reach <= 0 or weight <= 0 switches it off.  std::out_of_range where the reach is
  // wider than 254 cells.
  void setClearanceCost(float reach, float weight);
  bool clearanceCostOn() const { return clear_on_; }
  uint32_t clearanceC2() const;
  uint32_t clearanceWeight10() const { return clear_on_ ? weight10_ : 0u; }
  // pen_by_d2[0 .. c2]: 0 for d2 <= r2, else weight10 * (c2 - d2) / (c2 - r2) in integers (64-bit product); all
  // zero when c2 <= r2
  static std::vector<uint32_t> clearanceTable(uint32_t weight10, uint32_t r2, uint32_t c2);
  // the last solve's clear2 and penalty per cell, width x height as the grid (cap: cells either output holds)
  void getClearance(uint16_t *clear2_out, uint32_t *pen_out, size_t cap);
  // sqrt(smallest clear2 along the path) * resolution; +inf when no blocking cell is within reach of it
  float getPathMinClearance() const;
  // the last solve's cost field and validity map, width x height as the grid (cap: cells either output holds)
  void getField(uint32_t *field_out, uint8_t *valid_out, size_t cap);

  // The oriented footprint (rules 13 to 18), BOX robots only.  The state is (cell, class); class k = 0 .. 3 is the
  // box's x axis along (1, 0), (1, 1), (0, 1), (-1, 1).  A2 = radiusToR2(x / 2 + margin, resolution) and B2 likewise
  // from y, evaluated with the bounds and again when they change.  turn_cost: straight-cell lengths per 45 degrees,
  // turn10 = lround(turn_cost * 10) in 1 .. 10000 (std::out_of_range beyond).  The start class comes from
  // setupProblem's start_yaw; goal_yaw stays unused: every valid class at the goal cell is a goal state.
  // std::invalid_argument for a shape that is no box, together with a clearance cost (here or in setClearanceCost,
  // whichever comes second), and from the getAnyAngle* calls while it is on.  getCost includes the turns,
  // getPathLength is the steps alone, getPath / getPathCells collapse the repeated cell of a turn.
  void setOrientedFootprint(bool on, float turn_cost = 1.0f);
  bool orientedOn() const { return oriented_on_; }
  uint32_t orientedTurn10() const { return oriented_on_ ? turn10_ : 0u; }
  // A2, B2 of the bounds set (0, 0 while the mode is off)
  void orientedA2B2(uint32_t *a2_out, uint32_t *b2_out) const;
  // the (i, j, k) triples of the last solve's state walk, start first; empty without a path or with the mode off.  With
  // car motion: (i, j, h), one per primitive boundary.
  std::vector<int32_t> getPathStates();
  // the last oriented solve's field (four layers, class 0 first), validity bits (bit k = class k) and turn validity
  void getOrientedField(uint32_t *field4_out, uint8_t *valid4_out, uint8_t *turn_valid_out, size_t cap);
  // k0 = ((lround(yaw / (pi / 4)) mod 4) + 4) mod 4, in double, halves away from zero; needs no device
  static int orientationClass(double yaw);
  // rule 14's offsets of class k as (di, dj) pairs, row by row (dj rising, then di); needs no device.
  // std::invalid_argument for k outside 0 .. 3, std::out_of_range where A2 + B2 reaches beyond 254 cells.
  static std::vector<int32_t> orientedMask(int k, uint32_t a2, uint32_t b2);
  // Car motion (rules 27 to 36).  The state is (cell, heading h = 0 .. 7: E, NE, N, NW, W, SW, S, SE); the primitives are
  // S, L, R and, with allow_reverse, B, BL, BR at reverse_weight (1 .. 16) times the forward cost; the legs of an arc are
  // n = turnCells(min_turning_radius, resolution) cells, evaluated with the bounds and again when they change.  The
  // footprint is the disc, or with setOrientedFootprint(true) the box by heading (rule 28; turn_cost then plays no part:
  // a car does not pivot).  The start heading comes from setupProblem's start_yaw, the goal heading from goal_yaw when
  // honour_goal_yaw, else every valid heading at the goal cell ends the path.  A corner of the planned polyline has n
  // cells of tangent on either side, so a fillet of radius n / tan(pi / 8) >= min_turning_radius / resolution cells
  // fits; it leaves the polyline by at most 0.199 n cells, which `margin` has to allow for.  The polyline is what is
  // planned and checked.  getPath / getPathCells give every unit step of every primitive; getCost weighs reverse,
  // getPathLength does not.  replan() is a full solve.  std::invalid_argument together with a clearance cost (here or in
  // setClearanceCost, whichever comes second) and from getAnyAngle* and explore while it is on; std::out_of_range for a
  // radius of more than KC_PLANNER_MAX_TURN_CELLS turn cells or a reverse weight outside 1 .. 16.
  void setCarMotion(bool on, float min_turning_radius = 0.0f, bool allow_reverse = false, int reverse_weight = 2,
                    bool honour_goal_yaw = true);
  bool carOn() const { return car_on_; }
  // n of the bounds set (0 while the mode is off) / rw as the context gets it (0 without reverse)
  int carTurnCells() const;
  uint32_t carReverseWeight() const { return car_on_ && car_reverse_ ? car_rw_ : 0u; }
  // the last car solve's field [8 layers], moves bytes [8 layers] and validity bits (bit h = heading h)
  void getCarField(uint32_t *field8_out, uint8_t *moves8_out, uint8_t *valid_out, size_t cap);
  // the primitive ids (0 .. 5: S, L, R, B, BL, BR) between the states of getPathStates(); empty without a path or with
  // the mode off
  std::vector<int32_t> getPathMoves();
  // h = ((lround(yaw / (pi / 4)) mod 8) + 8) mod 8, in double, halves away from zero; needs no device
  static int headingClass(double yaw);
  // n = max(1, (int)ceil(radius / resolution * tan(pi / 8))), in double with tan(pi / 8) a literal; needs no device.
  // std::invalid_argument for a radius or resolution that is not finite and positive, std::out_of_range where no int
  // holds n
  static int turnCells(double radius, double resolution);
  // Exploration (rules 21 to 26): the reachable frontiers of the grid from the cell of (robot_x, robot_y), the
  // footprint the disc (only occupied cells inflate, unknown cells are never crossed: allow_unknown plays no part).
  // min_distance_m: a frontier cell lies at least that far along the field, min_cost = lround(min_distance_m /
  // resolution * 10) in double; min_size: the cells a frontier has at least (std::out_of_range for 0).  true when at
  // least one is kept.  A solve-type call: getPath / getCost describe nothing until the next solve(), getField gives
  // the explore field.  The problem of the last setupProblem is not touched: the robot's position is this call's
  // own argument, and the next solve() or replan() (a full solve then) plans from the start that was set up.
  // std::invalid_argument with a clearance cost or the oriented footprint on: a frontier is ranked by plain travel
  // cost to a cell, which neither defines (rule 22).
  struct Frontier {
    float entry_x, entry_y;        // the nearest cell of the frontier, in the map's frame
    int entry_i, entry_j;
    float centroid_x, centroid_y;  // origin + (sum of the indices / size) * resolution, in double, cast to float
    float cost;                    // field[entry] * resolution / 10, as getCost
    uint32_t size, root;
  };
  bool explore(double robot_x, double robot_y, double min_distance_m = 0.0, uint32_t min_size = 8);
  // the kept frontiers of the last explore(), sorted by (cost, entry flat index); empty after anything else
  std::vector<Frontier> frontiers();
  uint32_t components() const { return components_; }
  int labelPasses() const { return label_passes_; }
  // the path to kept frontier k, robot first; std::out_of_range for k outside the list
  std::optional<Path::Path> frontierPath(size_t k);
  std::vector<int32_t> frontierPathCells(size_t k);
  // rule 24's labels, width x height as the grid, 0xFFFFFFFF where the cell is no frontier cell
  void frontierLabels(uint32_t *labels_out, size_t cap);
  static uint32_t minDistanceToCost(double min_distance_m, float resolution);
  int width() const { return width_; }
  int height() const { return height_; }

  int status() const { return status_; }
  int passes() const { return passes_; }
  uint32_t footprintR2() const;
  float footprintRadius() const { return radius_; }
  void cells(int start_out[2], int goal_out[2]) const;
  // the goal of the last setupProblem in the world frame; false before one
  bool goalWorld(double *x_out, double *y_out) const;
  kc_planner *hipContext() const { return ctx_.get(); }

  // (int)((x - origin) / resolution) in float, as localToGrid; false for what no int holds
  static bool worldToCell(float x, float origin, float resolution, int *cell);
  static float cellToWorld(int cell, float origin, float resolution) { return origin + static_cast<float>(cell) * resolution; }
  // floor((radius / resolution)^2 * (1 + 2^-20)) in double
  static uint32_t radiusToR2(double radius, float resolution);

 private:
  hip::PlannerHandle ctx_;
  double radius_ = 0.0;
  bool allow_unknown_ = true;
  float ox_ = 0.0f, oy_ = 0.0f, res_ = 0.0f;
  int width_ = 0, height_ = 0;
  bool have_bounds_ = false, have_grid_ = false, have_problem_ = false;
  int start_[2] = {-1, -1}, goal_[2] = {-1, -1};
  double problem_[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // the last setupProblem in the world frame, for bounds that move
  int status_ = -1, passes_ = 0;
  uint32_t cost_ = 0xFFFFFFFFu;
  bool replanned_ = false;
  uint32_t replan_threshold_ = 0xFFFFFFFFu;
  bool explored_ = false;  // the last solve-type call was explore(): status_ is its status, cost_ stays at "none"
  uint32_t components_ = 0;
  int label_passes_ = 0;
  bool clear_on_ = false;
  double reach_ = 0.0;
  uint32_t weight10_ = 0;
  bool clear_applied_ = false;  // the context holds the table of (applied_r2_, applied_c2_, applied_w10_)
  uint32_t applied_r2_ = 0, applied_c2_ = 0, applied_w10_ = 0;
  bool is_box_ = false;
  double box_x_ = 0.0, box_y_ = 0.0, margin_ = 0.0;
  bool oriented_on_ = false;
  uint32_t turn10_ = 0;
  int start_class_ = 0;
  bool oriented_applied_ = false;  // the context holds (applied_a2_, applied_b2_, applied_turn10_)
  uint32_t applied_a2_ = 0, applied_b2_ = 0, applied_turn10_ = 0;
  bool car_on_ = false, car_reverse_ = false, car_goal_yaw_ = true;
  double car_radius_ = 0.0;
  uint32_t car_rw_ = 0;
  int start_heading_ = 0, goal_heading_ = -1;
  bool car_applied_ = false;  // the context holds (applied_turn_, applied_rw_, applied_car_a2_, applied_car_b2_)
  int applied_turn_ = 0;
  uint32_t applied_rw_ = 0, applied_car_a2_ = 0, applied_car_b2_ = 0;
  void applyCar();
  static void checkTurnCells(int n);  // std::out_of_range above KC_PLANNER_MAX_TURN_CELLS
  void applyModes();
  void applyOriented();
  void applyClearanceCost();
  void needBounds() const;
  void needDiscMode() const {  // the any-angle calls: a segment at an arbitrary angle has no heading class (rule 18)
    if (oriented_on_) throw std::invalid_argument("GridPlanner: no any-angle path with the oriented footprint on");
    if (car_on_) throw std::invalid_argument("GridPlanner: no any-angle path with car motion on: a segment at an arbitrary angle is no primitive");
  }
  bool havePath() const { return status_ == KC_PLAN_FOUND && !explored_; }  // of a solve: explore() hands out frontier paths
  void forgetSolve();
  void beginSolve();
  Path::Path cellsToPath(const std::vector<int32_t> &ij) const;  // (i, j) pairs -> the cells' world points
};

}  // namespace Planning
}  // namespace Kompass
