// Planning::GridPlanner: frames, the footprint rule and the Path on the host; validity, cost field and the walk
// on the device through kc_planner_* (DESIGN.md 4.10).
#include "planning/grid_planner.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <stdexcept>
#include <string>

namespace Kompass {
namespace Planning {

namespace {
// the circumscribed horizontal radius: cylinder (r, h) and sphere (r) -> r, box (x, y, z) -> half the diagonal
double circumscribedRadius(const CollisionChecker::ShapeType &shape, const std::vector<float> &dims) {
  switch (shape) {
    case CollisionChecker::ShapeType::CYLINDER:
      if (dims.size() < 2) throw std::invalid_argument("a cylinder needs (radius, height)");
      return static_cast<double>(dims[0]);
    case CollisionChecker::ShapeType::SPHERE:
      if (dims.empty()) throw std::invalid_argument("a sphere needs (radius)");
      return static_cast<double>(dims[0]);
    case CollisionChecker::ShapeType::BOX: {
      if (dims.size() < 3) throw std::invalid_argument("a box needs (x, y, z)");
      const double x = dims[0], y = dims[1];
      return 0.5 * std::sqrt(x * x + y * y);
    }
  }
  throw std::invalid_argument("Invalid robot geometry type");
}
}  // namespace

GridPlanner::GridPlanner(const CollisionChecker::ShapeType &shape, const std::vector<float> &dims, bool allow_unknown,
                         float margin)
    : allow_unknown_(allow_unknown) {
  radius_ = circumscribedRadius(shape, dims) + static_cast<double>(margin);
  if (!(radius_ >= 0.0) || !std::isfinite(radius_)) throw std::invalid_argument("the footprint radius must be finite and >= 0");
  is_box_ = shape == CollisionChecker::ShapeType::BOX;
  if (is_box_) {
    box_x_ = static_cast<double>(dims[0]);
    box_y_ = static_cast<double>(dims[1]);
  }
  margin_ = static_cast<double>(margin);
  ctx_ = hip::make<hip::PlannerHandle>(kc_planner_create, 0);
}

void GridPlanner::setSpaceBoundsFromMap(float origin_x, float origin_y, int width, int height, float resolution) {
  if (!(resolution > 0.0f) || !std::isfinite(resolution)) throw std::invalid_argument("resolution must be a positive finite float");
  if (width <= 0 || height <= 0) throw std::invalid_argument("width and height must be positive");
  if (!std::isfinite(origin_x) || !std::isfinite(origin_y)) throw std::invalid_argument("the origin must be finite");
  if (have_grid_ && (width != width_ || height != height_)) have_grid_ = false;  // the grid of another map
  forgetSolve();  // a path of the last frame is not one of this frame
  ox_ = origin_x;
  oy_ = origin_y;
  width_ = width;
  height_ = height;
  res_ = resolution;
  have_bounds_ = true;
  applyClearanceCost();  // R2 and C2 are cells of this resolution
  applyModes();          // and so are A2 and B2, and the turn cells
}

void GridPlanner::setOrientedFootprint(bool on, float turn_cost) {
  uint32_t t10 = 0;
  if (on) {
    if (!is_box_) throw std::invalid_argument("the oriented footprint needs a BOX robot");
    if (clear_on_) throw std::invalid_argument("the oriented footprint cannot be combined with a clearance cost");
    const double t = static_cast<double>(turn_cost) * 10.0;
    if (!std::isfinite(t) || !(t >= 0.5) || !(t < 10000.5)) throw std::out_of_range("turn_cost must give a turn10 in 1 .. 10000");
    t10 = static_cast<uint32_t>(std::lround(t));
  }
  const bool was_on = oriented_on_;
  const uint32_t old_t10 = turn10_;
  oriented_on_ = on;
  turn10_ = t10;
  if (!have_bounds_) return;
  try {
    applyModes();
  } catch (...) {  // a refused footprint leaves the one before
    oriented_on_ = was_on;
    turn10_ = old_t10;
    throw;
  }
}

void GridPlanner::orientedA2B2(uint32_t *a2_out, uint32_t *b2_out) const {
  *a2_out = *b2_out = 0;
  if (!oriented_on_) return;
  needBounds();
  *a2_out = radiusToR2(box_x_ / 2.0 + margin_, res_);
  *b2_out = radiusToR2(box_y_ / 2.0 + margin_, res_);
}

// hands the box to the context when it is not the one the context holds, as applyClearanceCost does
void GridPlanner::applyOriented() {
  if (!oriented_on_ || car_on_) {  // with car motion the box goes to the context through applyCar
    if (oriented_applied_) {
      hip::check(kc_planner_set_oriented(ctx_.get(), 0, 0, 0));
      oriented_applied_ = false;
      forgetSolve();
    }
    return;
  }
  uint32_t a2 = 0, b2 = 0;
  orientedA2B2(&a2, &b2);
  if (a2 == 0) throw std::out_of_range("the box's half length is less than a cell: the oriented footprint has no length axis");
  if (oriented_applied_ && applied_a2_ == a2 && applied_b2_ == b2 && applied_turn10_ == turn10_) return;
  oriented_applied_ = false;
  hip::check(kc_planner_set_oriented(ctx_.get(), a2, b2, turn10_));
  oriented_applied_ = true;
  applied_a2_ = a2;
  applied_b2_ = b2;
  applied_turn10_ = turn10_;
  forgetSolve();
}

// the context holds one of the two state modes at a time: the one that leaves is switched off first
void GridPlanner::applyModes() {
  if (car_on_) {
    applyOriented();
    applyCar();
  } else {
    applyCar();
    applyOriented();
  }
}

void GridPlanner::setCarMotion(bool on, float min_turning_radius, bool allow_reverse, int reverse_weight, bool honour_goal_yaw) {
  if (on) {
    if (clear_on_) throw std::invalid_argument("car motion cannot be combined with a clearance cost");
    if (!std::isfinite(min_turning_radius) || !(min_turning_radius > 0.0f)) throw std::invalid_argument("min_turning_radius must be positive and finite");
    if (allow_reverse && (reverse_weight < 1 || reverse_weight > KC_PLANNER_MAX_REVERSE_WEIGHT))
      throw std::out_of_range("reverse_weight must be in 1 .. " + std::to_string(KC_PLANNER_MAX_REVERSE_WEIGHT));
    // refused before anything changes: the context keeps the mode it has
    if (have_bounds_) checkTurnCells(turnCells(static_cast<double>(min_turning_radius), static_cast<double>(res_)));
  }
  const bool was_on = car_on_, old_reverse = car_reverse_, old_goal = car_goal_yaw_;
  const double old_radius = car_radius_;
  const uint32_t old_rw = car_rw_;
  car_on_ = on;
  car_reverse_ = on && allow_reverse;
  car_goal_yaw_ = honour_goal_yaw;
  car_radius_ = on ? static_cast<double>(min_turning_radius) : 0.0;
  car_rw_ = car_reverse_ ? static_cast<uint32_t>(reverse_weight) : 0u;
  forgetSolve();  // the goal heading may count differently now
  if (!have_bounds_) return;
  try {
    applyModes();
  } catch (...) {  // a refused mode leaves the one before
    car_on_ = was_on;
    car_reverse_ = old_reverse;
    car_goal_yaw_ = old_goal;
    car_radius_ = old_radius;
    car_rw_ = old_rw;
    throw;
  }
}

void GridPlanner::checkTurnCells(int n) {
  if (n > KC_PLANNER_MAX_TURN_CELLS)
    throw std::out_of_range("a turning radius of " + std::to_string(n) + " turn cells is above the cap of " +
                            std::to_string(KC_PLANNER_MAX_TURN_CELLS) + ": plan on a coarser grid");
}

int GridPlanner::carTurnCells() const {
  if (!car_on_) return 0;
  needBounds();
  return turnCells(car_radius_, static_cast<double>(res_));
}

// hands the mode to the context when it is not the one the context holds, as applyClearanceCost does
void GridPlanner::applyCar() {
  if (!car_on_) {
    if (car_applied_) {
      hip::check(kc_planner_set_car(ctx_.get(), 0, 0, 0, 0));
      car_applied_ = false;
      forgetSolve();
    }
    return;
  }
  const int n = carTurnCells();
  uint32_t a2 = 0, b2 = 0;
  orientedA2B2(&a2, &b2);
  if (n > KC_PLANNER_MAX_TURN_CELLS || (oriented_on_ && a2 == 0)) {
    // new bounds the mode does not fit: the context drops the mode of the old ones, so that a solve says so instead of
    // planning with the old turn length
    if (car_applied_) {
      hip::check(kc_planner_set_car(ctx_.get(), 0, 0, 0, 0));
      car_applied_ = false;
      forgetSolve();
    }
    checkTurnCells(n);
    throw std::out_of_range("the box's half length is less than a cell: the oriented footprint has no length axis");
  }
  if (car_applied_ && applied_turn_ == n && applied_rw_ == car_rw_ && applied_car_a2_ == a2 && applied_car_b2_ == b2) return;
  car_applied_ = false;
  hip::check(kc_planner_set_car(ctx_.get(), n, car_rw_, a2, b2));
  car_applied_ = true;
  applied_turn_ = n;
  applied_rw_ = car_rw_;
  applied_car_a2_ = a2;
  applied_car_b2_ = b2;
  forgetSolve();
}

int GridPlanner::headingClass(double yaw) {
  const long q = std::lround(yaw / (M_PI / 4.0));
  return static_cast<int>(((q % 8) + 8) % 8);
}

int GridPlanner::turnCells(double radius, double resolution) {
  if (!std::isfinite(radius) || !(radius >= 0.0)) throw std::invalid_argument("the turning radius must be finite and >= 0");
  if (!std::isfinite(resolution) || !(resolution > 0.0)) throw std::invalid_argument("resolution must be positive and finite");
  const double n = std::ceil(radius / resolution * 0.41421356237309503);  // tan(pi / 8) as a literal: no libm result takes part
  if (!(n < 2147483647.0)) throw std::out_of_range("the turning radius is too many cells");
  return std::max(1, static_cast<int>(n));
}

int GridPlanner::orientationClass(double yaw) {
  const long q = std::lround(yaw / (M_PI / 4.0));
  return static_cast<int>(((q % 4) + 4) % 4);
}

std::vector<int32_t> GridPlanner::orientedMask(int k, uint32_t a2, uint32_t b2) {
  if (k < 0 || k > 3) throw std::invalid_argument("class " + std::to_string(k) + " is outside 0 .. 3");
  const uint64_t t2 = static_cast<uint64_t>(a2) + b2;
  if (t2 > static_cast<uint64_t>(KC_PLANNER_MAX_RADIUS_CELLS) * KC_PLANNER_MAX_RADIUS_CELLS)
    throw std::out_of_range("a turning disc of T2 = " + std::to_string(t2) + " is wider than " +
                            std::to_string(KC_PLANNER_MAX_RADIUS_CELLS) + " cells");
  int64_t r = 0;
  while (static_cast<uint64_t>((r + 1) * (r + 1)) <= t2) ++r;  // T2 contains every mask
  const int64_t A = a2, B = b2;
  std::vector<int32_t> out;
  for (int64_t dj = -r; dj <= r; ++dj)
    for (int64_t di = -r; di <= r; ++di) {
      const int64_t s = (di + dj) * (di + dj), d = (dj - di) * (dj - di);
      bool in = false;
      switch (k) {
        case 0: in = di * di <= A && dj * dj <= B; break;
        case 2: in = dj * dj <= A && di * di <= B; break;
        case 1: in = s <= 2 * A && d <= 2 * B; break;
        default: in = d <= 2 * A && s <= 2 * B; break;
      }
      if (in) {
        out.push_back(static_cast<int32_t>(di));
        out.push_back(static_cast<int32_t>(dj));
      }
    }
  return out;
}

void GridPlanner::setClearanceCost(float reach, float weight) {
  const bool on = reach > 0.0f && weight > 0.0f;
  if (on && oriented_on_) throw std::invalid_argument("a clearance cost cannot be combined with the oriented footprint");
  if (on && car_on_) throw std::invalid_argument("a clearance cost cannot be combined with car motion");
  if (on && (!std::isfinite(reach) || !std::isfinite(weight))) throw std::invalid_argument("reach and weight must be finite");
  uint32_t w10 = 0;
  if (on) {
    const double w = static_cast<double>(weight) * 10.0;
    if (!(w < 4294967295.0)) throw std::out_of_range("the clearance weight does not fit 32 bits");
    w10 = static_cast<uint32_t>(std::lround(w));
  }
  const bool was_on = clear_on_;
  const double old_reach = reach_;
  const uint32_t old_w10 = weight10_;
  clear_on_ = on && w10 > 0;
  reach_ = clear_on_ ? static_cast<double>(reach) : 0.0;
  weight10_ = clear_on_ ? w10 : 0u;
  if (!have_bounds_) return;
  try {
    applyClearanceCost();
  } catch (...) {  // a refused cost leaves the one before
    clear_on_ = was_on;
    reach_ = old_reach;
    weight10_ = old_w10;
    throw;
  }
}

uint32_t GridPlanner::clearanceC2() const {
  needBounds();
  return clear_on_ ? radiusToR2(radius_ + reach_, res_) : 0u;
}

// hands the table to the context when it is not the one the context holds: a call forgets the last solve and the
// validity map, so an unchanged table (the bounds of the same map again) is left alone
void GridPlanner::applyClearanceCost() {
  if (!clear_on_) {
    if (clear_applied_) {
      hip::check(kc_planner_set_clearance_cost(ctx_.get(), 0, nullptr, 0));
      clear_applied_ = false;
      forgetSolve();
    }
    return;
  }
  const uint32_t r2 = footprintR2(), c2 = clearanceC2();
  if (c2 > static_cast<uint32_t>(KC_PLANNER_MAX_RADIUS_CELLS) * KC_PLANNER_MAX_RADIUS_CELLS)
    throw std::out_of_range("the clearance reach is wider than " + std::to_string(KC_PLANNER_MAX_RADIUS_CELLS) + " cells");
  if (clear_applied_ && applied_r2_ == r2 && applied_c2_ == c2 && applied_w10_ == weight10_) return;
  const std::vector<uint32_t> table = clearanceTable(weight10_, r2, c2);
  clear_applied_ = false;
  hip::check(kc_planner_set_clearance_cost(ctx_.get(), c2, c2 ? table.data() : nullptr, c2 ? table.size() : 0));
  clear_applied_ = c2 > 0;  // a reach of less than a cell at radius 0: no cell is surcharged, the cost stays off
  applied_r2_ = r2;
  applied_c2_ = c2;
  applied_w10_ = weight10_;
  forgetSolve();
}

std::vector<uint32_t> GridPlanner::clearanceTable(uint32_t weight10, uint32_t r2, uint32_t c2) {
  if (c2 > static_cast<uint32_t>(KC_PLANNER_MAX_RADIUS_CELLS) * KC_PLANNER_MAX_RADIUS_CELLS)
    throw std::out_of_range("a clearance reach of C2 = " + std::to_string(c2) + " is wider than " +
                            std::to_string(KC_PLANNER_MAX_RADIUS_CELLS) + " cells");
  std::vector<uint32_t> t(static_cast<size_t>(c2) + 1, 0u);
  for (uint64_t d2 = static_cast<uint64_t>(r2) + 1; d2 <= c2; ++d2)
    t[d2] = static_cast<uint32_t>(static_cast<uint64_t>(weight10) * (c2 - d2) / (c2 - r2));
  return t;
}

void GridPlanner::needBounds() const {
  if (!have_bounds_) throw std::runtime_error("GridPlanner: set_space_bounds_from_map first");
}

void GridPlanner::setSpaceBoundsCheck(int width, int height) const {
  needBounds();
  if (width != width_ || height != height_)
    throw std::invalid_argument("the grid is " + std::to_string(width) + " x " + std::to_string(height) +
                                " cells, the map's bounds say " + std::to_string(width_) + " x " + std::to_string(height_));
}

void GridPlanner::waitForStream(void *stream) { hip::check(kc_planner_after_stream(ctx_.get(), stream)); }

// a new grid leaves nothing of the last solve: get_solution() is None and get_cost() infinite until the next one
void GridPlanner::forgetSolve() {
  status_ = -1;
  passes_ = 0;
  cost_ = 0xFFFFFFFFu;
  explored_ = false;
  components_ = 0;
  label_passes_ = 0;
}

void GridPlanner::setGrid(const void *host_grid, int elem_bytes) {
  needBounds();
  forgetSolve();
  hip::check(kc_planner_set_grid_host(ctx_.get(), host_grid, elem_bytes, width_, height_));
  have_grid_ = true;
}

void GridPlanner::setGridOnDevice(const void *dev_grid, int elem_bytes) {
  needBounds();
  forgetSolve();
  hip::check(kc_planner_set_grid_device(ctx_.get(), dev_grid, elem_bytes, width_, height_));
  have_grid_ = true;
}

void GridPlanner::setGridFromMapper(Mapping::LocalMapper &mapper) {
  const float res = mapper.resolution();
  // cell (i, j) of the mapper sits at ((i - c0) res, (j - c1) res): kc_dwa_set_grid_device's inverse of localToGrid
  setSpaceBoundsFromMap(-static_cast<float>(mapper.centralCell(0)) * res, -static_cast<float>(mapper.centralCell(1)) * res,
                        mapper.gridHeight(), mapper.gridWidth(), res);
  void *dev = nullptr;
  hip::check(kc_mapper_grid_device(mapper.hipContext(), &dev));
  hip::check(kc_mapper_sync(mapper.hipContext()));
  setGridOnDevice(dev, 4);
}

bool GridPlanner::setGridFromWorldMap(const Mapping::WorldMap &map) {
  const float ox = static_cast<float>(map.originX()), oy = static_cast<float>(map.originY());
  const bool moved = !have_bounds_ || ox != ox_ || oy != oy_ || map.width() != width_ || map.height() != height_ ||
                     map.resolution() != res_;
  if (moved) {
    setSpaceBoundsFromMap(ox, oy, map.width(), map.height(), map.resolution());
    if (have_problem_) setupProblem(problem_[0], problem_[1], problem_[2], problem_[3], problem_[4], problem_[5]);
  }
  setGridOnDevice(map.deviceGrid(), 1);
  return moved;
}

bool GridPlanner::worldToCell(float x, float origin, float resolution, int *cell) {
  const float q = (x - origin) / resolution;
  if (!std::isfinite(q) || std::fabs(q) >= 1073741824.0f) return false;
  *cell = static_cast<int>(q);
  return true;
}

uint32_t GridPlanner::radiusToR2(double radius, float resolution) {
  const double r = radius / static_cast<double>(resolution);
  const double r2 = std::floor(r * r * (1.0 + 1.0 / 1048576.0));
  if (!(r2 < 4294967296.0)) throw std::out_of_range("the footprint radius is too many cells");
  return static_cast<uint32_t>(r2);
}

uint32_t GridPlanner::footprintR2() const {
  needBounds();
  return radiusToR2(radius_, res_);
}

void GridPlanner::setupProblem(double start_x, double start_y, double start_yaw, double goal_x, double goal_y, double goal_yaw) {
  needBounds();
  const double problem[6] = {start_x, start_y, start_yaw, goal_x, goal_y, goal_yaw};
  std::copy(problem, problem + 6, problem_);
  start_class_ = std::isfinite(start_yaw) ? orientationClass(start_yaw) : 0;  // the oriented footprint's k0; it leaves goal_yaw unused
  start_heading_ = std::isfinite(start_yaw) ? headingClass(start_yaw) : 0;    // car motion's h0 and hg; a goal_yaw that is no number: any
  goal_heading_ = std::isfinite(goal_yaw) ? headingClass(goal_yaw) : -1;
  // a coordinate no cell holds is outside the grid
  if (!worldToCell(static_cast<float>(start_x), ox_, res_, &start_[0])) start_[0] = -1;
  if (!worldToCell(static_cast<float>(start_y), oy_, res_, &start_[1])) start_[1] = -1;
  if (!worldToCell(static_cast<float>(goal_x), ox_, res_, &goal_[0])) goal_[0] = -1;
  if (!worldToCell(static_cast<float>(goal_y), oy_, res_, &goal_[1])) goal_[1] = -1;
  have_problem_ = true;
  status_ = -1;
}

// what solve() and replan() start with
void GridPlanner::beginSolve() {
  if (!have_grid_) throw std::runtime_error("GridPlanner: no grid set");
  if (!have_problem_) throw std::runtime_error("GridPlanner: setup_problem first");
  forgetSolve();
  replanned_ = false;
  replan_threshold_ = 0xFFFFFFFFu;
}

uint32_t GridPlanner::minDistanceToCost(double min_distance_m, float resolution) {
  if (!(min_distance_m >= 0.0) || !std::isfinite(min_distance_m)) throw std::invalid_argument("min_distance must be finite and >= 0");
  const double c = min_distance_m / static_cast<double>(resolution) * 10.0;
  if (!(c < 4294967294.5)) throw std::out_of_range("min_distance is too many cells");
  return static_cast<uint32_t>(std::llround(c));
}

bool GridPlanner::explore(double robot_x, double robot_y, double min_distance_m, uint32_t min_size) {
  if (oriented_on_) throw std::invalid_argument("GridPlanner: no exploration with the oriented footprint on: a frontier is ranked by the disc's travel cost to a cell");
  if (clear_on_) throw std::invalid_argument("GridPlanner: no exploration with a clearance cost set: a frontier is ranked by plain travel cost");
  if (car_on_) throw std::invalid_argument("GridPlanner: no exploration with car motion on: a frontier is ranked by the disc's travel cost to a cell");
  needBounds();
  if (!have_grid_) throw std::runtime_error("GridPlanner: no grid set");
  const uint32_t min_cost = minDistanceToCost(min_distance_m, res_);
  forgetSolve();
  replanned_ = false;
  replan_threshold_ = 0xFFFFFFFFu;
  // a coordinate no cell holds is outside the grid.  The robot's cell is this call's own: the start and the goal of
  // the last setupProblem stay what they are for the next solve() or replan()
  int robot[2] = {-1, -1};
  if (!worldToCell(static_cast<float>(robot_x), ox_, res_, &robot[0])) robot[0] = -1;
  if (!worldToCell(static_cast<float>(robot_y), oy_, res_, &robot[1])) robot[1] = -1;
  size_t kept = 0;
  hip::check(kc_planner_explore(ctx_.get(), robot, footprintR2(), min_cost, min_size, &status_, &components_, &kept, &passes_, &label_passes_));
  explored_ = true;
  return status_ == KC_PLAN_FOUND;
}

std::vector<GridPlanner::Frontier> GridPlanner::frontiers() {
  std::vector<Frontier> out;
  if (!explored_) return out;
  size_t n = 0;
  hip::check(kc_planner_get_frontiers(ctx_.get(), nullptr, 0, &n));
  std::vector<kc_planner_frontier> rec(n);
  if (n) hip::check(kc_planner_get_frontiers(ctx_.get(), rec.data(), n, &n));
  out.reserve(n);
  for (const kc_planner_frontier &r : rec) {
    Frontier f;
    f.entry_i = r.entry_i;
    f.entry_j = r.entry_j;
    f.entry_x = cellToWorld(r.entry_i, ox_, res_);
    f.entry_y = cellToWorld(r.entry_j, oy_, res_);
    const double size = static_cast<double>(r.size);
    f.centroid_x = static_cast<float>(static_cast<double>(ox_) + static_cast<double>(r.sum_i) / size * static_cast<double>(res_));
    f.centroid_y = static_cast<float>(static_cast<double>(oy_) + static_cast<double>(r.sum_j) / size * static_cast<double>(res_));
    f.cost = static_cast<float>(r.cost) * res_ / 10.0f;
    f.size = r.size;
    f.root = r.root;
    out.push_back(f);
  }
  return out;
}

std::vector<int32_t> GridPlanner::frontierPathCells(size_t k) {
  if (!explored_) throw std::runtime_error("GridPlanner: frontier paths come after explore()");
  size_t n = 0;
  hip::check(kc_planner_get_frontier_path(ctx_.get(), k, nullptr, 0, &n));
  std::vector<int32_t> ij(2 * n);
  if (n) hip::check(kc_planner_get_frontier_path(ctx_.get(), k, ij.data(), n, &n));
  return ij;
}

std::optional<Path::Path> GridPlanner::frontierPath(size_t k) {
  return cellsToPath(frontierPathCells(k));
}

void GridPlanner::frontierLabels(uint32_t *labels_out, size_t cap) {
  if (!explored_) throw std::runtime_error("GridPlanner: frontier labels come after explore()");
  hip::check(kc_planner_get_frontier_labels(ctx_.get(), labels_out, cap));
}

bool GridPlanner::solve() {
  beginSolve();
  if (car_on_)
    hip::check(kc_planner_solve_car(ctx_.get(), start_, start_heading_, goal_, car_goal_yaw_ ? goal_heading_ : -1, footprintR2(),
                                    allow_unknown_ ? 1 : 0, &status_, &cost_, &passes_));
  else if (oriented_on_)
    hip::check(kc_planner_solve_oriented(ctx_.get(), start_, start_class_, goal_, allow_unknown_ ? 1 : 0, &status_, &cost_, &passes_));
  else
    hip::check(kc_planner_solve(ctx_.get(), start_, goal_, footprintR2(), allow_unknown_ ? 1 : 0, &status_, &cost_, &passes_));
  return status_ == KC_PLAN_FOUND;
}

bool GridPlanner::replan() {
  if (oriented_on_ || car_on_) return solve();  // the state fields are not kept (rules 20 and 35)
  beginSolve();
  hip::check(kc_planner_replan(ctx_.get(), start_, goal_, footprintR2(), allow_unknown_ ? 1 : 0, &status_, &cost_, &passes_));
  int kept = 0;
  hip::check(kc_planner_replan_info(ctx_.get(), &kept, &replan_threshold_, nullptr, nullptr));
  replanned_ = kept != 0;
  return status_ == KC_PLAN_FOUND;
}

bool GridPlanner::replan(const Mapping::WorldMap &map) {
  if (setGridFromWorldMap(map)) return solve();  // rule 51: replanned() says false
  return replan();
}

bool GridPlanner::goalWorld(double *x_out, double *y_out) const {
  if (!have_problem_) return false;
  *x_out = problem_[3];
  *y_out = problem_[4];
  return true;
}

void GridPlanner::cells(int start_out[2], int goal_out[2]) const {
  start_out[0] = start_[0];
  start_out[1] = start_[1];
  goal_out[0] = goal_[0];
  goal_out[1] = goal_[1];
}

std::vector<int32_t> GridPlanner::getPathCells(bool simplify) {
  std::vector<int32_t> ij;
  if (!havePath()) return ij;
  size_t n = 0;
  hip::check(kc_planner_get_path(ctx_.get(), nullptr, 0, &n));
  ij.resize(2 * n);
  if (n) hip::check(kc_planner_get_path(ctx_.get(), ij.data(), n, &n));
  if (!simplify || n < 3) return ij;
  // a cell goes when the step into it equals the step out of it: exactly collinear runs, nothing geometric
  std::vector<int32_t> out{ij[0], ij[1]};
  for (size_t k = 1; k + 1 < n; ++k) {
    const int32_t di0 = ij[2 * k] - ij[2 * k - 2], dj0 = ij[2 * k + 1] - ij[2 * k - 1];
    const int32_t di1 = ij[2 * k + 2] - ij[2 * k], dj1 = ij[2 * k + 3] - ij[2 * k + 1];
    if (di0 != di1 || dj0 != dj1) {
      out.push_back(ij[2 * k]);
      out.push_back(ij[2 * k + 1]);
    }
  }
  out.push_back(ij[2 * n - 2]);
  out.push_back(ij[2 * n - 1]);
  return out;
}

Path::Path GridPlanner::cellsToPath(const std::vector<int32_t> &ij) const {
  std::vector<Path::Point> pts;
  pts.reserve(ij.size() / 2);
  for (size_t k = 0; k + 1 < ij.size(); k += 2)
    pts.emplace_back(cellToWorld(ij[k], ox_, res_), cellToWorld(ij[k + 1], oy_, res_), 0.0f);
  return Path::Path(pts);
}

std::optional<Path::Path> GridPlanner::getPath(bool simplify) {
  if (!havePath()) return std::nullopt;
  return cellsToPath(getPathCells(simplify));
}

void GridPlanner::getField(uint32_t *field_out, uint8_t *valid_out, size_t cap) {
  if (status_ < 0) throw std::runtime_error("GridPlanner: no solve since the last grid or problem");
  hip::check(kc_planner_get_field(ctx_.get(), field_out, valid_out, cap));
}

float GridPlanner::getCost() const {
  if (!havePath()) return std::numeric_limits<float>::infinity();
  return static_cast<float>(cost_) * res_ / 10.0f;
}

float GridPlanner::getPathLength() {
  if (!havePath()) return std::numeric_limits<float>::infinity();
  const std::vector<int32_t> ij = getPathCells(false);
  uint64_t steps = 0;
  for (size_t k = 2; k + 1 < ij.size(); k += 2) steps += (ij[k] != ij[k - 2] && ij[k + 1] != ij[k - 1]) ? 14u : 10u;
  return static_cast<float>(steps) * res_ / 10.0f;
}

std::vector<int32_t> GridPlanner::getPathStates() {
  std::vector<int32_t> ijk;
  if (!havePath() || !(oriented_on_ || car_on_)) return ijk;
  size_t n = 0;
  if (car_on_) {
    hip::check(kc_planner_get_car_path(ctx_.get(), nullptr, nullptr, 0, &n));
    ijk.resize(3 * n);
    if (n) hip::check(kc_planner_get_car_path(ctx_.get(), ijk.data(), nullptr, n, &n));
    return ijk;
  }
  hip::check(kc_planner_get_oriented_path(ctx_.get(), nullptr, 0, &n));
  ijk.resize(3 * n);
  if (n) hip::check(kc_planner_get_oriented_path(ctx_.get(), ijk.data(), n, &n));
  return ijk;
}

std::vector<int32_t> GridPlanner::getPathMoves() {
  std::vector<int32_t> moves;
  if (!havePath() || !car_on_) return moves;
  size_t n = 0;
  hip::check(kc_planner_get_car_path(ctx_.get(), nullptr, nullptr, 0, &n));
  moves.resize(n ? n - 1 : 0);
  if (n > 1) hip::check(kc_planner_get_car_path(ctx_.get(), nullptr, moves.data(), n, &n));
  return moves;
}

void GridPlanner::getCarField(uint32_t *field8_out, uint8_t *moves8_out, uint8_t *valid_out, size_t cap) {
  if (status_ < 0) throw std::runtime_error("GridPlanner: no solve since the last grid or problem");
  hip::check(kc_planner_get_car_field(ctx_.get(), field8_out, moves8_out, valid_out, cap));
}

void GridPlanner::getOrientedField(uint32_t *field4_out, uint8_t *valid4_out, uint8_t *turn_valid_out, size_t cap) {
  if (status_ < 0) throw std::runtime_error("GridPlanner: no solve since the last grid or problem");
  hip::check(kc_planner_get_oriented_field(ctx_.get(), field4_out, valid4_out, turn_valid_out, cap));
}

std::vector<int32_t> GridPlanner::getAnyAngleCells(int max_span, std::vector<int32_t> *indices_out) {
  needDiscMode();
  std::vector<int32_t> ij;
  if (indices_out) indices_out->clear();
  if (!havePath()) return ij;
  size_t n = 0;
  hip::check(kc_planner_shortcut(ctx_.get(), max_span, &n, nullptr));
  ij.resize(2 * n);
  if (indices_out) indices_out->resize(n);
  hip::check(kc_planner_get_shortcut(ctx_.get(), ij.data(), indices_out ? indices_out->data() : nullptr, n, &n));
  return ij;
}

std::optional<Path::Path> GridPlanner::getAnyAnglePath(int max_span) {
  needDiscMode();
  if (!havePath()) return std::nullopt;
  return cellsToPath(getAnyAngleCells(max_span));
}

float GridPlanner::getAnyAngleLength(int max_span) {
  needDiscMode();
  if (!havePath()) return std::numeric_limits<float>::infinity();
  const std::vector<int32_t> ij = getAnyAngleCells(max_span);
  double sum = 0.0;
  for (size_t k = 2; k + 1 < ij.size(); k += 2) {
    const double dx = static_cast<double>(ij[k] - ij[k - 2]), dy = static_cast<double>(ij[k + 1] - ij[k - 1]);
    sum += std::sqrt(dx * dx + dy * dy);
  }
  return static_cast<float>(static_cast<double>(res_) * sum);
}

float GridPlanner::getAnyAngleMinClearance(int max_span) {
  needDiscMode();
  if (!havePath()) throw std::runtime_error("GridPlanner: no path");
  uint32_t c2 = KC_PLANNER_CLEAR_FAR;
  hip::check(kc_planner_shortcut(ctx_.get(), max_span, nullptr, &c2));
  if (c2 == KC_PLANNER_CLEAR_FAR) return std::numeric_limits<float>::infinity();
  return std::sqrt(static_cast<float>(c2)) * res_;
}

void GridPlanner::getClearance(uint16_t *clear2_out, uint32_t *pen_out, size_t cap) {
  if (status_ < 0) throw std::runtime_error("GridPlanner: no solve since the last grid or problem");
  hip::check(kc_planner_get_clearance(ctx_.get(), clear2_out, pen_out, cap));
}

float GridPlanner::getPathMinClearance() const {
  if (!havePath()) throw std::runtime_error("GridPlanner: no path");
  uint32_t c2 = KC_PLANNER_CLEAR_FAR;
  hip::check(kc_planner_path_clearance(ctx_.get(), &c2));
  if (c2 == KC_PLANNER_CLEAR_FAR) return std::numeric_limits<float>::infinity();
  return std::sqrt(static_cast<float>(c2)) * res_;
}

}  // namespace Planning
}  // namespace Kompass
