// MPPI path follower over a WorldMap's distance plane (kc_mppi_*, csrc/kc_mppi.hip).
//
// Nothing in the reference to restate: its controllers commit to one velocity for the whole look-ahead.  The samples,
// their roll-outs and the blend run on the device in the ABI's integers; this class does the doubles at both ends.  It
// quantises the limits, the sigmas, the pose and the path window once each, keeps the nominal sequence between steps
// (the warm start: shifted by one after every step) and turns the first control of the new sequence into a command.
// Path, closest point and goal test are the Follower's.
//
// Moving obstacles (rules 13 to 18): a list of discs with a velocity in the world, kept until replaced or cleared, and
// quantised at every step against the map's origin of that step.  The device costs each at the time of each roll-out
// step; finding them, and keeping them out of the map's cells, is the caller's.
//
// The grid planner's cost field (rules 19 to 24): setCostField attaches a GridPlanner, and from then on a step needs no
// path and builds no window.  The device reads the planner's kept cost-to-go field where it lies: every state a sample
// reaches pays for how far it still is from the goal, not for how far it is from a polyline.  The planner must have
// solved (or replanned) on this map at its present window offset; that is the caller's to see to (the Python front end
// checks it).
//
// Acceleration limits (rules 25 to 29): with MPPIConfig.acceleration_limits every sample is rolled out by the control the
// robot can apply, from the velocity this class applied last.  The command is then the first applied control of the new
// sequence (kc_mppi_apply_rates), kept as integers for the next step; restrictVelocityTolimits plays no part.
//
// A box footprint (rules 30 to 36): setBoxFootprint(length, width) covers the box by up to eight equal discs along its
// length axis, the pose at its centre (footprintOf, rule 36), and every state of a roll-out is a hit when any disc is, at
// the state's own heading.  The discs' r2 stands in the place of hit_radius' while the box is set; the offsets are formed
// again when the map's resolution changes.
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "datatypes/tracking.h"

#include "controllers/follower.h"
#include "mapping/world_map.h"
#include "planning/grid_planner.h"
#include "utils/hip_backend.h"

namespace Kompass {
namespace Control {

// Judgement, not measurement: the values of the closed-loop scene of DESIGN.md 4.12, which nobody has tuned on a robot.
// Lengths are in cells of the map, a step is the control time step.
struct MPPIConfig {
  size_t samples = 1024, horizon = 32, window = 96;  // K, T, M
  double sigma_forward = 0.5, sigma_lateral = 0.5;   // cells a step (lateral: OMNI only)
  double sigma_turn = 500.0 / 65536.0 * 2.0 * M_PI;  // radians a step
  double lambda = 64.0;                              // temperature: wtab[i] = lrint(65535 exp(-(i << w_shift) / lambda))
  int w_shift = 2, n_w = 256;
  double hit_radius = 3.0;                           // cells: r2 = lrint(hit_radius^2)
  double clearance = 7.0;                            // cells: c2 = lrint(clearance^2)
  double clearance_weight = 60.0;                    // pen_d2[d] = lrint(weight max(0, 1 - sqrt(d) / clearance))
  uint16_t pen_far = 0;
  uint32_t pen_hit = 4000, w_path = 8, w_goal = 20;
  double path_cap = 20.0;                            // cells: qcap = lrint(path_cap^2) << 16
  int reach = 8;                                     // the plane's reach when this class has to enable it
  bool allow_reverse = false;                        // F_lo = -F_hi instead of 0
  double min_turning_radius = 0.5;                   // metres, ACKERMANN only: kq = lrint(65536 / (2 pi R / resolution))
  uint64_t seed = 0;
  // Moving obstacles.  Judgement too, and tried only on the crossing scene of DESIGN.md 4.12: a mover is hit inside
  // hit_radius + its own radius (cells), the ramp starts mover_margin cells farther out and is mover_weight at its top
  double mover_margin = 4.0;                         // cells
  double mover_weight = 200.0;
  uint32_t mover_hit_penalty = 4000;
  // The planner's cost field (rules 19 to 21; the field counts 10 a straight cell).  Judgement, not tuning: the values
  // the two scenes of DESIGN.md 4.12 were tried with
  uint32_t field_run_weight = 32;                    // w_run: a state adds (fc w_run) >> 8
  uint32_t field_goal_weight = 2;                    // w_term: the last state adds w_term fl
  uint32_t field_cap = 1u << 20;                     // fcap: an unreachable cell costs as one this far away
  // Rules 25 to 29: roll every sample out under the control limits' accelerations.  Off: the step of rules 1 to 24
  bool acceleration_limits = false;
  // Rule 36's margin in cells around the discs of a box footprint: sqrt(2) rounded up to half a cell.  Derived, not
  // judged: a disc centre lies within sqrt(2) / 2 of its cell's centre and an occupied cell reaches
  // sqrt(2) / 2 beyond its own
  double footprint_margin = 1.5;
};

// A disc that moves in a straight line: world metres and m/s at the time of the state handed to execute()
struct MovingObstacle {
  double x = 0.0, y = 0.0, vx = 0.0, vy = 0.0, radius = 0.0;
};

class MPPI : public Follower {
 public:
  using Config = MPPIConfig;
  struct Quantised {  // what a step hands to kc_mppi_set_model
    int32_t f_lo = 0, f_hi = 0, l_hi = 0, h_hi = 0, kq = 0;
    std::array<int32_t, 3> s = {0, 0, 0};
    // rule 25's rates (F_up, F_dn, L_up, L_dn, H_up, H_dn), formed while acceleration_limits is set
    std::array<int32_t, 6> rates = {1, 1, 1, 1, 1, 1};
  };
  struct Costs {  // ... and to kc_mppi_set_costs
    uint32_t r2 = 0;
    std::vector<uint16_t> pen_d2;
    uint16_t pen_far = 0;
    uint32_t pen_hit = 0, w_path = 0;
    uint64_t qcap = 0;
    uint32_t w_goal = 0;
    std::vector<uint32_t> wtab;
    int w_shift = 0;
  };
  struct Footprint {  // rule 36: what a box hands to kc_mppi_set_footprint, and the r2 that goes with it
    std::vector<int32_t> offsets;  // 16 fraction bits of a cell, along the forward axis from the pose
    uint32_t r2 = 0;
    double rho = 0.0;              // cells: the radius at which the discs cover the box
  };
  struct Movers {  // ... and to kc_mppi_set_movers
    std::vector<int64_t> ox, oy;
    std::vector<int32_t> vx, vy;
    std::vector<uint64_t> hq, sq, g;
    uint32_t pen_hit = 0;
    size_t dropped = 0;  // obstacles beyond the 64 nearest
  };
  struct Inputs {  // the last step's, as the device took them
    int64_t tx = 0, ty = 0;
    uint32_t h = 0, step = 0;
    std::vector<int64_t> px, py;
    std::vector<int32_t> u;  // T x 3
    Movers movers;
    bool field = false;      // a cost field was attached: px, py are empty
    bool limited = false;    // rules 25 to 29 were on: rates and v0 are what the device took
    std::array<int32_t, 6> rates = {0, 0, 0, 0, 0, 0};
    std::array<int32_t, 3> v0 = {0, 0, 0};
    std::vector<int32_t> offsets;  // rule 30's list while a box is set, empty otherwise
    uint32_t r2 = 0;               // rule 5's r2 of the step: the footprint's while a box is set, hit_radius' otherwise
  };

  MPPI(ControlType type, const ControlLimitsParams &limits, double time_step, const Config &config = Config());

  // One step at the robot's state over `map` (which must outlive the controller's use of it).  The map's distance plane
  // is enabled at config.reach when it is off or too short for the clearance; the map's cells are not changed.
  Controller::Result execute(const Mapping::WorldMap &map, const Path::State &state);
  void resetSequence();
  // The planner's kept cost field in the place of the path (rules 19 to 24), from the next execute() on and until
  // clearCostField().  The planner must outlive the attachment, and its last solve-type call at every execute() must be
  // solve() or replan() in disc mode on this map at its present offset.  execute() then needs no path: its goal test is
  // the follower's goal tolerance around the planner's goal.
  void setCostField(Planning::GridPlanner &planner);
  void clearCostField();
  bool hasCostField() const { return field_ != nullptr; }
  // A box of length x width metres, the pose at its centre and the length along the heading, from the next execute() on
  // and until clearFootprint() (rules 30 to 36).  std::invalid_argument for a size that is not positive and finite;
  // execute() throws std::invalid_argument naming `clearance` when the discs' r2 is above the clearance's c2
  void setBoxFootprint(double length, double width);
  void clearFootprint();
  bool hasBoxFootprint() const { return box_; }
  // f0 of the last step in field mode: the field's value at the robot's cell, in the planner's units (10 a straight
  // cell); 0xFFFFFFFF when the robot stands in an invalid or cut-off cell or outside the map, and before such a step.
  // The controller does not refuse then: the caller decides
  uint32_t fieldAtRobot() const { return f0_; }
  uint32_t fieldNominal() const { return f_nom_; }  // f_nom: the field where the nominal sequence's roll-out ended
  // The moving obstacles of the steps to come, at the time of the state of the next execute(); kept until replaced or
  // cleared (an empty list).  More than 64: the 64 nearest to the robot are kept at every step, logged once.
  void setMovingObstacles(std::vector<MovingObstacle> obstacles);
  const std::vector<MovingObstacle> &movingObstacles() const { return movers_; }
  // A tracked box that already lies in the world frame: its centre, its velocity, half its footprint's diagonal
  static MovingObstacle fromTrackedBox(const TrackedBbox3D &box);

  const Config &mppiConfig() const { return cfg_; }
  double timeStep() const { return dt_; }
  const Inputs &lastInputs() const { return in_; }
  const std::vector<int32_t> &lastSequence() const { return out_; }  // U' of the last step, T x 3
  // With acceleration_limits: rule 28's applied sequence of U', T x 3 (empty otherwise), and the applied triple the last
  // command was formed from, which is the next step's V0: zero at the first step, after resetSequence() and when the
  // map's resolution changes
  const std::vector<int32_t> &lastApplied() const { return applied_; }
  const std::array<int32_t, 3> &lastVelocity() const { return v0_; }
  const kc_mppi_record &lastRecord() const { return rec_; }
  // the first n controls of U' as velocities (vx, vy, omega each); with acceleration_limits, of its applied sequence
  std::vector<std::array<double, 3>> controls(size_t n) const;
  // U' (with acceleration_limits its applied sequence) rolled out on the host by rule 4 from the last step's pose: (x,
  // y, yaw) in the world after each step
  std::vector<std::array<double, 3>> predictedPath() const;
  std::vector<uint32_t> sampleCosts() const;
  kc_mppi *hipContext() const { return ctx_.get(); }

  // ---- the host side's arithmetic, static: needs no device ----
  // quantise() forms rule 25's rates beside the box: lrint(a dt^2 / res 65536) from velXParams and velYParams, lrint(a
  // dt^2 / (2 pi) 65536) from omegaParams, maxAcceleration for up and maxDeceleration for dn, clamped into rule 25's range
  static Quantised quantise(ControlType type, const ControlLimitsParams &limits, double time_step, float resolution, const Config &c);
  static Costs costsOf(const Config &c);
  // The list in rule 13's integers against the origin (ox, oy): positions as the pose is quantised, V = llrint(v dt / res
  // 65536), hq = llrint((hit_radius + radius / res)^2 65536), sq likewise with + mover_margin, g = floor(mover_weight
  // 65536 / (((sq - hq) >> 16) + 1)).  (x, y): the robot, which picks the 64 nearest when there are more.  A quantity
  // beyond rule 13's bounds throws std::out_of_range naming the mover.
  // hit_cells >= 0 stands in the place of c.hit_radius: rho + margin while a box is set
  static Movers moversOf(const std::vector<MovingObstacle> &obstacles, double time_step, float resolution, double ox, double oy,
                         double x, double y, const Config &c, double hit_cells = -1.0);
  // Rule 36: a = length / (2 res), b = width / (2 res) cells; n = min(8, max(1, ceil(a / b))), s = 2 a / n, o_i =
  // llrint((-a + s / 2 + i s) 65536), rho = sqrt(b^2 + (s / 2)^2), r2 = ceil((rho + margin)^2).  std::invalid_argument
  // for a size, resolution or margin that is not finite or not positive (the margin may be 0), std::out_of_range for
  // an offset beyond rule 30's 2^22
  static Footprint footprintOf(double length_m, double width_m, float resolution, double margin_cells);

 private:
  using Handle = hip::Handle<kc_mppi, kc_mppi_destroy>;
  Config cfg_;
  double dt_;
  Handle ctx_;
  const kc_worldmap *bound_ = nullptr;  // the map ctx_ was made over
  float res_ = 0.0f;
  double ox_ = 0.0, oy_ = 0.0;          // the origin the last step quantised against
  std::vector<int32_t> u_, out_;
  std::vector<int32_t> applied_;            // rule 28's sequence of out_, while the mode is on
  std::array<int32_t, 3> v0_ = {0, 0, 0};   // what the robot was last told, in rule 2's units
  bool rates_on_device_ = false;            // ctx_ holds rates
  const std::vector<int32_t> &shown() const { return applied_.empty() ? out_ : applied_; }
  uint32_t step_ = 0;
  Inputs in_;
  kc_mppi_record rec_ = {};
  std::vector<MovingObstacle> movers_;
  bool movers_on_device_ = false, logged_drop_ = false;
  Planning::GridPlanner *field_ = nullptr;  // the attached planner, not owned
  bool field_on_device_ = false;            // ctx_ holds an attachment
  uint32_t f0_ = 0xFFFFFFFFu, f_nom_ = 0xFFFFFFFFu;
  bool box_ = false;                        // a box is set: box_len_ x box_wid_ metres
  double box_len_ = 0.0, box_wid_ = 0.0;
  bool footprint_on_device_ = false;        // ctx_ holds a footprint
  uint32_t r2_on_device_ = 0;               // the r2 ctx_'s costs were set with

  void bind(const Mapping::WorldMap &map);
  void buildWindow(const Mapping::WorldMap &map);
};

}  // namespace Control
}  // namespace Kompass
