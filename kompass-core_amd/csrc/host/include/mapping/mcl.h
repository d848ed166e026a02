// Monte-Carlo localisation over a WorldMap (kc_mcl_*, csrc/kc_mcl.hip; DESIGN.md 4.11 rules 28 to 41).
//
// Nothing in the reference to restate: it leaves localisation, like the world-frame map, to its ROS side.  The particles
// live on the device and every step ray-casts the map in place; this class does the doubles at both ends: it quantises
// the pose, the odometry increment between two robot states, the measured ranges and the sigmas on the way in, and
// turns the step's record of exact integer sums into an estimate in metres and radians on the way out.  It also takes
// the resample decision (rule 40), in exact integers.
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "mapping/world_map.h"
#include "utils/hip_backend.h"

namespace Kompass {
namespace Mapping {

class MCL {
 public:
  // The sensor model the tables are built from.  Judgement, not measurement: nobody has tuned it on a robot.
  //   pen[i]  = lrint(pen_scale * -log(floor + (1 - floor) exp(-d^2 / (2 sigma^2)))), d = i << err_shift the bin's lower
  //             edge in 2^-16 cells, sigma = sigma_hit metres in the same unit: a Gaussian hit over a uniform floor
  //   wtab[i] = lrint(wtab0 * exp(-(i << w_shift) / temperature))
  struct Model {
    double sigma_hit = 0.1;
    int err_shift = 12, n_pen = 256;
    double floor = 0.05, pen_scale = 64.0;
    int w_shift = 4, n_w = 1024;
    uint32_t wtab0 = 1u << 16;
    double temperature = 256.0;
  };
  struct Tables {
    std::vector<uint16_t> pen;
    int err_shift = 0;
    std::vector<uint32_t> wtab;
    int w_shift = 0;
  };
  // The likelihood-field model (rules 44 and 45).  Judgement as well:
  //   pen_d2[d] = lrint(pen_scale * -log(floor + (1 - floor) exp(-d / (2 sigma_cells^2)))), d the squared distance in
  //               cells, 0 .. c2 = reach^2, sigma_cells = sigma_hit / resolution
  //   pen_far   = lrint(pen_scale * -log(floor))
  //   reach 0: ceil(3 sigma_hit / resolution) clipped to 1 .. 63; wtab as Model's
  struct FieldModel {
    double sigma_hit = 0.1;
    int reach = 0;
    double floor = 0.05, pen_scale = 64.0;
    int w_shift = 4, n_w = 1024;
    uint32_t wtab0 = 1u << 16;
    double temperature = 256.0;
  };
  struct FieldTables {
    std::vector<uint16_t> pen_d2;
    uint16_t pen_far = 0;
    int reach = 0;
    std::vector<uint32_t> wtab;
    int w_shift = 0;
  };
  struct Estimate {
    double x = 0.0, y = 0.0, yaw = 0.0;  // rule 39
    double n_eff = 0.0;                  // W1^2 / W2
    double spread = 0.0;                 // weighted std of position in metres, from the read-back (0 when not asked for)
    bool resampled = false;
    uint32_t best_cost = 0;              // amin
    int64_t txe = 0, tye = 0;            // the estimate's position in 2^-16 cells
    kc_mcl_record record = {};
    // rules 59 to 61, always filled.  fit: the step's mean penalty a contributing beam in 1 / 256, -1 when no beam
    // contributed; unlike n_eff, spread and best_cost it is absolute: a filter that is confidently wrong shows here.
    // fit_slow, fit_fast: its two running averages (0 until a step has primed them); injected: the slots the step's
    // resample drew anew over the free cells, 0 with recovery off.
    int64_t fit = -1, fit_slow = 0, fit_fast = 0;
    size_t injected = 0;
    uint32_t cost_min = 0, cost_best = 0;  // the smallest step cost, and the best particle's
    size_t beams_used = 0;                 // rule 60's B_used
  };
  // Rule 61's parameters.  Judgement, not measurement: nobody has tuned them on a robot.
  struct Recovery {
    int a_slow = 4, a_fast = 1;
    uint32_t max_num = 1, max_den = 4;  // at most this share of the particles is injected in one step
  };
  struct Particles {
    std::vector<int64_t> tx, ty;
    std::vector<uint32_t> h, acc;
  };

  // The map must outlive the localiser.  angles: the beams in the scan frame (a sensor's yaw offset folded in).
  MCL(const WorldMap &map, size_t n_particles, const std::vector<double> &angles, float range_max, uint64_t seed = 0);

  void setModel(const Model &m);
  void setTables(const Tables &t);
  // Switches to the field model; setModel / setTables switch back.  The particles survive.  When the map's distance
  // plane is off, or its reach is below the tables', it is enabled at the tables' reach (unknown_blocks as setFlags
  // last said).  The map is the caller's: the const reference is a promise not to change its cells, which holds.
  void setFieldModel(const FieldModel &m);
  void setFieldTables(const FieldTables &t);
  bool fieldModel() const { return field_; }
  // sigmas of the noise a step adds: metres forward and lateral, radians of heading
  void setMotionNoise(double sigma_forward, double sigma_lateral, double sigma_yaw);
  // resample when n_eff < N num / den (default 1 / 2); num = 0: never
  void setResampleRatio(uint32_t num, uint32_t den);
  void setFlags(bool unknown_blocks, bool skip_no_return);
  // Recovery by injected particles (rules 61 to 63), off by default.  On: a step whose fast average of the fit lies above
  // the slow one ends with a resample that draws some slots anew over the map's free cells.  The parameters are checked
  // as kc_mcl_recovery_update checks them; the averages keep running across either call.  Such a resample reads the map
  // on the device and the step waits for it (kc_mcl_resample_inject): the map may be written once step() is back.
  void setRecovery(const Recovery &r);
  void clearRecovery() { recovery_on_ = false; }
  bool recovery() const { return recovery_on_; }
  // whether step() reads the particles back for Estimate::spread (default: yes; one copy of N states a step)
  void setSpread(bool on) { spread_ = on; }

  void init(double x, double y, double yaw, double sigma_xy, double sigma_yaw);
  size_t initGlobal();
  // odometry from -> to ({x, y, yaw} each, any common frame), ranges: one a beam, in metres
  Estimate step(const std::array<double, 3> &from, const std::array<double, 3> &to, const std::vector<double> &ranges);
  // the same in the ABI's integers; resample: let rule 40 decide (false: never)
  Estimate stepQuantised(int64_t d_f, int64_t d_l, int32_t d_h, int32_t s_f, int32_t s_l, int32_t s_h,
                         const std::vector<int32_t> &zq, unsigned flags, bool resample);
  void resample();
  Particles particles() const;

  size_t size() const { return n_; }
  size_t beams() const { return beams_; }
  int64_t zmax() const { return zmax_; }
  kc_mcl *hipContext() const { return ctx_.get(); }

  // ---- the host side's arithmetic, static: needs no device ----
  static int32_t noiseScale(double sigma_units);  // rule 30: lrint(sigma * 65536 / sqrt((65536^2 - 1) / 3))
  static uint32_t quantiseHeading(double yaw);    // lrint(yaw / 2 pi * 65536) & 0xFFFF
  static std::vector<int32_t> quantiseRanges(const std::vector<double> &ranges, float resolution, float range_max, unsigned flags);
  // (d_f, d_l, d_h): the displacement from -> to in from's frame in 2^-16 cells, the turn in heading units
  static std::array<int64_t, 3> odometryIncrement(float resolution, const std::array<double, 3> &from, const std::array<double, 3> &to);
  static Tables sensorTables(float resolution, const Model &m);
  static FieldTables fieldTables(float resolution, const FieldModel &m);
  static Estimate estimateOf(const kc_mcl_record &r, float resolution, double origin_x, double origin_y);
  static bool shouldResample(const kc_mcl_record &r, size_t n, uint32_t num, uint32_t den);

 private:
  using Handle = hip::Handle<kc_mcl, kc_mcl_destroy>;
  const WorldMap &map_;
  size_t n_, beams_;
  float range_max_;
  int64_t zmax_ = 0;
  Handle ctx_;
  Tables tables_;
  int32_t s_f_ = 0, s_l_ = 0, s_h_ = 0;
  uint32_t r_num_ = 1, r_den_ = 2;
  unsigned flags_ = 0;
  bool spread_ = true;
  bool field_ = false;
  bool recovery_on_ = false;
  Recovery recovery_;
  kc_mcl_recovery fit_state_ = {};  // un-primed by either init

  double spreadOf(const Estimate &e) const;
};

}  // namespace Mapping
}  // namespace Kompass
