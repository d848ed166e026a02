// Image-only target follower of the kompass_cpp surface (reference:
// controllers/rgb_follower.{h,cpp}): a proportional law on a 2-D box's size
// and centre, with a wait or search behaviour when the box is lost.  Host
// logic only.
#pragma once

#include <array>
#include <memory>
#include <optional>
#include <queue>

#include "datatypes/control.h"
#include "datatypes/parameter.h"
#include "datatypes/tracking.h"
#include "datatypes/trajectory.h"

namespace Kompass {
namespace Control {

class RGBFollower {
 public:
  class RGBFollowerConfig : public Parameters {
   public:
    RGBFollowerConfig() {
      addParameter("control_time_step", Parameter(0.1, 1e-4, 1e6, "Control time step (s)"));
      addParameter("tolerance", Parameter(0.1, 0.0, 1.0, "Tolerance value"));
      // -1 for None
      addParameter("target_distance",
                   Parameter(0.1, -1.0, 1e9, "Target distance to maintain with the target (m)"));
      addParameter("target_wait_timeout", Parameter(30.0, 0.0, 1e3));
      addParameter("target_search_timeout", Parameter(30.0, 0.0, 1e3));
      addParameter("target_search_radius", Parameter(0.5, 1e-4, 1e4));
      addParameter("target_search_pause", Parameter(1.0, 0.0, 1e3));
      addParameter("rotation_gain", Parameter(1.0, 1e-2, 10.0));
      addParameter("speed_gain", Parameter(1.0, 1e-2, 10.0));
      addParameter("min_vel", Parameter(0.1, 1e-9, 1e9));
      addParameter("enable_search", Parameter(false));
    }
    bool enable_search() const { return getParameter<bool>("enable_search"); }
    double control_time_step() const { return getParameter<double>("control_time_step"); }
    double target_search_timeout() const { return getParameter<double>("target_search_timeout"); }
    double target_wait_timeout() const { return getParameter<double>("target_wait_timeout"); }
    double target_search_radius() const { return getParameter<double>("target_search_radius"); }
    double search_pause() const { return getParameter<double>("target_search_pause"); }
    double tolerance() const { return getParameter<double>("tolerance"); }
    double target_distance() const {
      const double val = getParameter<double>("target_distance");
      return val < 0 ? -1.0 : val;
    }
    void set_target_distance(double value) { setParameter("target_distance", value); }
    double K_omega() const { return getParameter<double>("rotation_gain"); }
    double K_v() const { return getParameter<double>("speed_gain"); }
    double min_vel() const { return getParameter<double>("min_vel"); }
  };

  // (vx, vy, omega) of one queued search step
  using SearchCommand = std::array<double, 3>;

  RGBFollower(const ControlType robotCtrlType, const ControlLimitsParams ctrl_limits,
              const RGBFollowerConfig config = RGBFollowerConfig());
  virtual ~RGBFollower() = default;

  void resetTarget(const Bbox2D &tracking);
  bool run(const std::optional<Bbox2D> tracking);
  const TrajectoryVelocities2D getCtrl() const;
  Eigen::Vector2f getErrors() const { return Eigen::Vector2f(dist_error_, orientation_error_); }

  // the search commands still queued, front first (not in the reference's interface)
  std::vector<SearchCommand> pendingSearchCommands() const;

 protected:
  bool rotate_in_place_ = false;
  ControlLimitsParams ctrl_limits_;
  double recorded_search_time_ = 0.0, recorded_wait_time_ = 0.0;
  std::queue<SearchCommand> search_commands_queue_;
  SearchCommand search_command_{0.0, 0.0, 0.0};
  std::unique_ptr<Bbox2D> last_tracking_ = nullptr;
  float dist_error_ = 0.0f, orientation_error_ = 0.0f;

  void generateSearchCommands(float total_rotation, float search_radius, float max_rotation_time,
                              bool enable_pause = false);
  void getFindTargetCmds(const int last_direction = 1);

 private:
  RGBFollowerConfig config_;
  TrajectoryVelocities2D out_vel_;

  void trackTarget(const Bbox2D &tracking);
};

}  // namespace Control
}  // namespace Kompass
