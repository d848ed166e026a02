// Tracks the clusters WorldMap::detectMovers finds from scan to scan and hands them to the MPPI controller as moving
// discs (the tracker behind rules 64 to 70; stated in tests/worldmap_movers_ref.py).  Host only, in
// doubles; nothing in the reference to restate.
//
// An alpha-beta filter a track with a two-point start, greedy nearest-neighbour association in track order.  Not built:
// association better than that, accelerating movers, settling a long-stationary track into the map.
#pragma once

#include <cstdint>
#include <vector>

#include "controllers/mppi.h"
#include "mapping/world_map.h"

namespace Kompass {
namespace Mapping {

// The prototype's values: judgement, not measurement
struct MoverTrackerConfig {
  double alpha = 0.5;   // the share of a residual that moves the position
  double beta = 0.3;    // ... and, over dt, the velocity
  int max_misses = 3;   // a track unmatched for more updates in a row than this is dropped
  double gate = 6.0;    // the furthest a cluster may lie from a track's prediction, in the clusters' length unit
};

class MoverTracker {
 public:
  struct Track {
    uint64_t id = 0;
    double x = 0.0, y = 0.0, vx = 0.0, vy = 0.0, radius = 0.0;  // radius: the largest seen
    int hits = 1, misses = 0;
  };

  explicit MoverTracker(const MoverTrackerConfig &config = MoverTrackerConfig());

  // One scan's clusters, dt > 0 after the last (std::invalid_argument otherwise).  The tracks in creation order: each
  // predicts p = x + v dt and takes the nearest cluster no earlier track took within `gate` of p, the lowest index among
  // equals.  On its second sighting v = (z - x) / dt, x = z; afterwards, with r = z - p: x = p + alpha r, v += beta / dt
  // r.  A track without a cluster coasts, x = p, and is dropped after max_misses such updates in a row.  The clusters
  // left over open tracks in cluster order, with increasing ids.
  void update(const std::vector<MoverCluster> &clusters, double dt);
  void update(const MoverDetection &detection, double dt) { update(detection.clusters, dt); }
  const std::vector<Track> &tracks() const { return tracks_; }
  // a disc for every live track, as MPPI::setMovingObstacles takes them
  std::vector<Control::MovingObstacle> movingObstacles() const;
  // one entry a beam, 1 for the member beams of every kept cluster (label >= 0): WorldMap::integrateScan's skip
  static std::vector<uint8_t> skipMask(const std::vector<int32_t> &labels);
  void clear();

 private:
  MoverTrackerConfig cfg_;
  std::vector<Track> tracks_;
  uint64_t next_id_ = 0;
};

}  // namespace Mapping
}  // namespace Kompass
