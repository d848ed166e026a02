// MoverTracker: the statement of tests/worldmap_movers_ref.py in C++, operation for operation (see the header).
#include "mapping/mover_tracker.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace Kompass {
namespace Mapping {

MoverTracker::MoverTracker(const MoverTrackerConfig &config) : cfg_(config) {
  if (!(config.alpha >= 0.0 && config.alpha <= 1.0) || !(config.beta >= 0.0) || !std::isfinite(config.beta))
    throw std::invalid_argument("MoverTracker: alpha must lie in 0 .. 1 and beta be finite and not negative");
  if (config.max_misses < 0) throw std::invalid_argument("MoverTracker: max_misses must not be negative");
  if (!(config.gate >= 0.0)) throw std::invalid_argument("MoverTracker: the gate must not be negative");
}

void MoverTracker::update(const std::vector<MoverCluster> &clusters, double dt) {
  if (!(dt > 0.0) || !std::isfinite(dt)) throw std::invalid_argument("MoverTracker: dt must be positive");
  std::vector<char> used(clusters.size(), 0);
  std::vector<Track> kept;
  kept.reserve(tracks_.size() + clusters.size());
  for (Track tr : tracks_) {
    const double px = tr.x + tr.vx * dt, py = tr.y + tr.vy * dt;
    long best = -1;
    double best_d = 0.0;
    for (size_t i = 0; i < clusters.size(); ++i) {
      if (used[i]) continue;
      const double d = std::hypot(clusters[i].x - px, clusters[i].y - py);
      if (d <= cfg_.gate && (best < 0 || d < best_d)) {  // the lowest index among equals
        best = static_cast<long>(i);
        best_d = d;
      }
    }
    if (best < 0) {  // coasts
      tr.x = px;
      tr.y = py;
      if (++tr.misses <= cfg_.max_misses) kept.push_back(tr);
      continue;
    }
    used[static_cast<size_t>(best)] = 1;
    const MoverCluster &z = clusters[static_cast<size_t>(best)];
    if (tr.hits == 1) {  // the two-point start: an exactly linear input is tracked exactly
      tr.vx = (z.x - tr.x) / dt;
      tr.vy = (z.y - tr.y) / dt;
      tr.x = z.x;
      tr.y = z.y;
    } else {
      const double rx = z.x - px, ry = z.y - py;
      tr.x = px + cfg_.alpha * rx;
      tr.y = py + cfg_.alpha * ry;
      tr.vx = tr.vx + cfg_.beta / dt * rx;
      tr.vy = tr.vy + cfg_.beta / dt * ry;
    }
    tr.radius = std::max(tr.radius, z.radius);
    tr.hits += 1;
    tr.misses = 0;
    kept.push_back(tr);
  }
  for (size_t i = 0; i < clusters.size(); ++i) {  // the clusters left over, in cluster order
    if (used[i]) continue;
    Track tr;
    tr.id = next_id_++;
    tr.x = clusters[i].x;
    tr.y = clusters[i].y;
    tr.radius = clusters[i].radius;
    kept.push_back(tr);
  }
  tracks_.swap(kept);
}

std::vector<Control::MovingObstacle> MoverTracker::movingObstacles() const {
  std::vector<Control::MovingObstacle> out;
  out.reserve(tracks_.size());
  for (const Track &t : tracks_) out.push_back({t.x, t.y, t.vx, t.vy, t.radius});
  return out;
}

std::vector<uint8_t> MoverTracker::skipMask(const std::vector<int32_t> &labels) {
  std::vector<uint8_t> out(labels.size());
  for (size_t k = 0; k < labels.size(); ++k) out[k] = labels[k] >= 0 ? 1 : 0;
  return out;
}

void MoverTracker::clear() {
  tracks_.clear();
  next_id_ = 0;
}

}  // namespace Mapping
}  // namespace Kompass
