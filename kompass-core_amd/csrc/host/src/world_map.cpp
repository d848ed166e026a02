// WorldMap host side: argument plumbing over kc_worldmap_* (no reference counterpart, see the header).
#include "mapping/world_map.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>

namespace Kompass {
namespace Mapping {

WorldMap::WorldMap(int width, int height, float resolution, double origin_x, double origin_y)
    : width_(width), height_(height), res_(resolution), ox_(origin_x), oy_(origin_y),
      ctx_(hip::make<hip::WorldMapHandle>(kc_worldmap_create, 0, width, height, resolution, origin_x, origin_y)) {}

void WorldMap::setModel(int hit, int miss, int e_min, int e_max, int occ_thr) {
  hip::check(kc_worldmap_set_model(ctx_.get(), hit, miss, e_min, e_max, occ_thr));
  last_ = {0, -1, -1, -1, -1};
}

void WorldMap::setPrior(const void *host_grid, int elem_bytes, int width, int height) {
  hip::check(kc_worldmap_set_prior_host(ctx_.get(), host_grid, elem_bytes, width, height));
  last_ = {0, -1, -1, -1, -1};
}

void WorldMap::setPriorOnDevice(const void *dev_grid, int elem_bytes, int width, int height) {
  hip::check(kc_worldmap_set_prior_device(ctx_.get(), dev_grid, elem_bytes, width, height));
  last_ = {0, -1, -1, -1, -1};
}

void WorldMap::waitForStream(void *stream) { hip::check(kc_worldmap_after_stream(ctx_.get(), stream)); }

kc_worldmap_pose WorldMap::quantisePose(float resolution, double origin_x, double origin_y, double x, double y, double yaw) {
  kc_worldmap_pose p{};
  hip::check(kc_worldmap_quantise_pose(resolution, origin_x, origin_y, x, y, yaw, &p));
  return p;
}

// the mapper's central cell (local_mapper.h)
WorldMap::GridSource::GridSource(Kind k, const int32_t *g, int grid_height, int grid_width)
    : kind(k), mapper(nullptr), grid(g), height(grid_height), width(grid_width), central_i(grid_height / 2 - 1),
      central_j(grid_width / 2 - 1) {}

uint32_t WorldMap::updateFrom(const GridSource &s, const kc_worldmap_pose &p) {
  if (s.kind == GridSource::Mapper) {
    hip::check(kc_worldmap_update_from_mapper(ctx_.get(), s.mapper->hipContext(), &p, &last_));
  } else {
    const auto entry = s.kind == GridSource::Host ? kc_worldmap_update_host : kc_worldmap_update_device;
    hip::check(entry(ctx_.get(), s.grid, s.height, s.width, s.central_i, s.central_j, res_, &p, &last_));
  }
  return last_.changed;
}

uint32_t WorldMap::update(const LocalMapper &mapper, double x, double y, double yaw) {
  return updateFrom(mapper, quantisePose(res_, ox_, oy_, x, y, yaw));
}

uint32_t WorldMap::update(const int32_t *grid, int grid_height, int grid_width, double x, double y, double yaw) {
  return updateFrom({GridSource::Host, grid, grid_height, grid_width}, quantisePose(res_, ox_, oy_, x, y, yaw));
}

uint32_t WorldMap::updateOnDevice(const int32_t *dev_grid, int grid_height, int grid_width, double x, double y, double yaw) {
  return updateFrom({GridSource::Device, dev_grid, grid_height, grid_width}, quantisePose(res_, ox_, oy_, x, y, yaw));
}

uint32_t WorldMap::updateAt(const LocalMapper &mapper, const kc_worldmap_pose &pose) { return updateFrom(mapper, pose); }

uint32_t WorldMap::updateAt(const int32_t *grid, int grid_height, int grid_width, const kc_worldmap_pose &pose) {
  return updateFrom({GridSource::Host, grid, grid_height, grid_width}, pose);
}

WorldMap::Match WorldMap::matchFrom(const GridSource &s, double x, double y, double yaw, int n_yaw, double yaw_step, int reach) {
  hip::check(kc_worldmap_match_check_window(n_yaw, yaw_step, reach));
  const kc_worldmap_pose guess = quantisePose(res_, ox_, oy_, x, y, yaw);
  std::vector<kc_worldmap_rotation> rot(static_cast<size_t>(2 * n_yaw + 1));
  hip::check(kc_worldmap_match_rotations(yaw, n_yaw, yaw_step, rot.data(), rot.size()));
  kc_worldmap_match_result r{};
  if (s.kind == GridSource::Mapper) {
    hip::check(kc_worldmap_match_from_mapper(ctx_.get(), s.mapper->hipContext(), &guess, rot.data(), n_yaw, reach, &r));
  } else {
    const auto entry = s.kind == GridSource::Host ? kc_worldmap_match_host : kc_worldmap_match_device;
    hip::check(entry(ctx_.get(), s.grid, s.height, s.width, s.central_i, s.central_j, res_, &guess, rot.data(), n_yaw, reach, &r));
  }
  ++match_count_;
  match_rot_ = 2 * n_yaw + 1;
  match_side_ = 2 * reach + 1;
  Match m;
  m.k = r.k;
  m.u = r.u;
  m.v = r.v;
  m.score = r.score;
  m.score_guess = r.score_guess;
  m.points = r.n_points;
  const double R = static_cast<double>(res_);
  m.yaw = yaw + static_cast<double>(r.k) * yaw_step;
  m.x = x + r.u * R;
  m.y = y + r.v * R;
  m.pose = r.pose;
  m.n_yaw = n_yaw;
  m.reach = reach;
  return m;
}

WorldMap::Match WorldMap::match(const LocalMapper &mapper, double x, double y, double yaw, int n_yaw, double yaw_step, int reach) {
  return matchFrom(mapper, x, y, yaw, n_yaw, yaw_step, reach);
}

WorldMap::Match WorldMap::match(const int32_t *grid, int grid_height, int grid_width, double x, double y, double yaw, int n_yaw,
                                double yaw_step, int reach) {
  return matchFrom({GridSource::Host, grid, grid_height, grid_width}, x, y, yaw, n_yaw, yaw_step, reach);
}

WorldMap::Match WorldMap::matchOnDevice(const int32_t *dev_grid, int grid_height, int grid_width, double x, double y, double yaw,
                                        int n_yaw, double yaw_step, int reach) {
  return matchFrom({GridSource::Device, dev_grid, grid_height, grid_width}, x, y, yaw, n_yaw, yaw_step, reach);
}

std::vector<uint32_t> WorldMap::matchScores() const {
  std::vector<uint32_t> out(static_cast<size_t>(match_rot_) * static_cast<size_t>(match_side_) * static_cast<size_t>(match_side_));
  hip::check(kc_worldmap_match_scores(ctx_.get(), out.data(), out.size()));
  return out;
}

void WorldMap::clear() {
  hip::check(kc_worldmap_clear(ctx_.get()));
  last_ = {0, -1, -1, -1, -1};
}

// rules 46 and 48 on the host: the origin as the context now gives it, and no changed cells
void WorldMap::afterShift() {
  hip::check(kc_worldmap_info(ctx_.get(), nullptr, nullptr, nullptr, &ox_, &oy_));
  last_ = {0, -1, -1, -1, -1};
}

void WorldMap::shift(int di, int dj) {
  hip::check(kc_worldmap_shift(ctx_.get(), di, dj));
  afterShift();
}

std::array<int, 2> WorldMap::recentre(double x, double y, int margin, int stride) {
  int32_t di = 0, dj = 0;
  hip::check(kc_worldmap_recentre(ctx_.get(), x, y, margin, stride, &di, &dj));
  afterShift();
  return {di, dj};
}

std::array<int, 2> WorldMap::offset() const {
  int32_t oi = 0, oj = 0;
  hip::check(kc_worldmap_offset(ctx_.get(), &oi, &oj));
  return {oi, oj};
}

std::array<int, 2> WorldMap::recentrePlan(int width, int height, int ic, int jc, int margin, int stride) {
  int32_t di = 0, dj = 0;
  hip::check(kc_worldmap_recentre_plan(width, height, ic, jc, margin, stride, &di, &dj));
  return {di, dj};
}

std::vector<Path::Point> WorldMap::points(double x, double y, float max_sensor_range) const {
  static_assert(sizeof(Path::Point) == 3 * sizeof(float), "Path::Point must be packed (x, y, z)");
  size_t n = 0;
  int32_t bounds[4];
  hip::check(kc_worldmap_points(ctx_.get(), x, y, max_sensor_range, nullptr, 0, &n, bounds));
  std::vector<Path::Point> out(n);
  if (n) hip::check(kc_worldmap_points(ctx_.get(), x, y, max_sensor_range, out.data()->data(), n, &n, bounds));
  out.resize(n);
  return out;
}

std::vector<double> WorldMap::scanPoses(const std::vector<std::array<double, 3>> &poses, const std::vector<double> &angles,
                                        float range_max, bool unknown_blocks, std::vector<int32_t> *cells_out) const {
  const unsigned flags = unknown_blocks ? KC_SCAN_UNKNOWN_BLOCKS : 0u;
  hip::check(kc_worldmap_scan_check(res_, poses.size(), angles.size(), range_max, flags, nullptr));
  std::vector<kc_worldmap_pose> q;
  q.reserve(poses.size());
  for (const auto &p : poses) q.push_back(quantisePose(res_, ox_, oy_, p[0], p[1], p[2]));
  std::vector<double> out(poses.size() * angles.size());
  if (cells_out) cells_out->assign(out.size(), -1);
  hip::check(kc_worldmap_scan(ctx_.get(), q.data(), q.size(), angles.data(), angles.size(), range_max, flags, out.data(),
                              cells_out ? cells_out->data() : nullptr));
  return out;
}

std::vector<double> WorldMap::scan(double x, double y, double yaw, const std::vector<double> &angles, float range_max,
                                   bool unknown_blocks) const {
  return scanPoses({{x, y, yaw}}, angles, range_max, unknown_blocks, nullptr);
}

std::vector<double> WorldMap::scans(const std::vector<std::array<double, 3>> &poses, const std::vector<double> &angles, float range_max,
                                    bool unknown_blocks) const {
  return scanPoses(poses, angles, range_max, unknown_blocks, nullptr);
}

std::vector<double> WorldMap::scanCells(double x, double y, double yaw, const std::vector<double> &angles, float range_max,
                                        bool unknown_blocks, std::vector<int32_t> &cells_out) const {
  return scanPoses({{x, y, yaw}}, angles, range_max, unknown_blocks, &cells_out);
}

uint32_t WorldMap::integrateScanAt(const kc_worldmap_pose &pose, const std::vector<double> &angles, const std::vector<double> &ranges,
                                   float range_max, float range_min, bool clear_no_return, const std::vector<uint8_t> &skip) {
  if (angles.size() != ranges.size()) throw std::invalid_argument("integrateScan: one range a beam angle");
  if (!skip.empty() && skip.size() != ranges.size()) throw std::invalid_argument("integrateScan: one skip entry a beam, or none");
  std::vector<int32_t> zq(ranges.size());
  hip::check(kc_worldmap_quantise_ranges(res_, ranges.data(), ranges.size(), range_max, range_min, zq.data()));
  for (size_t k = 0; k < skip.size(); ++k)
    if (skip[k]) zq[k] = -1;  // rule 54: the beam says nothing
  hip::check(kc_worldmap_integrate(ctx_.get(), &pose, angles.data(), angles.size(), zq.data(), range_max,
                                   clear_no_return ? KC_INTEGRATE_CLEAR_NO_RETURN : 0u, &last_));
  return last_.changed;
}

uint32_t WorldMap::integrateScan(double x, double y, double yaw, const std::vector<double> &angles, const std::vector<double> &ranges,
                                 float range_max, float range_min, bool clear_no_return, const std::vector<uint8_t> &skip) {
  return integrateScanAt(quantisePose(res_, ox_, oy_, x, y, yaw), angles, ranges, range_max, range_min, clear_no_return, skip);
}

MoverCluster WorldMap::clusterToWorld(const kc_worldmap_cluster &c, float resolution, double origin_x, double origin_y) {
  if (c.n < 1) throw std::invalid_argument("clusterToWorld: a cluster has at least one beam");
  const double r = static_cast<double>(resolution), n = static_cast<double>(c.n);
  MoverCluster out;
  out.x = origin_x + (static_cast<double>(c.sx) / n - 32768.0) / 65536.0 * r;
  out.y = origin_y + (static_cast<double>(c.sy) / n - 32768.0) / 65536.0 * r;
  // half the longer side of the endpoints' box: at most the mover's own radius, which half the diagonal can pass by sqrt(2)
  out.radius = static_cast<double>(std::max(c.max_x - c.min_x, c.max_y - c.min_y)) / 2.0 / 65536.0 * r;
  out.raw = c;
  return out;
}

MoverDetection WorldMap::detectMoversAt(const kc_worldmap_pose &pose, const std::vector<double> &angles,
                                        const std::vector<double> &ranges, float range_max, float range_min,
                                        const MoverDetectConfig &config) const {
  if (angles.size() != ranges.size()) throw std::invalid_argument("detectMovers: one range a beam angle");
  std::vector<int32_t> zq(ranges.size());
  hip::check(kc_worldmap_quantise_ranges(res_, ranges.data(), ranges.size(), range_max, range_min, zq.data()));
  MoverDetection out;
  out.labels.assign(ranges.size(), -1);
  std::vector<kc_worldmap_cluster> raw(KC_WORLDMAP_MAX_CLUSTERS);
  hip::check(kc_worldmap_movers(ctx_.get(), &pose, angles.data(), angles.size(), zq.data(), range_max, config.m2, config.gap,
                                config.join_q, config.min_beams, out.labels.data(), raw.data(), raw.size(), &out.record));
  out.clusters.reserve(out.record.n_returned);
  for (uint32_t i = 0; i < out.record.n_returned; ++i) out.clusters.push_back(clusterToWorld(raw[i], res_, ox_, oy_));  // rule 46's origin
  return out;
}

MoverDetection WorldMap::detectMovers(double x, double y, double yaw, const std::vector<double> &angles, const std::vector<double> &ranges,
                                      float range_max, float range_min, const MoverDetectConfig &config) const {
  return detectMoversAt(quantisePose(res_, ox_, oy_, x, y, yaw), angles, ranges, range_max, range_min, config);
}

void WorldMap::enableDistance(int reach, bool unknown_blocks) {
  hip::check(kc_worldmap_set_distance(ctx_.get(), reach, (reach != 0 && unknown_blocks) ? KC_WORLDMAP_DIST_UNKNOWN_BLOCKS : 0u));
}

int WorldMap::distanceReach() const {
  int reach = 0;
  hip::check(kc_worldmap_distance_info(ctx_.get(), &reach, nullptr, nullptr, nullptr));
  return reach;
}

std::vector<uint16_t> WorldMap::distanceField() const {
  std::vector<uint16_t> out(static_cast<size_t>(width_) * static_cast<size_t>(height_));
  hip::check(kc_worldmap_get_distance(ctx_.get(), out.data(), out.size()));
  return out;
}

const void *WorldMap::deviceDistance() const {
  void *p = nullptr;
  hip::check(kc_worldmap_distance_device(ctx_.get(), &p));
  return p;
}

std::array<int, 4> WorldMap::distanceLastBox() const {
  int b[4] = {-1, -1, -1, -1};
  hip::check(kc_worldmap_distance_info(ctx_.get(), nullptr, nullptr, b, nullptr));
  return {b[0], b[1], b[2], b[3]};
}

std::vector<int8_t> WorldMap::cls() const {
  std::vector<int8_t> out(static_cast<size_t>(width_) * static_cast<size_t>(height_));
  hip::check(kc_worldmap_get(ctx_.get(), out.data(), nullptr, out.size()));
  return out;
}

std::vector<int8_t> WorldMap::evidence() const {
  std::vector<int8_t> out(static_cast<size_t>(width_) * static_cast<size_t>(height_));
  hip::check(kc_worldmap_get(ctx_.get(), nullptr, out.data(), out.size()));
  return out;
}

const void *WorldMap::deviceGrid() const {
  void *p = nullptr;
  hip::check(kc_worldmap_grid_device(ctx_.get(), &p));
  return p;
}

}  // namespace Mapping
}  // namespace Kompass
