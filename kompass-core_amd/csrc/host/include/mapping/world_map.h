// World-frame occupancy map that stays on the device, fused from the LocalMapper's egocentric grids
// (kc_worldmap_*, csrc/kc_worldmap.hip).
//
// Nothing in the reference to restate: it leaves the world-frame map to its ROS side.  This is the map between
// Mapping::LocalMapper, whose grid turns with the robot and forgets what leaves its window, and
// Planning::GridPlanner::replan, which wants a world-frame map that changes: seeded from a prior (the PCD grid),
// updated from each local grid where that grid lies, read in place by the planner.
#pragma once

#include <array>
#include <cstdint>
#include <vector>

#include "datatypes/path.h"
#include "mapping/local_mapper.h"
#include "utils/hip_backend.h"

namespace Kompass {
namespace Mapping {

// WorldMap::detectMovers' parameters (DESIGN.md 4.11 rule 64) and results.  The defaults are the prototype's values:
// judgement, not measurement.
struct MoverDetectConfig {
  uint32_t m2 = 4;               // cells^2: a return nearer than this to an occupied cell is the wall's
  uint32_t gap = 2;              // beams that may be missing inside a run
  uint64_t join_q = 9ull << 16;  // 2^-16 cells^2: neighbours further apart than this start a new run
  uint32_t min_beams = 3;        // a run of fewer beams is dropped
};
struct MoverCluster {
  double x = 0.0, y = 0.0, radius = 0.0;  // world metres: the mean endpoint, half the longer side of the endpoints' box
  kc_worldmap_cluster raw = {};           // rule 68's integers
};
struct MoverDetection {
  std::vector<MoverCluster> clusters;     // the first n_returned
  std::vector<int32_t> labels;            // rule 69, a beam
  kc_worldmap_movers_record record = {};
};

class WorldMap {
 public:
  // width x height cells, cell (I, J) at I + J * width; (origin_x, origin_y): the world position of cell (0, 0)'s
  // centre.  std::invalid_argument / std::out_of_range for a bad shape, before a device is looked for.
  WorldMap(int width, int height, float resolution, double origin_x = 0.0, double origin_y = 0.0);

  // hit / miss: evidence an OCCUPIED / EMPTY observation adds / takes away, within e_min .. e_max; a cell is
  // OCCUPIED from occ_thr up.  Clears the map.
  void setModel(int hit, int miss, int e_min, int e_max, int occ_thr);
  // A grid of the map's shape and layout, int8 or int32 (elem_bytes 1 or 4): OCCUPIED -> e_max, EMPTY -> e_min,
  // anything else never observed.  Replaces the whole state.  The device overload reads a finished grid in place.
  void setPrior(const void *host_grid, int elem_bytes, int width, int height);
  void setPriorOnDevice(const void *dev_grid, int elem_bytes, int width, int height);
  // orders the next device grid's read after the work queued so far on a producer's stream (no host wait)
  void waitForStream(void *stream);

  // One update from the mapper's last grid where it lies on the device, ordered after its scan without a host
  // wait; (x, y, yaw): the robot's pose in the world, i.e. the pose of the grid's frame.  Returns changed().
  uint32_t update(const LocalMapper &mapper, double x, double y, double yaw);
  // ... from a grid on the host: int32, column-major grid_height x grid_width, the mapper's central cell
  uint32_t update(const int32_t *grid, int grid_height, int grid_width, double x, double y, double yaw);
  // ... from a finished grid on the device, read in place
  uint32_t updateOnDevice(const int32_t *dev_grid, int grid_height, int grid_width, double x, double y, double yaw);
  void clear();

  // The rolling window (DESIGN.md 4.11 rules 46 to 49).  shift: the window moves by whole cells on the device, a positive
  // di towards +x; what leaves is forgotten, what enters is never observed.  originX() / originY() follow (the origin at
  // creation plus offset * resolution, never accumulated), changed() is 0 and changedBox() all -1 afterwards, the distance
  // plane is wholly dirty, deviceGrid() and deviceDistance() keep their addresses.  std::out_of_range for an offset above
  // 2^30 cells.  recentre: rule 49's plan for the robot at world (x, y) -- no shift while its cell is `margin` cells or
  // more from every border, else the whole multiple of `stride` that brings it nearest the centre -- then the shift;
  // returns the shift made.  recentrePlan is the policy alone and needs no device.
  void shift(int di, int dj);
  std::array<int, 2> recentre(double x, double y, int margin, int stride);
  std::array<int, 2> offset() const;
  static std::array<int, 2> recentrePlan(int width, int height, int ic, int jc, int margin, int stride);

  // Correlative match (DESIGN.md 4.11 rules 9 to 15): the pose within n_yaw steps of yaw_step each side of the guess's
  // yaw and `reach` cells each side of its position that puts the grid's occupied cells onto the map best.  The map is
  // not modified.  Same three sources as update.
  struct Match {
    int k = 0, u = 0, v = 0;                         // the winner: yaw step, cells along x and y
    uint32_t score = 0, score_guess = 0, points = 0;  // the winner's score, the guess's, the occupied local cells
    double x = 0.0, y = 0.0, yaw = 0.0;              // the corrected pose: yaw + k * yaw_step, x + u * resolution, y + v * resolution
    kc_worldmap_pose pose = {0, 0, 0, 0};            // ... as the update kernel takes it
    int n_yaw = 0, reach = 0;                        // the window
  };
  Match match(const LocalMapper &mapper, double x, double y, double yaw, int n_yaw, double yaw_step, int reach);
  Match match(const int32_t *grid, int grid_height, int grid_width, double x, double y, double yaw, int n_yaw, double yaw_step,
              int reach);
  Match matchOnDevice(const int32_t *dev_grid, int grid_height, int grid_width, double x, double y, double yaw, int n_yaw,
                      double yaw_step, int reach);
  // rule 13's table of the last match: (2 n_yaw + 1) x (2 reach + 1) x (2 reach + 1), [k][v][u]
  std::vector<uint32_t> matchScores() const;
  // matches made so far: a Match whose number this is owns the table
  uint64_t matchCount() const { return match_count_; }
  // One update at a quantised pose (a Match's), from the same three sources
  uint32_t updateAt(const LocalMapper &mapper, const kc_worldmap_pose &pose);
  uint32_t updateAt(const int32_t *grid, int grid_height, int grid_width, const kc_worldmap_pose &pose);

  // The occupied cells within max_sensor_range of (x, y) as world-frame points, z = 0, in no particular order (DESIGN.md
  // 4.11 rules 16 to 19): a cloud to show, or to hand to a consumer of point lists.  The controllers take the map itself
  // (CollisionChecker::updateSensorData) and never see this list.  std::invalid_argument unless max_sensor_range is a
  // finite float > 0, std::out_of_range above 2048 cells of radius.
  std::vector<Path::Point> points(double x, double y, float max_sensor_range) const;

  // The map's virtual laser scan (DESIGN.md 4.11 rules 20 to 27): what a lidar whose frame is at (x, y, yaw) in the world
  // would range over the beam `angles` (scan frame), by the map's memory: the distance to the first OCCUPIED cell (with
  // unknown_blocks also a never-observed one) within range_max, else range_max.  One launch on the device.  scans: a batch
  // of poses {x, y, yaw} in one launch, ranges[p * angles.size() + k].  scanCells: also the hit cells I + J * width, -1
  // where a beam has no hit.  Exceptions as points(): std::invalid_argument (range_max, a non-finite angle or pose, no
  // beam), std::out_of_range (above 2048 cells of range, 65536 beams or 2^22 rays).
  std::vector<double> scan(double x, double y, double yaw, const std::vector<double> &angles, float range_max,
                           bool unknown_blocks = false) const;
  std::vector<double> scans(const std::vector<std::array<double, 3>> &poses, const std::vector<double> &angles, float range_max,
                            bool unknown_blocks = false) const;
  std::vector<double> scanCells(double x, double y, double yaw, const std::vector<double> &angles, float range_max,
                                bool unknown_blocks, std::vector<int32_t> &cells_out) const;

  // One measured laser scan into the map by an inverse ray cast (DESIGN.md 4.11 rules 52 to 58), no local grid in
  // between: (x, y, yaw) is the scan frame's pose in the world, `angles` the beams in that frame, `ranges` one measured
  // range a beam in metres.  A NaN, a negative range or one below range_min says nothing; +inf or a range >= range_max
  // is a beam without a return, which clears the cells it crosses up to range_max with clear_no_return and says nothing
  // without; any other beam marks the cell its range ends in occupied and the cells before it empty, a hit beating a
  // miss where beams disagree.  Two launches on the device.  Returns changed(); changedBox() follows.
  // std::invalid_argument (sizes that differ, no beam, range_max, range_min, a non-finite angle or pose),
  // std::out_of_range (above 2048 cells of range or 65536 beams).  ...At: at a quantised pose (a Match's).
  // skip: empty, or one entry a beam; a beam whose entry is not 0 says nothing (rule 54), whatever its range: zq_k = -1
  // behind the quantiser, on the host, so the kernels see nothing new and a call without a mask is what it was.  What
  // MoverTracker::skipMask gives keeps a mover's returns out of the map.
  uint32_t integrateScan(double x, double y, double yaw, const std::vector<double> &angles, const std::vector<double> &ranges,
                         float range_max, float range_min = 0.0f, bool clear_no_return = false,
                         const std::vector<uint8_t> &skip = {});
  uint32_t integrateScanAt(const kc_worldmap_pose &pose, const std::vector<double> &angles, const std::vector<double> &ranges,
                           float range_max, float range_min = 0.0f, bool clear_no_return = false,
                           const std::vector<uint8_t> &skip = {});

  // Moving obstacles in a measured scan (DESIGN.md 4.11 rules 64 to 69): the returns that end in cells the map has seen
  // EMPTY, more than sqrt(m2) cells from anything occupied, grouped into runs of neighbouring beams.  Arguments as
  // integrateScan's; the map is read and never written, the distance plane must be on (std::runtime_error otherwise,
  // and for m2 above its reach^2).  Two launches on the device and one read-back.  The defaults are the prototype's
  // values: judgement, not measurement.
  MoverDetection detectMovers(double x, double y, double yaw, const std::vector<double> &angles, const std::vector<double> &ranges,
                              float range_max, float range_min = 0.0f, const MoverDetectConfig &config = MoverDetectConfig()) const;
  MoverDetection detectMoversAt(const kc_worldmap_pose &pose, const std::vector<double> &angles, const std::vector<double> &ranges,
                                float range_max, float range_min = 0.0f, const MoverDetectConfig &config = MoverDetectConfig()) const;
  // A cluster in world metres: centre origin + ((SX / n) - 32768) / 65536 * resolution -- rule 65's EX of a return in the
  // middle of cell I is (I << 16) + 2^15, and the origin is cell (0, 0)'s centre -- with rule 46's origin at the current
  // offset; radius max(max_x - min_x, max_y - min_y) / 2 / 65536 * resolution, which a disc's returns never push past the
  // disc's own radius (half the box's diagonal would, by up to sqrt(2)).  Needs no device.
  static MoverCluster clusterToWorld(const kc_worldmap_cluster &c, float resolution, double origin_x, double origin_y);

  // The distance plane (DESIGN.md 4.11 rules 42 and 43), off by default: per cell the squared distance in cells to the
  // nearest OCCUPIED cell (with unknown_blocks also a never-observed one) within `reach` cells, KC_WORLDMAP_DIST_FAR
  // beyond.  Kept lazily: an update only notes its changed box, whoever reads the plane refreshes that box grown by
  // reach.  reach 0 switches it off and frees it.  std::out_of_range for a reach outside 0 .. 254.
  void enableDistance(int reach, bool unknown_blocks = false);
  int distanceReach() const;
  // a refreshed copy, width x height as the map; std::runtime_error while the plane is off
  std::vector<uint16_t> distanceField() const;
  // the refreshed plane on the device: uint16, width x height; valid until the next enableDistance
  const void *deviceDistance() const;
  // (i_min, j_min, i_max, j_max) the last refresh recomputed, all -1 when it had nothing to do
  std::array<int, 4> distanceLastBox() const;

  // copies of the planes, width x height as the map
  std::vector<int8_t> cls() const;
  std::vector<int8_t> evidence() const;
  // the last update: cells whose class changed and their box (i_min, j_min, i_max, j_max), all -1 when none did
  uint32_t changed() const { return last_.changed; }
  std::array<int, 4> changedBox() const { return {last_.i_min, last_.j_min, last_.i_max, last_.j_max}; }
  // the cls plane on the device: int8, width x height, what GridPlanner::setGridOnDevice(ptr, 1) reads in place
  const void *deviceGrid() const;

  int width() const { return width_; }
  int height() const { return height_; }
  float resolution() const { return res_; }
  double originX() const { return ox_; }
  double originY() const { return oy_; }
  kc_worldmap *hipContext() const { return ctx_.get(); }
  // the pose as the kernel takes it; needs no device
  static kc_worldmap_pose quantisePose(float resolution, double origin_x, double origin_y, double x, double y, double yaw);

 private:
  int width_, height_;
  float res_;
  double ox_, oy_;  // rule 46's origin at the current offset: read again from the context after every shift
  hip::WorldMapHandle ctx_;
  kc_worldmap_result last_ = {0, -1, -1, -1, -1};
  uint64_t match_count_ = 0;
  int match_rot_ = 0, match_side_ = 0;  // the last match's table: rotations, candidates a side

  // Where a local grid comes from: the mapper's last grid where it lies, or a grid on the host or on the device with its
  // shape and the mapper's central cell.  Every public update / match names one and goes through updateFrom / matchFrom.
  struct GridSource {
    enum Kind { Mapper, Host, Device } kind;
    const LocalMapper *mapper;
    const int32_t *grid;
    int height, width, central_i, central_j;
    GridSource(const LocalMapper &m) : kind(Mapper), mapper(&m), grid(nullptr), height(0), width(0), central_i(0), central_j(0) {}
    GridSource(Kind k, const int32_t *grid, int grid_height, int grid_width);
  };
  void afterShift();
  uint32_t updateFrom(const GridSource &s, const kc_worldmap_pose &pose);
  Match matchFrom(const GridSource &s, double x, double y, double yaw, int n_yaw, double yaw_step, int reach);
  std::vector<double> scanPoses(const std::vector<std::array<double, 3>> &poses, const std::vector<double> &angles, float range_max,
                                bool unknown_blocks, std::vector<int32_t> *cells_out) const;
};

}  // namespace Mapping
}  // namespace Kompass
