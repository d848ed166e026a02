/*
 * kompass_hip.h -- C ABI of libkompass_hip.so: the MI355X (gfx950) hot path of
 * kompass_cpp's sampling controller (DWA sampler -> roll-out -> collision ->
 * weighted cost -> argmin) and of the laserscan -> occupancy LocalMapper.
 *
 * The reference (automatika-robotics/kompass-core v0.8.1) has no C ABI: its
 * boundary is a C++ class surface + a nanobind module.
 * This header is the thin shim the host C++ classes
 * (kompass-core_amd/csrc/host/) and any other binding call into.  Every entry
 * point names the reference interface it replaces; paths are relative to
 * <reference>/src/kompass_cpp/kompass_cpp/.
 *
 * Conventions
 *  - plain C types only: pointers + sizes, caller-owned host buffers, opaque
 *    contexts; no C++/torch types.
 *  - every call returns KC_OK (0) or a negative kc_status; the message of the
 *    last failure on the calling thread is kc_last_error().  A HIP failure
 *    never crosses the boundary as UB.  There is NO CPU fallback: without a
 *    usable HIP device every compute call returns KC_ERR_HIP.
 *  - one HIP stream per context; calls on one context are serial, distinct
 *    contexts may be driven from distinct threads (reference objects are not
 *    thread-safe either: trajectory_sampler.cpp:18, local_mapper.cpp:15).
 *  - results are bit-exact on integers/indices and on float costs w.r.t. the
 *    reference CPU path with maxNumThreads = 1 ordering.
 */
#ifndef KOMPASS_HIP_H
#define KOMPASS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KC_ABI_VERSION 1

typedef enum {
  KC_OK = 0,
  KC_ERR_INVALID = -1,     /* bad argument (reference: std::invalid_argument) */
  KC_ERR_RANGE = -2,       /* capacity / range (reference: std::out_of_range) */
  KC_ERR_HIP = -3,         /* HIP runtime failure or no device */
  KC_ERR_UNSUPPORTED = -4, /* outside the restated domain (e.g. non-planar
                              sensor rotation for the collision checker) */
  KC_ERR_STATE = -5        /* call order (e.g. evaluate before roll-out) */
} kc_status;

/* datatypes/control.h:12 */
enum { KC_ACKERMANN = 0, KC_DIFFERENTIAL_DRIVE = 1, KC_OMNI = 2 };
/* utils/collision_check.h:25 */
enum { KC_CYLINDER = 0, KC_BOX = 1, KC_SPHERE = 2 };
/* mapping/local_mapper.h:9 */
enum { KC_UNEXPLORED = -1, KC_EMPTY = 0, KC_OCCUPIED = 100 };

const char *kc_last_error(void);
int kc_abi_version(void);
/* number of visible HIP devices (0 when none; never fails) */
int kc_device_count(void);

/* ------------------------------------------------------------------------ */
/* plain structs                                                            */
/* ------------------------------------------------------------------------ */
typedef struct { /* Path::State, datatypes/path.h:14-22 */
  double x, y, yaw, speed;
} kc_state;

typedef struct { /* ControlLimitsParams, datatypes/control.h:191-235 */
  double vx_max, vx_acc, vx_dec;
  double vy_max, vy_acc, vy_dec;
  double omega_max_angle, omega_max, omega_acc, omega_dec;
} kc_limits;

typedef struct { /* TrajectoryCostsWeights, utils/cost_evaluator.h:22-50 */
  double reference_path_distance_weight;
  double goal_distance_weight;
  double obstacles_distance_weight;
  double smoothness_weight;
  double jerk_weight;
} kc_weights;

typedef struct {
  /* CollisionChecker ctor, utils/collision_check.h:46-50 */
  int shape;                /* KC_CYLINDER / KC_BOX / KC_SPHERE */
  float dims[3];            /* cylinder (r,h) / box (x,y,z) / sphere (r) */
  int ndims;
  float sensor_pos[3];      /* sensor position in the body frame */
  float sensor_rot_xyzw[4]; /* Eigen coefficient order (x,y,z,w) */
  double octree_res;
  /* TrajectorySampler / CostEvaluator sizing, trajectory_sampler.h:75-83,
   * cost_evaluator.h:69-71 (device buffers sized once, like
   * cost_evaluator_gpu.cpp:54-120; segment / obstacle buffers grow) */
  double time_step;
  size_t max_samples;       /* capacity N (numTrajectories) */
  size_t max_points;        /* capacity P (numPointsPerTrajectory) */
  size_t max_segment;       /* initial tracked-segment capacity */
  size_t max_obstacles;     /* initial obstacle capacity */
  float acc_limits[3];      /* cost_evaluator.cpp:18-20 */
  int device;               /* HIP device ordinal */
} kc_dwa_params;

typedef struct {
  /* TrajSearchResult (trajectory.h:611-618) + LowestCost (:621-644) */
  int found;           /* isTrajFound */
  float cost;          /* trajCost (minCost) */
  int64_t index;       /* index into the admissible-only list (reference
                          numbering); -1 if not found */
  int64_t raw_index;   /* index into the generated sample list (global, i.e.
                          including the shard offset); -1 if not found */
  int64_t n_admissible;/* samples->size() on this context's shard (kc_dwa_cycle_sharded:
                          over all ranks) */
  int64_t n_samples;   /* samples rolled out on this context's shard
                          (kc_dwa_cycle_sharded: over all ranks) */
} kc_result;

/* ------------------------------------------------------------------------ */
/* sampling controller                                                      */
/* ------------------------------------------------------------------------ */
typedef struct kc_dwa kc_dwa;

/* TrajectorySampler::TrajectorySampler (trajectory_sampler.cpp:23-60) +
 * CostEvaluator::CostEvaluator (cost_evaluator.cpp:23-37) */
int kc_dwa_create(const kc_dwa_params *params, kc_dwa **out);
void kc_dwa_destroy(kc_dwa *ctx);

/* adopt an external hipStream_t for all work of this context; NULL restores the
 * context's own (non-blocking) stream.  NB: the handle of the legacy default
 * stream IS NULL -- to share a stream with a framework create an explicit one
 * there (torch.cuda.Stream()) and pass its handle. */
int kc_dwa_set_stream(kc_dwa *ctx, void *hip_stream);
/* CollisionChecker::resetOctreeResolution, collision_check.cpp:70-75 */
int kc_dwa_set_resolution(kc_dwa *ctx, double octree_res);
/* CostEvaluator::updateCostWeights, cost_evaluator.cpp:39-41 */
int kc_dwa_set_weights(kc_dwa *ctx, const kc_weights *w);

/* Per-context switches of the device path (no counterpart in the reference, whose
 * SYCL path has none; every setting gives bit-identical results -- tests/
 * test_gpu_parity.py runs the cycle under each).  value: 0 / 1 unless stated.
 *   "fused_cycle"    (1) kc_dwa_cycle runs the whole cycle as ONE launch when the
 *                        cost tables fit in LDS beside the roll-out tile, the shard is one
 *                        resident wave of workgroups (<= 32 samples x CUs) and either fills
 *                        half the CUs or left few survivors last cycle; 2: whenever the
 *                        tables fit; 0: roll-out, cost and publish kernels
 *   "cycle_samples"  (0) samples per workgroup of the single-launch cycle: 0 = 32, or 16 when
 *                        32 would give at most half of the CUs a workgroup (shards <= 4096
 *                        samples on an MI355X); 16 / 32: fixed
 *   "velocity_group" (0) kc_cost_evaluate with velocity profiles: samples per wavefront of the
 *                        ordered smoothness / jerk sums -- 1: inside the cost kernel, 4 / 16: a
 *                        pass of its own (velocity_sums_kernel); 0: by batch size (1 below
 *                        ~5 profiles per SIMD, 16 from ~96)
 *   "velocity_beside" (1) that pass on a second stream beside the wavefront-per-sample cost kernel
 *                        (its serial chains leave most issue slots idle); a short kernel behind both
 *                        adds the two terms and forms the keys.  0: one after the other
 *   "near_table"   (128) cells per side (16..512) of the near table of the tracked segment
 *                        (per cell of a grid over the reachable box: the chunk range that can
 *                        hold a point's nearest segment point + a seed), built when the
 *                        wavefront-per-sample cost search is expected to run; 0: off (the
 *                        chunk hierarchy alone).  Same minimum, same index, same bits
 *   "host_reduce"    (1) single-GPU single-launch cycles end without a device-side reduction:
 *                        every workgroup posts a 32-byte slot to pinned memory, the host
 *                        reduces them in kc_dwa_fetch_result; 0: arrival ticket + last
 *                        workgroup (what kc_dwa_cycle_sharded always uses)
 *   "write_paths"    (0) the single-launch cycle also stores every float row
 *                        (otherwise rows are produced on demand by kc_dwa_get_samples)
 *   "cost_kernel"    (0) stand-alone cost stage: 0 = 2 (round 4: the wavefront-per-sample kernel is ahead at
 *                        every list length), 1 workgroup per sample, 2 wavefront per sample
 *   "drop_samples"   (1) TrajectorySampler::setSampleDroppingMode (trajectory_sampler.cpp:103-105).  0: a
 *                        sample that collides at loop step i with last_free_index = i - 1 beyond
 *                        "num_ctrl_points" is KEPT (:157-168): path points i + 1 .. P - 1 repeat point
 *                        i - 1, velocities i .. P - 2 are zero, and smoothness / jerk see that step
 *   "num_ctrl_points" (0) numCtrlPoints_ = control_horizon / time_step as size_t (:88: the config-object
 *                        constructor's definition; the explicit-argument constructor leaves it
 *                        uninitialised)
 *   "obs_near"       (1) LaserScan input (beams without a return -- inf / NaN -- stay out of the boxes): consecutive beams are a polyline -- the
 *                        obstacle term of long admissible lists goes through a near table of the scan
 *                        (per cell of the reachable box: the beam chunks that can hold the nearest
 *                        obstacle, a seed, a floor; obs_near_kernel) instead of the bucket ring search
 *                        From the second cycle on kc_dwa_set_scan builds the table for the pose it
 *                        is given inside the launch of the sensor tables; a cycle that starts
 *                        elsewhere (or reaches further) builds its own
 *   "obs_union"     (512) obstacle term of long admissible lists, point-cloud / costmap input: where a
 *                        trajectory runs through occupied bucket cells, the obstacles of the ONE
 *                        rectangle of cells that can hold the trajectory's nearest obstacle are
 *                        broadcast to all of its points (obstacle_union_scan) instead of a ring walk
 *                        per point; rectangles with more obstacles than this fall back.  0: off
 *   "box_cover"      (1) BOX robots at least twice as long as wide whose inscribed and circumscribed circles are
 *                        4.5 voxels or more apart: the pose gate of the fused kernels looks up several circles
 *                        laid along the long axis in the dilated sensor masks (2 .. 8 of them) instead of one
 *                        around the centre; 0: the single look-up.  Takes effect with the next sensor update
 *   "cost_batch"     (1) the long-list cost kernel leaves the per-sample part (ordered sum, the end
 *                        point's index, weighted total, key) to a pass over 64 samples at once, a lane a
 *                        sample (sample_cost_batched_kernel), when the list fills several buffers per
 *                        workgroup (>= 10240 expected); 2: for every list length; 0: off
 *   "device_trig"    (1) cos / sin(yaw_k) formed by the roll-out kernels themselves (below:
 *                        kc_trig_selfcheck); 0: the FALLBACK -- the host's libm table, complete before the
 *                        launch (no kernel ever waits for the host)
 *   "sensor_on_host" (0) voxel bitmap / obstacle buckets built on the host (spheres beyond 32 k points or 32 z layers are)
 *   "sensor_two_launch" (0) the sensor build of clouds beyond 32 k points (two launches) for every size
 *   "force_split"    (0) roll-out, collision and compaction as separate kernels
 *   "team_max"       (4) workgroups of the single-launch cycle with up to this many survivors cost them by teams
 *                        (R survivors: R teams of floor(16 / R) wavefronts, eight at most; a team's last place forms
 *                        the obstacle term, the others hold every trajectory point at once, eight, four or two
 *                        lanes a point, whichever is the widest that fits: csrc/kc_team_layout.h.  Trajectories
 *                        of more than 64 points and cycles without an obstacle weight keep halves / quarters of
 *                        the workgroup, eight / four lanes a point); more: a wavefront a sample.
 *                        0: always a wavefront a sample
 * kc_dwa_get_option also reads "last_cycle_single_launch", "last_cycle_samples",
 * "host_threads", "trig_rows" (rows of the host's cos / sin table: distinct omegas of
 * this context's share), "shard_samples", and the counters "obs_near_rides" /
 * "obs_near_builds" (near tables built inside a sensor launch / by a launch of their own),
 * "pattern_hits" / "pattern_builds" (index patterns of a window lattice found on the device /
 * walking orders built for a new one).
 * Waits for the context's stream.  Nothing that selects a path is read from the environment (round 4); the
 * variables that remain are diagnostics (Switches). */
int kc_dwa_set_option(kc_dwa *ctx, const char *name, double value);
int kc_dwa_get_option(kc_dwa *ctx, const char *name, double *value);
/* threads of the process-wide host pool that evaluates the libm trig table of a
 * roll-out (path.h:24-30 calls cos/sin per step; here once per distinct omega and
 * step): 1..64, the calling thread included.  Default: from the CPUs the process
 * may use (cgroup quota / ranks on the node) or KC_HOST_THREADS. */
int kc_set_host_threads(int n);
/* Device trig (option "device_trig", default 1; csrc/kc_trig_exact.h): the roll-out kernels form
 * yaw_k of their omega rows by repeated addition and evaluate glibc's `sincos` algorithm themselves
 * (State::update, datatypes/path.h:24-30, calls cos / sin of the host libm per step; gcc folds the
 * pair into `sincos`) -- every operation a correctly rounded IEEE double add / multiply in the
 * library's order over its 440-entry table, so the bits are the host's.
 * kc_trig_selfcheck compares the restatement with the INSTALLED sincos on a fixed argument set
 * (run once when the first context asks; a difference switches device trig off for the process and
 * the host table of rounds 1-3 is used); kc_trig_table fills cos_sin_out[k * n_rows + r] =
 * {cos, sin}(yaw_k of row r), yaw_0 = yaw0, yaw_{k+1} = yaw_k + omega[r] * dt, on the current
 * device (tests: against the host's sincos). */
int kc_trig_selfcheck(int64_t *compared_out);
int kc_trig_table(double yaw0, const double *omega, size_t n_rows, size_t n_steps, double dt,
                  double *cos_sin_out);

/* A1 on the host: TrajectorySampler::UpdateReachableVelocityRange
 * (trajectory_sampler.cpp:328-372) + the lattice loops (:181-220 / :256-272,
 * maxNumThreads = 1 ordering) with the all-zero filter of :122-125.
 * max_angular_samples is the un-bumped constructor value.  The list becomes
 * the context's sample set (uploaded); returns the count in *n_out.  Optional
 * vx/vy/omega receive the list (capacity cap). */
int kc_dwa_sample_window(kc_dwa *ctx, int ctr_type, const kc_limits *limits,
                         double cur_vx, double cur_vy, double cur_omega,
                         int max_linear_samples, int max_angular_samples,
                         size_t *n_out, double *vx, double *vy, double *omega,
                         size_t cap);
/* explicit sample list in generation order (what getAdmissibleTrajsFromVel is
 * called with, trajectory_sampler.cpp:213,260,268) */
int kc_dwa_set_samples(kc_dwa *ctx, size_t n, const double *vx,
                       const double *vy, const double *omega);
/* multi-GPU sharding: this context rolls out only samples [first, first+count)
 * of the list; raw indices and the packed key carry the global index.  Clears a
 * rule set with kc_dwa_set_shard_rule. */
int kc_dwa_set_shard(kc_dwa *ctx, size_t first, size_t count);
/* Sharding by RULE (what kc_dwa_cycle_sharded needs with more than one rank: every
 * rank must know every rank's share to turn the exchanged bitmaps into the
 * reference's admissible-only index).  Every rank passes the FULL list to
 * kc_dwa_sample_window / kc_dwa_set_samples (the reference generates the whole
 * lattice on the host too, trajectory_sampler.cpp:181-275); the context keeps its
 * share.  Applies to the current list and to every later one.
 *   KC_SHARD_BLOCKS  rank r owns the contiguous block [n r / W, n (r + 1) / W)
 *   KC_SHARD_ROWS    samples are dealt by trig row (distinct omega): row k (in order
 *                    of first appearance) -> rank k mod W, a row with more than twice
 *                    the mean number of samples (omni: the omega = 0 row) sample by
 *                    sample.  A rank then evaluates 1 / W of the host's cos / sin
 *                    table (path.h:24-30: one libm pair per step and omega) instead
 *                    of all of it, and uploads only its own samples.
 * Raw indices in results, keys and kc_dwa_get_samples stay GLOBAL (positions in the
 * full list = the reference's generation order) under either rule.
 * mode < 0 clears the rule (the context owns the whole list again). */
enum { KC_SHARD_BLOCKS = 0, KC_SHARD_ROWS = 1 };
int kc_dwa_set_shard_rule(kc_dwa *ctx, int rank, int world, int mode);
/* the deal itself, as a pure host function (no device): rows[i] = trig row of
 * sample i (any labelling of the distinct omegas), owner_out[i] = rank that owns it */
int kc_shard_plan(const int32_t *rows, size_t n, int world, int mode, int32_t *owner_out);
/* the reduced exchange record of a sharded cycle -> result (pure host function;
 * layout in kc_shard.h / DESIGN.md section 8: [key, error, world x words_per_rank
 * bitmap words]).  owner: as from kc_shard_plan (NULL with KC_SHARD_BLOCKS).
 * Returns KC_ERR_HIP when the record carries a rank's error word. */
int kc_shard_merge(const int64_t *record, size_t words_per_rank, int world, int mode,
                   const int32_t *owner, size_t n_total, kc_result *out);
/* 1 when sample global_raw_index of the current list belongs to this context's
 * share (its row can be fetched here), else 0 */
int kc_dwa_owns_sample(kc_dwa *ctx, int64_t global_raw_index, int *owned_out);

/* sensor data for BOTH consumers, once per cycle:
 *  CollisionChecker::updateState + updateSensorData<T> (collision_check.cpp:
 *  125-135, collision_check.h:91-136) and CostEvaluator::setPointScan
 *  (cost_evaluator.h:174-223; maxObstaclesDist = max_sensor_range / 3). */
int kc_dwa_set_scan(kc_dwa *ctx, const kc_state *state, const double *ranges,
                    const double *angles, size_t n, float max_sensor_range);
int kc_dwa_set_points(kc_dwa *ctx, const kc_state *state, const float *xyz,
                      size_t n, float max_sensor_range);
/* the same with the list in the SENSOR frame -- updateSensorData(cloud, global_frame = false),
 * collision_check.h:119-131: the octree frame is body->tf * sensor_tf_body (as for a laser scan), the obstacle
 * list of the cost term is the same (setPointScan(cloud), cost_evaluator.h:205-223).  Mounts that are not a
 * rotation about z: KC_ERR_UNSUPPORTED for point lists (laser scans take any mount). */
int kc_dwa_set_points_sensor_frame(kc_dwa *ctx, const kc_state *state, const float *xyz, size_t n,
                                   float max_sensor_range);

/* SURVEY 8f rank 4 -- occupancy grid -> obstacle set without the host round
 * trip (the reference goes grid -> host -> point list -> DWA, control/dwa.py:
 * 298-299 with local_map).  dev_grid: int32, column-major [H x W] (the
 * LocalMapper layout, kc_mapper_grid_device); every OCCUPIED (100) cell (i,j)
 * becomes the point ((i - c0) res, (j - c1) res, 0), c0/c1 = the mapper's
 * central cell (local_mapper.h:26-27), i.e. the inverse of localToGrid
 * (:210-222).  State afterwards == kc_dwa_set_points with that list.  The grid
 * must be complete in stream order of the controller's stream, or finished. */
int kc_dwa_set_grid_device(kc_dwa *ctx, const kc_state *state, const int32_t *dev_grid,
                           int grid_height, int grid_width, float resolution, int central_i,
                           int central_j, float max_sensor_range);
/* same, from a mapper context of this library: geometry and stream ordering
 * (event wait, no host synchronisation) are taken from it */
struct kc_mapper;
int kc_dwa_set_grid_from_mapper(kc_dwa *ctx, const kc_state *state, struct kc_mapper *mapper,
                                float max_sensor_range);
/* The obstacles of a world map (kc_worldmap, below) within sensor range of the robot,
 * without leaving the device.  Nothing in the reference to cite: it leaves the world map
 * to its ROS side, and its controllers see the current scan only.  The centre is
 * (state->x, state->y); the list is that of kc_worldmap_points (DESIGN.md 4.11 rules 16
 * to 19).  State afterwards == kc_dwa_set_points(ctx, state, list, n, max_sensor_range):
 * global frame.  Every argument is checked before the device is used: KC_ERR_INVALID for
 * a null pointer, a map on another device or a max_sensor_range that is not a finite
 * float > 0, KC_ERR_RANGE as kc_worldmap_window says.  The controller's stream waits for
 * the map's (event wait, no host synchronisation of the map) and runs the extraction;
 * the call returns with the list extracted, so the map may be updated again at once. */
struct kc_worldmap;
int kc_dwa_set_worldmap(kc_dwa *ctx, const kc_state *state, struct kc_worldmap *map, float max_sensor_range);

/* the (reference_path, tracked_segment) arguments of getMinTrajectoryCost
 * (cost_evaluator.h:139-142): segment points (Path::View X/Y/Z, path.h:39-76),
 * acc_at_seg[j] = reference_path->getDistanceAtIndex(seg_start + j)
 * (path.h:190-194), ref_path_length = reference_path->totalPathLength(). */
int kc_dwa_set_tracked_segment(kc_dwa *ctx, const float *x, const float *y,
                               const float *z, const float *acc_at_seg,
                               size_t seg_size, float ref_path_length);
/* the same segment from ONE array of points, xyz[j] = {x, y, z} of segment point j (a std::vector<Path::Point>
 * / an (S, 3) float32 array where it lies, datatypes/path.h:14-21): the library de-interleaves while it fills
 * its rows, the caller makes no column copies (they were 6 us of a 12 us call through the Python binding). */
int kc_dwa_set_tracked_segment_xyz(kc_dwa *ctx, const float *xyz, const float *acc_at_seg,
                                   size_t seg_size, float ref_path_length);

/* SURVEY 8f rank 4, second half -- the reference path resident on the device.
 * kc_dwa_set_path: the whole (interpolated) path once per path: points, the
 * accumulated length at every point (Path::getDistanceAtIndex, path.h:74-76)
 * and the total length.  kc_dwa_set_tracked_window(start, size): the tracked
 * segment = points [start, start + size) of that path; same state as
 * kc_dwa_set_tracked_segment(x + start, y + start, z + start, acc + start,
 * size, total_length), with the search tables built by a kernel, stream-ordered
 * between two cycles (no host synchronisation). */
int kc_dwa_set_path(kc_dwa *ctx, const float *x, const float *y, const float *z,
                    const float *acc_length, size_t n, float total_length);
int kc_dwa_set_tracked_window(kc_dwa *ctx, size_t start, size_t size);

/* A2-A4: TrajectorySampler::generateTrajectories (trajectory_sampler.cpp:
 * 295-314 -> :118-179) for the context's samples; option "drop_samples" selects the mode.
 * num_points = numPointsPerTrajectory of this cycle (<= max_points). */
int kc_dwa_rollout(kc_dwa *ctx, const kc_state *start, size_t num_points);
/* CollisionChecker::checkCollisions (collision_check.cpp:149-162, 225-246) /
 * TrajectorySampler::checkStatesFeasibility (trajectory_sampler.cpp:378-407)
 * for a batch of poses against the sensor data of the last kc_dwa_set_scan /
 * kc_dwa_set_points: hit_out[i] = 1 when the robot shape at pose i touches an
 * occupied voxel. */
int kc_dwa_check_poses(kc_dwa *ctx, const double *x, const double *y,
                       const double *yaw, size_t n, uint8_t *hit_out);
/* PurePursuit::checkCommandCollisions / findSafeCommand (pure_pursuit.cpp:150-212):
 * candidate i is "clear" when none of the `horizon` poses reached by repeating
 * Path::State::update(cmd_i, (float)dt) from *start touches an occupied voxel.
 * *first_clear_out = smallest clear i, or -1. horizon == 0: every candidate is clear.
 * Same tests and sensor data as kc_dwa_check_poses on those poses, in one launch. */
int kc_dwa_first_clear_command(kc_dwa *ctx, const kc_state *start,
                               const double *vx, const double *vy, const double *omega,
                               size_t n, int horizon, double dt, int64_t *first_clear_out);

/* A5-A10: CostEvaluator::getMinTrajectoryCost (cost_evaluator.cpp:49-109) on
 * the rolled-out samples; result stays on the device until fetched */
int kc_dwa_evaluate(kc_dwa *ctx);
/* blocks until the cycle finished and copies the 32-byte result record */
int kc_dwa_fetch_result(kc_dwa *ctx, kc_result *out);
/* DWA::findBestPath body after the host glue (dwa.h:215-229):
 * roll-out + evaluate + fetch */
int kc_dwa_cycle(kc_dwa *ctx, const kc_state *start, size_t num_points,
                 kc_result *out);

/* ONE reference controller cycle in one call -- DWA::findBestPath (controllers/dwa.h:183-230): a new dynamic
 * window and lattice (trajectory_sampler.cpp:328-372), this cycle's sensor data (collision_check.h:91-136,
 * cost_evaluator.h:174-223), the tracked segment (dwa.cpp:208-233), roll-out + costs + argmin (dwa.h:215-229).
 * Exactly kc_dwa_sample_window + kc_dwa_set_points | kc_dwa_set_scan + kc_dwa_set_tracked_segment[_xyz] +
 * kc_dwa_cycle in that order, same state, same results; what it saves is the caller's per-call cost (a binding
 * crossing per entry: 4 x ~1.5 us through ctypes) on the host chain in front of the cycle kernel's launch.
 * Any part with a null / zero input is skipped and keeps what the context holds (limits NULL: the current sample
 * list; no points and no scan: the current sensor data; seg_size 0: the current segment). */
typedef struct kc_step_inputs {
  /* window: kc_dwa_sample_window(ctr_type, limits, cur_*, max_*); limits NULL: skip */
  int ctr_type;
  const kc_limits *limits;
  double cur_vx, cur_vy, cur_omega;
  int max_linear_samples, max_angular_samples;
  /* sensor data: points_xyz [n_points][3] (kc_dwa_set_points), else scan_ranges / scan_angles [n_beams]
   * (kc_dwa_set_scan); both NULL: skip */
  const float *points_xyz;
  size_t n_points;
  const double *scan_ranges, *scan_angles;
  size_t n_beams;
  float max_sensor_range;
  /* tracked segment: seg_xyz [seg_size][3] (kc_dwa_set_tracked_segment_xyz), else seg_x / seg_y / seg_z
   * (kc_dwa_set_tracked_segment); seg_size 0: skip */
  const float *seg_xyz, *seg_x, *seg_y, *seg_z, *acc_at_seg;
  size_t seg_size;
  float ref_path_length;
  /* kc_dwa_cycle(state, num_points) */
  size_t num_points;
} kc_step_inputs;
int kc_dwa_find_best_path(kc_dwa *ctx, const kc_state *state, const kc_step_inputs *in, kc_result *out);

/* winner row: TrajectorySamples2D::getIndex (trajectory.h:556-562).  path_* are
 * num_points floats, vel_* are num_points-1 floats; any pointer may be NULL */
int kc_dwa_get_best(kc_dwa *ctx, float *path_x, float *path_y, float *vel_vx,
                    float *vel_vy, float *vel_omega);
/* velocity triple of sample raw_index (global numbering) of the current list */
int kc_dwa_get_sample_velocity(kc_dwa *ctx, int64_t raw_index, double *vx,
                               double *vy, double *omega);
/* compacted samples in reference order (TrajectorySamples2D, trajectory.h:
 * 506-603): paths_* [n_admissible x num_points] row-major, raw_index and costs
 * [n_admissible]; any pointer may be NULL.  cap_rows bounds the rows copied. */
int kc_dwa_get_samples(kc_dwa *ctx, float *paths_x, float *paths_y,
                       int32_t *raw_index, float *costs, size_t cap_rows,
                       size_t *n_rows_out);

/* drop_samples = 0 only: per row of kc_dwa_get_samples the first zero-velocity step of a frozen
 * sample (its velocity profile is the sample's velocity before that step and zero from it on), 0 for
 * a sample that never collided.  All zero with drop_samples = 1. */
int kc_dwa_get_freeze_steps(kc_dwa *ctx, int32_t *steps_out, size_t cap_rows, size_t *n_rows_out);

/* CostEvaluator::getMinTrajectoryCost on caller-provided trajectories
 * (sample-major host matrices exactly as TrajectorySamples2D stores them;
 * vel_* may all be NULL => constant-velocity samples).  Uses the context's
 * tracked segment, obstacles and weights.  costs_out[N] may be NULL. */
int kc_cost_evaluate(kc_dwa *ctx, const float *paths_x, const float *paths_y,
                     const float *vel_vx, const float *vel_vy,
                     const float *vel_omega, size_t n, size_t num_points,
                     float *costs_out, kc_result *out);

/* the same in two steps, for callers that score one set of trajectories again and
 * again (the reference's own benchmark does: benchmarks/benchmark_runner.cpp:
 * 152-185 times getMinTrajectoryCost on pre-generated samples): the samples stay
 * resident in HBM, kc_cost_evaluate_resident runs cost kernels + argmin only */
int kc_cost_upload(kc_dwa *ctx, const float *paths_x, const float *paths_y,
                   const float *vel_vx, const float *vel_vy, const float *vel_omega,
                   size_t n, size_t num_points);
int kc_cost_evaluate_resident(kc_dwa *ctx, float *costs_out, kc_result *out);

/* multi-GPU exchange: after kc_dwa_evaluate the context
 * holds, on the device, int64 key = (sortable(cost) << 32) | global raw index
 * (signed-comparable; INT64_MAX = nothing found) and int64 n_admissible.
 * kc_dwa_result_device() returns the device address of that int64[2] record so
 * the caller can all-reduce(min) / all-gather it on the same stream. */
int kc_dwa_result_device(kc_dwa *ctx, void **dev_int64x2);
/* after the caller has reduced that record in place (all-reduce on the
 * context's stream): queue a one-wavefront kernel that hands the record to the
 * host through pinned memory, so that kc_dwa_fetch_result returns the REDUCED
 * key without a D2H copy or a stream wait (index / n_admissible of the result
 * are the local shard's and only meaningful on the owning rank) */
int kc_dwa_publish_result(kc_dwa *ctx);
/* number of admissible samples with raw index < raw_index on this shard (used
 * to rebuild the reference's compacted index across shards) */
int kc_dwa_count_admissible_before(kc_dwa *ctx, int64_t global_raw_index,
                                   int64_t *count_out);
/* The exchange itself, inside this library (no framework in the product path): one
 * process per GPU, RCCL over xGMI.  kc_comm_unique_id on one rank, the 128 bytes
 * to every rank by any transport the caller has, kc_comm_create on all of them
 * (collective: ncclCommInitRank).  librccl is opened on first use (dlopen). */
#define KC_COMM_ID_BYTES 128
typedef struct kc_comm kc_comm;
int kc_comm_unique_id(uint8_t id_out[KC_COMM_ID_BYTES]);
int kc_comm_create(int rank, int world, const uint8_t id_in[KC_COMM_ID_BYTES], int device, kc_comm **out);
/* Rehearsal / test transport for hosts with fewer GPUs than ranks (RCCL refuses two
 * ranks on one device): the ranks are processes of ONE host that meet in a POSIX
 * shared-memory segment called `name` (unique per communicator; rank 0 creates it),
 * the exchange record is reduced by the host (D2H, min, H2D in stream order).  Same
 * kc_dwa_cycle_sharded code on both sides of the one all-reduce call; not the
 * multi-GPU product path.  KC_SHM_TIMEOUT_MS bounds every wait for a peer (20 s). */
int kc_comm_create_shm(int rank, int world, const char *name, int device, kc_comm **out);
void kc_comm_destroy(kc_comm *comm);
int kc_comm_rank(const kc_comm *comm);
int kc_comm_world(const kc_comm *comm);
enum { KC_COMM_RCCL = 0, KC_COMM_SHM = 1 };
int kc_comm_transport(const kc_comm *comm);
/* What the transport ITSELF reports (any pointer may be null): RCCL -- ncclCommCount, ncclCommUserRank,
 * ncclCommCuDevice of the communicator (kc_comm_create fails when they disagree with its arguments); shared
 * memory -- the number of ranks attached to the segment.  kc_comm_world / kc_comm_rank return the constructor's
 * arguments.  The reference has no collective (cost_evaluator_gpu.cpp:55): nothing to cite. */
int kc_comm_query(kc_comm *comm, int *n_ranks, int *user_rank, int *device);
/* after kc_dwa_evaluate: ONE ncclAllReduce(1 x int64, ncclMin) of the packed key in
 * the device record, on the context's stream, and the hand-off of the reduced
 * record to the host (kc_dwa_fetch_result then returns the GLOBAL winner: found,
 * cost, raw_index; index / n_admissible stay the shard's).  Building block for
 * callers with a protocol of their own; kc_dwa_cycle_sharded does not use it. */
int kc_dwa_allreduce_best(kc_dwa *ctx, kc_comm *comm);
/* DWA::findBestPath body of a sharded controller: this context's share rolled out
 * and scored (single launch when it fits), ONE all-reduce(int64 x (2 + world x
 * words), min) of the exchange record -- best key, error word, every rank's
 * admissible bitmap -- and the result, the same on every rank: found, cost,
 * raw_index, index (the reference's admissible-only numbering over ALL ranks) and
 * n_admissible / n_samples over all ranks.  Collective: every rank of the
 * communicator calls it with the same start / num_points, after
 * kc_dwa_set_shard_rule(rank, world, ...) (a world of one may use kc_dwa_set_shard).
 * Errors are collective too: when any rank fails (a call failed before the exchange,
 * or its device error word is set) EVERY rank returns an error for this cycle and all
 * of them have taken part in exactly one all-reduce, so the next cycle pairs up again. */
int kc_dwa_cycle_sharded(kc_dwa *ctx, kc_comm *comm, const kc_state *start, size_t num_points,
                         kc_result *out);
/* The same exchange for a cycle whose LAST cost terms the host has added -- custom cost callbacks of a sharded
 * DWA ("evaluated on host over gathered paths"; cost_evaluator.cpp:96-100: customTrajCostsPtrs_
 * after the built-in terms, total += weight * cost in float-from-double).  Every rank runs kc_dwa_cycle on its
 * share, reads its admissible rows (kc_dwa_get_samples: GLOBAL raw indices, device totals), adds the callbacks
 * in registration order and hands its own best {found, cost, raw_index} in; the record that is all-reduced is
 * kc_dwa_cycle_sharded's (this key, the error word, the admissible bitmap of the cycle just run), the result the
 * same on every rank.  status != 0: this rank failed before -- it still takes part and every rank fails the
 * cycle.  Collective. */
int kc_dwa_exchange_best(kc_dwa *ctx, kc_comm *comm, int status, int found, float cost, int64_t raw_index,
                         kc_result *out);
/* the winner's index in the reference's admissible-only numbering: admissible
 * samples in front of it on every shard, one ncclAllReduce(1 x int64, ncclSum).
 * Collective.  kc_dwa_cycle_sharded returns that index already; this remains for
 * callers of kc_dwa_allreduce_best. */
int kc_dwa_global_index(kc_dwa *ctx, kc_comm *comm, int64_t global_raw_index, int64_t *index_out);

/* decode helpers for the packed key (pure host functions) */
float kc_key_cost(int64_t key);
int64_t kc_key_index(int64_t key);
int64_t kc_key_pack(float cost, int64_t index);

/* HIP-event timing of the kernels launched by the last cycle, on the stream
 * they were launched on (bench.py roofline leg).  enable=1 records events
 * around each kernel; names/ms arrays of capacity cap, returns count. */
int kc_dwa_timing_enable(kc_dwa *ctx, int enable);
int kc_dwa_timing_get(kc_dwa *ctx, const char **names, float *ms, size_t cap,
                      size_t *count_out);

/* ------------------------------------------------------------------------ */
/* LocalMapper                                                              */
/* ------------------------------------------------------------------------ */
typedef struct kc_mapper kc_mapper;

/* LocalMapper / LocalMapperGPU ctor (mapping/local_mapper.h:14-56,
 * local_mapper_gpu.h:15-66) -- the scan -> grid subset.  KC_ERR_RANGE for a
 * sensor whose offset position / resolution is not below 2^30 cells
 * (DESIGN.md §5). */
int kc_mapper_create(int grid_height, int grid_width, float resolution,
                     const float laserscan_position[3],
                     float laserscan_orientation, size_t max_scan_size,
                     int device, kc_mapper **out);
void kc_mapper_destroy(kc_mapper *ctx);
int kc_mapper_set_stream(kc_mapper *ctx, void *hip_stream);
/* LocalMapper::scanToGrid (local_mapper.cpp:204-220) with the CPU semantics
 * (super-cover Bresenham, line_drawing.h:55-124); grid_out is the
 * Eigen::MatrixXi layout: int32, column-major, cell (i,j) at i + j*height.
 * Same cell values as the reference CPU mapper, bit for bit. */
int kc_mapper_scan_to_grid(kc_mapper *ctx, const double *angles,
                           const double *ranges, size_t n, int32_t *grid_out);
/* same, but the grid stays on the device (no D2H); the address of the int32
 * column-major device grid is returned by kc_mapper_grid_device.  Plain scans
 * alternate between two device grids (the scan that follows clears the other
 * one while it runs): ask for the address after every scan; the grid of a scan
 * stays intact until the NEXT scan's kernels have run. */
int kc_mapper_scan_to_grid_device(kc_mapper *ctx, const double *angles,
                                  const double *ranges, size_t n);
int kc_mapper_grid_device(kc_mapper *ctx, void **dev_grid_int32);

/* LocalMapper's second ctor (local_mapper.h:58-103): the inverse sensor model of
 * the Bayesian update.  kc_mapper_enable_bayes allocates the probability grids
 * (float, column-major like the occupancy grid) and fills the previous grid
 * with p_prior (local_mapper.h:81-83). */
typedef struct kc_bayes_params {
  float p_prior, p_occupied, p_empty, range_sure, range_max, wall_size;
} kc_bayes_params;
int kc_mapper_enable_bayes(kc_mapper *ctx, const kc_bayes_params *params);
/* LocalMapper::scanToGridBaysian (local_mapper.cpp:161-202,222-241) in the
 * reference's single-thread order: the probability of a cell is
 * updateGridCellProbability (:106-125) of the LAST beam that crosses it and of
 * the previous grid; untouched cells hold p_prior.  The occupancy grid is the
 * one scanToGrid gives.  Parity is against this build's restatement only (the
 * reference tests print these grids without asserting on them). */
int kc_mapper_scan_to_grid_bayes(kc_mapper *ctx, const double *angles, const double *ranges,
                                 size_t n, int32_t *grid_out, float *prob_out);
int kc_mapper_scan_to_grid_bayes_device(kc_mapper *ctx, const double *angles,
                                        const double *ranges, size_t n);
/* device addresses of gridDataProb and (optional) previousGridDataProb; the
 * previous grid lives in two buffers that swap on every kc_mapper_warp_previous:
 * ask again after a warp */
int kc_mapper_prob_device(kc_mapper *ctx, void **dev_prob_f32, void **dev_prev_f32);
/* LocalMapper::getPreviousGridInCurrentPose (local_mapper.cpp:17-78): bilinear
 * warp of the previous probability grid, in place (stream-ordered).
 * KC_ERR_RANGE, before anything is queued and with the previous grid as it
 * was, for a pose whose offset position / resolution is not below 2^30 cells
 * on either axis (NaN and inf included: kc_mapper_create's rule);
 * a non-finite orientation is accepted and gives p_prior everywhere.
 * Probabilities fed back scan after scan saturate: cells reach exactly 1.0f
 * and 0.0f (benchmark sensor model) and then never move, or settle at the
 * rounding fixed points 1 - 2^-24 and 2^-52 (defaults); subnormals are kept.
 * Where the reference's arithmetic gives NaN (previous 1 with p_empty 0,
 * p_prior 0 or 1, range_max 0, NaN / inf / out-of-[0, 1] previous values) the
 * result is some NaN: its sign and payload are not part of the contract. */
int kc_mapper_warp_previous(kc_mapper *ctx, const float current_position_in_previous_pose[2],
                            double current_orientation_in_previous_pose);
int kc_mapper_get_previous_prob(kc_mapper *ctx, float *prob_out);
/* not in the reference, whose previous grid is only ever warped: upload a
 * previous grid (in != NULL) or feed the last scan's probabilities back on the
 * device (in == NULL) */
int kc_mapper_set_previous_prob(kc_mapper *ctx, const float *in);
int kc_mapper_sync(kc_mapper *ctx);
int kc_mapper_timing_enable(kc_mapper *ctx, int enable);
int kc_mapper_timing_get(kc_mapper *ctx, const char **names, float *ms,
                         size_t cap, size_t *count_out);

/* ------------------------------------------------------------------------ */
/* Raw point cloud -> laserscan                           */
/* ------------------------------------------------------------------------ */
typedef struct kc_cloud kc_cloud;

/* scratch for clouds of up to max_bytes bytes / max_bins angular bins (both
 * grow on demand) */
int kc_cloud_create(size_t max_bytes, size_t max_bins, int device, kc_cloud **out);
void kc_cloud_destroy(kc_cloud *ctx);
/* pointCloudToLaserScanFromRaw (utils/pointcloud.h:116-177: angle_step > 0,
 * bins = ceil(2 pi / angle_step), angles_out[i] = i * angle_step; and
 * :205-259: angle_step <= 0, num_bins bins, angles_out may be NULL).  data is
 * a PointCloud2-style byte buffer (float32 x, y, z at the given byte offsets of
 * every point_step-byte record; rows row_step bytes apart); data_on_device != 0
 * means `data` is a device address on ctx's device.  ranges_out[bin] = the
 * smallest planar distance of the points of that bin that pass the origin and z
 * filters, max_range where there is none: the same doubles as the reference's
 * CPU loop (bins from the host libm's atan2f: the device bins every point, the
 * few within 1e-6 rad of a bin edge are re-binned on the host).  Points with a
 * non-finite x or y are skipped (the reference indexes out of bounds). */
int kc_cloud_to_laserscan(kc_cloud *ctx, const int8_t *data, size_t nbytes,
                          int data_on_device, int point_step, int row_step,
                          int height, int width, int x_offset, int y_offset,
                          int z_offset, double max_range, double min_z,
                          double max_z, double angle_step, int num_bins,
                          double *ranges_out, double *angles_out, size_t cap,
                          size_t *bins_out);
/* the same for x / y / z fields of any PointCloud2 datatype (PointFieldType, utils/pointcloud.h:37-46:
 * ids 1-8), decoded as load_and_cast_val does (:49-87: byte by byte, value cast to float) -- what the
 * reference's device paths accept (local_mapper_gpu.cpp:117-140, critical_zone_check_gpu.h:36-53); the
 * bounds check uses the field's own size.  KC_FIELD_FLOAT32 is kc_cloud_to_laserscan.  The reference
 * holds no vector for the other types: parity is against this build's restatement. */
enum { KC_FIELD_INT8 = 1, KC_FIELD_UINT8 = 2, KC_FIELD_INT16 = 3, KC_FIELD_UINT16 = 4, KC_FIELD_INT32 = 5,
       KC_FIELD_UINT32 = 6, KC_FIELD_FLOAT32 = 7, KC_FIELD_FLOAT64 = 8 };
int kc_cloud_to_laserscan_typed(kc_cloud *ctx, const int8_t *data, size_t nbytes,
                                int data_on_device, int point_step, int row_step,
                                int height, int width, int x_offset, int y_offset,
                                int z_offset, int field_type, double max_range, double min_z,
                                double max_z, double angle_step, int num_bins,
                                double *ranges_out, double *angles_out, size_t cap,
                                size_t *bins_out);
/* Points -> 2-D occupancy grid: the two loops of readPCDToOccupancyGrid
 * (utils/pointcloud.h:468-540) over a cloud that crosses to the device once.
 *
 * kc_cloud_grid_extent is the bounding-box pass and the sizes (:486-503).
 * data: n_points records of point_step bytes with float32 x, y, z at the given
 * byte offsets (a packed (N, 3) float array is point_step 12, offsets 0 / 4 / 8);
 * data_on_device as in kc_cloud_to_laserscan, and such a cloud is read in place
 * (KC_ERR_INVALID, before any read, unless it is device memory of ctx's device
 * and its nbytes lie inside one allocation); it must stay valid until the grid
 * call that follows.  origin_out = {min_x, min_y, 0}; cells = (int)ceilf((max -
 * min) / grid_resolution) per axis, in float.  A cloud with no extent on an axis
 * has 0 cells on it.  Defined here, undefined in the reference: a point with a
 * non-finite x or y takes part in neither pass; an empty cloud, or one in which
 * no point has both x and y finite, gives 0 x 0 cells and origin {0, 0, 0}
 * (:482-484).  The sign of
 * a zero origin depends on point order there and is not defined here.
 * KC_ERR_RANGE: grid_resolution not a positive finite float (before any launch),
 * or more than KC_CLOUD_GRID_MAX_CELLS cells on an axis or in all (the
 * reference overflows its int; nothing is allocated for the grid). */
#define KC_CLOUD_GRID_MAX_CELLS (1u << 30)
int kc_cloud_grid_extent(kc_cloud *ctx, const int8_t *data, size_t nbytes, int data_on_device,
                         int point_step, size_t n_points, int x_offset, int y_offset, int z_offset,
                         float grid_resolution, float origin_out[3], int *cells_x, int *cells_y);
/* the classify-and-scatter pass (:506-536) over the cloud of the last extent
 * call: cell = (int)((v - min) * (1.0f / grid_resolution)) per axis, a point
 * outside [0, cells) on either axis is dropped (the points on the max edge of
 * an extent that is a whole multiple of the resolution are); class 100 if
 * z > z_ground_limit && z <= robot_height, else 0 if z <= z_ground_limit, else
 * -1; a cell holds the maximum over its points, -1 where there is none.
 * grid_out: int8, column-major [cells_x x cells_y], cell (i, j) at
 * i + j * cells_x (Eigen's layout).  Bit-equal to the reference's loop whatever
 * the order of the points.  KC_ERR_STATE without an extent call, KC_ERR_RANGE
 * when the cells do not fit cap. */
int kc_cloud_grid_fill(kc_cloud *ctx, float z_ground_limit, float robot_height,
                       int8_t *grid_out, size_t cap);
/* the same pass without the copy to the host: *dev_grid_int8 is the grid on
 * ctx's device (NULL for an empty grid), valid until the next call on ctx */
int kc_cloud_grid_device(kc_cloud *ctx, float z_ground_limit, float robot_height,
                         void **dev_grid_int8);
/* orders ctx's next reads after the work queued so far on a producer's stream
 * (a hipStream_t; NULL = the legacy default stream): for clouds another
 * library wrote on the device (kc_depth_after_stream is the same for frames) */
int kc_cloud_after_stream(kc_cloud *ctx, void *stream);
/* points the last call sent back to the host for exact binning */
int kc_cloud_last_rebinned(kc_cloud *ctx, size_t *count_out);
int kc_cloud_timing_enable(kc_cloud *ctx, int enable);
int kc_cloud_timing_get(kc_cloud *ctx, const char **names, float *ms, size_t cap,
                        size_t *count_out);

/* ------------------------------------------------------------------------ */
/* CriticalZoneChecker                                    */
/* ------------------------------------------------------------------------ */
typedef struct kc_zone kc_zone;

/* CriticalZoneChecker ctor + preset (utils/critical_zone_check.cpp:13-83;
 * critical_zone_check_gpu.h ctor for the device variant).  shape / dims as in
 * kc_dwa_params; sensor_rot_xyzw is the Eigen::Vector4f of the reference
 * ((x, y, z, w), not normalised by the reference either); critical_angle in
 * degrees; angles = the scan angles the index sets are preset for.
 * KC_ERR_INVALID when slowdown_distance <= critical_distance (:52-56). */
int kc_zone_create(int shape, const float *dims, int ndims,
                   const float sensor_pos[3], const float sensor_rot_xyzw[4],
                   float critical_angle, float critical_distance,
                   float slowdown_distance, const double *angles, size_t n,
                   float min_height, float max_height, float range_max,
                   int device, kc_zone **out);
void kc_zone_destroy(kc_zone *ctx);
/* check(ranges, forward) (:85-117): 0.0 stop, (0, 1) slow-down factor, 1.0 clear;
 * ranges has one entry per preset angle */
int kc_zone_check(kc_zone *ctx, const double *ranges, size_t n, int forward,
                  float *factor_out);
/* check(raw cloud, forward) (:119-131): cloud -> ranges over the preset number
 * of bins (kc_cloud_to_laserscan semantics) -> check */
int kc_zone_check_cloud(kc_zone *ctx, const int8_t *data, size_t nbytes,
                        int point_step, int row_step, int height, int width,
                        int x_offset, int y_offset, int z_offset, int forward,
                        float *factor_out);
/* ... with the cloud_field_type of CriticalZoneCheckerGPU's constructor (critical_zone_check_gpu.h:36-53) */
int kc_zone_check_cloud_typed(kc_zone *ctx, const int8_t *data, size_t nbytes,
                              int point_step, int row_step, int height, int width,
                              int x_offset, int y_offset, int z_offset, int field_type, int forward,
                              float *factor_out);
/* the preset index sets (tests / debugging) */
int kc_zone_indices(kc_zone *ctx, int forward, int64_t *out, size_t cap,
                    size_t *count_out);

/* ------------------------------------------------------------------------ */
/* Deformable Virtual Zone (kompass_core/algorithms/dvz.py)                 */
/* ------------------------------------------------------------------------ */
typedef struct kc_dvz kc_dvz;

/* The zone of DeformableVirtualZone as update_zone_size / _init_constant_zone_
 * parameters (dvz.py:105-117, 151-172) leave it: zone_major_radius,
 * zone_minor_radius, zone_center_shift_x / _y, zone_ori_shift.  The constant
 * term C of _get_undeformed_radius (:232-236) is formed from them by the call. */
typedef struct kc_dvz_zone {
  double major_radius, minor_radius;
  double center_shift_x, center_shift_y;
  double ori_shift;
} kc_dvz_zone;

/* A context for scans of up to max_beams (1 .. 2^24) beams on `device`. */
int kc_dvz_create(int device, size_t max_beams, kc_dvz **out);
void kc_dvz_destroy(kc_dvz *ctx);
/* get_total_deformation's loop (dvz.py:372-404) in one launch: per beam the
 * undeformed radius (_get_undeformed_radius, :213-245, squares as products),
 * the deformed radius (_get_deformation_radius, :247-266) and, for a deformed
 * beam, (undeformed - deformed) / deformed and that times convert_to_0_2pi(angle).
 * out = {sum of the first, sum of the second, number of deformed beams}, summed
 * in double in a fixed order (the same bits on every call); the caller
 * normalises (_regulate_deformation).  radii_or_null: n deformed radii
 * (deformation_plot).  n == 0 launches nothing and gives zeros.  KC_ERR_INVALID
 * for null pointers or a radius that is not > 0, KC_ERR_RANGE for n above the
 * context's capacity, both before any device use. */
int kc_dvz_deform(kc_dvz *ctx, const kc_dvz_zone *zone, const double *angles,
                  const double *ranges, size_t n, double out[3],
                  double *radii_or_null);

/* ------------------------------------------------------------------------ */
/* DepthDetector: 2-D detections -> 3-D boxes (vision/depth_detector.cpp)    */
/* ------------------------------------------------------------------------ */
typedef struct kc_depth kc_depth;

/* DepthDetector ctor (depth_detector.cpp:10-42): depth_range = (min, max) in
 * meters, camera_in_body from the translation and the (x, y, z, w) quaternion
 * (not normalised, as in the reference), focal / principal = (fx, fy) /
 * (cx, cy).  KC_ERR_INVALID unless factor is finite, > 0 and 65535 * factor is
 * finite in float (every converted depth is then finite).  Needs no device: the
 * first compute call opens the stream (KC_ERR_HIP there when none is usable). */
int kc_depth_create(const float depth_range[2], const float cam_pos[3],
                    const float cam_rot_xyzw[4], const float focal[2],
                    const float principal[2], float factor, int device,
                    kc_depth **out);
void kc_depth_destroy(kc_depth *ctx);
/* updateBoxes + get3dDetections (:44-81, :84-151).  img: a rows x cols uint16
 * frame, element (r, c) at img[r * row_stride + c * col_stride] (any memory
 * order); data_on_device != 0: img is a device address on ctx's device and is
 * read in place (KC_ERR_INVALID, before any read, unless hipPointerGetAttributes
 * reports device memory of ctx's device and the whole frame lies inside that
 * allocation), else the bounding rectangle of the clipped boxes is uploaded.
 * boxes: n x (top.x, top.y, size.x, size.y); a box covers rows top.y ..
 * top.y + size.y and columns top.x .. top.x + size.x, inclusive, computed in
 * 64 bits; pixels outside the frame are skipped (the reference reads out of
 * bounds).  state: (x, y, yaw) of the robot, or NULL to keep the previous
 * body_in_world (the identity at first).  Per kept box (> 1 depth in range),
 * in input order: out[6 m ..] = center[3], size[3] in the world frame and
 * kept_index[m] = its input index; cap >= n. */
int kc_depth_boxes(kc_depth *ctx, const uint16_t *img, int data_on_device,
                   int64_t rows, int64_t cols, int64_t row_stride,
                   int64_t col_stride, const int32_t *boxes, size_t n,
                   const double *state, float *out, int32_t *kept_index,
                   size_t cap, size_t *count_out);
/* the raw per-box statistics of the same pass (tests): count_out[i] = depths
 * kept, stats_out[4 i ..] = median, mad, min_d, max_d (zeros when count <= 1) */
int kc_depth_box_stats(kc_depth *ctx, const uint16_t *img, int data_on_device,
                       int64_t rows, int64_t cols, int64_t row_stride,
                       int64_t col_stride, const int32_t *boxes, size_t n,
                       int64_t *count_out, float *stats_out);
/* orders ctx's next reads after the work queued so far on a producer's stream
 * (a hipStream_t; NULL = the legacy default stream), by an event the context
 * stream waits for: no host wait.  For frames another library wrote on the
 * device. */
int kc_depth_after_stream(kc_depth *ctx, void *stream);
/* bytes of frame the last call uploaded (0 for a frame on the device) */
int kc_depth_last_upload(kc_depth *ctx, size_t *bytes_out);
int kc_depth_timing_enable(kc_depth *ctx, int enable);
int kc_depth_timing_get(kc_depth *ctx, const char **names, float *ms, size_t cap,
                        size_t *count_out);

/* ------------------------------------------------------------------------ */
/* Grid planner: occupancy grid -> collision-free path      */
/* ------------------------------------------------------------------------ */
typedef struct kc_planner kc_planner;

/* Nothing in the reference to cite for the method: its planning submodule wraps
 * OMPL (planning/ompl.h:18-89), which stays out of scope.  What is kept is the
 * shape of that surface (setSpaceBoundsFromMap / setupProblem / solve / getPath /
 * getCost, ompl.h:37-74), in the host class Planning::GridPlanner; this ABI is
 * the integer core under it and works in cells.
 *
 * A grid is width x height cells, cell (i, j) at i + j * width: i runs along x
 * and is the fast index.  That is the LocalMapper's layout (kc_mapper_grid_device:
 * int32, width = grid_height, height = grid_width) and the PCD grid's
 * (kc_cloud_grid_device: int8, width = cells_x, height = cells_y).  elem_bytes is
 * 4 or 1 accordingly.  KC_OCCUPIED cells block, KC_UNEXPLORED cells block unless
 * allow_unknown, every other value is free.  KC_ERR_RANGE above
 * KC_PLANNER_MAX_CELLS cells (14 * cells must fit 32 bits). */
#define KC_PLANNER_MAX_CELLS (1u << 28)
#define KC_PLANNER_MAX_RADIUS_CELLS 254
int kc_planner_create(int device, kc_planner **out);
void kc_planner_destroy(kc_planner *ctx);
/* the grid from host memory (one copy to the device) */
int kc_planner_set_grid_host(kc_planner *ctx, const void *grid, int elem_bytes, int width, int height);
/* the grid where it lies on ctx's device: read in place, no host round trip
 * (KC_ERR_INVALID, before any read, unless it is device memory of ctx's device,
 * inside one allocation and aligned to its cells).  The grid must be finished
 * (kc_cloud_grid_device returns it so; kc_mapper_sync after a device scan); it is
 * not read after the call returns. */
int kc_planner_set_grid_device(kc_planner *ctx, const void *dev_grid, int elem_bytes, int width, int height);
/* orders ctx's next read of a device grid after the work queued so far on a
 * producer's stream (a hipStream_t; NULL = the legacy default stream), as
 * kc_cloud_after_stream does: no host wait */
int kc_planner_after_stream(kc_planner *ctx, void *stream);
/* Validity, cost field and the start's status for one (start, goal) pair.
 *  - a cell is invalid when a blocking cell (bi, bj) has (bi - i)^2 + (bj - j)^2
 *    <= r2; cells outside the grid do not block.  KC_ERR_RANGE when r2 reaches
 *    further than KC_PLANNER_MAX_RADIUS_CELLS cells.
 *  - field[cell] = the exact length of the shortest 8-connected walk over valid
 *    cells to the goal cell, a straight step 10 and a diagonal one 14, a diagonal
 *    step only between two valid orthogonal neighbours; 0xFFFFFFFF where there
 *    is none (and everywhere when the goal is outside the grid or invalid).
 *  - *status_out: KC_PLAN_FOUND or why there is no path; that is not an error,
 *    the call returns KC_OK.  *cost_out = field[start] (0xFFFFFFFF without a
 *    path), *passes_out = relaxation passes the field needed, the one that found
 *    nothing left to change included.
 * KC_ERR_RANGE if the field still changes after cells + 1 passes (it cannot: every
 * pass but the last settles a cell); KC_ERR_STATE without a grid. */
enum { KC_PLAN_FOUND = 0, KC_PLAN_START_OUTSIDE = 1, KC_PLAN_GOAL_OUTSIDE = 2, KC_PLAN_START_INVALID = 3,
       KC_PLAN_GOAL_INVALID = 4, KC_PLAN_UNREACHABLE = 5,
       KC_PLAN_NO_FRONTIER = 6 /* kc_planner_explore alone: no frontier is kept */ };
int kc_planner_solve(kc_planner *ctx, const int start_cell[2], const int goal_cell[2], uint32_t r2,
                     int allow_unknown, int *status_out, uint32_t *cost_out, int *passes_out);
/* the last solve's cost field and validity map (1 valid, 0 invalid), laid out as
 * the grid (tests); either pointer may be NULL */
int kc_planner_get_field(kc_planner *ctx, uint32_t *field_out, uint8_t *valid_out, size_t cap);
/* The kept cost field where it lies on the device (width * height uint32, cell (I, J) at
 * I + J * width, 0xFFFFFFFF: no walk reaches the goal), its shape and the planner's stream
 * (a hipStream_t), for a reader that orders itself behind that stream: kc_mppi_step with a field
 * attached.  Host only, queues nothing.  The field's two buffers alternate between solves, so
 * the pointer holds until the next solve-type call and a reader asks again after each.
 * KC_ERR_STATE unless the last solve-type call was kc_planner_solve or kc_planner_replan (plain
 * or with the clearance cost): before any solve, after kc_planner_solve_oriented,
 * kc_planner_solve_car and kc_planner_explore. */
int kc_planner_field_device(kc_planner *ctx, const uint32_t **field_out, int *width_out, int *height_out, void **stream_out);
/* the path of the last solve by steepest descent: from the start cell, the
 * neighbour with the smallest field value among those a step may go to (valid,
 * and for a diagonal between two valid orthogonal neighbours), the first of
 * them in the order E, N, W, S, NE, NW, SW, SE ((+1, 0), (0, +1), (-1, 0),
 * (0, -1), (+1, +1), (-1, +1), (-1, -1), (+1, -1)), until the goal cell.
 * cells_ij_out: (i, j) pairs, start first; NULL asks for the count only.
 * Zero points when the last solve found no path. */
int kc_planner_get_path(kc_planner *ctx, int32_t *cells_ij_out, size_t cap_points, size_t *count_out);
/* The clearance cost (rules 6 to 8), off by default.
 *  - clear2[cell] = the smallest (bi - i)^2 + (bj - j)^2 over blocking cells when
 *    that is <= c2, KC_PLANNER_CLEAR_FAR otherwise; pen[cell] =
 *    pen_by_d2[clear2[cell]], 0 for CLEAR_FAR cells.
 *  - a step pays for the cell it leaves: field[goal] = 0, field[a] = pen[a] + min
 *    over the allowed steps a -> b of (step + field[b]).  kc_planner_solve answers
 *    KC_ERR_RANGE when (14 + max(pen_by_d2)) * cells > 0xFFFFFFFE.
 *  - the walk takes the neighbour with the smallest field + step (the same tie
 *    order), so the steps and the penalties of the cells left sum to *cost_out.
 * Validity, status and passes keep their meaning; with the cost off every output
 * is what it is without these three calls. */
#define KC_PLANNER_CLEAR_FAR 0xFFFFu
/* n == c2 + 1 entries; c2 == 0 or a NULL table switches the clearance cost off.
   KC_ERR_RANGE for c2 > 254^2, KC_ERR_INVALID for n != c2 + 1.  Forgets the last solve. */
int kc_planner_set_clearance_cost(kc_planner *ctx, uint32_t c2, const uint32_t *pen_by_d2, size_t n);
/* the last solve's clear2 and per-cell penalty, laid out as the grid; either may be NULL;
   KC_ERR_STATE before a solve or with the clearance cost off */
int kc_planner_get_clearance(kc_planner *ctx, uint16_t *clear2_out, uint32_t *penalty_out, size_t cap);
/* smallest clear2 along the last path (KC_PLANNER_CLEAR_FAR: nothing within reach); KC_ERR_STATE without a path */
int kc_planner_path_clearance(kc_planner *ctx, uint32_t *min_clear2_out);
/* The any-angle path (rules 9 to 12), on request only.
 *  - the segment between cells a and b touches cell (i, j) when (i, j) lies in the
 *    bounding box of a and b and 2 |dx (j - ay) - dy (i - ax)| <= |dx| + |dy|; it is
 *    clear when every touched cell is valid and, while a clearance cost is set, holds
 *    clear2 >= the walk's own smallest clear2 (kc_planner_path_clearance).
 *  - from index s = 0 of the walk p[0 .. n-1] (kc_planner_get_path) the largest t in
 *    (s, min(n - 1, s + max_span)] with p[s] -> p[t] clear is kept, s + 1 untested,
 *    then s = t, until the last index.
 * *count_out = kept indices, first and last of the walk among them; *min_clear2_out =
 * the smallest clear2 over the kept cells and the touched cells of the kept segments
 * that were tested (KC_PLANNER_CLEAR_FAR with the clearance cost off); either may be
 * NULL.  Walks first if needed; one launch, kept per (solve, max_span).  KC_ERR_STATE
 * unless the last solve found a path, KC_ERR_RANGE for max_span outside
 * 1 .. KC_PLANNER_MAX_SPAN.  Cost, path and path clearance keep describing the walk. */
#define KC_PLANNER_MAX_SPAN 1024
int kc_planner_shortcut(kc_planner *ctx, int max_span, size_t *count_out, uint32_t *min_clear2_out);
/* the last kc_planner_shortcut's kept cells ((i, j) pairs) and their indices into the
 * walk, ascending; either may be NULL, both NULL asks for the count only;
 * KC_ERR_STATE without one (a new solve forgets it) */
int kc_planner_get_shortcut(kc_planner *ctx, int32_t *cells_ij_out, int32_t *index_out, size_t cap, size_t *count_out);
/* The oriented box footprint (rules 13 to 18), off by default.  The
 * state is (cell, class); class k = 0 .. 3 is the box's length axis along (1, 0),
 * (1, 1), (0, 1), (-1, 1).  a2 / b2: the squared half length / half width in cells
 * (rule 2's R2 formula on x / 2 + margin and y / 2 + margin).
 *  - (cell, k) is valid when no blocking cell lies at cell + (di, dj) for an offset of
 *    mask k: k = 0: di^2 <= a2 and dj^2 <= b2; k = 2: dj^2 <= a2 and di^2 <= b2;
 *    k = 1: (di + dj)^2 <= 2 a2 and (dj - di)^2 <= 2 b2; k = 3: (dj - di)^2 <= 2 a2 and
 *    (di + dj)^2 <= 2 b2.  Cells outside the grid do not block.
 *  - a cell is turn-valid when no blocking cell has di^2 + dj^2 <= a2 + b2 (the disc
 *    test of kc_planner_solve with r2 = a2 + b2; it contains all four masks).
 * turn10: the cost of a turn by one class (a straight step is 10), 1 .. 10000.
 * a2 = 0 switches the mode off and forgets the last solve; every output of
 * kc_planner_solve is then what it is without this call.  KC_ERR_RANGE for turn10
 * outside 1 .. 10000 and for a2 + b2 > KC_PLANNER_MAX_RADIUS_CELLS^2; KC_ERR_STATE while a
 * clearance cost is set (and kc_planner_set_clearance_cost answers the same while
 * this mode is on).  While it is on, kc_planner_solve answers KC_ERR_STATE. */
int kc_planner_set_oriented(kc_planner *ctx, uint32_t a2, uint32_t b2, uint32_t turn10);
/* Validity, state field and the start's status for (start cell, start class) -> goal cell.
 *  - field[k][cell] = 0 for every valid (goal, k); otherwise the minimum of cost +
 *    field[next] over the moves (cell, k) -> (cell +- d_k, k), both states valid, 10 for
 *    k = 0, 2 and 14 for k = 1, 3, and the turns (cell, k) -> (cell, k +- 1 mod 4) at
 *    turn10 where the cell is turn-valid; 0xFFFFFFFF where nothing arrives.
 *  - *status_out as kc_planner_solve: KC_PLAN_START_INVALID when (start, start_class)
 *    is invalid, KC_PLAN_GOAL_INVALID when no class is valid at the goal, then
 *    KC_PLAN_UNREACHABLE.  *cost_out = field[start_class][start], the turns included.
 * KC_ERR_RANGE when max(14, turn10) * 4 * cells > 0xFFFFFFFE, or if the field still
 * changes after 4 * cells + 1 passes (it cannot); KC_ERR_STATE without a grid or with
 * the mode off; KC_ERR_INVALID for a class outside 0 .. 3. */
int kc_planner_solve_oriented(kc_planner *ctx, const int start_cell[2], int start_class, const int goal_cell[2],
                              int allow_unknown, int *status_out, uint32_t *cost_out, int *passes_out);
/* the last oriented solve's field (four layers of width x height cells, class 0
 * first), validity (a byte a cell, bit k = class k valid) and turn validity (1 / 0),
 * laid out as the grid; any may be NULL; cap: cells (field4_out holds 4 * cap words);
 * KC_ERR_STATE unless the last solve was kc_planner_solve_oriented */
int kc_planner_get_oriented_field(kc_planner *ctx, uint32_t *field4_out, uint8_t *valid4_out, uint8_t *turn_valid_out, size_t cap);
/* the state walk of the last oriented solve: from (start, start_class) the allowed
 * transition with the smallest field[next] + cost, the first among equals in the
 * order: the class's direction that comes first in E, N, W, S, NE, NW, SW, SE, its
 * opposite, the turn to k + 1, the turn to k - 1; that minimum equals field[current].
 * states_ijk_out: (i, j, k) triples, start first; NULL asks for the count only; zero
 * states when the solve found no path.  kc_planner_get_path then gives the same
 * walk's cells with the repeated cell of a turn collapsed; kc_planner_shortcut answers
 * KC_ERR_STATE (a segment at an arbitrary angle has no class). */
int kc_planner_get_oriented_path(kc_planner *ctx, int32_t *states_ijk_out, size_t cap, size_t *count_out);
/* Car motion (rules 27 to 36), off by default.  The state is (cell,
 * heading); heading h = 0 .. 7 is the direction the front points: E, NE, N, NW, W, SW, S,
 * SE = D[h].  step(h) is 10 for even h, 14 for odd h.  Six primitives out of (c, h), n =
 * turn_cells, rw = reverse_weight, tried and ranked in this order:
 *   0 S   one unit step along +D[h]                                cost step(h)
 *   1 L   n steps along +D[h], then n along +D[h+1] in heading h+1   24 n
 *   2 R   n steps along +D[h], then n along +D[h-1] in heading h-1   24 n
 *   3 B   one unit step along -D[h]                                rw step(h)
 *   4 BL  n steps along -D[h], then n along -D[h-1] in heading h-1   rw 24 n
 *   5 BR  n steps along -D[h], then n along -D[h+1] in heading h+1   rw 24 n
 * A unit step from (c, h) to c +- D[h] is allowed when both cells are inside the grid
 * and valid in heading h (a cell outside the grid is never stepped on), and, with the
 * disc and odd h, both orthogonal neighbours it passes between are valid.  An arc is
 * allowed when each of its 2 n unit steps is.  There is no turn in place, and with
 * rw = 0 no B, BL, BR.
 * a2 = b2 = 0: the disc of kc_planner_solve_car's r2, every heading alike.  a2 > 0: the
 * box of kc_planner_set_oriented's rule, heading h valid where class h & 3 is; turn
 * validity plays no part.  turn_cells = 0 switches the mode off and forgets the last
 * solve; every other call then answers what it answers without this one.
 * KC_ERR_RANGE for turn_cells outside 0 .. KC_PLANNER_MAX_TURN_CELLS, reverse_weight above
 * KC_PLANNER_MAX_REVERSE_WEIGHT and a2 + b2 > KC_PLANNER_MAX_RADIUS_CELLS^2; KC_ERR_STATE
 * while a clearance cost or the oriented mode is set (and their setters answer the
 * same while this mode is on).  While it is on, kc_planner_solve, kc_planner_solve_oriented,
 * kc_planner_replan and kc_planner_explore answer KC_ERR_STATE. */
#define KC_PLANNER_MAX_TURN_CELLS 8
#define KC_PLANNER_MAX_REVERSE_WEIGHT 16
int kc_planner_set_car(kc_planner *ctx, int turn_cells, uint32_t reverse_weight, uint32_t a2, uint32_t b2);
/* Validity, moves, state field and the start's status for (start cell, start heading) ->
 * (goal cell, goal heading); goal_heading -1: any.
 *  - field[h][cell] = 0 for the valid goal states; otherwise the minimum over the
 *    allowed primitives of cost + field[target]; 0xFFFFFFFF where nothing arrives.
 *  - *status_out as kc_planner_solve: KC_PLAN_START_INVALID when (start, start_heading)
 *    is invalid, KC_PLAN_GOAL_INVALID when no goal state is valid, then
 *    KC_PLAN_UNREACHABLE.  *cost_out = field[start_heading][start].
 * r2 is the disc's and ignored with a box.  KC_ERR_RANGE when 24 * n * max(rw, 1) * 8 *
 * cells > 0xFFFFFFFE, or if the field still changes after 8 * cells + 1 passes (it
 * cannot); KC_ERR_STATE without a grid or with the mode off; KC_ERR_INVALID for a start
 * heading outside 0 .. 7 or a goal heading outside -1 .. 7. */
int kc_planner_solve_car(kc_planner *ctx, const int start_cell[2], int start_heading, const int goal_cell[2], int goal_heading,
                         uint32_t r2, int allow_unknown, int *status_out, uint32_t *cost_out, int *passes_out);
/* the last car solve's field (eight layers of width x height cells, heading 0 first),
 * moves (eight layers of bytes, bit p = primitive p allowed out of the state) and
 * validity (a byte a cell, bit h = heading h valid), laid out as the grid; any may be
 * NULL; cap: cells (field8_out holds 8 * cap words, moves8_out 8 * cap bytes);
 * KC_ERR_STATE unless the last solve was kc_planner_solve_car */
int kc_planner_get_car_field(kc_planner *ctx, uint32_t *field8_out, uint8_t *moves8_out, uint8_t *valid_out, size_t cap);
/* the walk of the last car solve: from (start, start_heading) the allowed primitive
 * with the smallest cost + field[target], the first among equals; that minimum equals
 * field[current].  states_ijh_out: (i, j, h) triples, one per primitive boundary, start
 * first; moves_out: the count - 1 primitive ids between them; both NULL asks for the
 * count only; zero states when the solve found no path.  kc_planner_get_path then gives
 * every unit step of every primitive, first leg then second; kc_planner_shortcut answers
 * KC_ERR_STATE. */
int kc_planner_get_car_path(kc_planner *ctx, int32_t *states_ijh_out, int32_t *moves_out, size_t cap, size_t *count_out);
/* the mode as set (0, 0 while off) and what the last kc_planner_solve_car and its walk
 * took on the host clock (tools): maps and moves, field, walk, in ms; any may be NULL */
int kc_planner_car_info(kc_planner *ctx, int *turn_cells_out, uint32_t *reverse_weight_out, float phase_ms_out[3]);
/* Replan from the kept cost field (rules 19 and 20).  Arguments and
 * outputs as kc_planner_solve, and the same field, validity, status, cost and path bit
 * for bit; what differs is the work.  A context keeps the field of its last
 * kc_planner_solve / kc_planner_replan whose goal was a valid cell, and through
 * kc_planner_set_grid_host / _device of a grid of the same shape also the validity map
 * and penalty it was made for.  When goal_cell, r2, allow_unknown, the clearance table
 * and the shape are those of the kept field:
 *  - no grid was set since (a new start alone): the field stays, no pass runs;
 *  - else the new grid's maps are made and compared with the kept ones.  A cell is
 *    touched when its validity differs, or with the clearance cost on when it is valid
 *    in both and its penalty differs.  T = the minimum over touched cells of min(old
 *    value, old values of the 8 neighbours inside the grid + 10), 0xFFFFFFFF terms left
 *    out and 0xFFFFFFFF when there is none: every cell whose old value is below T keeps
 *    it.  T == 0xFFFFFFFF: the field stays, no pass runs.  Otherwise the cells that are
 *    valid now and were below T keep their value, the others start at 0xFFFFFFFF (the
 *    goal at 0), and the passes of kc_planner_solve run over the 64 x 64 tiles whose
 *    66 x 66 halo region holds a valid cell that was put back to 0xFFFFFFFF.
 * *passes_out: passes by kc_planner_solve's rule, 0 when none ran; never more than
 * kc_planner_solve needs on the same grid.  In every other case (no kept field, another
 * goal, r2, allow_unknown, table or shape) the call is kc_planner_solve, its refusals
 * included: KC_ERR_STATE with the oriented footprint on. */
int kc_planner_replan(kc_planner *ctx, const int start_cell[2], const int goal_cell[2], uint32_t r2,
                      int allow_unknown, int *status_out, uint32_t *cost_out, int *passes_out);
/* what the last kc_planner_replan did: *replanned_out 1 when it kept a field, 0 when
 * it was a full solve (or none was made); *threshold_out T, *touched_out the touched
 * cells, *active_tiles_out the tiles a pass ran over (0xFFFFFFFF, 0, 0 unless a grid
 * was compared).  Any pointer may be NULL. */
int kc_planner_replan_info(kc_planner *ctx, int *replanned_out, uint32_t *threshold_out, uint32_t *touched_out,
                           uint32_t *active_tiles_out);
/* Exploration (rules 21 to 26): the frontiers of the known map that the
 * robot can reach, nearest first, and the way to each.  A solve-type call like
 * kc_planner_solve: it replaces the last solve's outputs.
 *  - rule 21: a cell is explore-valid when no KC_OCCUPIED cell lies within r2 of it (the
 *    test of kc_planner_solve with allow_unknown = 1) and it is not KC_UNEXPLORED itself.
 *    No allow_unknown argument: unknown cells neither inflate nor can be crossed.
 *  - rule 22: field = kc_planner_solve's field over explore-valid cells with robot_cell
 *    as its root.  *status_out = KC_PLAN_START_OUTSIDE for a robot cell outside the grid,
 *    KC_PLAN_START_INVALID for one that is not explore-valid; both with zero frontiers.
 *  - rule 23: a frontier cell is explore-valid, has min_cost <= field < 0xFFFFFFFF and a
 *    KC_UNEXPLORED cell among its four orthogonal neighbours inside the grid.
 *  - rule 24: a frontier is an 8-connected component of frontier cells, its label the
 *    smallest flat index i + j * width among them; *components_out counts them; one is
 *    kept when it has at least min_size cells.
 *  - rule 25: *count_out kept frontiers, sorted by (cost, entry flat index); *status_out =
 *    KC_PLAN_FOUND with at least one, KC_PLAN_NO_FRONTIER with none.
 * *passes_out: the field's passes by kc_planner_solve's rule; *label_passes_out: the
 * labelling's by the same rule (0 when there is no frontier cell).  Any of the last four
 * pointers may be NULL.  Before any device use: KC_ERR_RANGE for r2 beyond
 * KC_PLANNER_MAX_RADIUS_CELLS cells and for min_size == 0; KC_ERR_STATE without a grid,
 * with a clearance cost set or with the oriented footprint on.  Afterwards
 * kc_planner_get_field gives the explore field and rule 21's map; kc_planner_get_path,
 * kc_planner_shortcut and kc_planner_path_clearance answer KC_ERR_STATE until the next
 * solve; kc_planner_solve gives what a fresh context gives and kc_planner_replan is a
 * full solve: neither rule 21's map nor the robot's field is kept for them. */
typedef struct kc_planner_frontier {
  uint64_t sum_i, sum_j;     /* exact sums of the cells' indices: the centroid is (sum_i, sum_j) / size */
  uint32_t size;             /* cells */
  uint32_t root;             /* the label */
  uint32_t cost;             /* field[entry cell] */
  int32_t entry_i, entry_j;  /* the cell with the smallest (field, flat index) */
  uint32_t reserved_;
} kc_planner_frontier;
int kc_planner_explore(kc_planner *ctx, const int robot_cell[2], uint32_t r2, uint32_t min_cost, uint32_t min_size,
                       int *status_out, uint32_t *components_out, size_t *count_out, int *passes_out,
                       int *label_passes_out);
/* rule 25: the kept frontiers of the last kc_planner_explore in their order; NULL asks
 * for the count only; KC_ERR_RANGE when they do not fit cap; KC_ERR_STATE unless the last
 * solve-type call was kc_planner_explore */
int kc_planner_get_frontiers(kc_planner *ctx, kc_planner_frontier *out, size_t cap, size_t *count_out);
/* rule 26: the path to kept frontier k: the walk from its entry cell down the field,
 * at each cell the allowed neighbour with the smallest field + step (10 / 14), the first
 * in kc_planner_get_path's order among equals (that minimum equals the cell's field:
 * the steps sum to the frontier's cost exactly), handed out reversed: (i, j) pairs, the
 * robot's cell first, the entry cell last.  NULL asks for the count only.  KC_ERR_RANGE for
 * k outside the kept list; KC_ERR_STATE unless the last solve-type call was
 * kc_planner_explore */
int kc_planner_get_frontier_path(kc_planner *ctx, size_t k, int32_t *cells_ij_out, size_t cap, size_t *count_out);
/* rule 24's labels of every frontier cell, kept or not, laid out as the grid, 0xFFFFFFFF
 * where the cell is no frontier cell (tests); KC_ERR_STATE as above */
int kc_planner_get_frontier_labels(kc_planner *ctx, uint32_t *labels_out, size_t cap);
/* what the last kc_planner_explore did (tools): the 64 x 64 tiles that hold a frontier
 * cell and so were labelled (rule 24 runs over those alone), all tiles, and the host's
 * clock in milliseconds around its three phases, each ended by a read-back: validity +
 * field, mark + label, sizes + records.  Any pointer may be NULL; KC_ERR_STATE as above */
int kc_planner_explore_info(kc_planner *ctx, uint32_t *listed_tiles_out, uint32_t *tiles_out, float phase_ms_out[3]);

/* ------------------------------------------------------------------------ */
/* World map: the mapper's egocentric grids fused on the device */
/* ------------------------------------------------------------------------ */
typedef struct kc_worldmap kc_worldmap;

/* Nothing in the reference to cite for the method: it leaves the world-frame map to
 * its ROS side.  This is the layer between kc_mapper (an egocentric grid that turns
 * with the robot) and kc_planner_replan (which wants a world-frame map that changes):
 * the map lives on the device, is updated from each local grid where that grid lies
 * and is read in place by kc_planner_set_grid_device(ctx, cls, 1, width, height).
 *
 * The map is width x height cells, cell (I, J) at I + J * width (the planner's
 * layout), (origin_x, origin_y) the world position of cell (0, 0)'s centre.  Two int8
 * planes: evidence (-128 never observed, else e_min .. e_max) and cls (KC_UNEXPLORED
 * while never observed, KC_OCCUPIED when evidence >= occ_thr, KC_EMPTY otherwise).
 * Integers only, and independent of thread order: DESIGN.md 4.11 has the rules, the
 * tests hold every plane to them bit for bit.  KC_ERR_RANGE above 32768 cells a side
 * or KC_PLANNER_MAX_CELLS cells. */
typedef struct kc_worldmap_pose { /* the local grid's frame in the map, 16 fraction bits */
  int32_t cq, sq;                 /* lrint(cos(yaw) * 65536), lrint(sin(yaw) * 65536) */
  int64_t tx, ty;                 /* llrint((p - origin) / resolution * 65536) per axis */
} kc_worldmap_pose;
typedef struct kc_worldmap_result { /* what an update did to the cls plane */
  uint32_t changed;                 /* cells whose cls byte changed */
  int32_t i_min, j_min, i_max, j_max; /* their bounding box in cells; all -1 when changed == 0 */
} kc_worldmap_result;

/* a map of never-observed cells with the default model (hit 3, miss 1, e_min -8, e_max
 * 14, occ_thr 1).  The shape is checked before the device is looked for. */
int kc_worldmap_create(int device, int width, int height, float resolution, double origin_x, double origin_y,
                       kc_worldmap **out);
void kc_worldmap_destroy(kc_worldmap *ctx);
/* the geometry given to kc_worldmap_create, the origin at the current offset (rule 46: the
 * one given while no shift has been made); any pointer may be NULL */
int kc_worldmap_info(kc_worldmap *ctx, int *width_out, int *height_out, float *resolution_out, double *origin_x_out,
                     double *origin_y_out);
/* The update model: an observation of KC_OCCUPIED adds hit (up to e_max), one of
 * KC_EMPTY takes miss away (down to e_min), a never-observed cell counts from 0.
 * hit, miss in 1 .. 127, e_min in -127 .. 0, e_max in 0 .. 127, e_min < occ_thr <=
 * e_max, KC_ERR_INVALID otherwise (kc_worldmap_check_model is that test alone: host
 * only).  hit = miss = 127, e_min = -127, e_max = 127: the latest observation wins.
 * Evidence counted by one model means nothing under another: set_model clears the map. */
int kc_worldmap_check_model(int hit, int miss, int e_min, int e_max, int occ_thr);
int kc_worldmap_set_model(kc_worldmap *ctx, int hit, int miss, int e_min, int e_max, int occ_thr);
/* The pose (px, py, yaw) of a local grid's frame in a map of this resolution and
 * origin, quantised as kc_worldmap_pose says; all of it in double, cos / sin from
 * libm, lrint / llrint to nearest even.  Host only: it takes the map's geometry
 * rather than a context, so that it works without a device.  KC_ERR_RANGE when the pose
 * lies more than 2^20 cells from the origin, KC_ERR_INVALID for anything non-finite. */
int kc_worldmap_quantise_pose(float resolution, double origin_x, double origin_y, double px, double py, double yaw,
                              kc_worldmap_pose *out);
/* what every update checks of its local grid before the device is used (host only):
 * positive sides, central cell within 2^30, and `resolution` the very float
 * `world_resolution` is (KC_ERR_INVALID: resampling is out of scope) */
int kc_worldmap_check_grid(float world_resolution, int grid_height, int grid_width, int central_i, int central_j,
                           float resolution);
/* One update from a local grid: int32, column-major [grid_height x grid_width] (the
 * LocalMapper layout, kc_mapper_grid_device), local cell (i, j) the point ((i -
 * central_i) res, (j - central_j) res) of the frame `pose` places in the map -- the
 * frame of kc_dwa_set_grid_device.  Every map cell looks up the one local cell it
 * falls into (a gather: no holes under rotation, no write conflicts); KC_OCCUPIED and
 * KC_EMPTY observations count, every other value and every cell outside the local
 * grid leaves the map cell as it is.  One kernel launch and the read-back of *out; the
 * call returns with the map finished, so a planner may read it at once.
 * _device: the grid where it lies on ctx's device, finished (KC_ERR_INVALID, before
 * any read, unless it is device memory of ctx's device inside one allocation);
 * _host: one copy up. */
int kc_worldmap_update_device(kc_worldmap *ctx, const int32_t *dev_grid, int grid_height, int grid_width, int central_i,
                              int central_j, float resolution, const kc_worldmap_pose *pose, kc_worldmap_result *out);
int kc_worldmap_update_host(kc_worldmap *ctx, const int32_t *grid, int grid_height, int grid_width, int central_i,
                            int central_j, float resolution, const kc_worldmap_pose *pose, kc_worldmap_result *out);
/* same, from a mapper context of this library: geometry and stream ordering (event
 * wait, no host synchronisation of the mapper) are taken from it, as
 * kc_dwa_set_grid_from_mapper does */
int kc_worldmap_update_from_mapper(kc_worldmap *ctx, struct kc_mapper *mapper, const kc_worldmap_pose *pose,
                                   kc_worldmap_result *out);
/* A prior replaces the whole state: a grid of the map's shape and layout, int8 or int32
 * (elem_bytes 1 or 4; kc_cloud_grid_device gives the former): KC_OCCUPIED -> e_max,
 * KC_EMPTY -> e_min, anything else never observed.  KC_ERR_INVALID for another shape.
 * _device reads a finished grid in place, checked as above; kc_worldmap_after_stream
 * orders that read (and kc_worldmap_update_device's) after the work queued so far on a
 * producer's stream, as kc_planner_after_stream does. */
int kc_worldmap_set_prior_host(kc_worldmap *ctx, const void *grid, int elem_bytes, int width, int height);
int kc_worldmap_set_prior_device(kc_worldmap *ctx, const void *dev_grid, int elem_bytes, int width, int height);
int kc_worldmap_after_stream(kc_worldmap *ctx, void *stream);
/* every cell never observed again */
int kc_worldmap_clear(kc_worldmap *ctx);
/* the cls plane on the device (int8, width x height): valid until destroy, finished
 * whenever no call on ctx is running */
int kc_worldmap_grid_device(kc_worldmap *ctx, void **dev_cls_int8);
/* copies of the planes, cap the cells either output holds; either pointer may be NULL */
int kc_worldmap_get(kc_worldmap *ctx, int8_t *cls_out, int8_t *evidence_out, size_t cap);

/* The map's obstacles near the robot as a world-frame point list (DESIGN.md 4.11 rules 16
 * to 19).  Nothing in the reference to cite, as above: it leaves the world map to its
 * ROS side.
 * Rule 16: the robot's position is quantised as kc_worldmap_quantise_pose does with yaw 0;
 * the centre cell is Ic = (tx + 2^15) >> 16, Jc = (ty + 2^15) >> 16 (arithmetic shifts),
 * the radius Rc = (int)ceil((double)max_sensor_range / (double)resolution).  Rule 17: cell
 * (I, J) counts iff it lies inside the map, its cls byte is KC_OCCUPIED and (I - Ic)^2 +
 * (J - Jc)^2 <= Rc^2 in int64.  Rule 18: its point is x = (float)(origin_x + (double)I *
 * (double)resolution), y alike with J and origin_y, z = 0: the cell's centre, product and
 * sum rounded once each in double.  Rule 19: the list is the set of those points in no
 * particular order, with its count and the index bounds of the counted cells.
 * kc_worldmap_window is rule 16 alone (host only, needs no device): KC_ERR_INVALID unless
 * max_sensor_range is a finite float > 0 and everything else finite, KC_ERR_RANGE for Rc >
 * 2048 (which bounds the scratch list) or a position more than 2^20 cells from the
 * origin. */
int kc_worldmap_window(float resolution, double origin_x, double origin_y, double x, double y, float max_sensor_range,
                       int32_t *ic_out, int32_t *jc_out, int32_t *rc_out);
/* The list into host memory: one launch over the window's box clipped to the map, and the
 * read-back; returns with the list final.  xyz_out: cap points of three floats, or NULL
 * for the count and the bounds only.  bounds_out: i_min, i_max, j_min, j_max of the
 * counted cells, every one -1 when *count_out is 0.  cap < count: KC_ERR_RANGE with
 * *count_out set and nothing written to xyz_out.  A robot outside the map is no error:
 * the window is clipped, perhaps to nothing.  Every argument is checked before the
 * device is used. */
int kc_worldmap_points(kc_worldmap *ctx, double x, double y, float max_sensor_range, float *xyz_out, size_t cap,
                       size_t *count_out, int32_t bounds_out[4]);

/* A virtual laser scan ray-cast from the map (DESIGN.md 4.11 rules 20 to 27): what a lidar
 * at a pose would range, by the map's memory.  Nothing in the reference to cite, as above.
 * Integers throughout (int64, arithmetic shifts) except where a range becomes a double, so
 * every range is independent of thread order; the map is not modified.
 * Rule 20: the scan frame's pose (Cq, Sq, TX, TY) as kc_worldmap_quantise_pose gives it;
 * X0 = TX + 2^15, Y0 = TY + 2^15, start cell I0 = X0 >> 16, J0 = Y0 >> 16, fractions fx =
 * X0 & 0xFFFF, fy = Y0 & 0xFFFF; Rc = (int)ceil((double)range_max / (double)resolution).
 * Rule 21: beam k of angle a_k (scan frame) has ac_k = lrint(cos(a_k) * 2^30), as_k =
 * lrint(sin(a_k) * 2^30), int32, cos / sin the host libm's in double.  Rule 22: dx = (Cq
 * ac_k - Sq as_k + 2^15) >> 16, dy = (Sq ac_k + Cq as_k + 2^15) >> 16.  Rule 23, the walk:
 * sx = dx > 0 ? 1 : -1, ex = dx > 0 ? 65536 - fx : fx, y alike; a start cell that blocks
 * ends the beam with e = 0; otherwise step along x if dy == 0, along y if dx == 0, else
 * along x iff ex |dy| <= ey |dx| (a tie: x first, the y step follows at the same distance,
 * so a ray through a corner visits the cell beside it); a step along x sets e = ex, a =
 * |dx|, I += sx, ex += 65536, one along y alike; after it the beam ends without a hit if
 * |I - I0| > Rc + 1 or |J - J0| > Rc + 1, and with the candidate (I, J, e, a) if the cell
 * blocks.  Cells outside the map never block; a scan may start outside and look in.  Rule
 * 24: r = ((double)e * 16384.0 / (double)a) * (double)resolution, one division and one
 * product, each rounded once; the first blocking cell decides, and counts iff r <=
 * (double)range_max.  Rule 25: a cell blocks if its cls byte is KC_OCCUPIED, with
 * KC_SCAN_UNKNOWN_BLOCKS also if it is KC_UNEXPLORED.  Rule 26: ranges[p * B + k] is r on a
 * hit and (double)range_max otherwise, cells[p * B + k] is I + J * width on a hit and -1
 * otherwise.  Rule 27: with a present scan real[k] the stored range is real[k] < v ? real[k]
 * : v, a NaN or an infinite real[k] leaves v. */
#define KC_SCAN_UNKNOWN_BLOCKS 1u
/* rule 21's table (host only, needs no device): ac_as_out[2 k], ac_as_out[2 k + 1] = ac_k,
 * as_k.  KC_ERR_INVALID for a non-finite angle, and then nothing is written. */
int kc_worldmap_scan_table(const double *angles, size_t n, int32_t *ac_as_out);
/* the refusals of rules 20, 21 and 25 (host only), in this order: KC_ERR_INVALID for no
 * pose or no beam, KC_ERR_RANGE above 65536 beams or n_poses * n_beams > 2^22,
 * KC_ERR_INVALID unless range_max is a finite float > 0, KC_ERR_RANGE for Rc > 2048,
 * KC_ERR_INVALID for unknown flag bits.  rc_out (may be NULL): Rc, 0 on a refusal. */
int kc_worldmap_scan_check(float resolution, size_t n_poses, size_t n_beams, float range_max, unsigned int flags,
                           int32_t *rc_out);
/* The scan of n_poses poses x n_beams angles into host memory: one launch (a lane a beam,
 * a single pose in the kernel arguments, a batch from a device buffer) and one read-back;
 * returns with the outputs final.  ranges_out and cells_or_null hold n_poses * n_beams
 * values.  The context keeps the table of the last angle array and forms it again only
 * when the bytes differ.  Checks: null arguments, then kc_worldmap_scan_check, the angles
 * (finite) and the poses (as an update's), then the device; a refused call queues nothing. */
int kc_worldmap_scan(kc_worldmap *ctx, const kc_worldmap_pose *poses, size_t n_poses, const double *angles,
                     size_t n_beams, float range_max, unsigned int flags, double *ranges_out, int32_t *cells_or_null);
/* kc_dvz_deform on the map's scan at `pose` (rules 26 and 27), without the ranges leaving
 * the device: the scan is queued on the DVZ context's stream, behind an event on the
 * map's stream (no host wait on the map), straight into the buffer the deformation kernel
 * reads; that kernel follows unchanged, so out[3] and radii_or_null are kc_dvz_deform's on
 * those ranges, bit for bit.  real_or_null: n present ranges to merge by rule 27.
 * ranges_or_null: the n ranges the zone was deformed by.  Checks: null arguments; n (1 ..
 * the context's max_beams), the zone, the angles, range_max and flags, the pose; the
 * map's device against the context's (KC_ERR_INVALID); then the device. */
int kc_dvz_deform_worldmap(kc_dvz *ctx, const kc_dvz_zone *zone, kc_worldmap *map, const kc_worldmap_pose *pose,
                           const double *angles, size_t n, float range_max, unsigned int flags,
                           const double *real_or_null, double out[3], double *radii_or_null, double *ranges_or_null);
/* kc_zone_check on the map's scan at `pose`, the scan frame (the sensor's pose in the
 * world): the checker's own preset angles, whose table kc_zone_create formed, and its
 * range_max; the scan is queued on the checker's stream into the buffer zone_check_kernel
 * reads, ordered as above.  real_or_null: the preset's count of present ranges (rule 27).
 * A checker without angles gives 1.  Checks as above. */
int kc_zone_check_worldmap(kc_zone *ctx, kc_worldmap *map, const kc_worldmap_pose *pose, unsigned int flags,
                           const double *real_or_null, int forward, float *factor_out);

/* Correlative match of a local grid against the map (DESIGN.md 4.11 rules 9 to 15): which
 * pose near a guess puts the grid's occupied cells onto the map's?  Integers only, sums
 * of integers, so no result depends on thread order; the map is not modified.
 * Rule 9: every local cell (i, j) that holds KC_OCCUPIED is a point (a, b) = (i -
 * central_i, j - central_j); no other value counts.  Rule 10: the window is n_yaw = K
 * rotations each side of the guess's yaw, yaw_step apart, and reach = S whole cells each
 * side along both axes.  Rule 11: under rotation k a point lands at I0 = (TX + Cq_k a -
 * Sq_k b + 2^15) >> 16, J0 = (TY + Sq_k a + Cq_k b + 2^15) >> 16 (int64, arithmetic
 * shifts; the guess's fraction is kept), under translation (u, v) in world cell (I0 + u,
 * J0 + v).  Rule 12: a world cell weighs 3 if its cls byte is KC_OCCUPIED, else 2 if one
 * of its four orthogonal neighbours inside the map is, else 1 if a diagonal one is, else
 * 0; a cell outside the map weighs 0 and is nobody's neighbour.  Rule 13: score(k, u,
 * v) is the sum of the landing cells' weights over all points, uint32, stored at (k + K)
 * (2S+1)^2 + (v + S) (2S+1) + (u + S).  Rule 14: the largest score wins, among equals
 * the smallest (u u + v v, |k|, k, v, u): a flat score returns the guess. */
#define KC_WORLDMAP_MATCH_MAX_YAW 31    /* K */
#define KC_WORLDMAP_MATCH_MAX_REACH 31  /* S */
#define KC_WORLDMAP_MATCH_MAX_SIDE 8192 /* cells a side of the local grid */
typedef struct kc_worldmap_rotation { /* rule 10: rotation k of the window */
  int32_t cq, sq;                     /* lrint(cos(yaw_k) * 65536), lrint(sin(yaw_k) * 65536) */
} kc_worldmap_rotation;
typedef struct kc_worldmap_match_result { /* rule 15 */
  int32_t k, u, v;                        /* the winner: rotation step, translation in cells */
  uint32_t score, score_guess;            /* the winner's, and score(0, 0, 0) */
  uint32_t n_points;                      /* rule 9's count; 0: every score is 0, the guess wins */
  kc_worldmap_pose pose;                  /* (Cq_k, Sq_k, TX + (u << 16), TY + (v << 16)): ready for an update */
} kc_worldmap_match_result;
/* rule 10's ranges (host only): n_yaw and reach in 0 .. 31, yaw_step a finite double >=
 * 0, KC_ERR_INVALID otherwise */
int kc_worldmap_match_check_window(int n_yaw, double yaw_step, int reach);
/* rule 9's test of the local grid (host only): kc_worldmap_check_grid, then KC_ERR_RANGE
 * for a side above 8192 or a cell more than 8192 cells from the central cell along an
 * axis (which bounds the scratch plane) */
int kc_worldmap_match_check_grid(float world_resolution, int grid_height, int grid_width, int central_i, int central_j,
                                 float resolution);
/* rule 10's table (host only, compare kc_worldmap_quantise_pose): out[k + n_yaw] for k =
 * -n_yaw .. n_yaw from yaw_k = yaw + (double)k * yaw_step, in double with libm's cos /
 * sin and lrint.  KC_ERR_RANGE when cap < 2 n_yaw + 1. */
int kc_worldmap_match_rotations(double yaw, int n_yaw, double yaw_step, kc_worldmap_rotation *out, size_t cap);
/* One match.  The grid arguments, pointer checks and stream ordering are those of the
 * three kc_worldmap_update_* entries; guess: the quantised pose guess (its tx, ty are
 * rule 11's TX, TY), rotations: 2 n_yaw + 1 pairs as kc_worldmap_match_rotations gives
 * them (KC_ERR_INVALID for a pair that is no unit vector in 16 fraction bits).  Every
 * argument is checked before the device is used.  Four launches (weights over a scratch
 * plane, points, scores, pick) and the read-back of the record; returns with it final. */
int kc_worldmap_match_device(kc_worldmap *ctx, const int32_t *dev_grid, int grid_height, int grid_width, int central_i,
                             int central_j, float resolution, const kc_worldmap_pose *guess,
                             const kc_worldmap_rotation *rotations, int n_yaw, int reach, kc_worldmap_match_result *out);
int kc_worldmap_match_host(kc_worldmap *ctx, const int32_t *grid, int grid_height, int grid_width, int central_i,
                           int central_j, float resolution, const kc_worldmap_pose *guess,
                           const kc_worldmap_rotation *rotations, int n_yaw, int reach, kc_worldmap_match_result *out);
int kc_worldmap_match_from_mapper(kc_worldmap *ctx, struct kc_mapper *mapper, const kc_worldmap_pose *guess,
                                  const kc_worldmap_rotation *rotations, int n_yaw, int reach,
                                  kc_worldmap_match_result *out);
/* rule 13's table of the last match, (2K+1) (2S+1)^2 words; KC_ERR_RANGE when they do not
 * fit cap, KC_ERR_STATE before the first match */
int kc_worldmap_match_scores(kc_worldmap *ctx, uint32_t *out, size_t cap);
/* HIP-event times of the last match's four launches in milliseconds (weight, points,
 * score, pick), for tools; recorded only while enabled.  KC_ERR_STATE when the last
 * match was not timed. */
int kc_worldmap_match_set_timing(kc_worldmap *ctx, int enable);
int kc_worldmap_match_times(kc_worldmap *ctx, float ms_out[4]);

/* ------------------------------------------------------------------------ */
/* Monte-Carlo localisation over the world map (DESIGN.md 4.11 rules 28 to 41) */
/* ------------------------------------------------------------------------ */
/* Nothing in the reference to cite: it leaves localisation, like the world map, to its ROS
 * side.  N particles on the device, advanced by odometry with seeded integer noise, scored
 * against a laser scan by ray-casting the map in place with the scan's own walk, reduced to
 * one record the host turns into an estimate.  Integers throughout (int64, arithmetic
 * shifts, exact sums): no result depends on thread order, tests/worldmap_mcl_ref.py states
 * every rule in Python ints and the device equals it bit for bit.  No kernel modifies the map.
 * Rule 28, particle: (TX, TY, h, acc).  TX, TY: int64 with 16 fraction bits of a cell, as
 * kc_worldmap_pose's, clamped to +-2^36; h: heading in 2^-16 turn, 0 .. 65535, it wraps;
 * acc: uint32 accumulated penalty.  The particle is the scan frame's pose: a sensor's yaw
 * offset is folded into the beam angles by the caller, a translated mount is out of scope.
 * Rule 29, heading table: Cq(h) = lrint(cos(2 pi h / 65536) * 65536), Sq(h) alike, the
 * host libm's in double; 65536 pairs built once on the host, kept on the device.
 * Rule 30, random numbers, counter-based, all mod 2^64: mix64(x): z = x +
 * 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) *
 * 0x94D049BB133111EB; z ^ (z >> 31) (mix64(0) = 0xE220A8397B1DCDAF).  draw(seed, step, p, c)
 * = mix64(mix64(seed ^ (step << 32)) ^ ((p << 8) | c)), c < 256.  noise(v, s): with the four
 * 16-bit fields a0 .. a3 of v, g = a0 + a1 + a2 + a3 - 131070, noise = (g s + 2^15) >> 16,
 * s >= 0 an int32.  g's standard deviation is sqrt((65536^2 - 1) / 3); a front end forms s =
 * lrint(sigma * 65536 / that) for a sigma in the quantity's units; this ABI takes s as given.
 * Rule 31, predict: increments d_f, d_l (forward, lateral; 2^-16 cells, |d| <= 2^36) and d_h
 * (heading units), scales s_f, s_l, s_h.  With (C, S) = (Cq(h), Sq(h)) of the heading BEFORE
 * the step: F = d_f + noise(draw(.., p, 0), s_f), L = d_l + noise(draw(.., p, 1), s_l), TX +=
 * (C F - S L + 2^15) >> 16, TY += (S F + C L + 2^15) >> 16, both clamped, h = (h + d_h +
 * noise(draw(.., p, 2), s_h)) & 0xFFFF.
 * Rule 32, expected range: beam k of the new particle walks as rules 21 to 23 and 25 say from
 * the pose (Cq(h), Sq(h), TX, TY), box Rc + 1, KC_SCAN_UNKNOWN_BLOCKS honoured.  ZMAX =
 * llrint((double)range_max / (double)resolution * 65536).  The first blocking cell gives q =
 * floor(e 2^30 / a) (e < 2^28); a start cell that blocks q = 0; no hit or q > ZMAX: q = ZMAX.
 * Rule 33, measured range, quantised by the caller: zq_k = llrint(z_k / resolution * 65536)
 * for a finite 0 <= z_k < range_max, else ZMAX (a beam without a return), or -1 with
 * KC_MCL_SKIP_NO_RETURN: such a beam contributes nothing.  A step refuses a zq outside 0 ..
 * ZMAX, and a -1 without the flag.
 * Rule 34, penalty: bin = min(|q - zq_k| >> err_shift, E - 1), cost_p = sum_k pen[bin],
 * uint32; pen: E <= 4096 uint16 entries, err_shift in 0 .. 30.
 * Rule 35, accumulate: acc_p = min(acc_p - min_prev + cost_p, 2^30), min_prev the smallest
 * acc after the previous step, 0 after an init or a resample; amin = min_p acc_p, best the
 * lowest index with acc_p == amin.
 * Rule 36, weight: w_p = wtab[min((acc_p - amin) >> w_shift, EW - 1)]; wtab: EW <= 4096
 * uint32 entries that do not increase, 1 <= wtab[0] <= 2^20, w_shift in 0 .. 30.
 * Rule 37, record: exact sums over all particles, kc_mcl_record.
 * Rule 38, limits: 1 <= N <= 65536, 1 <= B <= 1024, N B <= 2^22; kc_mcl_check's order.
 * Rule 39, estimate (the host's, from the record): TXe = TX_best + floor(SX / W1), TYe alike;
 * yaw = atan2((double)SS, (double)SC); x = origin_x + (double)TXe / 65536 * resolution;
 * n_eff = (double)W1 * (double)W1 / (double)W2.
 * Rule 40, resample: the host decides (W1 W1 r_den < r_num N W2 in exact integers, 1 / 2 by
 * default); systematic: cum_i the inclusive prefix sum of w in index order, u0 = draw(seed,
 * step, N, 15) mod W1, slot j takes the state of the smallest i with N cum_i > u0 + j W1 and
 * acc 0; double-buffered, no slot reads what another writes.
 * Rule 41, init; either sets the step counter to 0, a step increments it before it draws.
 * Gaussian: TX = TX0 + noise(draw(seed, 0, p, 0), s_xy), TY with channel 1, h = (h0 +
 * noise(draw(seed, 0, p, 2), s_h)) & 0xFFFF, TX and TY clamped, acc 0.  Global: the free
 * cells are those whose cls byte is KC_EMPTY, in the order of I + J * width, n_free of them;
 * particle p takes number draw(seed, 0, p, 0) mod n_free; with v = draw(seed, 0, p, 1): TX = (I
 * << 16) + (v & 0xFFFF) - 2^15, TY = (J << 16) + ((v >> 16) & 0xFFFF) - 2^15, h = (v >> 32) &
 * 0xFFFF. */
typedef struct kc_mcl kc_mcl;
#define KC_MCL_SKIP_NO_RETURN 2u /* beside KC_SCAN_UNKNOWN_BLOCKS in a step's flags */
#define KC_MCL_MAX_PARTICLES 65536
#define KC_MCL_MAX_BEAMS 1024
#define KC_MCL_MAX_TABLE 4096
typedef struct kc_mcl_record { /* rule 37 */
  uint64_t w1, w2;             /* sum w, sum w^2 */
  uint64_t sx_lo;              /* SX = sum w (TX_p - TX_best) as a 128-bit two's complement (lo, hi) */
  int64_t sx_hi;
  uint64_t sy_lo;              /* SY alike */
  int64_t sy_hi;
  int64_t sc, ss;              /* sum w Cq(h_p), sum w Sq(h_p) */
  int64_t best_tx, best_ty;    /* the best particle's state */
  uint32_t best_h;
  uint32_t amin, best;         /* rule 35 */
  uint32_t step;               /* the step counter of the step that formed the record */
} kc_mcl_record;
/* Rule 38's refusals (host only), in this order: KC_ERR_INVALID unless the resolution is a
 * finite float > 0; KC_ERR_INVALID for no particle or no beam; KC_ERR_RANGE above 65536
 * particles, then above 1024 beams, then above 2^22 rays; KC_ERR_INVALID unless range_max is a
 * finite float > 0; KC_ERR_RANGE for Rc > 2048; pen (skipped when NULL): KC_ERR_INVALID for no
 * entry, KC_ERR_RANGE above 4096, KC_ERR_INVALID for err_shift outside 0 .. 30; wtab (skipped
 * when NULL): the same three, then KC_ERR_INVALID for wtab[0] outside 1 .. 2^20 and for an
 * entry above the one before it; KC_ERR_INVALID for unknown flag bits.  rc_out, zmax_out (may
 * be NULL): Rc and ZMAX, 0 on a refusal. */
int kc_mcl_check(float resolution, size_t n_particles, size_t n_beams, float range_max, const uint16_t *pen_or_null, size_t n_pen,
                 int err_shift, const uint32_t *wtab_or_null, size_t n_wtab, int w_shift, unsigned int flags, int32_t *rc_out,
                 int64_t *zmax_out);
/* rule 29 for one heading (host only); KC_ERR_RANGE above 65535 */
int kc_mcl_heading(uint32_t h, int32_t *cq_out, int32_t *sq_out);
/* A localiser of n_particles over `map`, on its device, with its own stream; the map must
 * outlive it.  angles: the n_beams beam angles in the scan frame (rule 21's table is formed
 * here).  Checks: null arguments, kc_mcl_check without tables, the angles (finite), then the
 * device. */
int kc_mcl_create(kc_worldmap *map, size_t n_particles, const double *angles, size_t n_beams, float range_max, uint64_t seed,
                  kc_mcl **out);
void kc_mcl_destroy(kc_mcl *ctx);
/* what the context was made with, Rc, ZMAX and the step counter; any pointer may be NULL */
int kc_mcl_info(kc_mcl *ctx, size_t *n_particles_out, size_t *n_beams_out, int32_t *rc_out, int64_t *zmax_out, uint32_t *step_out);
/* rules 34 and 36's tables and shifts, checked as kc_mcl_check does; the particles stay, the
 * weights of the last step do not (a resample needs a new step) */
int kc_mcl_set_model(kc_mcl *ctx, const uint16_t *pen, size_t n_pen, int err_shift, const uint32_t *wtab, size_t n_wtab, int w_shift);
/* rule 41.  init_pose: KC_ERR_RANGE for |TX0|, |TY0| > 2^36 or h0 > 65535, KC_ERR_INVALID for
 * a negative scale.  init_global: two launches around a read-back of the row counts, ordered
 * behind the map's stream; *n_free_out (may be NULL) the free cells; KC_ERR_STATE with none.
 * A refused init of either kind leaves the particles, weights and fit of an earlier one. */
int kc_mcl_init_pose(kc_mcl *ctx, int64_t tx0, int64_t ty0, uint32_t h0, int32_t s_xy, int32_t s_h);
int kc_mcl_init_global(kc_mcl *ctx, size_t *n_free_out);
/* One step (rules 31 to 37): two launches (predict + walk + penalty; weight + record) behind
 * an event on the map's stream, and the read-back of *out; returns with it final.  zq: n_beams
 * quantised ranges (rule 33).  Checks, in this order: null arguments; KC_ERR_STATE without a
 * model, then without an init; KC_ERR_RANGE for |d_f|, |d_l| > 2^36; KC_ERR_INVALID for a
 * negative scale, unknown flag bits, a zq outside rule 33; then the device.  A refused call
 * queues nothing. */
int kc_mcl_step(kc_mcl *ctx, int64_t d_f, int64_t d_l, int32_t d_h, int32_t s_f, int32_t s_l, int32_t s_h, const int32_t *zq,
                unsigned int flags, kc_mcl_record *out);
/* rule 40's copy by the last step's weights: two launches (prefix sum, select), no read-back.
 * KC_ERR_STATE unless a step has run since the last init, resample or set_model. */
int kc_mcl_resample(kc_mcl *ctx);
/* the states and acc into host memory, for tests and tools; any output may be NULL; cap: the
 * particles each holds (KC_ERR_RANGE below N); KC_ERR_STATE before an init */
int kc_mcl_particles(kc_mcl *ctx, int64_t *tx_out, int64_t *ty_out, uint32_t *h_out, uint32_t *acc_out, size_t cap);
/* where they lie on the device (int64, int64, uint32, uint32; N each): valid until the next
 * step, resample or init, which change buffers */
int kc_mcl_particles_device(kc_mcl *ctx, void **tx_out, void **ty_out, void **h_out, void **acc_out);
/* HIP-event times in milliseconds of the last step's two launches (walk, weigh) and the last
 * resample's (prefix, select; 0 when none ran), for tools; recorded only while enabled.
 * KC_ERR_STATE when no step was timed. */
int kc_mcl_set_timing(kc_mcl *ctx, int enable);
int kc_mcl_times(kc_mcl *ctx, float ms_out[4]);

/* ------------------------------------------------------------------------ */
/* The map's distance plane and the likelihood-field model (DESIGN.md 4.11 rules 42 to 45) */
/* ------------------------------------------------------------------------ */
/* Off by default: with the plane off every entry above does what it did without it.
 * Rule 42, plane: dist2[I + J W], uint16: the smallest (bI - I)^2 + (bJ - J)^2 over the blocking
 * cells when that is <= reach^2, KC_WORLDMAP_DIST_FAR otherwise.  A cell blocks when its cls
 * byte is KC_OCCUPIED, with KC_WORLDMAP_DIST_UNKNOWN_BLOCKS also when it is KC_UNEXPLORED;
 * cells outside the map never block.  1 <= reach <= 254 (kc_planner_set_clearance_cost's
 * clear2, on purpose).
 * Rule 43, refresh: the plane is kept lazily behind a dirty box of cells whose class may have
 * changed.  kc_worldmap_set_distance (reach > 0), kc_worldmap_set_prior_*, kc_worldmap_clear
 * and kc_worldmap_set_model make it the whole map; an update merges the box of its result
 * (changed != 0) into it on the host: no extra launch, no extra read-back.  A refresh
 * recomputes dist2 over the dirty box grown by reach on every side and clipped to the map (one
 * launch up to reach 63, two above), then empties the box; with an empty box it launches
 * nothing.  Every entry that reads the plane refreshes first.  dist2 of a cell depends only on
 * the cls bytes of the (2 reach + 1)^2 square around it, so the plane equals a full recompute
 * after any sequence of updates and refreshes. */
#define KC_WORLDMAP_DIST_FAR 0xFFFFu
#define KC_WORLDMAP_DIST_UNKNOWN_BLOCKS 1u
#define KC_WORLDMAP_DIST_MAX_REACH 254
/* reach 0 switches the plane off and frees it (flags must then be 0 too).  KC_ERR_RANGE for a
 * reach outside 0 .. 254, KC_ERR_INVALID for unknown flag bits; both before the device. */
int kc_worldmap_set_distance(kc_worldmap *ctx, int reach, unsigned int flags);
/* any pointer may be NULL.  reach 0: off (and KC_OK).  last_box: (i_min, j_min, i_max, j_max)
 * the last refresh recomputed, all -1 when it found the dirty box empty or none has run since
 * kc_worldmap_set_distance; *last_full: whether that box was the whole map. */
int kc_worldmap_distance_info(kc_worldmap *ctx, int *reach_out, unsigned int *flags_out, int last_box[4], int *last_full_out);
/* queues the refresh on the map's stream; the host does not wait.  KC_ERR_STATE while off,
 * as for the two below. */
int kc_worldmap_distance_refresh(kc_worldmap *ctx);
/* refreshes, then copies the plane; cap: the cells out holds (KC_ERR_RANGE below W H) */
int kc_worldmap_get_distance(kc_worldmap *ctx, uint16_t *out, size_t cap);
/* refreshes and returns with the plane complete; *ptr: uint16 [W x H] on the device, valid
 * until the next kc_worldmap_set_distance or the context's destruction */
int kc_worldmap_distance_device(kc_worldmap *ctx, void **ptr);

/* Rule 44, endpoint: for the particle after rule 31's step and rule 22's (dx, dy) of its heading
 * and beam k: X0 = TX + 2^15, EX = X0 + ((zq_k dx + 2^29) >> 30), EY alike, I = EX >> 16, J = EY
 * >> 16 (arithmetic shifts; |zq_k dx| < 2^58).
 * Rule 45, penalty: d2 = dist2[I + J W] inside the map, FAR outside; cost_p = sum over the
 * beams with 0 <= zq_k < ZMAX of (d2 <= c2 ? pen_d2[d2] : pen_far).  A beam with zq_k == ZMAX
 * (no return) or -1 contributes nothing.  pen_d2: c2 + 1 uint16 entries, 1 <= c2 <= min(reach^2,
 * 4095).  Rules 35 to 41 apply unchanged.
 * kc_mcl_field_check (host only), in this order: kc_mcl_check's refusals up to Rc; pen_d2
 * (skipped when NULL): KC_ERR_INVALID below 2 entries, KC_ERR_RANGE above 4096; reach (skipped
 * when 0): KC_ERR_RANGE outside 1 .. 254, KC_ERR_INVALID for n_pen - 1 > reach^2; wtab as
 * kc_mcl_check; KC_ERR_INVALID for flag bits other than KC_MCL_SKIP_NO_RETURN (the plane's own
 * flag decides what blocks: KC_SCAN_UNKNOWN_BLOCKS is refused). */
#define KC_MCL_MODEL_NONE 0
#define KC_MCL_MODEL_BEAM 1
#define KC_MCL_MODEL_FIELD 2
int kc_mcl_field_check(float resolution, size_t n_particles, size_t n_beams, float range_max, const uint16_t *pen_d2_or_null,
                       size_t n_pen, int reach, const uint32_t *wtab_or_null, size_t n_wtab, int w_shift, unsigned int flags,
                       int32_t *rc_out, int64_t *zmax_out);
/* The field model: pen_d2 (n = c2 + 1 entries), pen_far and rule 36's table, checked as
 * kc_mcl_field_check does with reach 0.  kc_mcl_step then runs rules 44 and 45 in place of 32
 * to 34, until kc_mcl_set_model switches back; the particles survive either switch, the last
 * step's weights do not.  A field step is two launches and the read-back, plus the plane's
 * refresh when its dirty box is not empty.  It answers KC_ERR_INVALID for
 * KC_SCAN_UNKNOWN_BLOCKS in its flags, and KC_ERR_STATE (after a step's other checks, before
 * anything is queued) while the map's plane is off or c2 > reach^2. */
int kc_mcl_set_field_model(kc_mcl *ctx, const uint16_t *pen_d2, size_t n, uint16_t pen_far, const uint32_t *wtab, size_t n_wtab,
                           int w_shift);
/* KC_MCL_MODEL_*: what kc_mcl_step runs */
int kc_mcl_model_kind(kc_mcl *ctx, int *kind_out);

/* ------------------------------------------------------------------------ */
/* The rolling window: whole-cell shifts on the device (DESIGN.md 4.11 rules 46 to 51) */
/* ------------------------------------------------------------------------ */
/* With no shift made, every entry above gives bit for bit what it gave without these.
 * Rule 46, offset and origin: the context keeps the origin given at creation (ox0, oy0) and an
 * integer cell offset (OI, OJ), initially 0.  The map's origin is ox0 + (double)OI * (double)
 * resolution per axis -- one product and one sum in double, never accumulated from shift to
 * shift -- and everything that reads the origin uses that value: kc_worldmap_info,
 * kc_worldmap_points, kc_worldmap_recentre, kc_dwa_set_worldmap, and whoever quantises a pose
 * for the scan, update and match entries (from kc_worldmap_info's origin).  A shift that
 * would take |OI| or |OJ| above 2^30 answers KC_ERR_RANGE and leaves the state untouched.
 * Rule 47, shift by (di, dj) cells: for both planes P'[I, J] = P[I + di, J + dj] where that
 * source cell lies inside the map; elsewhere the cell is never observed (evidence -128, cls
 * KC_UNEXPLORED).  Then OI += di, OJ += dj: a positive di moves the window towards +x.
 * di = dj = 0 launches nothing; |di| >= width or |dj| >= height is a clear at the new offset.
 * Integers only.  One launch (worldmap_shift_kernel) into scratch planes the context keeps
 * from its first shift on, and two device-to-device copies back; the call returns with the map
 * finished, as an update does.
 * Rule 48, what a shift leaves behind: the distance plane, when on, is wholly dirty (the next
 * reader's refresh is a full recompute of the shifted map); the kept match table and point
 * list are unaffected; every device pointer handed out (kc_worldmap_grid_device,
 * kc_worldmap_distance_device) stays valid and points at the shifted content.
 * Check order of kc_worldmap_shift: the context, the offset cap, then the device. */
int kc_worldmap_shift(kc_worldmap *ctx, int di, int dj);
/* rule 46's cap alone (host only, needs no device): KC_ERR_RANGE when a shift by (di, dj) from
 * the offset (oi, oj) would leave |OI| or |OJ| above 2^30 */
int kc_worldmap_check_shift(int32_t oi, int32_t oj, int di, int dj);
/* rule 46's (OI, OJ); either pointer may be NULL */
int kc_worldmap_offset(kc_worldmap *ctx, int32_t *oi_out, int32_t *oj_out);
/* Rule 49, the recentring policy (host only, integers, needs no device): (ic, jc) the robot's
 * cell by rule 16's quantisation.  Per axis, with size S and cell c: the shift is 0 while margin
 * <= c <= S - 1 - margin, otherwise ((c - S / 2) / stride) * stride with C's truncating
 * division.  KC_ERR_INVALID unless margin >= 0, stride >= 1 and 2 * margin < min(width,
 * height) (and for a non-positive side). */
int kc_worldmap_recentre_plan(int width, int height, int ic, int jc, int margin, int stride, int32_t *di_out,
                              int32_t *dj_out);
/* plan plus shift: (x, y) quantised by rule 16 at the current origin, rule 49, then rule 47;
 * *di_out, *dj_out: the shift made (0, 0 on any refusal).  Check order: null arguments, the
 * policy's, the position's (kc_worldmap_quantise_pose), the offset cap, then the device. */
int kc_worldmap_recentre(kc_worldmap *ctx, double x, double y, int margin, int stride, int32_t *di_out, int32_t *dj_out);
/* Rule 50, the localiser follows: a kc_mcl records the (OI, OJ) its particles are expressed in
 * (kc_mcl_init_* set it to the map's).  kc_mcl_step, kc_mcl_resample, kc_mcl_particles and
 * kc_mcl_particles_device first apply a difference (di, dj) as TX' = clamp(TX - (di << 16),
 * +-2^36), TY alike, in one launch (mcl_shift_kernel); h, acc and the kept weights are
 * untouched.
 * Rule 51 (the planner does not carry its field across a shift) is the host classes'. */

/* Integrating a measured laser scan by an inverse ray cast (DESIGN.md 4.11 rules 52 to 58): the
 * one way into the map that needs no local grid.  Nothing in the reference to cite, as above;
 * integers throughout, bit-equal to tests/worldmap_integrate_ref.py.
 * Rule 52, input: the scan frame's pose (rule 20), the beam angles through rule 21's table (1 to
 * 65536 beams, Rc <= 2048), and one int32 zq_k a beam: -1 (the beam says nothing), ZMAX =
 * llrint((double)range_max / (double)resolution * 65536) (no return), or a range in 2^-16 cells,
 * 0 <= zq_k < ZMAX.  Rule 53, crossed cells: rule 23's walk from the start cell, the map's
 * content taking no part; step s enters its cell at q_s = floor(e_s 2^30 / a_s); a beam with
 * limit z crosses the start cell and every step cell with q_s <= z, tested as e_s 2^30 < (z + 1)
 * a_s; q_s never decreases, so the crossed cells are a prefix of the walk, and the step that
 * leaves rule 23's box has q > ZMAX.  Rule 54, marks: a return beam (0 <= zq_k < ZMAX) marks its
 * last crossed cell HIT and every one before it MISS; a no-return beam (zq_k == ZMAX) marks every
 * crossed cell MISS with KC_INTEGRATE_CLEAR_NO_RETURN and nothing without; -1 marks nothing;
 * cells outside the map are walked and never marked; a cell's marks are the OR over all beams.
 * Rule 55, observation: HIT set -> 100, only MISS set -> 0 (a hit beats a miss); rule 5 is
 * applied once a marked cell a scan, rule 6's record formed over the cells whose class changed.
 * Rule 56: no thread order takes part.  Rule 57: the changed box merges into the distance
 * plane's dirty box as an update's does; between calls the mark plane is all zero. */
#define KC_INTEGRATE_CLEAR_NO_RETURN 1u
/* rule 52's refusals (host only, needs no device), in this order: the resolution and the counts
 * (KC_ERR_INVALID for no beam, KC_ERR_RANGE above 65536), range_max (KC_ERR_INVALID unless a
 * finite float > 0, KC_ERR_RANGE for Rc > 2048), flags (KC_ERR_INVALID for any bit but
 * KC_INTEGRATE_CLEAR_NO_RETURN), then zq_or_null when given (KC_ERR_INVALID for a value outside
 * -1 .. ZMAX).  rc_out, zmax_out (each may be NULL): Rc and ZMAX, 0 on a refusal. */
int kc_worldmap_integrate_check(float resolution, size_t n_beams, float range_max, unsigned int flags,
                                const int32_t *zq_or_null, int32_t *rc_out, int64_t *zmax_out);
/* rule 52's quantiser (host only, needs no device): zq_out[k] is -1 for a NaN, a negative range
 * or a range below range_min; ZMAX for +inf or a range >= range_max; else llrint(ranges[k] /
 * resolution * 65536), rule 33's arithmetic.  -0.0 is not negative.  Refusals: null arguments,
 * kc_worldmap_integrate_check's without flags and zq, KC_ERR_INVALID unless range_min is a finite
 * float >= 0; then nothing is written. */
int kc_worldmap_quantise_ranges(float resolution, const double *ranges, size_t n, float range_max, float range_min,
                                int32_t *zq_out);
/* Rules 52 to 57 on the map: two launches on the map's stream (worldmap_mark_kernel, a beam's
 * walk shared among lanes in segments of 8 steps; worldmap_integrate_apply_kernel over the walk's
 * box clipped to the map) and the 20-byte read-back of rule 6's record; returns with the map final.  A scan whose box lies wholly outside
 * the map launches nothing and returns the empty record.  Checks: null arguments, then
 * kc_worldmap_integrate_check with zq, the angles (finite), the pose (as an update's), then the
 * device; a refused call queues nothing and leaves the map and the mark plane as they were. */
int kc_worldmap_integrate(kc_worldmap *ctx, const kc_worldmap_pose *pose, const double *angles, size_t n_beams,
                          const int32_t *zq, float range_max, unsigned int flags, kc_worldmap_result *result_out);
/* The same arguments, the mark launch alone (rules 53 and 54): the mark plane, a byte a cell at I
 * + J * width with bit 0 = MISS and bit 1 = HIT, is copied into marks_out (cap cells, at least
 * width * height, else KC_ERR_RANGE) and zeroed again; the map is untouched.  For tests, and for
 * finding out which half is wrong. */
int kc_worldmap_integrate_marks(kc_worldmap *ctx, const kc_worldmap_pose *pose, const double *angles, size_t n_beams,
                                const int32_t *zq, float range_max, unsigned int flags, uint8_t *marks_out, size_t cap);
/* Measurement only (rule 54's marks do not depend on it): a byte load in front of the mark kernel's
 * atomic that skips the atomic where the bit stands already.  Off by default: measured, it makes
 * the walk wait for a load every step. */
int kc_worldmap_integrate_set_precheck(kc_worldmap *ctx, int enable);
/* HIP events around the two launches of kc_worldmap_integrate; ms_out: mark, apply of the last
 * call.  KC_ERR_STATE when no integration has been timed. */
int kc_worldmap_integrate_set_timing(kc_worldmap *ctx, int enable);
int kc_worldmap_integrate_times(kc_worldmap *ctx, float ms_out[2]);

/* Finding moving obstacles in a measured scan (DESIGN.md 4.11 rules 64 to 70): the returns that
 * end where the map has seen free space far from anything occupied, grouped into runs of
 * neighbouring beams.  Nothing in the reference to cite, as above; integers throughout, bit-equal
 * to tests/worldmap_movers_ref.py.  The map is read and never written.
 * Rule 64, input: pose, angles and zq as rule 52's; m2 (1 <= m2 <= reach^2), gap (<= 64), join_q
 * (<= 2^40, in 2^-16 cells^2) and min_beams (1 .. 65536).  The distance plane must be on and m2
 * <= reach^2; it is refreshed first (rule 43) and read in place.  Rule 65, endpoint: for 0 <= zq_k
 * < ZMAX, (EX_k, EY_k) by rule 44 from the pose's (TX, TY) and rule 22's direction, I = EX >> 16,
 * J = EY >> 16; a beam with zq_k of -1 or ZMAX has none.  Rule 66, dynamic beam: it has an
 * endpoint, the endpoint lies inside the map, cls is KC_EMPTY there and dist2 > m2 (FAR counts as
 * above); a never-observed cell is new territory, not motion.  Rule 67, runs: over the dynamic
 * beams in scan order, beam k whose nearest earlier dynamic beam is p continues p's run iff k - p
 * <= gap + 1 and ((EX_k - EX_p) >> 8)^2 + ((EY_k - EY_p) >> 8)^2 <= join_q (arithmetic shifts);
 * otherwise, and for the first dynamic beam, it starts one.  The scan is not circular.  Rule 68,
 * kept clusters: the runs of at least min_beams members, numbered from 0 in the order of their
 * first beam, each with the record below; integer sums, minima and maxima, so no thread order
 * takes part.  Rule 69, outputs: label[k] is the kept cluster's number (beyond 255 too), -1 for a
 * beam that is not dynamic, -2 for a dynamic beam of a dropped run; the record; the first
 * n_returned cluster records. */
#define KC_WORLDMAP_MAX_CLUSTERS 256
typedef struct kc_worldmap_cluster { /* rule 68; 64 bytes */
  int32_t k_first, k_last;           /* the run's first and last beam */
  int32_t n;                         /* its members */
  int32_t reserved;                  /* 0 */
  int64_t sx, sy;                    /* the sums of EX and EY, below 2^54 in magnitude */
  int64_t min_x, max_x, min_y, max_y; /* of EX and EY */
} kc_worldmap_cluster;
typedef struct kc_worldmap_movers_record { /* rule 69 */
  uint32_t n_dynamic, n_runs, n_kept;
  uint32_t n_returned;                     /* min(n_kept, KC_WORLDMAP_MAX_CLUSTERS) */
} kc_worldmap_movers_record;
/* Rule 70's refusals (host only, needs no device), in this order: kc_worldmap_integrate_check's
 * without flags (the resolution and the counts, range_max, zq_or_null when given); then m2 == 0
 * (KC_ERR_INVALID), gap > 64, join_q > 2^40 (KC_ERR_RANGE), min_beams == 0 (KC_ERR_INVALID),
 * min_beams > 65536 (KC_ERR_RANGE).  zmax_out (may be NULL): ZMAX, 0 on a refusal. */
int kc_worldmap_movers_check(float resolution, size_t n_beams, float range_max, const int32_t *zq_or_null, uint32_t m2,
                             uint32_t gap, uint64_t join_q, uint32_t min_beams, int64_t *zmax_out);
/* Rules 64 to 69: the refresh of the distance plane where its box is dirty, then two launches on
 * the map's stream (worldmap_movers_flag_kernel, a lane a beam: the endpoint, the bounds test and
 * the two loads; worldmap_movers_cluster_kernel, one workgroup of 1024 lanes with a chunk of
 * consecutive beams a lane: compaction, rule 67's head test, the run and kept numbering by prefix
 * counts, a wavefront a returned cluster for the sums, the labels) and one read-back of record,
 * clusters and labels; returns with the outputs final.  label_out_or_null: n_beams int32.
 * clusters_out: cap records, of which min(n_returned, cap) are written.  Checks: null arguments,
 * then kc_worldmap_movers_check with zq, the angles (finite), the pose (as an update's), then
 * KC_ERR_STATE while the distance plane is off or for m2 > reach^2; a refused call queues
 * nothing, the refresh included, and writes an all-zero record. */
int kc_worldmap_movers(kc_worldmap *ctx, const kc_worldmap_pose *pose, const double *angles, size_t n_beams,
                       const int32_t *zq, float range_max, uint32_t m2, uint32_t gap, uint64_t join_q, uint32_t min_beams,
                       int32_t *label_out_or_null, kc_worldmap_cluster *clusters_out, size_t cap,
                       kc_worldmap_movers_record *record_out);
/* HIP events around the two launches of kc_worldmap_movers; ms_out: flag, cluster of the last
 * call.  KC_ERR_STATE when no detection has been timed. */
int kc_worldmap_movers_set_timing(kc_worldmap *ctx, int enable);
int kc_worldmap_movers_times(kc_worldmap *ctx, float ms_out[2]);

/* ------------------------------------------------------------------------ */
/* The localiser's fit record and its recovery by injected particles (DESIGN.md 4.11 rules 59 to 63) */
/* ------------------------------------------------------------------------ */
/* The recovery is off unless a caller asks for it: kc_mcl_step, kc_mcl_resample, kc_mcl_record
 * and the particles are what they were; the fit is formed at every step, beside the record.
 * Integers throughout, bit-equal to tests/worldmap_mcl_recovery_ref.py.
 * Rule 59, fit: with cost_p the penalty sum of particle p in this step alone (rule 34, or rules
 * 44 and 45), cost_sum = sum_p cost_p (uint64: N B <= 2^22 times a uint16 penalty passes 32
 * bits), cost_min = min_p cost_p, cost_best = cost_p of rule 35's best particle.  Unlike acc,
 * amin and the weights, which are relative to the particle set, these are absolute.  Formed by
 * the step's second launch from the costs it already reads, exact sums, no thread order; written
 * next to the record and read back with it in one copy.
 * Rule 60, the step's fit m: B_used is the number of beams that contributed, those with zq_k !=
 * -1 under the beam model (rule 33) and those with 0 <= zq_k < ZMAX under the field model (rule
 * 45); m = floor(cost_sum * 256 / (N * B_used)), the mean penalty a beam in 1 / 256, at most
 * 65535 * 256; a step with B_used = 0 says nothing.
 * Rule 61, two averages (Thrun's augmented MCL, in integers): a state (slow, fast, primed).
 * B_used = 0 leaves it as it is, n_inject = 0.  Not primed: slow = fast = m, primed, n_inject =
 * 0.  Primed: slow += (m - slow) >> a_slow, fast += (m - fast) >> a_fast, arithmetic shifts on
 * int64 (both stay within 0 .. 65535 * 256); n_inject = 0 when fast <= slow, else min(floor(N *
 * max_num / max_den), floor(N * (fast - slow) / fast)).  a_slow = 4, a_fast = 1 and max = 1 / 4
 * are the front ends' defaults: judgement, not measurement.  No threshold on m for "lost" is
 * given: a good one depends on the tables and the map, and none has been measured.
 * Rule 62, injecting resample with n of N slots injected: slot j is injected iff floor((j + 1)
 * n / N) > floor(j n / N): exactly n slots, spread evenly (the i-th is ceil((i + 1) N / n) - 1),
 * because rule 40 orders the slots by source index and a tail would drop the high indices.
 * Every other slot takes rule 40's state, u0 and the prefix sums over all N slots as there.  An
 * injected slot takes a free cell as rule 41's global draw does, with the current step counter
 * and channels 16 and 17: cell number draw(seed, step, j, 16) mod n_free in the order of I + J *
 * width over the KC_EMPTY cells of the class plane as it is at the resample (behind the map's
 * stream by the event, and behind rule 50's pending shift); with v = draw(seed, step, j, 17) the
 * sub-cell offsets and the heading come from v as in rule 41; acc = 0 as for every slot.  With
 * no free cell the injected slots keep rule 40's state, which is not an error.  n = 0 is
 * kc_mcl_resample.
 * Rule 63 (the host classes'): after every step m and rule 61 run, whether or not recovery is
 * on; with it on, the step ends with an injecting resample when rule 40 asks for a resample or
 * n_inject > 0; either init un-primes the averages. */
typedef struct kc_mcl_fit { /* rule 59 */
  uint64_t cost_sum;
  uint32_t cost_min, cost_best;
  uint32_t step; /* the step counter of the step that formed it, as the record's */
} kc_mcl_fit;
typedef struct kc_mcl_recovery { /* rule 61's state */
  int64_t slow, fast;
  int32_t primed;
} kc_mcl_recovery;
/* the last step's fit, from the host copy the step's read-back filled: no device work.
 * KC_ERR_STATE before the first step and after an init, kc_mcl_set_model or
 * kc_mcl_set_field_model; a resample leaves it. */
int kc_mcl_last_fit(kc_mcl *ctx, kc_mcl_fit *out);
/* Rules 60 and 61 (host only, needs no device).  *state is read and, unless the call is refused,
 * written; *m_out (may be NULL): m, or -1 when B_used = 0 or on a refusal; *n_inject_out: rule
 * 61's, 0 on a refusal.  Refusals, in this order: null arguments; KC_ERR_INVALID for a_slow, then
 * a_fast, outside 0 .. 30, for max_den == 0, for max_num > max_den; KC_ERR_RANGE for n_particles
 * outside 1 .. 65536, for beams_used above 1024, for cost_sum above n_particles * beams_used *
 * 65535 (no step forms one), and for a primed state with an average outside 0 .. 65535 * 256. */
int kc_mcl_recovery_update(uint64_t cost_sum, size_t n_particles, size_t beams_used, int a_slow, int a_fast, uint32_t max_num,
                           uint32_t max_den, kc_mcl_recovery *state, int64_t *m_out, size_t *n_inject_out);
/* Rule 62.  n_inject == 0 is kc_mcl_resample itself.  Otherwise five launches, no read-back:
 * the row counts and a one-workgroup exclusive prefix over the rows (the free-cell index, built
 * anew at every injecting resample, n_free read on the device), rule 40's prefix sum and select
 * over all N slots, then a wavefront an injected slot that overwrites it.  With n_inject > 0 the
 * call returns once its stream is idle: two of its kernels read the map's class plane, the map's
 * writers wait for no reader, and so the map may be written as soon as the call is back (the
 * plain resample reads no plane and returns without a wait, as before).  Checks: null context;
 * KC_ERR_RANGE for n_inject above N; then kc_mcl_resample's KC_ERR_STATE. */
int kc_mcl_resample_inject(kc_mcl *ctx, size_t n_inject);
/* HIP-event times in milliseconds of the last injecting resample's three own launches (row
 * counts, row prefix, inject), recorded while kc_mcl_set_timing is on; its prefix and select are
 * kc_mcl_times' last two.  KC_ERR_STATE when none was timed. */
int kc_mcl_inject_times(kc_mcl *ctx, float ms_out[3]);

/* ------------------------------------------------------------------------ */
/* MPPI control over the map's distance plane (DESIGN.md 4.12 rules 1 to 36) */
/* ------------------------------------------------------------------------ */
/* Nothing in the reference to cite: its controllers commit to one velocity for the whole
 * look-ahead.  K noisy control sequences of T steps around a nominal one, rolled out in the
 * localiser's integers, costed against the distance plane and a window of path points, blended
 * by table weights.  Integers throughout, exact sums: no result depends on thread order,
 * tests/mppi_ref.py states every rule in Python ints and the device equals it bit for bit.  No
 * kernel modifies the map; the context keeps no sequence between calls (the warm start is the
 * caller's).  "Rule 28 .. 45" below are 4.11's, above.
 * Rule 1, state: (TX, TY, h) as rule 28: int64 with 16 fraction bits of a cell, clamped to
 * +-2^36; h in 2^-16 turn.  Its cell: I = (TX + 2^15) >> 16, J alike (cell (0, 0)'s centre is
 * the origin).
 * Rule 2, control sequence: U[t] = (F, L, H), int32, t < T, 1 <= T <= 64.  F: the forward
 * displacement a step, L the lateral one, 2^-16 cells; H: the heading change a step, heading
 * units.  Limits F_lo <= F <= F_hi, |L| <= L_hi, |H| <= H_hi with |F_lo|, |F_hi|, L_hi <= 2^22,
 * H_hi <= 32767.  The cone kq, 0 <= kq <= 2^24: when kq > 0 also |H| <= (|F| kq) >> 16 (a
 * car: a front end forms kq = lrint(65536 / (2 pi R_min_cells))).  clampU(F, L, H) applies the
 * box, then the cone with the clamped F.
 * Rule 3, samples: 1 <= K <= 65536.  key = mix64(seed ^ (step << 32)), step the call's.  For
 * sample k, step t, channel c in 0 .. 2: eps = noise(mix64(key ^ ((k << 8) | (3 t + c))), s_c),
 * rule 30's mix64 and noise, s_c >= 0; sample 0 has eps = 0, so the nominal sequence is among
 * the samples.  X_k[t] = clampU(U[t] + eps).
 * Rule 4, roll-out: rule 31 without its noise.  With (C, S) = (Cq(h), Sq(h)) of the heading
 * before the step: TX += (C F - S L + 2^15) >> 16, TY += (S F + C L + 2^15) >> 16, both
 * clamped, h = (h + H) & 0xFFFF.
 * Rule 5, obstacle term, at the state after each step t: d2 = dist2[I + J W] inside the map,
 * FAR outside (rule 45).  d2 <= r2: the sample has hit; it adds pen_hit (T - t), its state is
 * frozen and its later steps add nothing from rules 5 and 6.  Otherwise it adds d2 <= c2 ?
 * pen_d2[d2] : pen_far.  pen_d2: c2 + 1 uint16 entries, 1 <= c2 <= min(reach^2, 4095), r2 <=
 * c2, pen_hit <= 2^20.
 * Rule 6, path term, the same states, samples that have not hit: M points (PX_j, PY_j) in the
 * state's units, 1 <= M <= 256, |PX|, |PY| <= 2^36.  q_j = ((TX - PX_j) >> 8)^2 + ((TY - PY_j)
 * >> 8)^2 (q >> 16 is cells^2), key_j = (min(q_j, qcap) << 8) | j; the smallest key gives qm
 * and jm: the lowest index among equals, equals at the cap included.  It adds (qm w_path) >>
 * 16.  qcap <= 2^40, w_path <= 2^16, (qcap >> 16) w_path <= 2^24.
 * Rule 7, terminal term: w_goal (M - 1 - jm), jm of the last state rule 6 saw, 0 for a sample
 * that hit at step 0; w_goal <= 2^20.
 * Rule 8, total: the terms summed in 64 bits, S_k = min(sum, 2^30).  S_min the smallest,
 * k_best the lowest index with it.
 * Rule 9, weights: w_k = wtab[min((S_k - S_min) >> w_shift, EW - 1)], wtab as rule 36's: the
 * best sample's weight is wtab[0] >= 1.
 * Rule 10, update: den = sum_k w_k; for every t and channel num = sum_k w_k (X_k[t][c] -
 * U[t][c]), exact in int64 (2^20 2^23 2^16); U'[t][c] = U[t][c] + floor((2 num + den) / (2
 * den)), then clampU.
 * Rule 11, record: kc_mppi_record.
 * Rule 12, refusals: kc_mppi_check (host only, needs no device), in this order: KC_ERR_INVALID
 * for no sample, no step or no path point; KC_ERR_RANGE above 65536 samples, then above 64
 * steps, then above 256 path points; limits (skipped when NULL; five words F_lo, F_hi, L_hi,
 * H_hi, kq): KC_ERR_INVALID for F_lo > F_hi or a negative L_hi, H_hi or kq, KC_ERR_RANGE for a
 * displacement limit beyond 2^22, then H_hi above 32767, then kq above 2^24, KC_ERR_INVALID for
 * s NULL or a negative scale; costs (skipped when pen_d2 is NULL): KC_ERR_INVALID below 2
 * entries, KC_ERR_RANGE above 4096, KC_ERR_INVALID for r2 > c2, KC_ERR_RANGE for pen_hit above
 * 2^20, w_path above 2^16, qcap above 2^40, (qcap >> 16) w_path above 2^24, w_goal above 2^20,
 * in that order; reach (skipped when 0): KC_ERR_RANGE outside 1 .. 254, KC_ERR_INVALID for c2 >
 * reach^2; then wtab as kc_mcl_check has it (KC_ERR_INVALID when NULL).
 * Moving obstacles, costed at each roll-out step's own time (tests/mppi_movers_ref.py states
 * rules 13 to 18; with no mover every result is rules 1 to 12's, bit for bit):
 * Rule 13, movers: 0 <= N <= 64, each (OX, OY, VX, VY, hq, sq, g).  OX, OY: int64 in the
 * state's units and the map's present offset, valid at the time of the step's pose, |.| <=
 * 2^36.  VX, VY: int32 displacements a control step, |.| <= 2^22.  hq <= sq <= 2^40: uint64
 * squared centre distances in rule 6's q units, the hit distance and where the soft term
 * begins.  g <= 2^32: the ramp's gain, with (((sq - hq) >> 16) g) >> 16 <= 2^20.  pen_hit_mv <=
 * 2^20 is one value for all movers.
 * Rule 14, position: at the state after step t mover i stands at OX_i + (t + 1) VX_i, OY_i + (t
 * + 1) VY_i, exact and unclamped.  dx = (TX - OXt) >> 8, dy alike (|.| < 2^30), q_i = min(dx^2 +
 * dy^2, 2^40).
 * Rule 15, order inside a step: rule 4 moves the state, rule 5 tests the plane; a sample that
 * hit the plane is frozen as before and rule 16 is not evaluated for it at that state or later
 * (a static hit wins a tie).  A sample still alive meets rule 16, then rule 5's penalty, then
 * rule 6.
 * Rule 16, mover term: any q_i <= hq_i: the sample has hit; it adds pen_hit_mv (T - t), is
 * frozen and adds nothing more from rules 5, 6 and 16.  Otherwise it adds the sum over i of q_i
 * < sq_i ? (((sq_i - q_i) >> 16) g_i) >> 16 : 0, a ramp in the squared distance.  Rule 7's jm
 * is that of the last state rule 6 saw.
 * Rule 17, record: n_hit counts samples ended by either kind of hit, n_hit_moving those a
 * mover ended; 0 with no mover.
 * Rule 18, refusals: kc_mppi_check_movers (host only), in this order: N = 0 is never an error;
 * KC_ERR_RANGE above 64 movers; KC_ERR_INVALID for a NULL array; KC_ERR_RANGE for pen_hit_mv
 * above 2^20; then mover by mover in index order KC_ERR_RANGE for a position beyond 2^36, then
 * a velocity beyond 2^22, KC_ERR_INVALID for hq > sq, KC_ERR_RANGE for sq above 2^40, then g
 * above 2^32, then the ramp's top above 2^20.
 * The grid planner's cost field, read in place (tests/mppi_field_ref.py states rules 19 to 24;
 * with no field attached every result is rules 1 to 18's, bit for bit):
 * Rule 19, field: fld[I + J W], uint32, with the map's W x H and the map's cell frame;
 * 0xFFFFFFFF: no walk reaches the goal.  fv(I, J) is the plane's value inside the map and
 * 0xFFFFFFFF outside; fc = min(fv, fcap), 1 <= fcap <= 2^24.
 * Rule 20, mode: with a field attached rules 6 and 7 are not evaluated; no path window is
 * needed (kc_mppi_set_path need not have been called, M plays no part).  At every state a live
 * sample reaches it adds (fc w_run) >> 8, w_run <= 2^12, behind rule 5's test, rule 16 where
 * movers are set, and rule 5's penalty.
 * Rule 21, terminal term: w_term fl, w_term <= 64; fl is the fc of the last state rule 20 saw,
 * for a sample that hit at step 0 the fc of the step's own pose cell.  Rule 8 sums and caps.
 * Rule 22, read-back: behind the record, in the same copy, f0 (the uncapped fv of the pose's
 * cell) and f_nom (the fl of sample 0): kc_mppi_last_field.  kc_mppi_record keeps its layout.
 * Rule 23, refusals: kc_mppi_check_field (host only), in this order: KC_ERR_INVALID for fcap ==
 * 0; KC_ERR_RANGE for fcap above 2^24, then w_run above 2^12, then w_term above 64.  A step with
 * a field attached answers KC_ERR_STATE, before anything is queued, when the planner holds no
 * goal-rooted disc-mode field (its last solve-type call was not kc_planner_solve or
 * kc_planner_replan, plain or with the clearance cost: none yet, or the oriented, car or explore
 * call), then when the field's shape is not the map's.
 * Rule 24, frame: the ABI works in cells; the caller sees to it that the field was solved on
 * this map at its present window offset.
 * Acceleration limits inside the roll-out (tests/mppi_rates_ref.py states rules 25 to 29; off by
 * default, and with no rates set every result, launch, upload and read-back is rules 1 to 24's):
 * Rule 25, rates and start velocity: R = (F_up, F_dn, L_up, L_dn, H_up, H_dn), int32, a change a
 * control step in rule 2's units, each at least 1; the F and L rates at most 2^23, the H rates at
 * most 65535.  V0 = (F0, L0, H0), int32: the robot's velocity in front of the step, |F0|, |L0| <=
 * 2^22, |H0| <= 32767; it need not lie inside rule 2's box.
 * Rule 26, applied control: lim(p, x, up, dn) = p < x ? min(p + up, x) : max(p - dn, x) (up for
 * a rising value, dn for a falling one, signed).  A_k[-1] = V0; for each t, channel by channel, A
 * = lim(A_k[t - 1], X_k[t], up, dn); then, when kq > 0, A_H is clamped to +-((|A_F| kq) >> 16)
 * with the F just applied.  The value behind the cone is the p of the next step; a shrinking
 * cone may move A_H faster than H_dn (a car's yaw rate is tied to its speed).
 * Rule 27, roll-out: rule 4 moves the state by A_k[t] in place of X_k[t].  Rules 5 to 9, 13 to
 * 17 and 19 to 22 are unchanged, and so is rule 10: it blends X_k, not A_k.  Sample 0 is the
 * nominal sequence under the limits: S_0 and f_nom are what the robot would pay for U.  With V0
 * inside the box and every rate at least the box's width (F_hi - F_lo, 2 L_hi, 2 H_hi), A = X.
 * Rule 28, applied sequence: kc_mppi_apply_rates (host only) is rule 26 over a sequence; a front
 * end forms its command from out[0] of U' and keeps that triple as the next step's V0.
 * Rule 29, refusals: kc_mppi_check_rates (host only), in this order: NULL rates are never an
 * error (the mode is off, whatever v0 is); KC_ERR_INVALID for a rate below 1, in index order;
 * KC_ERR_RANGE for an F or L rate above 2^23, then an H rate above 65535; v0 (skipped when
 * NULL): KC_ERR_RANGE for |F0| or |L0| beyond 2^22, then |H0| above 32767.
 * A box footprint as a chain of discs (tests/mppi_box_ref.py states rules 30 to 36; off by
 * default, and with no footprint set every result, launch, upload and read-back is rules 1 to
 * 29's):
 * Rule 30, footprint list: NB offsets o_i along the body's forward axis, 1 <= NB <= 8, int32 in
 * 16 fraction bits of a cell, |o_i| <= 2^22; they need not be symmetric about the pose.  All
 * discs share rule 5's r2.
 * Rule 31, disc centres: with (C, S) the heading pair of the state's heading after the step
 * (not the pair the step moved by), CX_i = TX + ((C o_i + 2^15) >> 16), CY_i = TY + ((S o_i +
 * 2^15) >> 16), not clamped; their cells by rule 5's rounding, d2_i from the plane or FAR outside
 * the map, dm = min d2_i.  Rule 5 runs on dm in the place of d2.
 * Rule 32, movers: rule 14's q is the least over the discs of the capped squared distance from
 * (CX_i, CY_i) to the mover, in the same >> 8 arithmetic.
 * Rule 33, field mode: the field is still read at the pose's own cell.
 * Rule 34, rates: the discs turn with the heading the applied control produced.
 * Rule 35, refusals: kc_mppi_check_footprint (host only), in this order: n = 0 is never an
 * error; KC_ERR_RANGE for n above 8; KC_ERR_INVALID for a NULL array; KC_ERR_RANGE for an offset
 * beyond 2^22, in index order.
 * Rule 36, cover: the front ends' doubles (Control::MPPI::footprintOf), not the ABI's. */
typedef struct kc_mppi kc_mppi;
#define KC_MPPI_MAX_SAMPLES 65536
#define KC_MPPI_MAX_HORIZON 64
#define KC_MPPI_MAX_PATH 256
#define KC_MPPI_MAX_TABLE 4096
#define KC_MPPI_MAX_MOVERS 64
#define KC_MPPI_MAX_DISCS 8
typedef struct kc_mppi_record { /* rules 11 and 17 */
  uint64_t den;                 /* sum of the weights */
  uint32_t s_min, k_best;       /* rule 8 */
  uint32_t s_0;                 /* the nominal sequence's cost */
  uint32_t n_hit;               /* samples that hit, the plane or a mover */
  uint32_t step;                /* the call's */
  uint32_t n_hit_moving;        /* those among them that a mover ended; 0 with no mover */
} kc_mppi_record;
int kc_mppi_check(size_t n_samples, size_t horizon, size_t n_path, const int32_t *limits_or_null, const int32_t *s_or_null, uint32_t r2,
                  const uint16_t *pen_d2_or_null, size_t n_pen, uint32_t pen_hit, uint32_t w_path, uint64_t qcap, uint32_t w_goal,
                  int reach, const uint32_t *wtab_or_null, size_t n_wtab, int w_shift);
/* A controller of n_samples sequences of `horizon` steps over `map`, on its device, with its
 * own stream; the map must outlive it.  Checks: null arguments, kc_mppi_check's counts, then
 * the device. */
int kc_mppi_create(kc_worldmap *map, size_t n_samples, size_t horizon, uint64_t seed, kc_mppi **out);
void kc_mppi_destroy(kc_mppi *ctx);
/* rule 2's limits and rule 3's three scales, checked as kc_mppi_check does */
int kc_mppi_set_model(kc_mppi *ctx, int32_t f_lo, int32_t f_hi, int32_t l_hi, int32_t h_hi, int32_t kq, const int32_t *s);
/* rules 5 to 9's tables and scalars, checked as kc_mppi_check does with reach 0 */
int kc_mppi_set_costs(kc_mppi *ctx, uint32_t r2, const uint16_t *pen_d2, size_t n_pen, uint16_t pen_far, uint32_t pen_hit, uint32_t w_path,
                      uint64_t qcap, uint32_t w_goal, const uint32_t *wtab, size_t n_wtab, int w_shift);
/* rule 6's window, in the map's present offset (rule 46): KC_ERR_INVALID for none, KC_ERR_RANGE
 * above 256 points or for a coordinate beyond +-2^36 */
int kc_mppi_set_path(kc_mppi *ctx, const int64_t *px, const int64_t *py, size_t n);
/* rule 18's refusals of a list of n movers; host only, needs no device */
int kc_mppi_check_movers(const int64_t *ox, const int64_t *oy, const int32_t *vx, const int32_t *vy, const uint64_t *hq,
                         const uint64_t *sq, const uint64_t *g, size_t n, uint32_t pen_hit_mv);
/* rule 13's list, in the map's present offset and at the time of the next step's pose; checked
 * as kc_mppi_check_movers does, then uploaded on the context's stream (one copy of 3 KB; the
 * call returns with it over).  It holds for every later step until the next call; n = 0 clears
 * it, and the steps after that are those of a context that never had one.  A refused call
 * leaves the list as it was. */
int kc_mppi_set_movers(kc_mppi *ctx, const int64_t *ox, const int64_t *oy, const int32_t *vx, const int32_t *vy, const uint64_t *hq,
                       const uint64_t *sq, const uint64_t *g, size_t n, uint32_t pen_hit_mv);
/* rule 23's refusals of the field term's three scalars; host only, needs no device */
int kc_mppi_check_field(uint32_t fcap, uint32_t w_run, uint32_t w_term);
/* Attaches `planner`'s kept cost field (rules 19 to 24), checked as kc_mppi_check_field does;
 * the planner must be on the controller's device and outlive the attachment.  Nothing is read
 * here: every later step asks the planner for its field (kc_planner_field_device; its two
 * buffers alternate between solves), orders its stream behind the planner's and reads the field
 * where it lies.  A step ends in its read-back, so once it has returned no reader is in flight
 * and the planner may solve or replan.  planner NULL detaches, whatever else is given: the
 * steps after that are those of a context that never had a field.  A refused call leaves the
 * attachment as it was. */
int kc_mppi_set_field(kc_mppi *ctx, kc_planner *planner_or_null, uint32_t fcap, uint32_t w_run, uint32_t w_term);
/* rule 22's two words of the last step; KC_ERR_STATE (both 0xFFFFFFFF) when that step had no
 * field attached or there was none */
int kc_mppi_last_field(kc_mppi *ctx, uint32_t *f0_out, uint32_t *f_nom_out);
/* rule 29's refusals of six rates and, when given, a start velocity; host only, needs no device */
int kc_mppi_check_rates(const int32_t *rates_or_null, const int32_t *v0_or_null);
/* Rule 25's six rates for every later step, checked as kc_mppi_check_rates does: the roll-out is
 * mppi_rollout_kernel<TEAM, MOVERS, FIELD, true> from then on.  NULL turns the mode off: the
 * steps after that are those of a context that never had rates.  A refused call leaves the rates
 * as they were. */
int kc_mppi_set_rates(kc_mppi *ctx, const int32_t *rates_or_null);
/* Rule 25's V0 (three words) for every later step until the next call; zero in a new context.
 * Kept on the host: it rides behind U in the step's one upload while rates are set and plays no
 * part while none are.  KC_ERR_INVALID for NULL, then rule 29's two refusals of a v0. */
int kc_mppi_set_velocity(kc_mppi *ctx, const int32_t *v0);
/* Rule 28: rule 26 over the sequence u (horizon x 3, inside rule 2's bounds) from v0, into out
 * (horizon x 3; it may be u).  Host only.  limits: rule 12's five words, of which the cone kq
 * plays a part.  Checks, in this order: null arguments; the horizon and the limits as
 * kc_mppi_check has them; kc_mppi_check_rates; KC_ERR_RANGE for a control of u outside +-2^22,
 * +-2^22, +-32767. */
int kc_mppi_apply_rates(const int32_t *limits, const int32_t *rates, const int32_t *v0, const int32_t *u, size_t horizon, int32_t *out);
/* rule 35's refusals of a list of n disc offsets; host only, needs no device */
int kc_mppi_check_footprint(const int32_t *offsets_or_null, size_t n);
/* Rule 30's list for every later step, checked as kc_mppi_check_footprint does: the roll-out is
 * mppi_rollout_kernel<TEAM, MOVERS, FIELD, RATE, true> from then on, the offsets eight ints
 * among its arguments (no upload).  n = 0 clears it: the steps after that are those of a context
 * that never had a footprint.  A refused call leaves the list as it was. */
int kc_mppi_set_footprint(kc_mppi *ctx, const int32_t *offsets_or_null, size_t n);
/* One step (rules 3 to 11): two launches (mppi_rollout_kernel, mppi_update_kernel) behind the
 * plane's refresh and an event on the map's stream, and one read-back of U' and the record;
 * returns with both final.  u_in, u_out: T x 3 int32 (F, L, H a step); they may be one array.
 * Checks, in this order: null arguments; KC_ERR_STATE without a model, then without costs,
 * then without a path; KC_ERR_RANGE for |tx|, |ty| > 2^36, then h > 65535, then a control of
 * u_in outside +-2^22, +-2^22, +-32767; KC_ERR_STATE while the map's distance plane is off or
 * c2 > reach^2; then the device.  A refused call queues nothing.  With a field attached (rules
 * 19 to 24) no path is asked for, rule 23's KC_ERR_STATE comes behind the plane's (then
 * KC_ERR_INVALID for a planner on another device), the roll-out is mppi_rollout_kernel<TEAM,
 * MOVERS, true> and the read-back carries f0 and f_nom behind the record: still two launches,
 * one upload and one read-back.  With rates set (rules 25 to 29) V0 rides behind U in the upload
 * and rule 4 moves every sample by its applied control: the same counts again.  With a footprint
 * set (rules 30 to 36) the offsets ride in the roll-out's arguments: the same counts once more. */
int kc_mppi_step(kc_mppi *ctx, int64_t tx, int64_t ty, uint32_t h, const int32_t *u_in, uint32_t step, int32_t *u_out,
                 kc_mppi_record *record);
/* all S_k of the last step, for tests and plots; cap: the entries s_out holds (KC_ERR_RANGE
 * below K); KC_ERR_STATE before a step */
int kc_mppi_costs(kc_mppi *ctx, uint32_t *s_out, size_t cap);
/* Measurement only (no result depends on it): the lanes that share a sample in the roll-out, 1,
 * 4 or 8; the default is what DESIGN.md 4.12 measured as the faster: 8, and in the field mode 4
 * while neither a mover nor a footprint is set.  A call fixes the count for both modes.
 * KC_ERR_INVALID otherwise. */
int kc_mppi_set_team(kc_mppi *ctx, int lanes);
/* HIP-event times in milliseconds of the last step's two launches (rollout, update), recorded
 * only while enabled.  KC_ERR_STATE when no step was timed. */
int kc_mppi_set_timing(kc_mppi *ctx, int enable);
int kc_mppi_times(kc_mppi *ctx, float ms_out[2]);

#ifdef __cplusplus
}
#endif
#endif /* KOMPASS_HIP_H */
