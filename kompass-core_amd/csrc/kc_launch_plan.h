// Launch plans of the DWA host path: which kernel, which template instance, how many samples per workgroup, how much
// LDS -- decided here as pure functions from plain facts to plain plans, carried out in kc_dwa_sensor.hip and
// kc_dwa_cycle.hip.  Host-only like kc_hostmath.h: no HIP include, compiles with plain g++ (tests/native/launch_plan.cpp).
// The sizing constants the plans need live here; the device headers include this file.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace kc {

// ---- sizing constants ------------------------------------------------------------------------------------------
constexpr int kSensorBlock = 1024;
constexpr int kHistRowsMax = 16;   // the host picks points per thread so that the histogram rows fit (plan_sensor: ppt)
// largest point list the device-side sensor update takes (bucket grid of at most 64 x 64 cells: about one obstacle per
// cell up to 4 k points, hundreds per cell here); beyond: the host path, finer grid.  (262144 until a raw depth image --
// 307 200 points -- was priced: 6 ms of host build at 500 k points against 0.16 ms here, tools/big_cloud_sweep.py.)
constexpr size_t kSensorDeviceMax = 1048576;
// sensor_points_kernel packs id | rank << 12 into a signed int: 12 bits of bucket id, 19 of the rank of a point among its
// workgroup's kSensorBlock * ppt points.  The largest workgroup holds kSensorDeviceMax / kHistRowsMax points (64 k today).
static_assert(kSensorDeviceMax / kHistRowsMax < (1u << 19), "the rank field of id | rank << 12 is 19 bits");
constexpr size_t kSensorFusedMax = 32768;       // points up to which the one-launch sensor build CAN be used (spheres: it is their only device build)
constexpr size_t kSensorFusedPays = 18432;      // ... and up to which it is ahead: every workgroup reads every point (tools/big_cloud_sweep.py,
                                                // set_points + cycle with the one launch / the two: 10 k points 80.6 / 86.4 us, 16 k 161 / 160,
                                                // 20 k 84.1 / 79.6, 24 k 91.7 / 84.4, 30 k 100.3 / 93.6)
constexpr size_t kSensorFusedLds = 100 * 1024;  // dynamic LDS of sensor_fused_kernel (band rows; bucket tables + point ids)
constexpr int kCompactMaxPer = 64;  // compact_kernel: 1024 threads x 64 = 65536 samples
constexpr int kCostGrid = 256;      // one workgroup per CU
constexpr size_t kCostLdsBudget = 150 * 1024;  // LDS the search tables of a sample_cost_kernel workgroup may take
constexpr size_t kBlkLdsBudget = 78 * 1024;    // ... and of a sample_cost_block_kernel workgroup (two per CU)
// Longest list the workgroup-per-sample kernel gets by itself.  Round 2 measured a crossover near 650 samples; since then
// the wavefront-per-sample kernel got the near table, the union-rectangle scan and the folded publish, and round 4's
// density sweep finds it ahead at every list length (cfg3: 0 / 123 / 489 admissible: 10.4 / 24.2 / 25.7 us against
// 7.3 + 6.5 / 27.7 + 6.6 / 36.7 + 6.6 with the publish kernel the block kernel needs; cfg2's three-kernel cycle at 393:
// 18.9 against 16.4 + 6.6).  The block kernel stays behind option cost_kernel = 1.
constexpr long long kBlockKernelMaxAdm = -1;

inline unsigned blocks_for(size_t n, unsigned per) { return static_cast<unsigned>((n + per - 1) / per); }

// ---- trig ------------------------------------------------------------------------------------------------------
// The one range rule of kc_trig_exact.h: the kernels form cos / sin(yaw_k) themselves only while every yaw_k of the
// chain yaw0 + k * omega * dt stays inside the range the restated algorithm covers (|yaw| < 105414350; this bound on
// |yaw0| + steps * |omega|max * dt decides).  What a caller does otherwise -- the host's libm, or KC_ERR_RANGE -- is its own.
inline bool yaw_reach_ok(double yaw0, double om_max, double dt, size_t steps, double *reach_out = nullptr) {
  const double reach = std::fabs(yaw0) + om_max * dt * static_cast<double>(steps);
  if (reach_out) *reach_out = reach;
  return std::isfinite(reach) && reach < 1.0e8;
}

// ---- roll-out / cycle ------------------------------------------------------------------------------------------
struct RollFacts {
  size_t n, P, lds_limit;    // samples of the shard, poses per sample, dynamic LDS the kernels may take (0: option force_split)
  int num_cus;
  bool want_cycle;           // kc_dwa_cycle asks for the single launch
  bool sphere, tilted, have_gbits, gz_valid;
  bool win_enabled;          // the collision window (CollDev): there is sensor data; rows, words per row, dilated masks
  int win_H, win_wpr, win_dil;
  int cycle_samples_opt, fused_samples, fused_block;  // options
  bool cycle_fused, cycle_forced, fused_shape_fixed;
};
struct RollPlan {
  int cs;                    // samples per workgroup of the cycle kernel
  unsigned cyc_G;            // ... and its workgroups
  bool cycle;                // the single launch: a candidate after plan_rollout, settled by cycle_fits
  bool fused;                // roll-out + collision gate in one kernel (else the split path)
  int fs, fb;                // fused tile: samples per workgroup, threads
  unsigned grid;             // ... and its workgroups
  size_t pos_bytes, bits_bytes, tab_off;
};

inline RollPlan plan_rollout(const RollFacts &f) {
  RollPlan p{};
  // One launch pays while every workgroup of the shard is resident at once (32 samples per workgroup, one workgroup per
  // CU: 8192 samples on an MI355X -- the per-GPU share of every BASELINE config on 8 GPUs).  Beyond, the cycle kernel's
  // LDS footprint (one workgroup per CU) loses to the three-kernel cycle, whose roll-out kernel fits two per CU (cfg5 on
  // ONE GPU, 65536 samples: 0.214 against 0.129 ms).
  // 32 samples per workgroup; 16 when that would leave half of the CUs without one (a 4096-sample shard -- cfg3 split
  // over 8 GPUs -- or any mid-size lattice): twice the workgroups, half the poses and survivors in each.  (Option
  // "cycle_samples": 0 = this rule, 16 / 32 = fixed.)
  p.cs = f.cycle_samples_opt;
  if (p.cs == 0) p.cs = 2 * blocks_for(f.n, 32) <= static_cast<unsigned>(f.num_cus) ? 16 : 32;
  // the last arriver of the ticket epilogue holds two workgroup keys per lane (kc_cycle_dev.h): at most
  // 2048 workgroups, whatever the option says (65536 samples in 16-sample workgroups would be 4096)
  if (blocks_for(f.n, static_cast<unsigned>(p.cs)) > 2048u) p.cs = 32;
  p.cyc_G = blocks_for(f.n, static_cast<unsigned>(p.cs));
  // (Rounds 2-3 sent small lattices with many survivors to the stand-alone cost kernels -- "they spread the survivors
  // over all CUs".  Round 4's lattice sweep, 110 .. 2025 samples, half or all of them admissible: the single launch is
  // 3 us ahead everywhere -- the second launch costs more than the spreading gains.  One resident round of workgroups is
  // the only condition left.)
  const bool cyc_wave = p.cyc_G <= static_cast<unsigned>(f.num_cus);
  const bool sphere_ok = !f.sphere || (f.have_gbits && f.gz_valid);  // (fused path)
  p.cycle = f.want_cycle && f.cycle_fused && sphere_ok && f.n <= 1024u * kCompactMaxPer && (f.cycle_forced || cyc_wave);
  // fused path: trig rows + poses (fs x P double2) and the window bits in LDS.  Roll-out tile of the three-kernel cycle:
  // 32 samples per workgroup; 1024 threads, or 512 for a large lattice of short trajectories (cfg5, 65536 x 50: more
  // workgroups resident per CU hide the serial recurrence of each other, 80 -> 45 us; P = 100 or one resident round:
  // 1024 is better, tools/fused_cfg_sweep.sh)
  int plain_fb = f.fused_block;
  if (!f.fused_shape_fixed && f.P <= 64 && blocks_for(f.n, 32) > 4u * static_cast<unsigned>(f.num_cus)) plain_fb = 512;
  p.fs = p.cycle ? p.cs : f.fused_samples;
  p.fb = p.cycle ? 1024 : plain_fb;
  p.grid = blocks_for(f.n, static_cast<unsigned>(p.fs));
  p.pos_bytes = static_cast<size_t>(p.fs) * (f.P | 1) * 16;  // (double2)
  p.bits_bytes = (f.win_enabled ? static_cast<size_t>(f.win_H) * f.win_wpr * 4 * (f.win_dil ? 3 : 1) : 0) +
                 static_cast<size_t>(p.fs) * f.P * sizeof(int);  // + queue of undecided poses
  p.fused = sphere_ok && !f.tilted && (!f.win_enabled || f.have_gbits) && p.pos_bytes + p.bits_bytes + 512 <= f.lds_limit;
  p.tab_off = (p.pos_bytes + p.bits_bytes + 15) & ~size_t(15);
  return p;
}
// the cycle's cost tables (table_bytes: cycle_table_bytes of the cost arguments, known once they are built) behind the tile
inline bool cycle_fits(const RollFacts &f, const RollPlan &p, size_t table_bytes) {
  return p.cycle && p.fused && p.tab_off + table_bytes + 2048 <= f.lds_limit;
}
// The plan of a roll-out whose cycle was dropped.  A fused tile sized for the cycle is planned again for the plain
// shape; the split path reads no tile shape and keeps its plan.
inline RollPlan without_cycle(RollFacts f, const RollPlan &p) {
  f.want_cycle = false;
  RollPlan q = p.fused ? plan_rollout(f) : p;
  q.cycle = false;
  return q;
}

// ---- sensor update ---------------------------------------------------------------------------------------------
// key of a coordinate in the 16-level octree (points beyond it are dropped by add_voxel anyway)
inline int voxel_key(double inv_res, float v) {
  const double f = std::floor(inv_res * static_cast<double>(v));
  return static_cast<int>(std::min(std::max(f, -32768.0), 32767.0));
}

// Spheres (round 4; the host build took 120 us of a 176 us cycle): a voxel's z gap to the sphere's centre is a function
// of its LAYER, so add_voxel's rule is evaluated once per layer the cloud's z range can hold -- accepted layers,
// their gaps in ascending order (the LUT of the exact tests), the code of every layer -- and the one-launch build keeps
// the smallest code of every voxel column (sensor_band_body).  The gap bound of the dilated masks is the largest gap of
// those layers: at least the largest gap present, so "certain hits" stay certain.  More than 36 layers or 32 gaps: the
// host build (ok = false).
struct SphereLayers {
  bool ok;
  int kz0, nkz;             // first layer, layers
  unsigned char code[36];   // per layer: 0 = rejected, else 1 + the rank of its gap in lut
  double lut[32];           // distinct gaps, ascending
  int nlut;
  double gmax;              // largest accepted gap (-1: no layer of the cloud can touch the sphere: no masks, no voxels)
};
inline SphereLayers plan_sphere_layers(int kz_lo, int kz_hi, double zc, double radius, double res, double inv_res) {
  SphereLayers s{};
  s.gmax = -1.0;
  // (only the layers that can touch the sphere: a 3-D cloud spans two metres of height, forty layers of 5 cm -- the
  // rule below rejects a layer whose gap exceeds the radius, i.e. every layer outside [zc - r, zc + r] and a layer of
  // slack; the kernel rejects whatever lies outside the table)
  const int k0 = std::max(kz_lo, static_cast<int>(std::max(std::floor((zc - radius) * inv_res) - 1.0, -32768.0)));
  const int k1 = std::min(kz_hi, static_cast<int>(std::min(std::floor((zc + radius) * inv_res) + 1.0, 32767.0)));
  if (k1 - k0 + 1 > 36) return s;
  double gap[36];
  double lut[36];
  int nlut = 0;
  for (int kz = k0; kz <= k1; ++kz) {  // add_voxel, the sphere branch
    const double zlo = static_cast<double>(kz) * res, zhi = static_cast<double>(kz + 1) * res;
    double ddz = 0.0;
    if (zlo - zc > ddz) ddz = zlo - zc;
    if (zc - zhi > ddz) ddz = zc - zhi;
    gap[kz - k0] = ddz > radius ? -1.0 : ddz;
    if (gap[kz - k0] >= 0.0) {
      s.gmax = std::max(s.gmax, ddz);
      bool seen = false;
      for (int q = 0; q < nlut; ++q) seen = seen || lut[q] == ddz;
      if (!seen) lut[nlut++] = ddz;
    }
  }
  std::sort(lut, lut + nlut);
  if (nlut > 32) return s;
  for (int kz = k0; kz <= k1; ++kz)
    if (gap[kz - k0] >= 0.0)
      s.code[kz - k0] = static_cast<unsigned char>(std::lower_bound(lut, lut + nlut, gap[kz - k0]) - lut + 1);
  std::copy(lut, lut + nlut, s.lut);
  s.nlut = nlut;
  s.kz0 = k0;
  s.nkz = std::max(k1 - k0 + 1, 0);
  s.ok = true;
  return s;
}

struct SensorFacts {
  size_t n;                  // points
  bool sphere, two_launch, fused_ok;  // option "sensor_two_launch"; sensor_fused_kernel may take kSensorFusedLds
  int gH, gwpr;              // the bitmap: rows, words per row
  int dilR;                  // halo rows of the dilated masks (-1: none)
  double blo[2], bhi[2];     // hull of the transformed bounding box (the bucket grid covers it)
};
struct SensorPlan {
  // bucket grid: origin (the hull's low corner minus the margin), cell size, cells
  double gx0, gy0, g, inv_g;
  int side, W, H;
  // bands of the one-launch build: rows per band, bands (= workgroups), LDS bytes of a band
  int band_rows, nb;
  size_t band_bytes;
  bool fused;                // one launch (sensor_fused_kernel); a sphere that is not fused takes the host build
  int ppt, rows;             // two launches: points per thread, workgroups of the points kernel
};
inline SensorPlan plan_sensor(const SensorFacts &f) {
  SensorPlan p{};
  double blo[2] = {f.blo[0], f.blo[1]}, bhi[2] = {f.bhi[0], f.bhi[1]};
  const double ext0 = std::max(bhi[0] - blo[0], bhi[1] - blo[1]);
  const double margin = 1e-4 * ext0 + 1e-4;  // float rounding of the transformed points
  blo[0] -= margin;
  blo[1] -= margin;
  bhi[0] += margin;
  bhi[1] += margin;
  p.side = std::min(64, std::max(8, static_cast<int>(std::ceil(std::sqrt(static_cast<double>(f.n))))));
  const double ext = std::max(bhi[0] - blo[0], bhi[1] - blo[1]);
  p.g = std::max(0.125, ext / (p.side - 1));
  p.inv_g = 1.0 / p.g;
  p.gx0 = blo[0];
  p.gy0 = blo[1];
  p.W = std::min(p.side, static_cast<int>((bhi[0] - blo[0]) * p.inv_g) + 1);
  p.H = std::min(p.side, static_cast<int>((bhi[1] - blo[1]) * p.inv_g) + 1);
  // One launch, no hand-over between workgroups (sensor_fused_kernel): every workgroup reads all points and keeps
  // its part -- bands of the bitmap with their dilations, slices of the bucket tables.  Beyond 32 k points (every
  // workgroup reading every point stops being free) or with bands that do not fit LDS: the two-launch build.
  int nb = std::min(64, f.gH);
  p.band_rows = (f.gH + nb - 1) / nb;
  // (LDS of a band: its rows + R rows of halo either side, and the two dilation accumulators of its own rows; a sphere
  // adds a byte per column of its rows)
  auto band_bytes = [&] {
    return (3 * static_cast<size_t>(p.band_rows) + 2 * static_cast<size_t>(std::max(f.dilR, 0)) +
            (f.sphere ? 32 * static_cast<size_t>(p.band_rows) : 0)) * f.gwpr * 4;
  };
  while (band_bytes() > kSensorFusedLds && p.band_rows > 1) p.band_rows = (p.band_rows + 1) / 2;
  p.nb = (f.gH + p.band_rows - 1) / p.band_rows;
  p.band_bytes = band_bytes();
  p.fused = !f.two_launch && f.fused_ok && f.n <= (f.sphere ? kSensorFusedMax : kSensorFusedPays) &&
            p.band_bytes <= kSensorFusedLds && p.nb <= 1024;
  p.ppt = static_cast<int>((f.n + static_cast<size_t>(kHistRowsMax) * kSensorBlock - 1) / (static_cast<size_t>(kHistRowsMax) * kSensorBlock));
  p.rows = static_cast<int>(blocks_for(f.n, static_cast<unsigned>(static_cast<size_t>(kSensorBlock) * p.ppt)));
  return p;
}

// ---- cost stage ------------------------------------------------------------------------------------------------
// Short admissible lists (the count of the previous cycle is the predictor) go to the workgroup-per-sample kernel, long
// ones to the wavefront-per-sample kernel; both are correct for any list.  (force: option "cost_kernel")
inline bool cost_use_block(long long last_nadm, int force) {
  bool use_block = last_nadm >= 0 && last_nadm <= kBlockKernelMaxAdm;
  if (force == 1) use_block = true;
  if (force == 2) use_block = false;
  return use_block;
}
struct CostFacts {
  size_t n, P, S;
  int num_cus;
  long long last_nadm;
  bool use_block;            // cost_use_block
  bool external, timing;     // caller-provided batch; kernels are being timed one by one
  bool use_seg, use_obs;
  bool have_vel, whole_batch;  // velocity profiles are there; the batch is the whole roll-out (n == n_roll, first == 0)
  int vel_kinds;             // of smoothness and jerk, how many have a weight
  int bW, bH, nobs;          // bucket grid
  size_t seg_pairs, nch, nsup;  // seg_pairs_padded, chunks, super chunks of the tracked segment
  size_t scan_floats, batch_bytes;  // scan block of the scan's near table (0: none); batch_buf_bytes(P)
  int velocity_group;        // options and limits
  bool velocity_beside, fold_publish, cost_batch, cost_batch_forced, cost_batch_ok, cost_lds_ok, cost_obs_lds;
};
struct CostPlan {
  bool use_block;
  int group;                 // samples per wavefront of the velocity sums: 1 = inside the cost kernel, 4 / 16 = a pass of their own
  bool vel_beside;           // ... on a second stream beside the cost kernel
  bool batched, tab_lds, obs_lds, fold;
  size_t tab_bytes, obs_bytes;  // LDS of the search tables (+ batch buffers), of the obstacles
  size_t lds;                // dynamic LDS of the launch
  unsigned grid;
};
inline CostPlan plan_cost(const CostFacts &f) {
  CostPlan p{};
  p.use_block = f.use_block;
  p.group = 1;
  if (f.have_vel && f.vel_kinds > 0 && f.whole_batch) {
    // ordered sums of the velocity profiles.  One sample per wavefront inside the cost kernel while the
    // batch leaves a SIMD fewer than ~5 of these serial chains (latency bound either way); beyond, 4 samples
    // per wavefront in a pass of their own (a quarter of the chain instructions), 16 for batches that still
    // give every SIMD several chains then (tools/cost5k_terms.py)
    const size_t simds = 4 * static_cast<size_t>(f.num_cus);
    p.group = f.velocity_group;
    if (p.group == 0) p.group = f.vel_kinds * f.n < 5 * simds ? 1 : (f.vel_kinds * f.n < 96 * simds ? 4 : 16);
  }
  // Beside the wavefront-per-sample cost kernel on a second stream: these chains leave most issue slots
  // of their SIMDs idle, the segment searches fill them (not while kernels are being timed one by one)
  p.vel_beside = p.group > 1 && !f.use_block && !f.timing && f.velocity_beside;
  // the long-list kernel publishes by itself (its last workgroup) unless the velocity sums finish behind it
  p.fold = !f.use_block && !p.vel_beside && f.fold_publish;
  size_t lds_tab = 0, lds_obs = 0;
  if (f.use_obs) {
    const size_t ncell = static_cast<size_t>(f.bW) * f.bH;
    lds_tab += (ncell + 1) * sizeof(int) + ((ncell + 3) & ~size_t(3));
    lds_obs = 2 * static_cast<size_t>(f.nobs) * sizeof(float);
    // (with a scan's near table the wavefront kernels keep the scan block there instead: x | y | chunk boxes)
    if (f.scan_floats) lds_obs = std::max(lds_obs, f.scan_floats * sizeof(float));
  }
  if (f.use_block) {
    p.grid = static_cast<unsigned>(std::min<size_t>(f.n, 512));
    const size_t lds = (f.P * 3 * sizeof(float) + 15) & ~size_t(15);
    if (f.use_seg) lds_tab += 5 * f.S * sizeof(float);
    p.tab_lds = f.cost_lds_ok && lds + lds_tab + 64 <= kBlkLdsBudget;
    p.obs_lds = p.tab_lds && f.use_obs && lds + lds_tab + lds_obs + 64 <= kBlkLdsBudget;
    p.lds = lds + (p.tab_lds ? lds_tab : 0) + (p.obs_lds ? lds_obs : 0);
  } else {
    // one workgroup per CU, sixteen samples (wavefronts) in flight in each
    p.grid = static_cast<unsigned>(std::min<size_t>(f.n, kCostGrid));
    if (f.use_seg) lds_tab += (8 * f.seg_pairs + 8 * f.nch + 12 * f.nsup) * sizeof(float);  // pair records, capsules, spheres
    // batched per-sample part (two buffers of 64 samples in front of the tables): the DWA cycle's lists, and
    // caller-provided batches whose velocity sums are precomputed or not asked for
    const size_t lds_batch = 2 * f.batch_bytes;
    const bool wave_sums = f.have_vel && f.vel_kinds > 0 && p.group == 1;  // (the sums are formed inside the kernel)
    // ... and lists that fill more than one buffer per workgroup now and then (the last cycle's count is the
    // predictor; measured: 141 samples per workgroup -14 % kernel time, 50: -3 %, 18: +4 %, 10: +6 %)
    const long long expect = f.external ? static_cast<long long>(f.n) : (f.last_nadm >= 0 ? f.last_nadm : static_cast<long long>(f.n));
    p.batched = f.cost_batch && f.cost_batch_ok && f.cost_lds_ok && !wave_sums &&
                (f.cost_batch_forced || expect >= 40ll * kCostGrid) && lds_tab + lds_batch + 64 <= kCostLdsBudget;
    if (p.batched) lds_tab += lds_batch;
    p.tab_lds = f.cost_lds_ok && lds_tab + 64 <= kCostLdsBudget;
    p.obs_lds = p.tab_lds && f.use_obs && lds_tab + lds_obs + 64 <= kCostLdsBudget && f.cost_obs_lds;
    p.lds = (p.tab_lds ? lds_tab : 0) + (p.obs_lds ? lds_obs : 0);
  }
  p.tab_bytes = lds_tab;
  p.obs_bytes = lds_obs;
  return p;
}

// ---- window patterns -------------------------------------------------------------------------------------------
// Kept patterns of a context whose windows hold n samples (find_pattern, kc_sample_pattern.h): 40 bytes of device
// memory a sample and pattern, 128 MB of them at most, 16 to 256 patterns.
inline size_t pattern_slots(size_t n) {
  return std::min<size_t>(256, std::max<size_t>(16, (size_t(128) << 20) / (40 * std::max<size_t>(n, 1))));
}

}  // namespace kc
