// The launch plans of the DWA host path (csrc/kc_launch_plan.h) against expectations worked out by hand from the rules
// the header's comments state -- none of them copied from the functions under test.  Plain g++, no GPU.
#include <cmath>
#include <cstdio>
#include <limits>

#include "kc_launch_plan.h"

using namespace kc;

static int checks = 0, bad = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    ++checks;                                                        \
    if (!(cond)) {                                                   \
      ++bad;                                                         \
      std::printf("line %d: %s\n", __LINE__, #cond);                 \
    }                                                                \
  } while (0)

constexpr size_t kLds = 150 * 1024;

// a 256-CU device, default options, no sensor data
static RollFacts roll(size_t n, size_t P, bool want_cycle = true) {
  RollFacts f{};
  f.n = n;
  f.P = P;
  f.lds_limit = kLds;
  f.num_cus = 256;
  f.want_cycle = want_cycle;
  f.cycle_fused = true;
  f.fused_samples = 32;
  f.fused_block = 1024;
  return f;
}

static void samples_per_workgroup() {
  CHECK(plan_rollout(roll(4096, 20)).cs == 16);  // 128 workgroups of 32 would leave half of 256 CUs idle
  RollPlan p = plan_rollout(roll(8192, 20));
  CHECK(p.cs == 32 && p.cyc_G == 256 && p.cycle);  // one resident round
  p = plan_rollout(roll(8193, 20));
  CHECK(p.cyc_G == 257 && !p.cycle);  // a 257th workgroup: no single resident round
  RollFacts f = roll(8193, 20);
  f.cycle_forced = true;
  CHECK(plan_rollout(f).cycle);
  f = roll(65536, 20);
  f.cycle_samples_opt = 16;
  CHECK(plan_rollout(f).cs == 32);  // 4096 workgroups of 16: beyond the 2048 of the ticket epilogue
  f = roll(32768, 20);
  f.cycle_samples_opt = 16;
  CHECK(plan_rollout(f).cs == 16 && plan_rollout(f).cyc_G == 2048);
  f = roll(1024 * static_cast<size_t>(kCompactMaxPer) + 1, 20);
  f.cycle_forced = true;
  CHECK(!plan_rollout(f).cycle);  // beyond compact_kernel: no cycle, whatever the option says
  f.n -= 1;
  CHECK(plan_rollout(f).cycle);
  f = roll(4096, 20);
  f.cycle_fused = false;
  CHECK(!plan_rollout(f).cycle);
  CHECK(!plan_rollout(roll(4096, 20, false)).cycle);
  f = roll(4096, 20);  // a sphere needs the device-built z codes
  f.sphere = true;
  CHECK(!plan_rollout(f).cycle && !plan_rollout(f).fused);
  f.have_gbits = f.gz_valid = true;
  CHECK(plan_rollout(f).cycle && plan_rollout(f).fused);
}

static void plain_tile() {
  RollPlan p = plan_rollout(roll(65536, 50, false));  // 2048 workgroups > 4 x 256, short trajectories
  CHECK(p.fs == 32 && p.fb == 512 && p.grid == 2048);
  p = plan_rollout(roll(65536, 100, false));
  CHECK(p.fs == 32 && p.fb == 1024);
  p = plan_rollout(roll(32768, 50, false));  // 1024 workgroups: not MORE than four rounds
  CHECK(p.fb == 1024);
  RollFacts f = roll(65536, 50, false);
  f.fused_shape_fixed = true;
  f.fused_samples = 16;
  f.fused_block = 256;
  p = plan_rollout(f);
  CHECK(p.fs == 16 && p.fb == 256 && p.grid == 4096);
  p = plan_rollout(roll(4096, 20));  // the cycle's tile: its samples, 1024 threads
  CHECK(p.cycle && p.fs == 16 && p.fb == 1024 && p.grid == 256);
}

static void byte_formulas() {
  for (int dil = 0; dil < 2; ++dil)
    for (size_t P : {8, 20, 21, 100}) {
      RollFacts f = roll(4096, P);
      f.win_enabled = f.have_gbits = true;
      f.win_H = 121;
      f.win_wpr = 5;
      f.win_dil = dil;
      RollPlan p = plan_rollout(f);
      const size_t pos = 16 * (P | 1) * 16, bits = 121 * 5 * 4 * (dil ? 3 : 1) + 16 * P * 4;
      CHECK(p.fs == 16 && p.pos_bytes == pos && p.bits_bytes == bits && p.tab_off == ((pos + bits + 15) / 16) * 16);
      CHECK(p.fused);
      f.lds_limit = pos + bits + 512;
      CHECK(plan_rollout(f).fused);
      f.lds_limit = pos + bits + 511;
      CHECK(!plan_rollout(f).fused);
      f.lds_limit = 0;  // option force_split
      CHECK(!plan_rollout(f).fused);
      f.win_enabled = false;  // no sensor data: no window bits
      f.lds_limit = kLds;
      CHECK(plan_rollout(f).bits_bytes == 16 * P * 4);
      // the cycle stays iff tab_off + tables + 2048 <= lds_limit
      f.win_enabled = true;
      p = plan_rollout(f);
      const size_t room = kLds - 2048 - p.tab_off;
      CHECK(cycle_fits(f, p, room) && !cycle_fits(f, p, room + 1) && cycle_fits(f, p, 0));
    }
  RollFacts f = roll(4096, 20);  // a window without the device bitmap, a tilted frame: the split path
  f.win_enabled = true;
  f.win_H = f.win_wpr = 4;
  CHECK(!plan_rollout(f).fused);
  f.have_gbits = true;
  CHECK(plan_rollout(f).fused);
  f.tilted = true;
  CHECK(!plan_rollout(f).fused);
}

static void dropped_cycle() {
  int dropped = 0;
  for (size_t n : {16, 110, 2025, 4096, 4097, 8192, 8193, 65536})
    for (size_t P : {8, 50, 64, 65, 100, 400})
      for (int side : {0, 41, 401, 2001})
        for (size_t lds : {size_t(0), size_t(64 * 1024), kLds}) {
          RollFacts f = roll(n, P);
          f.lds_limit = lds;
          f.win_enabled = f.have_gbits = side != 0;
          f.win_H = side;
          f.win_wpr = (side + 31) / 32;
          f.win_dil = 1;
          const RollPlan p = plan_rollout(f);
          if (!p.cycle) continue;
          const RollPlan q = without_cycle(f, p);  // (as if the tables did not fit)
          f.want_cycle = false;
          const RollPlan r = plan_rollout(f);
          CHECK(!q.cycle && !r.cycle && q.fused == r.fused && q.cs == r.cs);
          if (q.fused)
            CHECK(q.fs == r.fs && q.fb == r.fb && q.grid == r.grid && q.pos_bytes == r.pos_bytes && q.bits_bytes == r.bits_bytes);
          ++dropped;
        }
  CHECK(dropped > 100);
}

static SensorFacts sensor(size_t n, int gH, int gwpr, int dilR, bool sphere = false) {
  SensorFacts f{};
  f.n = n;
  f.sphere = sphere;
  f.fused_ok = true;
  f.gH = gH;
  f.gwpr = gwpr;
  f.dilR = dilR;
  f.bhi[0] = f.bhi[1] = 1.0;
  return f;
}

static void sensor_bands() {
  SensorPlan p = plan_sensor(sensor(1000, 64, 10, 3));  // 64 bands of one row: (3 + 2 x 3) rows of 10 words
  CHECK(p.band_rows == 1 && p.nb == 64 && p.band_bytes == 360 && p.fused);
  p = plan_sensor(sensor(1000, 100, 10, -1));  // 64 bands at most: two rows each, 50 bands; no masks, no halo
  CHECK(p.band_rows == 2 && p.nb == 50 && p.band_bytes == 240 && p.fused);
  // 8192 rows of 256 words, R = 30: 128 rows a band are (384 + 60) KB; halved to 64, 32, 16 (108 KB), 8 (84 KB)
  p = plan_sensor(sensor(1000, 8192, 256, 30));
  CHECK(p.band_rows == 8 && p.nb == 1024 && p.band_bytes == 84 * 1024 && p.fused);
  // a sphere adds 32 rows-worth of words per row: 8 rows are 340 KB, 4: 200, 2: 130, 1: 95 KB -- in 8192 bands
  p = plan_sensor(sensor(1000, 8192, 256, 30, true));
  CHECK(p.band_rows == 1 && p.nb == 8192 && p.band_bytes == 95 * 1024 && !p.fused);
  p = plan_sensor(sensor(1000, 100, 10, 2, true));
  CHECK(p.band_rows == 2 && p.band_bytes == (6 + 4 + 64) * 40 && p.fused);
  CHECK(kSensorFusedLds == 100 * 1024);
  p = plan_sensor(sensor(1000, 1, 256, 30));  // a single row cannot be halved: (3 + 60) KB fits
  CHECK(p.band_rows == 1 && p.nb == 1 && p.fused);
  p = plan_sensor(sensor(1000, 4, 256, 50));  // ... and (3 + 100) KB does not
  CHECK(p.band_rows == 1 && !p.fused);
  // fused versus two launches
  SensorFacts f = sensor(kSensorFusedPays, 64, 10, 3);
  CHECK(plan_sensor(f).fused);
  f.n += 1;
  CHECK(!plan_sensor(f).fused);
  f.sphere = true;  // a sphere's only device build: up to kSensorFusedMax
  CHECK(plan_sensor(f).fused);
  f.n = kSensorFusedMax + 1;
  CHECK(!plan_sensor(f).fused);
  f = sensor(1000, 64, 10, 3);
  f.two_launch = true;
  CHECK(!plan_sensor(f).fused);
  f = sensor(1000, 64, 10, 3);
  f.fused_ok = false;
  CHECK(!plan_sensor(f).fused);
}

static void sensor_bucket_grid() {
  SensorFacts f = sensor(100, 64, 10, 3);  // side = ceil(sqrt(100)) = 10 cells
  f.blo[0] = -1.0;
  f.bhi[0] = 3.0;  // 4 m x 1 m: margin 1e-4 x 4 + 1e-4 = 5e-4
  f.blo[1] = 0.0;
  f.bhi[1] = 1.0;
  SensorPlan p = plan_sensor(f);
  CHECK(p.side == 10 && std::fabs(p.gx0 - (-1.0005)) < 1e-12 && std::fabs(p.gy0 - (-0.0005)) < 1e-12);
  CHECK(std::fabs(p.g - 4.001 / 9) < 1e-12 && p.W == 10 && p.H == 3);  // 1.001 / 0.4446 = 2.25 -> 3 cells
  f.n = 9;  // at least 8 cells a side, at most 64; cells of at least 0.125 m
  CHECK(plan_sensor(f).side == 8);
  f.n = 1000000;
  p = plan_sensor(f);
  CHECK(p.side == 64 && p.g == 0.125 && p.W == 33 && p.H == 9);  // 4.001 / 0.125 = 32.008, 1.001 / 0.125 = 8.008
}

static void sphere_layers() {
  // centre 0, radius 0.12, 5 cm layers, a cloud over layers -10 .. 10: [-0.12, 0.12] is layers -3 .. 2, one layer of
  // slack either side -> -4 .. 3; the slack layers' gap (0.15) exceeds the radius: rejected
  SphereLayers s = plan_sphere_layers(-10, 10, 0.0, 0.12, 0.05, 20.0);
  CHECK(s.ok && s.kz0 == -4 && s.nkz == 8 && s.nlut == 3);
  CHECK(s.lut[0] == 0.0 && s.lut[1] == 0.05 && s.lut[2] == 2 * 0.05 && s.gmax == 2 * 0.05);
  const unsigned char want[8] = {0, 3, 2, 1, 1, 2, 3, 0};  // gaps 0.15 | 0.1 0.05 0 0 0.05 0.1 | 0.15: ranks from 1
  for (int k = 0; k < 8; ++k) CHECK(s.code[k] == want[k]);
  s = plan_sphere_layers(-1, 0, 0.0, 0.12, 0.05, 20.0);  // the cloud's own range clips
  CHECK(s.ok && s.kz0 == -1 && s.nkz == 2 && s.nlut == 1 && s.code[0] == 1 && s.code[1] == 1 && s.gmax == 0.0);
  s = plan_sphere_layers(10, 12, 0.0, 0.12, 0.05, 20.0);  // a cloud above the sphere: no layer
  CHECK(s.ok && s.nkz == 0 && s.nlut == 0 && s.gmax == -1.0);
  s = plan_sphere_layers(-18, 17, 0.0, 5.0, 0.05, 20.0);  // 36 layers (18 gaps, shared by the layers either side)
  CHECK(s.ok && s.nkz == 36 && s.nlut == 18);
  CHECK(!plan_sphere_layers(-18, 18, 0.0, 5.0, 0.05, 20.0).ok);  // 37 layers
  // layers 0 .. 31 above the centre: gaps 0, 0.05, ... 1.55, 32 of them; layer 32 is the 33rd
  s = plan_sphere_layers(0, 31, 0.0, 5.0, 0.05, 20.0);
  CHECK(s.ok && s.nlut == 32 && s.code[0] == 1 && s.code[31] == 32);
  CHECK(!plan_sphere_layers(0, 32, 0.0, 5.0, 0.05, 20.0).ok);
  CHECK(plan_sphere_layers(-16, 16, 0.0, 5.0, 0.05, 20.0).nlut == 17);  // (symmetric layers share their gaps)
  CHECK(voxel_key(20.0, 0.26f) == 5 && voxel_key(20.0, -0.01f) == -1 && voxel_key(20.0, 1e9f) == 32767 &&
        voxel_key(20.0, -1e9f) == -32768);
}

static void sensor_two_launch() {
  const size_t per = static_cast<size_t>(kHistRowsMax) * kSensorBlock;  // points of sixteen workgroups at one per thread
  CHECK(per == 16384);
  struct { size_t n; int ppt, rows; } want[] = {{1, 1, 1}, {1024, 1, 1}, {1025, 1, 2}, {per - 1, 1, 16}, {per, 1, 16},
                                                {per + 1, 2, 9}, {3 * per, 3, 16}, {3 * per + 1, 4, 13},
                                                {kSensorDeviceMax, 64, 16}};
  for (const auto &w : want) {
    const SensorPlan p = plan_sensor(sensor(w.n, 64, 10, 3));
    CHECK(p.ppt == w.ppt && p.rows == w.rows && p.rows <= kHistRowsMax);
  }
}

static CostFacts cost(size_t n, long long last_nadm) {
  CostFacts f{};
  f.n = n;
  f.P = 20;
  f.num_cus = 256;
  f.last_nadm = last_nadm;
  f.velocity_beside = f.fold_publish = f.cost_batch = f.cost_batch_ok = f.cost_lds_ok = f.cost_obs_lds = true;
  return f;
}

static void cost_plan() {
  for (long long nadm : {-1ll, 0ll, 1ll, 650ll, 100000ll}) {
    CHECK(cost_use_block(nadm, 0) == (nadm >= 0 && nadm <= kBlockKernelMaxAdm));
    CHECK(cost_use_block(nadm, 1) && !cost_use_block(nadm, 2));
  }
  // batched only from 40 x kCostGrid expected survivors, or forced
  CHECK(kCostGrid == 256);
  CHECK(plan_cost(cost(20000, 10240)).batched && !plan_cost(cost(20000, 10239)).batched);
  CHECK(plan_cost(cost(10240, -1)).batched && !plan_cost(cost(10239, -1)).batched);  // no count yet: every sample
  CostFacts f = cost(20000, 100);
  f.external = true;  // a caller's batch: every sample is admissible
  CHECK(plan_cost(f).batched);
  f = cost(100, 100);
  f.cost_batch_forced = true;
  CHECK(plan_cost(f).batched);
  f.cost_batch = false;
  CHECK(!plan_cost(f).batched);
  f = cost(20000, 20000);
  f.cost_lds_ok = false;
  CHECK(!plan_cost(f).batched && !plan_cost(f).tab_lds && plan_cost(f).lds == 0);
  f = cost(20000, 20000);  // ... without wave sums: velocity sums formed inside the kernel
  f.have_vel = true;
  f.vel_kinds = 1;
  f.whole_batch = false;
  CHECK(plan_cost(f).group == 1 && !plan_cost(f).batched);
  f.whole_batch = true;  // (20000 chains: a pass of their own, group 4)
  CHECK(plan_cost(f).group == 4 && plan_cost(f).batched);
  f = cost(20000, 20000);  // ... and within the LDS budget: two batch buffers + 64 bytes
  f.batch_bytes = (kCostLdsBudget - 64) / 2;
  CHECK(plan_cost(f).batched && plan_cost(f).lds == kCostLdsBudget - 64);
  f.batch_bytes += 1;
  CHECK(!plan_cost(f).batched && plan_cost(f).lds == 0);
  // velocity group 1 / 4 / 16 at 5 and 96 chains per SIMD (1024 SIMDs)
  f = cost(5119, -1);
  f.have_vel = f.whole_batch = true;
  f.vel_kinds = 1;
  CHECK(plan_cost(f).group == 1 && !plan_cost(f).vel_beside);
  f.n = 5120;
  CHECK(plan_cost(f).group == 4 && plan_cost(f).vel_beside);
  f.n = 98303;
  CHECK(plan_cost(f).group == 4);
  f.n = 98304;
  CHECK(plan_cost(f).group == 16);
  f.vel_kinds = 2;
  f.n = 2559;
  CHECK(plan_cost(f).group == 1);
  f.n = 2560;
  CHECK(plan_cost(f).group == 4);
  f.velocity_group = 16;
  f.n = 10;
  CHECK(plan_cost(f).group == 16);
  f.vel_kinds = 0;
  CHECK(plan_cost(f).group == 1);
  // fold only for the long-list kernel without the sums beside it
  f = cost(5120, -1);
  CHECK(plan_cost(f).fold);
  f.fold_publish = false;
  CHECK(!plan_cost(f).fold);
  f = cost(5120, -1);
  f.use_block = true;
  CHECK(!plan_cost(f).fold);
  f = cost(5120, -1);
  f.have_vel = f.whole_batch = true;
  f.vel_kinds = 1;
  CHECK(plan_cost(f).vel_beside && !plan_cost(f).fold);
  f.timing = true;  // kernels timed one by one: the pass stays on the stream, in front
  CHECK(!plan_cost(f).vel_beside && plan_cost(f).fold);
  f.timing = false;
  f.use_block = true;
  CHECK(!plan_cost(f).vel_beside);
  // grids and LDS
  CHECK(plan_cost(cost(100, -1)).grid == 100 && plan_cost(cost(1000, -1)).grid == 256);
  f = cost(1000, -1);
  f.use_block = true;
  CHECK(plan_cost(f).grid == 512 && plan_cost(f).lds == 240 && plan_cost(f).tab_lds && !plan_cost(f).obs_lds);
  f.use_seg = true;  // block kernel: five floats a segment point
  f.S = 100;
  CHECK(plan_cost(f).lds == 240 + 2000);
  f.S = (kBlkLdsBudget - 240 - 64) / 20;  // 78 KB budget
  CHECK(plan_cost(f).tab_lds);
  f.S += 1;
  CHECK(!plan_cost(f).tab_lds && plan_cost(f).lds == 240);
  f = cost(1000, -1);  // wave kernel: pair records 32 B, capsules 32 B, spheres 48 B; cells + skip bytes; obstacles
  f.use_seg = f.use_obs = true;
  f.seg_pairs = 100;
  f.nch = 10;
  f.nsup = 2;
  f.bW = f.bH = 10;
  f.nobs = 50;
  CostPlan p = plan_cost(f);
  CHECK(p.tab_bytes == 101 * 4 + 100 + 3200 + 320 + 96 && p.obs_bytes == 400 && p.tab_lds && p.obs_lds && p.lds == p.tab_bytes + 400);
  f.scan_floats = 1000;  // the scan block instead of the obstacle coordinates, when it is larger
  CHECK(plan_cost(f).obs_bytes == 4000);
  f.cost_obs_lds = false;
  CHECK(!plan_cost(f).obs_lds && plan_cost(f).lds == p.tab_bytes);
}

static void yaw_reach() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  CHECK(yaw_reach_ok(std::nextafter(1.0e8, 0.0), 0.0, 0.1, 100) && !yaw_reach_ok(1.0e8, 0.0, 0.1, 100));
  CHECK(yaw_reach_ok(-std::nextafter(1.0e8, 0.0), 0.0, 0.1, 100) && !yaw_reach_ok(-1.0e8, 0.0, 0.1, 100));
  CHECK(yaw_reach_ok(0.0, 1.0e5, 0.5, 1999) && !yaw_reach_ok(0.0, 1.0e5, 0.5, 2000));  // steps x |omega| dt
  CHECK(!yaw_reach_ok(nan, 1.0, 0.1, 10) && !yaw_reach_ok(0.0, nan, 0.1, 10) && !yaw_reach_ok(0.0, 1.0, nan, 10));
  CHECK(!yaw_reach_ok(inf, 1.0, 0.1, 10) && !yaw_reach_ok(-inf, 1.0, 0.1, 10) && !yaw_reach_ok(0.0, inf, 0.1, 10));
  double reach = 0.0;
  CHECK(yaw_reach_ok(-1.0, 2.0, 0.5, 10, &reach) && reach == 11.0);
}

// kept window patterns: 128 MB / (40 bytes x n samples), held between 16 and 256.  By hand: 2^27 / 40 = 3355443.2, so
// 256 patterns fit while n <= 13107 (3355443.2 / 256 = 13107.2) and the quotient falls below 16 past n = 209715
// (3355443.2 / 16 = 209715.2)
static void kept_patterns() {
  CHECK(pattern_slots(0) == 256);
  CHECK(pattern_slots(1) == 256);
  CHECK(pattern_slots(13107) == 256);
  CHECK(pattern_slots(13108) == 255);
  CHECK(pattern_slots(209715) == 16);
  CHECK(pattern_slots(209716) == 16);
  CHECK(pattern_slots(size_t(1) << 20) == 16);
}

int main() {
  kept_patterns();
  samples_per_workgroup();
  plain_tile();
  byte_formulas();
  dropped_cycle();
  sensor_bands();
  sensor_bucket_grid();
  sphere_layers();
  sensor_two_launch();
  cost_plan();
  yaw_reach();
  std::printf("launch plans: %d checks, %d bad\n", checks, bad);
  return bad ? 1 : 0;
}
