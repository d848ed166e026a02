// Raw point cloud -> laserscan on gfx950, and, in the second half of the file, points -> 2-D
// occupancy grid (readPCDToOccupancyGrid, utils/pointcloud.h:468-540).
//
// Reference: pointCloudToLaserScanFromRaw, utils/pointcloud.h:116-177 (angle
// step) and :205-259 (bin count); the SYCL kernel of the reference
// (local_mapper_gpu.cpp:59-164) is a float re-implementation with its own
// atan2 and is NOT what this reproduces: the contract here is the CPU loop.
//
// One lane per point record.  The bin of a point depends on the host libm's
// atan2f (std::atan2(float, float)); the device evaluates atan2 in double and
// keeps a point only when its angle is more than 1e-6 rad away from both edges
// of its bin -- the float result of a < 1 ulp atan2f (2.4e-7 rad at pi) cannot
// fall into another bin then.  (A float atan2 settles the points farther than
// 3e-6 rad from an edge first; only the rest pays for the double one.)  The few points closer to an edge go to a list
// the host re-bins with the reference expression.  Distances are
// sqrtf(x*x + y*y) (correctly rounded on both sides) and the per-bin minimum
// is a 64-bit atomic min on the bits of the non-negative double.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "kc_internal.h"
#include "kompass_hip.h"

namespace kc {

struct CloudArgs {
  const uint8_t *data;
  size_t nbytes;
  long long n_records;   // height * ceil(row_step / point_step)
  int per_row;           // records per row
  int point_step, row_step;
  int x_off, y_off, z_off, max_off;
  double min_z, max_z;
  double angle_step;     // > 0: bin = int(angle / angle_step); else int(angle / 2pi * num_bins)
  int num_bins;
  double edge;           // 1e-6 rad expressed in bins
  unsigned long long max_bits;   // bits of max_range
  unsigned long long *bins;      // [num_bins] double bits (kLds = false: armed with max_range)
  unsigned long long *partial;   // [gridDim.x][num_bins] per-workgroup minima (kLds = true)
  unsigned int *list_count;
  float2 *list;                  // (x, y) of the points the host has to bin
  int packed16;                  // aligned 16-byte records with x, y, z in front, rows contiguous
  long long n_packed;            // ... and how many of them fit the buffer
  int ftype, fsize;              // PointFieldType of the x / y / z fields (utils/pointcloud.h:37-46) and its size
};

// load_and_cast_val, utils/pointcloud.h:49-87: a field of any PointCloud2 datatype as float, byte by byte
__device__ __forceinline__ float load_field(const uint8_t *p, int t) {
  auto u16 = [&]() { return static_cast<uint16_t>(static_cast<uint16_t>(p[0]) | (static_cast<uint16_t>(p[1]) << 8)); };
  auto u32 = [&]() {
    return static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16) |
           (static_cast<uint32_t>(p[3]) << 24);
  };
  switch (t) {
    case KC_FIELD_INT8: return static_cast<float>(static_cast<int8_t>(p[0]));
    case KC_FIELD_UINT8: return static_cast<float>(p[0]);
    case KC_FIELD_INT16: return static_cast<float>(static_cast<int16_t>(u16()));
    case KC_FIELD_UINT16: return static_cast<float>(u16());
    case KC_FIELD_INT32: return static_cast<float>(static_cast<int32_t>(u32()));
    case KC_FIELD_UINT32: return static_cast<float>(u32());
    case KC_FIELD_FLOAT32: return __uint_as_float(u32());
    case KC_FIELD_FLOAT64: {
      const uint64_t lo = u32();
      p += 4;
      const uint64_t hi = u32();
      return static_cast<float>(__longlong_as_double(static_cast<long long>(lo | (hi << 32))));
    }
    default: return 0.0f;
  }
}

__device__ __forceinline__ float load_f32(const uint8_t *p) {
  uint32_t u;
  if ((reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
    u = *reinterpret_cast<const uint32_t *>(p);
  } else {
    u = static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8) |
        (static_cast<uint32_t>(p[2]) << 16) | (static_cast<uint32_t>(p[3]) << 24);
  }
  return __uint_as_float(u);
}

template <bool kLds>
__device__ __forceinline__ void cloud_point(const CloudArgs &a, unsigned long long *lbins, float x,
                                            float y, float z) {
  const double two_pi = 2.0 * M_PI;
  const float xx = x * x, yy = y * y;
  const float range_sq = xx + yy;                       // :153
  if (static_cast<double>(range_sq) < 1e-6) return;
  if (static_cast<double>(z) < a.min_z || (a.max_z >= 0.0 && static_cast<double>(z) > a.max_z))
    return;                                             // :159
  if (!isfinite(x) || !isfinite(y)) return;             // reference: int(NaN) index
  // Two tiers: a float atan2 decides the bin of a point more than 3e-6 rad
  // (six times the largest float-vs-float atan2 discrepancy at pi) away from
  // an edge; closer ones are redone in double against the 1e-6 rad margin.
  double ang = static_cast<double>(atan2f(y, x));
  if (ang < 0.0) ang += two_pi;
  double t = a.angle_step > 0.0 ? ang / a.angle_step : (ang / two_pi) * a.num_bins;
  double fl = floor(t);
  double frac = t - fl;
  if (frac < 3.0 * a.edge || frac > 1.0 - 3.0 * a.edge) {
    ang = atan2(static_cast<double>(y), static_cast<double>(x));
    if (ang < 0.0) ang += two_pi;
    t = a.angle_step > 0.0 ? ang / a.angle_step : (ang / two_pi) * a.num_bins;
    fl = floor(t);
    frac = t - fl;
    if (frac < a.edge || frac > 1.0 - a.edge) {
      // too close to a bin edge to trust a different atan2: the host decides
      a.list[atomicAdd(a.list_count, 1u)] = make_float2(x, y);
      return;
    }
  }
  int bin = static_cast<int>(fl);
  bin = min(bin, a.num_bins - 1);
  const float distf = kc::sqrt_rn(range_sq);  // std::sqrt(float)
  if (!(distf >= 0.0f)) return;
  if (kLds) {
    // the minimum of the widened floats is the widened minimum: the workgroup keeps FLOAT bits (non-negative
    // floats order like their bit patterns; half the LDS and half the row traffic), the merge widens once
    // and applies max_range
    uint32_t *l32 = reinterpret_cast<uint32_t *>(lbins);
    const uint32_t b32 = __float_as_uint(distf);
    if (b32 < l32[bin]) atomicMin(&l32[bin], b32);
  } else {
    const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(static_cast<double>(distf)));
    atomicMin(&a.bins[bin], bits);
  }
}

constexpr int kCloudBlock = 1024;
constexpr int kCloudMaxLdsBins = 8192;  // 64 KB of LDS bins per workgroup

// kLds: one workgroup per CU strides over the records and keeps its minima in
// LDS (ds_min_u64), then writes them out as one row of `partial` -- no global
// atomics; cloud_merge_kernel takes the column minima.  Otherwise (more bins
// than LDS holds) every point goes to a global atomic min.
template <bool kLds>
__global__ __launch_bounds__(kCloudBlock) void cloud_bins_kernel(CloudArgs a) {
  extern __shared__ unsigned long long lbins[];
  if (kLds) {
    uint32_t *l32 = reinterpret_cast<uint32_t *>(lbins);
    for (int b = threadIdx.x; b < a.num_bins; b += kCloudBlock) l32[b] = 0x7F800000u;  // +inf: no point yet
    __syncthreads();
  }
  const long long stride = static_cast<long long>(gridDim.x) * kCloudBlock;
  const long long first = static_cast<long long>(blockIdx.x) * kCloudBlock + threadIdx.x;
  if (a.packed16) {
    // x, y, z are the first 12 bytes of aligned 16-byte records: one 128-bit
    // load per point, four points in flight per lane
    const float4 *rec = reinterpret_cast<const float4 *>(a.data);
    const long long n = a.n_packed;  // records that lie completely inside the buffer
    for (long long i = first; i < n; i += 4 * stride) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long j = i + u * stride;
        v[u] = rec[j < n ? j : i];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i + u * stride < n) cloud_point<kLds>(a, lbins, v[u].x, v[u].y, v[u].z);
    }
  } else {
    for (long long i = first; i < a.n_records; i += stride) {
      const long long row = i / a.per_row;
      const long long col = (i - row * a.per_row) * a.point_step;
      const size_t start = static_cast<size_t>(row) * a.row_step + static_cast<size_t>(col);
      if (start + static_cast<size_t>(a.max_off) + static_cast<size_t>(a.fsize) > a.nbytes) continue;  // :139-146
      if (a.ftype == KC_FIELD_FLOAT32)
        cloud_point<kLds>(a, lbins, load_f32(a.data + start + a.x_off), load_f32(a.data + start + a.y_off),
                          load_f32(a.data + start + a.z_off));
      else
        cloud_point<kLds>(a, lbins, load_field(a.data + start + a.x_off, a.ftype),
                          load_field(a.data + start + a.y_off, a.ftype), load_field(a.data + start + a.z_off, a.ftype));
    }
  }
  if (kLds) {
    __syncthreads();
    uint32_t *rowp = reinterpret_cast<uint32_t *>(a.partial) + static_cast<size_t>(blockIdx.x) * a.num_bins;
    const uint32_t *l32 = reinterpret_cast<const uint32_t *>(lbins);
    for (int b = threadIdx.x; b < a.num_bins; b += kCloudBlock) rowp[b] = l32[b];
  }
}

// column minima of the per-workgroup rows
// ... and hands the result to the host: bins, edge-list count and (last
// workgroup) the sequence number go straight into pinned host memory, which
// the host polls instead of copying and waiting on the stream
constexpr int kMergeBins = 16;  // bins per workgroup of the merge: 64 row lanes each
__global__ __launch_bounds__(1024) void cloud_merge_kernel(const uint32_t *partial, int rows, int num_bins,
                                                           double max_range, unsigned long long *bins,
                                                           const unsigned int *count_now,
                                                           unsigned int *next_count, unsigned int *ticket,
                                                           unsigned long long *host_out, long long seq) {
  // 16 bins per workgroup (a 64-byte segment of every row), 64 lanes per bin over the rows -- every load of a
  // lane in flight at once (512 rows: eight) --, the minimum over the lanes of a bin by two DPP-free shuffles
  // inside the wavefront (4 row lanes x 16 bins) and an LDS pass over the 16 wavefronts
  __shared__ uint32_t part[16][kMergeBins];
  const int bl = threadIdx.x & (kMergeBins - 1), rg = threadIdx.x >> 4;  // rg: 0 .. 63
  const int b = blockIdx.x * kMergeBins + bl;
  uint32_t m = 0x7F800000u;
  if (b < num_bins) {
#pragma unroll 8
    for (int r = rg; r < rows; r += 64) {
      const uint32_t v = partial[static_cast<size_t>(r) * num_bins + b];
      m = v < m ? v : m;
    }
  }
  {
    const uint32_t o = static_cast<uint32_t>(__shfl_xor(static_cast<int>(m), 16, 64));
    m = o < m ? o : m;
    const uint32_t o2 = static_cast<uint32_t>(__shfl_xor(static_cast<int>(m), 32, 64));
    m = o2 < m ? o2 : m;
  }
  if ((threadIdx.x & 63) < kMergeBins) part[threadIdx.x >> 6][bl] = m;
  __syncthreads();
  if (threadIdx.x < kMergeBins && b < num_bins) {
#pragma unroll
    for (int k = 1; k < 16; ++k) m = part[k][bl] < m ? part[k][bl] : m;
    // widen once; `distance < ranges[bin]` against the initial max_range (pointcloud.h:170-175)
    const double d = static_cast<double>(__uint_as_float(m));
    const double out = d < max_range ? d : max_range;
    const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(out));
    bins[b] = bits;
    host_out[2 + b] = bits;
    __threadfence_system();
  }
  __syncthreads();
  if (threadIdx.x == 0 && atomicAdd(ticket, 1u) == gridDim.x - 1) {
    *ticket = 0u;
    host_out[1] = *count_now;
    *next_count = 0u;  // the edge-list counter of the NEXT call (the two alternate)
    __threadfence_system();
    *reinterpret_cast<volatile unsigned long long *>(host_out) = static_cast<unsigned long long>(seq);
  }
}

__global__ void cloud_arm_kernel(unsigned long long *bins, int n, double max_range,
                                 unsigned int *counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (bins && i < n) bins[i] = static_cast<unsigned long long>(__double_as_longlong(max_range));
  if (i == 0) counts[0] = counts[1] = 0u;  // both edge-list counters
}

// ---- points -> occupancy grid (readPCDToOccupancyGrid, utils/pointcloud.h:468-540) ----------------------
// Two streaming passes over the cloud.  Pass 1 (:486-497): bounding box of x / y, exact and order-free (min /
// max).  Pass 2 (:511-536): the class of a point (occupied / ground / overhead) is a bit, the cell's byte of
// a 32-bit word collects the bits with atomicOr, a decode pass turns the bits into the reference's -1 / 0 /
// 100 -- the maximum over the cell's points whatever order they arrive in.  Points with a non-finite x or y
// take part in neither pass.
struct GridCloud {
  const uint8_t *data;
  long long n;         // points
  int step, x_off, y_off, z_off;
  int packed12;        // 12-byte x y z records on a 16-byte aligned base: four points = three 16-byte loads
};

struct GridPoint4 {
  float x[4], y[4], z[4];
};

// points 4 g .. 4 g + 3 of a packed cloud
__device__ __forceinline__ GridPoint4 grid_load4(const GridCloud &c, long long g) {
  const float4 *q = reinterpret_cast<const float4 *>(c.data) + 3 * g;
  const float4 a = q[0], b = q[1], d = q[2];
  GridPoint4 p;
  p.x[0] = a.x; p.y[0] = a.y; p.z[0] = a.z;
  p.x[1] = a.w; p.y[1] = b.x; p.z[1] = b.y;
  p.x[2] = b.z; p.y[2] = b.w; p.z[2] = d.x;
  p.x[3] = d.y; p.y[3] = d.z; p.z[3] = d.w;
  return p;
}

__device__ __forceinline__ void grid_load1(const GridCloud &c, long long i, float &x, float &y, float &z) {
  const uint8_t *r = c.data + static_cast<size_t>(i) * static_cast<size_t>(c.step);
  x = load_f32(r + c.x_off);
  y = load_f32(r + c.y_off);
  z = load_f32(r + c.z_off);
}

constexpr int kGridBlock = 256;
constexpr int kGridMaxBlocks = 2048;  // 8 workgroups of 4 wavefronts for each of the 256 CUs

struct Extent {
  float min_x, min_y, max_x, max_y;
};

__device__ __forceinline__ void extent_add(Extent &e, float x, float y) {
  if (!isfinite(x) || !isfinite(y)) return;
  e.min_x = x < e.min_x ? x : e.min_x;
  e.min_y = y < e.min_y ? y : e.min_y;
  e.max_x = x > e.max_x ? x : e.max_x;
  e.max_y = y > e.max_y ? y : e.max_y;
}

__device__ __forceinline__ void extent_merge(Extent &e, const Extent &o) {
  e.min_x = o.min_x < e.min_x ? o.min_x : e.min_x;
  e.min_y = o.min_y < e.min_y ? o.min_y : e.min_y;
  e.max_x = o.max_x > e.max_x ? o.max_x : e.max_x;
  e.max_y = o.max_y > e.max_y ? o.max_y : e.max_y;
}

// the workgroup's extent in lane 0 of wavefront 0 (blockDim.x <= 1024)
__device__ __forceinline__ Extent extent_block_reduce(Extent e) {
  __shared__ Extent part[16];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    Extent o;
    o.min_x = __shfl_xor(e.min_x, d, 64);
    o.min_y = __shfl_xor(e.min_y, d, 64);
    o.max_x = __shfl_xor(e.max_x, d, 64);
    o.max_y = __shfl_xor(e.max_y, d, 64);
    extent_merge(e, o);
  }
  const int wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
  if ((threadIdx.x & 63) == 0) part[wave] = e;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < waves; ++w) extent_merge(e, part[w]);
  return e;
}

// pass 1: one partial row a workgroup
__global__ __launch_bounds__(kGridBlock) void cloud_extent_kernel(GridCloud c, Extent *partial) {
  Extent e{FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX};  // :487-490
  const long long stride = static_cast<long long>(gridDim.x) * kGridBlock;
  const long long first = static_cast<long long>(blockIdx.x) * kGridBlock + threadIdx.x;
  long long done = 0;
  if (c.packed12) {
    const long long groups = c.n >> 2;
    for (long long g = first; g < groups; g += stride) {
      const GridPoint4 p = grid_load4(c, g);
#pragma unroll
      for (int u = 0; u < 4; ++u) extent_add(e, p.x[u], p.y[u]);
    }
    done = groups << 2;
  }
  for (long long i = done + first; i < c.n; i += stride) {
    float x, y, z;
    grid_load1(c, i, x, y, z);
    extent_add(e, x, y);
  }
  e = extent_block_reduce(e);
  if (threadIdx.x == 0) partial[blockIdx.x] = e;
}

// ... reduced by one workgroup, straight into pinned host memory
__global__ __launch_bounds__(kGridBlock) void cloud_extent_merge_kernel(const Extent *partial, int rows, Extent *host_out) {
  Extent e{FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int r = threadIdx.x; r < rows; r += kGridBlock) extent_merge(e, partial[r]);
  e = extent_block_reduce(e);
  if (threadIdx.x == 0) {
    *host_out = e;
    __threadfence_system();
  }
}

struct GridFill {
  float min_x, min_y, inv_res, z_ground, z_robot;
  int cells_x, cells_y;
  uint32_t *words;  // the grid's bytes, four cells a word: bit 0 = a ground point, bit 1 = an occupied point
};

__device__ __forceinline__ void grid_point(const GridFill &f, float x, float y, float z) {
  if (!isfinite(x) || !isfinite(y)) return;
  uint32_t bit;
  if (z > f.z_ground && z <= f.z_robot) bit = 2u;  // :523 OCCUPIED
  else if (z <= f.z_ground) bit = 1u;              // :526 EMPTY
  else return;                                     // :529 UNEXPLORED (a NaN z too): the cell's initial value
  const float dx = x - f.min_x, dy = y - f.min_y;
  const float fx = dx * f.inv_res, fy = dy * f.inv_res;  // :517-518
  // an int the float does not fit (or NaN from 0 * inf) is outside every grid
  if (!(fx < 2147483648.0f) || !(fy < 2147483648.0f)) return;
  const int cx = static_cast<int>(fx), cy = static_cast<int>(fy);
  if (cx < 0 || cx >= f.cells_x || cy < 0 || cy >= f.cells_y) return;  // :520
  const uint32_t cell = static_cast<uint32_t>(cx) + static_cast<uint32_t>(cy) * static_cast<uint32_t>(f.cells_x);
  const uint32_t sh = (cell & 3u) * 8u;
  uint32_t *w = f.words + (cell >> 2);
  // a plain load first: when the cell already holds this class (or, for a ground point, the occupied one that
  // outranks it) the atomic adds nothing.  Whatever the load returns, skipping is only done on bits that are
  // set, and bits are never cleared during the pass.
  // -DKC_GRID_NO_PRELOAD builds the variant without the load, for the A/B of tools/pcd_grid_time.py.
#ifndef KC_GRID_NO_PRELOAD
  const uint32_t cur = (*reinterpret_cast<volatile uint32_t *>(w) >> sh) & 3u;
  if (cur >= bit) return;
#endif
  atomicOr(w, bit << sh);
}

// pass 2
__global__ __launch_bounds__(kGridBlock) void cloud_grid_scatter_kernel(GridCloud c, GridFill f) {
  const long long stride = static_cast<long long>(gridDim.x) * kGridBlock;
  const long long first = static_cast<long long>(blockIdx.x) * kGridBlock + threadIdx.x;
  long long done = 0;
  if (c.packed12) {
    const long long groups = c.n >> 2;
    for (long long g = first; g < groups; g += stride) {
      const GridPoint4 p = grid_load4(c, g);
#pragma unroll
      for (int u = 0; u < 4; ++u) grid_point(f, p.x[u], p.y[u], p.z[u]);
    }
    done = groups << 2;
  }
  for (long long i = done + first; i < c.n; i += stride) {
    float x, y, z;
    grid_load1(c, i, x, y, z);
    grid_point(f, x, y, z);
  }
}

// class bits -> OccupancyType bytes, four cells a word: 0 -> -1, 1 -> 0, 2 | 3 -> 100
__device__ __forceinline__ uint32_t grid_decode_word(uint32_t w) {
  const uint32_t occ = (w >> 1) & 0x01010101u, gnd = w & 0x01010101u;
  const uint32_t none = (occ | gnd) ^ 0x01010101u;
  return occ * 100u | none * 0xFFu;
}

__global__ __launch_bounds__(kGridBlock) void cloud_grid_decode_kernel(uint4 *words16, long long n16) {
  const long long stride = static_cast<long long>(gridDim.x) * kGridBlock;
  for (long long i = static_cast<long long>(blockIdx.x) * kGridBlock + threadIdx.x; i < n16; i += stride) {
    uint4 v = words16[i];
    v.x = grid_decode_word(v.x);
    v.y = grid_decode_word(v.y);
    v.z = grid_decode_word(v.z);
    v.w = grid_decode_word(v.w);
    words16[i] = v;
  }
}

}  // namespace kc

using namespace kc;

struct kc_cloud {
  int device = 0;
  hipStream_t stream = nullptr;
  Timing timing;
  DevBuf<uint8_t> d_data;
  DevBuf<unsigned long long> d_bins;
  DevBuf<unsigned long long> d_partial;
  DevBuf<unsigned int> d_count;   // [2]: edge-list counters, alternating between calls; [2]: ticket
  unsigned calls = 0;
  PinBuf<unsigned long long> h_out;  // [0] sequence, [1] edge count, [2..] bins (written by the merge kernel)
  long long seq = 0;
  DevBuf<float2> d_list;         // (x, y) of the edge points
  PinBuf<unsigned long long> h_bins;
  PinBuf<unsigned int> h_count;
  PinBuf<float2> h_list;
  bool lds_ok = false;
  size_t last_rebinned = 0;
  // points -> occupancy grid: the cloud of the last kc_cloud_grid_extent and its grid
  GridCloud g_cloud{};
  int g_state = 0;               // 0: no extent yet, 1: extent taken, 2: grid filled
  float g_min_x = 0.f, g_min_y = 0.f, g_res = 0.f;
  int g_cells_x = 0, g_cells_y = 0;
  DevBuf<uint8_t> d_points;      // a host cloud, uploaded once for both passes
  DevBuf<Extent> d_extent;       // [kGridMaxBlocks] partial rows
  PinBuf<Extent> h_extent;
  DevBuf<uint4> d_grid;          // the grid's bytes, padded to 16
};

extern "C" {

int kc_cloud_create(size_t max_bytes, size_t max_bins, int device, kc_cloud **out) {
  if (!out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *out = nullptr;
  hipStream_t stream = nullptr;
  KC_TRY(open_device_stream(device, &stream));
  auto *c = new kc_cloud();
  c->device = device;
  c->stream = stream;
  auto fail = [&](int rc) {
    kc_cloud_destroy(c);
    return rc;
  };
  int rc;
  if ((rc = c->d_data.reserve(std::max<size_t>(max_bytes, 64))) ||
      (rc = c->d_bins.reserve(std::max<size_t>(max_bins, 16))) ||
      (rc = c->h_bins.reserve(std::max<size_t>(max_bins, 16))) ||
      (rc = c->d_count.reserve(3)) || (rc = c->h_count.reserve(1)) ||
      (rc = c->h_out.reserve(std::max<size_t>(max_bins, 16) + 2)))
    return fail(rc);
  c->h_out.p[0] = 0;
  if (hipMemset(c->d_count.p, 0, 3 * sizeof(unsigned int)) != hipSuccess) {
    set_error("counter initialisation failed");
    return fail(KC_ERR_HIP);
  }
  c->lds_ok = hipFuncSetAttribute(reinterpret_cast<const void *>(cloud_bins_kernel<true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  kCloudMaxLdsBins * 8) == hipSuccess;
  if (!c->lds_ok) (void)hipGetLastError();
  *out = c;
  return KC_OK;
}

void kc_cloud_destroy(kc_cloud *c) {
  if (!c) return;
  close_device_stream(c->device, &c->stream);
  delete c;
}

int kc_cloud_to_laserscan(kc_cloud *c, const int8_t *data, size_t nbytes,
                          int data_on_device, int point_step, int row_step,
                          int height, int width, int x_offset, int y_offset,
                          int z_offset, double max_range, double min_z,
                          double max_z, double angle_step, int num_bins,
                          double *ranges_out, double *angles_out, size_t cap,
                          size_t *bins_out) {
  return kc_cloud_to_laserscan_typed(c, data, nbytes, data_on_device, point_step, row_step, height, width, x_offset,
                                     y_offset, z_offset, KC_FIELD_FLOAT32, max_range, min_z, max_z, angle_step, num_bins,
                                     ranges_out, angles_out, cap, bins_out);
}

int kc_cloud_to_laserscan_typed(kc_cloud *c, const int8_t *data, size_t nbytes,
                                int data_on_device, int point_step, int row_step,
                                int height, int width, int x_offset, int y_offset,
                                int z_offset, int field_type, double max_range, double min_z,
                                double max_z, double angle_step, int num_bins,
                                double *ranges_out, double *angles_out, size_t cap,
                                size_t *bins_out) {
  (void)width;  // pointcloud.h:137-138: the loops use row_step / point_step only
  if (!c || !ranges_out || (nbytes && !data)) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (field_type < KC_FIELD_INT8 || field_type > KC_FIELD_FLOAT64)
    KC_FAIL(KC_ERR_INVALID, "Invalid integer for PointFieldType. Must be 1-8.");
  static const int kFieldSize[9] = {0, 1, 1, 2, 2, 4, 4, 4, 8};
  if (point_step <= 0 || row_step < 0 || height < 0 || x_offset < 0 || y_offset < 0 ||
      z_offset < 0)
    KC_FAIL(KC_ERR_INVALID, "point_step must be positive, sizes and offsets non-negative");
  const double two_pi = 2.0 * M_PI;
  const bool by_step = angle_step > 0.0;
  if (by_step) num_bins = static_cast<int>(std::ceil(two_pi / angle_step));  // :124
  if (num_bins <= 0) KC_FAIL(KC_ERR_INVALID, "no angular bins");
  if (static_cast<size_t>(num_bins) > cap)
    KC_FAIL(KC_ERR_RANGE, "%d bins do not fit the output capacity %zu", num_bins, cap);
  if (bins_out) *bins_out = static_cast<size_t>(num_bins);
  for (int i = 0; i < num_bins; ++i) {
    if (by_step && angles_out) angles_out[i] = i * angle_step;  // :127-132
    ranges_out[i] = max_range;
  }
  c->last_rebinned = 0;
  const long long per_row = (static_cast<long long>(row_step) + point_step - 1) / point_step;
  const long long n_rec = per_row * height;
  // nothing can be closer than a negative / NaN max_range: the reference leaves
  // every bin at max_range.  -0.0 belongs here too (`distance < -0.0` never holds): its bit pattern is above every
  // distance's, so bins armed with it on the global-atomic path would take any point
  if (n_rec == 0 || nbytes == 0 || !(max_range >= 0.0) || std::signbit(max_range)) return KC_OK;
  if (n_rec > 0x7FFFFFFFll) KC_FAIL(KC_ERR_RANGE, "more than 2^31 point records");
  KC_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  c->timing.begin_cycle();
  const uint8_t *dev = reinterpret_cast<const uint8_t *>(data);
  if (!data_on_device) {
    KC_TRY(c->d_data.reserve(nbytes));
    KC_HIP(hipMemcpyAsync(c->d_data.p, data, nbytes, hipMemcpyHostToDevice, s));
    dev = c->d_data.p;
  }
  KC_TRY(c->d_bins.reserve(num_bins));
  KC_TRY(c->h_bins.reserve(num_bins));
  KC_TRY(c->d_list.reserve(static_cast<size_t>(n_rec)));
  const bool in_lds = c->lds_ok && num_bins <= kCloudMaxLdsBins;
  const unsigned grid = static_cast<unsigned>(
      std::min<long long>(256, (n_rec + kCloudBlock - 1) / kCloudBlock));
  if (in_lds) KC_TRY(c->d_partial.reserve(static_cast<size_t>(grid) * num_bins));
  double max_r = max_range;
  CloudArgs a{};
  a.data = dev;
  a.nbytes = nbytes;
  a.n_records = n_rec;
  a.per_row = static_cast<int>(per_row);
  a.point_step = point_step;
  a.row_step = row_step;
  a.x_off = x_offset;
  a.y_off = y_offset;
  a.z_off = z_offset;
  a.max_off = std::max(std::max(x_offset, y_offset), z_offset);
  a.min_z = min_z;
  a.max_z = max_z;
  a.angle_step = by_step ? angle_step : 0.0;
  a.num_bins = num_bins;
  a.edge = 1e-6 / (by_step ? angle_step : two_pi / num_bins);
  std::memcpy(&a.max_bits, &max_r, sizeof(double));
  a.ftype = field_type;
  a.fsize = kFieldSize[field_type];
  a.packed16 = field_type == KC_FIELD_FLOAT32 && point_step == 16 && x_offset == 0 && y_offset == 4 && z_offset == 8 &&
               row_step % 16 == 0 && (reinterpret_cast<uintptr_t>(dev) & 15u) == 0;
  a.n_packed = std::min<long long>(n_rec, static_cast<long long>(nbytes / 16));
  a.bins = c->d_bins.p;
  a.partial = c->d_partial.p;
  unsigned int *const count_now = c->d_count.p + (c->calls & 1u);
  unsigned int *const count_next = c->d_count.p + ((c->calls + 1u) & 1u);
  ++c->calls;
  a.list_count = count_now;
  // the edge list goes straight to pinned host memory (a few hundred 8-byte
  // PCIe writes) when the polled hand-off is used
  if (in_lds) KC_TRY(c->h_list.reserve(static_cast<size_t>(n_rec)));
  a.list = in_lds ? c->h_list.p : c->d_list.p;
  if (!in_lds)  // global-atomic path: the bins start at max_range (and both counters at 0)
    hipLaunchKernelGGL(cloud_arm_kernel, dim3((num_bins + 255) / 256), dim3(256), 0, s,
                       c->d_bins.p, num_bins, max_range, c->d_count.p);
  KC_TRY(c->timing.start("cloud_bins_kernel", s));
  if (in_lds)
    hipLaunchKernelGGL(cloud_bins_kernel<true>, dim3(grid), dim3(kCloudBlock),
                       static_cast<size_t>(num_bins) * 4, s, a);
  else
    hipLaunchKernelGGL(cloud_bins_kernel<false>, dim3(grid), dim3(kCloudBlock), 0, s, a);
  KC_TRY(c->timing.stop(s));
  size_t nl = 0;
  if (in_lds) {
    KC_TRY(c->h_out.reserve(static_cast<size_t>(num_bins) + 2));
    const long long seq = ++c->seq;
    KC_TRY(c->timing.start("cloud_merge_kernel", s));
    hipLaunchKernelGGL(cloud_merge_kernel, dim3((num_bins + kMergeBins - 1) / kMergeBins), dim3(1024), 0, s,
                       reinterpret_cast<const uint32_t *>(c->d_partial.p), static_cast<int>(grid), num_bins, max_range,
                       c->d_bins.p, count_now, count_next, c->d_count.p + 2, c->h_out.p, seq);
    KC_TRY(c->timing.stop(s));
    KC_HIP(hipGetLastError());
    // poll the sequence word (bounded: then wait on the stream)
    volatile unsigned long long *hp = c->h_out.p;
    const auto t0 = std::chrono::steady_clock::now();
    for (long spins = 0; hp[0] != static_cast<unsigned long long>(seq); ++spins) {
      if ((spins & 1023) == 1023 &&
          std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
        KC_HIP(hipStreamSynchronize(s));
        break;
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    for (int i = 0; i < num_bins; ++i) std::memcpy(&ranges_out[i], &c->h_out.p[2 + i], sizeof(double));
    nl = static_cast<size_t>(c->h_out.p[1]);
  } else {
    KC_HIP(hipGetLastError());
    KC_HIP(hipMemcpyAsync(c->h_bins.p, c->d_bins.p, num_bins * sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, s));
    KC_HIP(hipMemcpyAsync(c->h_count.p, count_now, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    KC_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < num_bins; ++i) std::memcpy(&ranges_out[i], &c->h_bins.p[i], sizeof(double));
    nl = c->h_count.p[0];
    if (nl) {
      KC_TRY(c->h_list.reserve(nl));
      KC_HIP(hipMemcpyAsync(c->h_list.p, c->d_list.p, nl * sizeof(float2), hipMemcpyDeviceToHost, s));
      KC_HIP(hipStreamSynchronize(s));
    }
  }
  c->last_rebinned = nl;
  // the edge cases: the reference expression on the host (pointcloud.h:148-175)
  for (size_t k = 0; k < nl; ++k) {
    const float x = c->h_list.p[k].x, y = c->h_list.p[k].y;
    const float xx = x * x, yy = y * y;
    const float range_sq = xx + yy;
    double angle = static_cast<double>(::atan2f(y, x));  // std::atan2(float, float)
    if (angle < 0.0) angle += two_pi;
    int bin = by_step ? static_cast<int>(angle / angle_step)
                      : static_cast<int>((angle / two_pi) * num_bins);
    bin = std::min(bin, num_bins - 1);
    const double distance = static_cast<double>(::sqrtf(range_sq));
    if (distance < ranges_out[bin]) ranges_out[bin] = distance;
  }
  return KC_OK;
}

int kc_cloud_last_rebinned(kc_cloud *c, size_t *count) {
  if (!c || !count) KC_FAIL(KC_ERR_INVALID, "null argument");
  *count = c->last_rebinned;
  return KC_OK;
}

int kc_cloud_timing_enable(kc_cloud *c, int enable) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  c->timing.enabled = enable != 0;
  return KC_OK;
}

int kc_cloud_timing_get(kc_cloud *c, const char **names, float *ms, size_t cap,
                        size_t *count) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  KC_HIP(hipSetDevice(c->device));
  return c->timing.get(names, ms, cap, count);
}

}  // extern "C"

namespace {

unsigned grid_blocks(long long work) {
  return static_cast<unsigned>(std::max<long long>(1, std::min<long long>(kGridMaxBlocks, (work + kGridBlock - 1) / kGridBlock)));
}

}  // namespace

extern "C" {

int kc_cloud_grid_extent(kc_cloud *c, const int8_t *data, size_t nbytes, int data_on_device, int point_step,
                         size_t n_points, int x_offset, int y_offset, int z_offset, float grid_resolution,
                         float origin_out[3], int *cells_x, int *cells_y) {
  if (!c || !origin_out || !cells_x || !cells_y || (n_points && !data)) KC_FAIL(KC_ERR_INVALID, "null argument");
  c->g_state = 0;
  origin_out[0] = origin_out[1] = origin_out[2] = 0.0f;
  *cells_x = *cells_y = 0;
  if (!(grid_resolution > 0.0f) || !std::isfinite(grid_resolution))
    KC_FAIL(KC_ERR_RANGE, "grid_resolution must be a positive finite float, got %g", static_cast<double>(grid_resolution));
  if (point_step <= 0 || x_offset < 0 || y_offset < 0 || z_offset < 0)
    KC_FAIL(KC_ERR_INVALID, "point_step must be positive, offsets non-negative");
  const int max_off = std::max(std::max(x_offset, y_offset), z_offset);
  if (max_off > point_step - 4) KC_FAIL(KC_ERR_INVALID, "x / y / z do not fit a %d-byte record", point_step);
  if (n_points > static_cast<size_t>(0x7FFFFFFF)) KC_FAIL(KC_ERR_RANGE, "more than 2^31 points");
  // every field read lies inside the buffer: the last record may end after its z
  if (n_points && (nbytes < static_cast<size_t>(max_off) + 4 ||
                   (n_points - 1) > (nbytes - static_cast<size_t>(max_off) - 4) / static_cast<size_t>(point_step)))
    KC_FAIL(KC_ERR_INVALID, "%zu records of %d bytes do not fit %zu bytes", n_points, point_step, nbytes);
  GridCloud g{};
  g.n = static_cast<long long>(n_points);
  g.step = point_step;
  g.x_off = x_offset;
  g.y_off = y_offset;
  g.z_off = z_offset;
  c->g_res = grid_resolution;
  c->g_cells_x = c->g_cells_y = 0;
  c->g_min_x = c->g_min_y = 0.0f;
  if (n_points == 0) {  // :482-484
    c->g_cloud = g;
    c->g_state = 1;
    return KC_OK;
  }
  KC_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  c->timing.begin_cycle();
  const uint8_t *dev = reinterpret_cast<const uint8_t *>(data);
  if (data_on_device) {
    // read in place: refused before any read unless all of it is this device's memory
    KC_TRY(check_device_range(c->device, data, 0, static_cast<long long>(nbytes), 1, "cloud"));
  } else {
    KC_TRY(c->d_points.reserve(nbytes));
    KC_HIP(hipMemcpyAsync(c->d_points.p, data, nbytes, hipMemcpyHostToDevice, s));
    dev = c->d_points.p;
    c->timing.mark("host:cloud_grid_upload");
  }
  g.data = dev;
  g.packed12 = point_step == 12 && x_offset == 0 && y_offset == 4 && z_offset == 8 &&
               (reinterpret_cast<uintptr_t>(dev) & 15u) == 0;
  const unsigned blocks = grid_blocks(g.packed12 ? (g.n + 3) / 4 : g.n);
  KC_TRY(c->d_extent.reserve(kGridMaxBlocks));
  KC_TRY(c->h_extent.reserve(1));
  KC_TRY(c->timing.start("cloud_extent_kernel", s));
  hipLaunchKernelGGL(cloud_extent_kernel, dim3(blocks), dim3(kGridBlock), 0, s, g, c->d_extent.p);
  hipLaunchKernelGGL(cloud_extent_merge_kernel, dim3(1), dim3(kGridBlock), 0, s, c->d_extent.p,
                     static_cast<int>(blocks), c->h_extent.p);
  KC_TRY(c->timing.stop(s));
  KC_HIP(hipGetLastError());
  KC_HIP(hipStreamSynchronize(s));
  const Extent e = c->h_extent.p[0];
  c->g_cloud = g;
  c->g_state = 1;
  if (e.min_x > e.max_x) return KC_OK;  // no point with a finite x and y: as the empty cloud
  // :500-503, float throughout; the cap is applied to the floats, before any cast or allocation
  const float fx = std::ceil((e.max_x - e.min_x) / grid_resolution);
  const float fy = std::ceil((e.max_y - e.min_y) / grid_resolution);
  const float cap = static_cast<float>(KC_CLOUD_GRID_MAX_CELLS);
  if (!(fx <= cap) || !(fy <= cap) ||
      static_cast<double>(fx) * static_cast<double>(fy) > static_cast<double>(KC_CLOUD_GRID_MAX_CELLS)) {
    c->g_state = 0;
    KC_FAIL(KC_ERR_RANGE, "a %g x %g cell grid is above the cap of %zu cells", static_cast<double>(fx),
            static_cast<double>(fy), static_cast<size_t>(KC_CLOUD_GRID_MAX_CELLS));
  }
  c->g_min_x = e.min_x;
  c->g_min_y = e.min_y;
  c->g_cells_x = static_cast<int>(fx);
  c->g_cells_y = static_cast<int>(fy);
  origin_out[0] = e.min_x;
  origin_out[1] = e.min_y;
  *cells_x = c->g_cells_x;
  *cells_y = c->g_cells_y;
  return KC_OK;
}

static int cloud_grid_run(kc_cloud *c, float z_ground_limit, float robot_height) {
  if (c->g_state < 1) KC_FAIL(KC_ERR_STATE, "kc_cloud_grid_fill before kc_cloud_grid_extent");
  const size_t cells = static_cast<size_t>(c->g_cells_x) * static_cast<size_t>(c->g_cells_y);
  c->g_state = 2;
  if (cells == 0) return KC_OK;
  KC_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const size_t n16 = (cells + 15) / 16;
  KC_TRY(c->d_grid.reserve(n16));
  KC_TRY(c->timing.start("cloud_grid_clear", s));
  KC_HIP(hipMemsetAsync(c->d_grid.p, 0, n16 * 16, s));
  KC_TRY(c->timing.stop(s));
  GridFill f{};
  f.min_x = c->g_min_x;
  f.min_y = c->g_min_y;
  f.inv_res = 1.0f / c->g_res;  // :506
  f.z_ground = z_ground_limit;
  f.z_robot = robot_height;
  f.cells_x = c->g_cells_x;
  f.cells_y = c->g_cells_y;
  f.words = reinterpret_cast<uint32_t *>(c->d_grid.p);
  const GridCloud &g = c->g_cloud;
  KC_TRY(c->timing.start("cloud_grid_scatter_kernel", s));
  hipLaunchKernelGGL(cloud_grid_scatter_kernel, dim3(grid_blocks(g.packed12 ? (g.n + 3) / 4 : g.n)), dim3(kGridBlock), 0,
                     s, g, f);
  KC_TRY(c->timing.stop(s));
  KC_TRY(c->timing.start("cloud_grid_decode_kernel", s));
  hipLaunchKernelGGL(cloud_grid_decode_kernel, dim3(grid_blocks(static_cast<long long>(n16))), dim3(kGridBlock), 0, s,
                     c->d_grid.p, static_cast<long long>(n16));
  KC_TRY(c->timing.stop(s));
  KC_HIP(hipGetLastError());
  return KC_OK;
}

int kc_cloud_grid_fill(kc_cloud *c, float z_ground_limit, float robot_height, int8_t *grid_out, size_t cap) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (c->g_state < 1) KC_FAIL(KC_ERR_STATE, "kc_cloud_grid_fill before kc_cloud_grid_extent");
  const size_t cells = static_cast<size_t>(c->g_cells_x) * static_cast<size_t>(c->g_cells_y);
  if (cells > cap) KC_FAIL(KC_ERR_RANGE, "%zu cells do not fit the output capacity %zu", cells, cap);
  if (cells && !grid_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  KC_TRY(cloud_grid_run(c, z_ground_limit, robot_height));
  if (cells == 0) return KC_OK;
  KC_HIP(hipMemcpyAsync(grid_out, c->d_grid.p, cells, hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  return KC_OK;
}

int kc_cloud_grid_device(kc_cloud *c, float z_ground_limit, float robot_height, void **dev_grid_int8) {
  if (!c || !dev_grid_int8) KC_FAIL(KC_ERR_INVALID, "null argument");
  *dev_grid_int8 = nullptr;
  KC_TRY(cloud_grid_run(c, z_ground_limit, robot_height));
  if (static_cast<size_t>(c->g_cells_x) * static_cast<size_t>(c->g_cells_y) == 0) return KC_OK;
  KC_HIP(hipStreamSynchronize(c->stream));
  *dev_grid_int8 = c->d_grid.p;
  return KC_OK;
}

int kc_cloud_after_stream(kc_cloud *c, void *stream) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  return stream_wait_for(c->device, c->stream, stream);
}

}  // extern "C"
