// World map on gfx950: a world-frame occupancy map that stays on the device, fused from the LocalMapper's
// egocentric grids.  Integer work only; the one place a float is read is the pose quantisation
// on the host, once per update.
//
// The reference has no counterpart: it leaves this layer to its ROS side.  The yardstick is the numpy statement
// of the rule in tests/worldmap_ref.py, bit for bit.
//
//  (a) state.  Two dense int8 planes of W x H cells, cell (I, J) at I + J * W: `evidence` (-128 = never observed,
//      else e_min .. e_max) and `cls` (KC_UNEXPLORED / KC_EMPTY / KC_OCCUPIED), the plane the planner reads in place.
//  (b) update.  worldmap_update_kernel is a gather over the clipped bounding box of the rotated local window: one
//      lane a world cell, 64 lanes along I (one wavefront is 64 consecutive bytes of a row), four rows a workgroup.
//      A lane maps its cell into the local grid by rules 3 and 4, reads at most one local cell and, for an
//      observation of 0 or 100, stores its own two bytes.  BYTE STORES, on purpose: W need not be a multiple of 4,
//      so the dword that holds a row's last cells can hold the next row's first ones, and a box as wide as the map
//      would have two lanes write one dword.  A lane that stores only its own bytes cannot meet another.
//      The box is a launch bound, not part of the rule: every lane runs the full test of rule 4.
//  (c) result record.  A wavefront counts its class changes by ballot + popcount and adds them with one atomic;
//      lanes that changed their class fold their cell into the box by atomic min / max (the wavefront's extremes,
//      one lane each).  Two records alternate: update n accumulates into record n & 1 and puts record (n + 1) & 1
//      back to its start values, which no lane of this launch reads, so an update is one launch plus the read-back
//      of five words.
//  (d) prior / clear.  worldmap_prior_kernel owns dwords by flat index (the planes start at an allocation, so cells
//      4 t .. 4 t + 3 are one aligned dword, whatever W is); the cells behind the last whole dword go as bytes.
//
// Plain vector loads and stores only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "kc_internal.h"
#include "kompass_hip.h"

namespace kc {

constexpr int kWmLanes = 64;               // cells along I per workgroup: one wavefront a row segment
constexpr int kWmRows = 4;                 // rows per workgroup
constexpr int kWmBlock = 256;
constexpr int kWmMaxBlocks = 2048;
constexpr int8_t kWmNever = -128;
constexpr int kWmMaxSide = 32768;
constexpr long long kWmMaxOffset = 1ll << 36;  // 2^20 cells in 16 fraction bits
constexpr int kWmRecWords = 5;             // changed, i_min, j_min, i_max, j_max

struct WmModel {
  int hit, miss, e_min, e_max, occ_thr;
};

struct WmUpdateArgs {
  const int32_t *local;   // [gh x gw] column-major: (i, j) at i + j * gh
  int8_t *evidence, *cls;
  int *rec, *rec_next;    // this update's record, and the one to put back for the next
  long long tx, ty;
  int cq, sq;
  int W;
  int gh, gw, c0, c1;
  int i_lo, j_lo, i_hi, j_hi;  // the launch box, inclusive, inside the map
  WmModel m;
};

__device__ __forceinline__ int8_t wm_class(int e, int occ_thr) {
  return static_cast<int8_t>(e >= occ_thr ? KC_OCCUPIED : KC_EMPTY);
}

__global__ __launch_bounds__(kWmBlock) void worldmap_update_kernel(WmUpdateArgs a) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) {
    a.rec_next[0] = 0;
    a.rec_next[1] = INT_MAX;
    a.rec_next[2] = INT_MAX;
    a.rec_next[3] = -1;
    a.rec_next[4] = -1;
  }
  const int I = a.i_lo + static_cast<int>(blockIdx.x) * kWmLanes + static_cast<int>(threadIdx.x);
  const int J = a.j_lo + static_cast<int>(blockIdx.y) * kWmRows + static_cast<int>(threadIdx.y);
  bool changed = false;
  if (I <= a.i_hi && J <= a.j_hi) {
    const long long dx = (static_cast<long long>(I) << 16) - a.tx;
    const long long dy = (static_cast<long long>(J) << 16) - a.ty;
    const long long cq = a.cq, sq = a.sq;
    const long long li = a.c0 + ((cq * dx + sq * dy + (1ll << 31)) >> 32);
    const long long lj = a.c1 + ((cq * dy - sq * dx + (1ll << 31)) >> 32);
    if (li >= 0 && li < a.gh && lj >= 0 && lj < a.gw) {
      const int obs = a.local[li + lj * a.gh];
      if (obs == KC_OCCUPIED || obs == KC_EMPTY) {
        const size_t cell = static_cast<size_t>(I) + static_cast<size_t>(J) * static_cast<size_t>(a.W);
        const int old = a.evidence[cell];
        const int base = old == kWmNever ? 0 : old;
        const int e = obs == KC_OCCUPIED ? min(base + a.m.hit, a.m.e_max) : max(base - a.m.miss, a.m.e_min);
        const int8_t k = wm_class(e, a.m.occ_thr);
        changed = a.cls[cell] != k;
        if (e != old) a.evidence[cell] = static_cast<int8_t>(e);
        if (changed) a.cls[cell] = k;
      }
    }
  }
  // one wavefront is one row segment (blockDim.x == 64): J is uniform in it
  const unsigned long long mask = __ballot(changed);
  if (mask == 0) return;
  const int lane = static_cast<int>(threadIdx.x);
  const int first = __ffsll(mask) - 1, last = 63 - __clzll(mask);
  if (lane == first) {
    atomicAdd(reinterpret_cast<unsigned int *>(&a.rec[0]), static_cast<unsigned int>(__popcll(mask)));
    atomicMin(&a.rec[1], I);
    atomicMin(&a.rec[2], J);
    atomicMax(&a.rec[4], J);
  }
  if (lane == last) atomicMax(&a.rec[3], I);
}

// grid == nullptr: clear.  Otherwise rule 8: 100 -> e_max, 0 -> e_min, anything else never observed.
template <typename T>
__device__ __forceinline__ void wm_prior_cell(const T *grid, long long k, WmModel m, int *e_out, int *c_out) {
  int e = kWmNever, c = KC_UNEXPLORED;
  if (grid) {
    const int v = static_cast<int>(grid[k]);
    if (v == KC_OCCUPIED) e = m.e_max;
    else if (v == KC_EMPTY) e = m.e_min;
    if (e != kWmNever) c = wm_class(e, m.occ_thr);
  }
  *e_out = e;
  *c_out = c;
}

template <typename T>
__global__ __launch_bounds__(kWmBlock) void worldmap_prior_kernel(const T *grid, int8_t *evidence, int8_t *cls, long long n,
                                                                  WmModel m) {
  const long long quads = n / 4, stride = static_cast<long long>(gridDim.x) * kWmBlock;
  const long long t0 = static_cast<long long>(blockIdx.x) * kWmBlock + threadIdx.x;
  for (long long q = t0; q < quads; q += stride) {
    unsigned int ew = 0, cw = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      int e, c;
      wm_prior_cell(grid, 4 * q + b, m, &e, &c);
      ew |= static_cast<unsigned int>(e & 0xFF) << (8 * b);
      cw |= static_cast<unsigned int>(c & 0xFF) << (8 * b);
    }
    reinterpret_cast<unsigned int *>(evidence)[q] = ew;
    reinterpret_cast<unsigned int *>(cls)[q] = cw;
  }
  const long long k = 4 * quads + t0;  // the up to three cells behind the last whole dword
  if (k < n) {
    int e, c;
    wm_prior_cell(grid, k, m, &e, &c);
    evidence[k] = static_cast<int8_t>(e);
    cls[k] = static_cast<int8_t>(c);
  }
}

}  // namespace kc

using namespace kc;

struct kc_worldmap {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t grid_ready = nullptr;  // the mapper's scan, for update_from_mapper
  int W = 0, H = 0;
  float res = 0.0f;
  double ox = 0.0, oy = 0.0;
  WmModel m = {3, 1, -8, 14, 1};
  DevBuf<int8_t> d_evidence, d_cls;
  DevBuf<int32_t> d_stage;   // a host grid (local, or an int32 prior) on its way to a kernel
  DevBuf<int> d_rec;         // two records of kWmRecWords
  PinBuf<int> h_rec;
  unsigned long long seq = 0;  // updates launched: record seq & 1 is the next one's
  bool rec_ready = false;      // both records hold their start values
};

namespace {

int wm_check_model(int hit, int miss, int e_min, int e_max, int occ_thr) {
  if (hit < 1 || hit > 127 || miss < 1 || miss > 127)
    KC_FAIL(KC_ERR_INVALID, "hit and miss must be in 1 .. 127, got %d and %d", hit, miss);
  if (e_min < -127 || e_min > 0) KC_FAIL(KC_ERR_INVALID, "e_min must be in -127 .. 0, got %d", e_min);
  if (e_max < 0 || e_max > 127) KC_FAIL(KC_ERR_INVALID, "e_max must be in 0 .. 127, got %d", e_max);
  if (!(e_min < occ_thr && occ_thr <= e_max))
    KC_FAIL(KC_ERR_INVALID, "occ_thr must satisfy e_min < occ_thr <= e_max, got %d for %d .. %d", occ_thr, e_min, e_max);
  return KC_OK;
}

int wm_check_shape(int W, int H, float res) {
  if (W <= 0 || H <= 0 || !(res > 0.0f) || !std::isfinite(res))
    KC_FAIL(KC_ERR_INVALID, "the map's width, height and resolution must be positive, got %d x %d at %g", W, H, static_cast<double>(res));
  if (W > kWmMaxSide || H > kWmMaxSide ||
      static_cast<unsigned long long>(W) * static_cast<unsigned long long>(H) > KC_PLANNER_MAX_CELLS)
    KC_FAIL(KC_ERR_RANGE, "a %d x %d map is above the cap of %d cells a side and %u cells", W, H, kWmMaxSide,
            static_cast<unsigned>(KC_PLANNER_MAX_CELLS));
  return KC_OK;
}

int wm_check_grid(float world_res, int gh, int gw, int c0, int c1, float res) {
  if (gh <= 0 || gw <= 0) KC_FAIL(KC_ERR_INVALID, "the local grid's height and width must be positive, got %d x %d", gh, gw);
  if (static_cast<unsigned long long>(gh) * static_cast<unsigned long long>(gw) > 0x3FFFFFFFull)
    KC_FAIL(KC_ERR_RANGE, "a %d x %d local grid is too large", gh, gw);
  if (c0 < -(1 << 30) || c0 > (1 << 30) || c1 < -(1 << 30) || c1 > (1 << 30))
    KC_FAIL(KC_ERR_RANGE, "central cell (%d, %d) not within 2^30 cells", c0, c1);
  if (std::memcmp(&world_res, &res, sizeof(float)) != 0)
    KC_FAIL(KC_ERR_INVALID, "the local grid's resolution %.9g is not the map's %.9g: resampling is out of scope",
            static_cast<double>(res), static_cast<double>(world_res));
  return KC_OK;
}

int wm_check_pose(const kc_worldmap_pose *p) {
  if (!p) KC_FAIL(KC_ERR_INVALID, "null pose");
  if (p->cq < -65536 || p->cq > 65536 || p->sq < -65536 || p->sq > 65536)
    KC_FAIL(KC_ERR_INVALID, "pose (cq, sq) = (%d, %d) is outside -65536 .. 65536", p->cq, p->sq);
  if (p->tx < -kWmMaxOffset || p->tx > kWmMaxOffset || p->ty < -kWmMaxOffset || p->ty > kWmMaxOffset)
    KC_FAIL(KC_ERR_RANGE, "the pose lies more than 2^20 cells from the map's origin");
  return KC_OK;
}

unsigned wm_blocks_for(long long work) {
  return static_cast<unsigned>(std::max<long long>(1, std::min<long long>(kWmMaxBlocks, (work + kWmBlock - 1) / kWmBlock)));
}

int wm_reset_records(kc_worldmap *c) {
  const int init[2 * kWmRecWords] = {0, INT_MAX, INT_MAX, -1, -1, 0, INT_MAX, INT_MAX, -1, -1};
  c->rec_ready = false;
  KC_HIP(hipMemcpyAsync(c->d_rec.p, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));  // `init` is on this frame
  c->rec_ready = true;
  return KC_OK;
}

// dev: the prior on the context's device (nullptr: clear), complete in the order of the context's stream
int wm_take_prior(kc_worldmap *c, const void *dev, int elem_bytes) {
  const long long n = static_cast<long long>(c->W) * c->H;
  const dim3 grid(wm_blocks_for((n + 3) / 4)), block(kWmBlock);
  if (elem_bytes == 4)
    hipLaunchKernelGGL(worldmap_prior_kernel<int32_t>, grid, block, 0, c->stream, static_cast<const int32_t *>(dev),
                       c->d_evidence.p, c->d_cls.p, n, c->m);
  else
    hipLaunchKernelGGL(worldmap_prior_kernel<int8_t>, grid, block, 0, c->stream, static_cast<const int8_t *>(dev),
                       c->d_evidence.p, c->d_cls.p, n, c->m);
  KC_HIP(hipGetLastError());
  KC_HIP(hipStreamSynchronize(c->stream));  // the caller's grid is not read after the call returns
  return KC_OK;
}

int wm_check_prior(const kc_worldmap *c, const void *grid, int elem_bytes, int W, int H) {
  if (!c || !grid) KC_FAIL(KC_ERR_INVALID, "null argument");
  if (elem_bytes != 1 && elem_bytes != 4) KC_FAIL(KC_ERR_INVALID, "prior cells are int8 (1) or int32 (4) bytes, got %d", elem_bytes);
  if (W != c->W || H != c->H) KC_FAIL(KC_ERR_INVALID, "a %d x %d prior does not fit the %d x %d map", W, H, c->W, c->H);
  return KC_OK;
}

// The inclusive box of world cells that rule 4 can map into the local grid, clipped to the map; false when empty.
// The local window is a in [-c0 - 1/2, gh - c0 - 1/2), b likewise; rule 4 rounds M (p - t) with M = [[C, S], [-S, C]],
// C = cq / 2^16, S = sq / 2^16, whose exact inverse is M^T / (C^2 + S^2).  C^2 + S^2 is within 2^-15 of 1, so the
// corners' images under M^T, widened by 2 cells and by 2^-13 of the window's reach, hold every such cell.
bool wm_box(const kc_worldmap *c, const kc_worldmap_pose *p, int gh, int gw, int c0, int c1, int box[4]) {
  const double C = p->cq / 65536.0, S = p->sq / 65536.0;
  const double tx = static_cast<double>(p->tx) / 65536.0, ty = static_cast<double>(p->ty) / 65536.0;
  const double a0 = -static_cast<double>(c0) - 0.5, a1 = static_cast<double>(gh) - c0 - 0.5;
  const double b0 = -static_cast<double>(c1) - 0.5, b1 = static_cast<double>(gw) - c1 - 0.5;
  double x_lo = INFINITY, x_hi = -INFINITY, y_lo = INFINITY, y_hi = -INFINITY;
  for (int k = 0; k < 4; ++k) {
    const double a = k & 1 ? a1 : a0, b = k & 2 ? b1 : b0;
    const double x = C * a - S * b, y = S * a + C * b;
    x_lo = std::min(x_lo, x);
    x_hi = std::max(x_hi, x);
    y_lo = std::min(y_lo, y);
    y_hi = std::max(y_hi, y);
  }
  const double reach = std::max(std::max(std::fabs(a0), std::fabs(a1)), std::max(std::fabs(b0), std::fabs(b1)));
  const double pad = 2.0 + 2.0 * reach / 16384.0;
  const double lo_i = std::floor(tx + x_lo - pad), hi_i = std::ceil(tx + x_hi + pad);
  const double lo_j = std::floor(ty + y_lo - pad), hi_j = std::ceil(ty + y_hi + pad);
  if (hi_i < 0.0 || hi_j < 0.0 || lo_i > c->W - 1.0 || lo_j > c->H - 1.0) return false;
  box[0] = static_cast<int>(std::max(lo_i, 0.0));
  box[1] = static_cast<int>(std::max(lo_j, 0.0));
  box[2] = static_cast<int>(std::min(hi_i, c->W - 1.0));
  box[3] = static_cast<int>(std::min(hi_j, c->H - 1.0));
  return true;
}

// dev: the local grid on the context's device, complete in the order of the context's stream
int wm_update(kc_worldmap *c, const int32_t *dev, int gh, int gw, int c0, int c1, const kc_worldmap_pose *p,
              kc_worldmap_result *out) {
  *out = kc_worldmap_result{0, -1, -1, -1, -1};
  int box[4];
  if (!wm_box(c, p, gh, gw, c0, c1, box)) {
    KC_HIP(hipStreamSynchronize(c->stream));  // nothing to do, but the grid is not read after the call returns
    return KC_OK;
  }
  if (!c->rec_ready) KC_TRY(wm_reset_records(c));
  WmUpdateArgs a{};
  a.local = dev;
  a.evidence = c->d_evidence.p;
  a.cls = c->d_cls.p;
  a.rec = c->d_rec.p + (c->seq & 1) * kWmRecWords;
  a.rec_next = c->d_rec.p + ((c->seq + 1) & 1) * kWmRecWords;
  a.tx = p->tx;
  a.ty = p->ty;
  a.cq = p->cq;
  a.sq = p->sq;
  a.W = c->W;
  a.gh = gh;
  a.gw = gw;
  a.c0 = c0;
  a.c1 = c1;
  a.i_lo = box[0];
  a.j_lo = box[1];
  a.i_hi = box[2];
  a.j_hi = box[3];
  a.m = c->m;
  const dim3 grid((box[2] - box[0]) / kWmLanes + 1, (box[3] - box[1]) / kWmRows + 1), block(kWmLanes, kWmRows);
  c->rec_ready = false;  // until the read-back below says this launch ran: a failure leaves the records unknown
  hipLaunchKernelGGL(worldmap_update_kernel, grid, block, 0, c->stream, a);
  KC_HIP(hipGetLastError());
  KC_HIP(hipMemcpyAsync(c->h_rec.p, a.rec, kWmRecWords * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  ++c->seq;
  c->rec_ready = true;
  const int *r = c->h_rec.p;
  out->changed = static_cast<uint32_t>(r[0]);
  if (r[0] != 0) {
    out->i_min = r[1];
    out->j_min = r[2];
    out->i_max = r[3];
    out->j_max = r[4];
  }
  return KC_OK;
}

}  // namespace

extern "C" {

int kc_worldmap_check_model(int hit, int miss, int e_min, int e_max, int occ_thr) {
  return wm_check_model(hit, miss, e_min, e_max, occ_thr);
}

int kc_worldmap_check_grid(float world_resolution, int grid_height, int grid_width, int central_i, int central_j,
                           float resolution) {
  return wm_check_grid(world_resolution, grid_height, grid_width, central_i, central_j, resolution);
}

int kc_worldmap_quantise_pose(float resolution, double origin_x, double origin_y, double px, double py, double yaw,
                              kc_worldmap_pose *out) {
  if (!out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *out = kc_worldmap_pose{0, 0, 0, 0};
  if (!(resolution > 0.0f) || !std::isfinite(resolution)) KC_FAIL(KC_ERR_INVALID, "the resolution must be positive");
  if (!std::isfinite(origin_x) || !std::isfinite(origin_y) || !std::isfinite(px) || !std::isfinite(py) || !std::isfinite(yaw))
    KC_FAIL(KC_ERR_INVALID, "the pose and the origin must be finite");
  const double R = static_cast<double>(resolution);
  const double fx = (px - origin_x) / R * 65536.0, fy = (py - origin_y) / R * 65536.0;
  const double cap = static_cast<double>(kWmMaxOffset);
  if (!(std::fabs(fx) <= cap + 0.5) || !(std::fabs(fy) <= cap + 0.5))
    KC_FAIL(KC_ERR_RANGE, "the pose lies more than 2^20 cells from the map's origin");
  kc_worldmap_pose p;
  p.cq = static_cast<int32_t>(std::lrint(std::cos(yaw) * 65536.0));
  p.sq = static_cast<int32_t>(std::lrint(std::sin(yaw) * 65536.0));
  p.tx = static_cast<int64_t>(std::llrint(fx));
  p.ty = static_cast<int64_t>(std::llrint(fy));
  KC_TRY(wm_check_pose(&p));
  *out = p;
  return KC_OK;
}

int kc_worldmap_create(int device, int width, int height, float resolution, double origin_x, double origin_y,
                       kc_worldmap **out) {
  if (!out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *out = nullptr;
  KC_TRY(wm_check_shape(width, height, resolution));
  if (!std::isfinite(origin_x) || !std::isfinite(origin_y)) KC_FAIL(KC_ERR_INVALID, "the map's origin must be finite");
  hipStream_t stream = nullptr;
  KC_TRY(open_device_stream(device, &stream));
  auto *c = new kc_worldmap();
  c->device = device;
  c->stream = stream;
  c->W = width;
  c->H = height;
  c->res = resolution;
  c->ox = origin_x;
  c->oy = origin_y;
  const size_t n = static_cast<size_t>(width) * static_cast<size_t>(height);
  int rc;
  if ((rc = c->d_evidence.reserve(n)) || (rc = c->d_cls.reserve(n)) || (rc = c->d_rec.reserve(2 * kWmRecWords)) ||
      (rc = c->h_rec.reserve(kWmRecWords)) || (rc = wm_reset_records(c)) || (rc = wm_take_prior(c, nullptr, 1))) {
    kc_worldmap_destroy(c);
    return rc;
  }
  *out = c;
  return KC_OK;
}

void kc_worldmap_destroy(kc_worldmap *c) {
  if (!c) return;
  close_device_stream(c->device, &c->stream);
  if (c->grid_ready) {
    hipError_t e = hipEventDestroy(c->grid_ready);
    (void)e;
  }
  delete c;
}

int kc_worldmap_info(kc_worldmap *c, int *width_out, int *height_out, float *resolution_out, double *origin_x_out,
                     double *origin_y_out) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (width_out) *width_out = c->W;
  if (height_out) *height_out = c->H;
  if (resolution_out) *resolution_out = c->res;
  if (origin_x_out) *origin_x_out = c->ox;
  if (origin_y_out) *origin_y_out = c->oy;
  return KC_OK;
}

int kc_worldmap_set_model(kc_worldmap *c, int hit, int miss, int e_min, int e_max, int occ_thr) {
  KC_TRY(wm_check_model(hit, miss, e_min, e_max, occ_thr));
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  KC_HIP(hipSetDevice(c->device));
  c->m = WmModel{hit, miss, e_min, e_max, occ_thr};
  return wm_take_prior(c, nullptr, 1);  // evidence counted by another model means nothing under this one
}

int kc_worldmap_clear(kc_worldmap *c) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  KC_HIP(hipSetDevice(c->device));
  return wm_take_prior(c, nullptr, 1);
}

int kc_worldmap_set_prior_host(kc_worldmap *c, const void *grid, int elem_bytes, int width, int height) {
  KC_TRY(wm_check_prior(c, grid, elem_bytes, width, height));
  KC_HIP(hipSetDevice(c->device));
  const size_t nbytes = static_cast<size_t>(width) * static_cast<size_t>(height) * static_cast<size_t>(elem_bytes);
  KC_TRY(c->d_stage.reserve((nbytes + 3) / 4));
  KC_HIP(hipMemcpyAsync(c->d_stage.p, grid, nbytes, hipMemcpyHostToDevice, c->stream));
  return wm_take_prior(c, c->d_stage.p, elem_bytes);
}

int kc_worldmap_set_prior_device(kc_worldmap *c, const void *dev_grid, int elem_bytes, int width, int height) {
  KC_TRY(wm_check_prior(c, dev_grid, elem_bytes, width, height));
  KC_HIP(hipSetDevice(c->device));
  const size_t nbytes = static_cast<size_t>(width) * static_cast<size_t>(height) * static_cast<size_t>(elem_bytes);
  KC_TRY(check_device_range(c->device, dev_grid, 0, static_cast<long long>(nbytes), static_cast<size_t>(elem_bytes), "prior"));
  return wm_take_prior(c, dev_grid, elem_bytes);
}

int kc_worldmap_after_stream(kc_worldmap *c, void *stream) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  return stream_wait_for(c->device, c->stream, stream);
}

int kc_worldmap_update_device(kc_worldmap *c, const int32_t *dev_grid, int grid_height, int grid_width, int central_i,
                              int central_j, float resolution, const kc_worldmap_pose *pose, kc_worldmap_result *out) {
  if (!c || !dev_grid || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  KC_TRY(wm_check_grid(c->res, grid_height, grid_width, central_i, central_j, resolution));
  KC_TRY(wm_check_pose(pose));
  KC_HIP(hipSetDevice(c->device));
  const long long nbytes = static_cast<long long>(grid_height) * grid_width * static_cast<long long>(sizeof(int32_t));
  KC_TRY(check_device_range(c->device, dev_grid, 0, nbytes, sizeof(int32_t), "grid"));
  return wm_update(c, dev_grid, grid_height, grid_width, central_i, central_j, pose, out);
}

int kc_worldmap_update_host(kc_worldmap *c, const int32_t *grid, int grid_height, int grid_width, int central_i,
                            int central_j, float resolution, const kc_worldmap_pose *pose, kc_worldmap_result *out) {
  if (!c || !grid || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  KC_TRY(wm_check_grid(c->res, grid_height, grid_width, central_i, central_j, resolution));
  KC_TRY(wm_check_pose(pose));
  KC_HIP(hipSetDevice(c->device));
  const size_t cells = static_cast<size_t>(grid_height) * static_cast<size_t>(grid_width);
  KC_TRY(c->d_stage.reserve(cells));
  KC_HIP(hipMemcpyAsync(c->d_stage.p, grid, cells * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  return wm_update(c, c->d_stage.p, grid_height, grid_width, central_i, central_j, pose, out);
}

int kc_worldmap_update_from_mapper(kc_worldmap *c, kc_mapper *mapper, const kc_worldmap_pose *pose, kc_worldmap_result *out) {
  if (!c || !mapper || !out) KC_FAIL(KC_ERR_INVALID, "null argument");
  MapperView v{};
  KC_TRY(mapper_view(mapper, &v));
  if (v.device != c->device) KC_FAIL(KC_ERR_INVALID, "mapper on device %d, world map on device %d", v.device, c->device);
  KC_TRY(wm_check_grid(c->res, v.H, v.W, v.c0, v.c1, v.res));
  KC_TRY(wm_check_pose(pose));
  KC_HIP(hipSetDevice(c->device));
  // the map's stream waits for the scan; the host does not
  if (!c->grid_ready) KC_HIP(hipEventCreateWithFlags(&c->grid_ready, hipEventDisableTiming));
  KC_HIP(hipEventRecord(c->grid_ready, v.stream));
  KC_HIP(hipStreamWaitEvent(c->stream, c->grid_ready, 0));
  return wm_update(c, v.grid, v.H, v.W, v.c0, v.c1, pose, out);
}

int kc_worldmap_grid_device(kc_worldmap *c, void **dev_cls_int8) {
  if (!c || !dev_cls_int8) KC_FAIL(KC_ERR_INVALID, "null argument");
  *dev_cls_int8 = c->d_cls.p;
  return KC_OK;
}

int kc_worldmap_get(kc_worldmap *c, int8_t *cls_out, int8_t *evidence_out, size_t cap) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  const size_t n = static_cast<size_t>(c->W) * static_cast<size_t>(c->H);
  if (n > cap) KC_FAIL(KC_ERR_RANGE, "%zu cells do not fit the output capacity %zu", n, cap);
  KC_HIP(hipSetDevice(c->device));
  if (cls_out) KC_HIP(hipMemcpyAsync(cls_out, c->d_cls.p, n, hipMemcpyDeviceToHost, c->stream));
  if (evidence_out) KC_HIP(hipMemcpyAsync(evidence_out, c->d_evidence.p, n, hipMemcpyDeviceToHost, c->stream));
  KC_HIP(hipStreamSynchronize(c->stream));
  return KC_OK;
}

}  // extern "C"
