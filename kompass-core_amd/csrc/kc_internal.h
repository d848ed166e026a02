// Internal helpers shared by the HIP translation units of libkompass_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "kompass_hip.h"

namespace kc {

// ---- error plumbing: nothing throws across the C ABI ----------------------
void set_error(const char *fmt, ...);

#define KC_FAIL(code, ...)        \
  do {                            \
    ::kc::set_error(__VA_ARGS__); \
    return (code);                \
  } while (0)

#define KC_HIP(expr)                                                        \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    if (_e != hipSuccess) {                                                 \
      ::kc::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                      __FILE__, __LINE__);                                  \
      return KC_ERR_HIP;                                                    \
    }                                                                       \
  } while (0)

#define KC_TRY(expr)            \
  do {                          \
    int _rc = (expr);           \
    if (_rc != KC_OK) return _rc; \
  } while (0)

// ---- grow-only buffers that own their memory ---------------------------------
// (the reference grows its buffers the same way: cost_evaluator_gpu.cpp:248-271, 314-333).  Move-only: the
// destructor frees, a moved-from buffer is empty.  HIP errors of a free are ignored.
struct DevAlloc {
  static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t free(void *p) { return hipFree(p); }
};
// pinned host memory (async H2D / D2H without a hidden sync)
struct PinAlloc {
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static hipError_t free(void *p) { return hipHostFree(p); }
};

template <typename T, typename Alloc>
struct OwnedBuf {
  T *p = nullptr;
  size_t cap = 0;
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf &) = delete;
  OwnedBuf &operator=(const OwnedBuf &) = delete;
  OwnedBuf(OwnedBuf &&o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  OwnedBuf &operator=(OwnedBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~OwnedBuf() { release(); }
  int reserve(size_t n) {
    if (n <= cap) return KC_OK;
    release();
    size_t want = n + n / 4 + 16;
    KC_HIP(Alloc::alloc(reinterpret_cast<void **>(&p), want * sizeof(T)));
    cap = want;
    return KC_OK;
  }
  void release() {
    if (p) {
      hipError_t e = Alloc::free(p);
      (void)e;
    }
    p = nullptr;
    cap = 0;
  }
};
template <typename T>
using DevBuf = OwnedBuf<T, DevAlloc>;
template <typename T>
using PinBuf = OwnedBuf<T, PinAlloc>;
static_assert(!std::is_copy_constructible<DevBuf<int>>::value && !std::is_copy_assignable<DevBuf<int>>::value &&
                  std::is_nothrow_move_constructible<DevBuf<int>>::value &&
                  std::is_nothrow_move_assignable<DevBuf<int>>::value,
              "DevBuf owns device memory: move-only, and a std::vector of it grows by move");
static_assert(!std::is_copy_constructible<PinBuf<int>>::value && !std::is_copy_assignable<PinBuf<int>>::value &&
                  std::is_nothrow_move_constructible<PinBuf<int>>::value &&
                  std::is_nothrow_move_assignable<PinBuf<int>>::value,
              "PinBuf owns pinned memory: move-only, and a std::vector of it grows by move");

// ---- an event that orders one stream behind another ---------------------------
// Created by its first stream_wait_through, without timing, and kept.  Move-only; destroyed with the context it is a
// member of, whose kc_*_destroy has made the device current by then (as for the buffers).
struct OrderEvent {
  hipEvent_t e = nullptr;
  OrderEvent() = default;
  OrderEvent(OrderEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
  ~OrderEvent() {
    if (e) (void)hipEventDestroy(e);
  }
};

// ---- a flip-flop record: a launch's few result words without a launch to reset them (kc_worldmap.hip (c), (f)) ----
// Two device blocks of start.size() words: call n works in block n & 1, its launch puts the other back to the start values,
// commit() reads the block back.  ready (both blocks hold their start values) is dropped by begin() and raised by
// commit(): a call that fails in between makes the next begin() arm the blocks again.
struct FlipRecord {
  std::vector<int> start;      // one block's start values
  DevBuf<int> d;
  PinBuf<int> h;               // the block of the last commit()
  unsigned long long seq = 0;  // calls committed
  bool ready = false;
  int *cur = nullptr;          // the block of the call between begin() and commit()

  int arm(hipStream_t s) {
    ready = false;
    KC_TRY(d.reserve(2 * start.size()));
    KC_TRY(h.reserve(start.size()));
    for (size_t b = 0; b < 2; ++b)
      KC_HIP(hipMemcpyAsync(d.p + b * start.size(), start.data(), start.size() * sizeof(int), hipMemcpyHostToDevice, s));
    KC_HIP(hipStreamSynchronize(s));
    ready = true;
    return KC_OK;
  }
  // -> cur, this call's block, and *rearm, the one its launch puts back
  int begin(hipStream_t s, int **rearm) {
    if (!ready) KC_TRY(arm(s));
    cur = d.p + (seq & 1) * start.size();
    *rearm = d.p + (~seq & 1) * start.size();
    ready = false;
    return KC_OK;
  }
  int commit(hipStream_t s) {
    KC_HIP(hipMemcpyAsync(h.p, cur, start.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    KC_HIP(hipStreamSynchronize(s));
    ++seq;
    ready = true;
    return KC_OK;
  }
};

// ---- per-kernel HIP-event timing on the launch stream ----------------------
// (owns its events: move-only, the destructor destroys them)
struct Timing {
  bool enabled = false;
  struct Rec {
    const char *name;
    hipEvent_t a, b;
  };
  std::vector<Rec> pool;  // events are created once and reused
  size_t used = 0;
  // host-side phases of the same cycle (wall clock), reported as "host:<name>"
  struct HostRec {
    const char *name;
    double ms;
  };
  std::vector<HostRec> host;
  std::chrono::steady_clock::time_point t_mark;
  Timing() = default;
  Timing(const Timing &) = delete;
  Timing &operator=(const Timing &) = delete;
  Timing(Timing &&o) noexcept { *this = std::move(o); }
  Timing &operator=(Timing &&o) noexcept {
    if (this != &o) {
      release();
      enabled = o.enabled;
      pool.swap(o.pool);  // (ours is empty after release)
      used = o.used;
      host.swap(o.host);
      t_mark = o.t_mark;
      o.used = 0;
      o.host.clear();
    }
    return *this;
  }
  ~Timing() { release(); }
  void begin_cycle() {
    used = 0;
    host.clear();
    if (enabled) t_mark = std::chrono::steady_clock::now();
  }
  // closes the host phase that started at the previous mark
  void mark(const char *name) {
    if (!enabled) return;
    const auto now = std::chrono::steady_clock::now();
    host.push_back({name, std::chrono::duration<double, std::milli>(now - t_mark).count()});
    t_mark = now;
  }
  int start(const char *name, hipStream_t s) {
    if (!enabled) return KC_OK;
    if (used == pool.size()) {
      Rec r{name, nullptr, nullptr};
      KC_HIP(hipEventCreate(&r.a));
      KC_HIP(hipEventCreate(&r.b));
      pool.push_back(r);
    }
    pool[used].name = name;
    KC_HIP(hipEventRecord(pool[used].a, s));
    return KC_OK;
  }
  int stop(hipStream_t s) {
    if (!enabled) return KC_OK;
    KC_HIP(hipEventRecord(pool[used].b, s));
    used++;
    return KC_OK;
  }
  int get(const char **names, float *ms, size_t cap, size_t *count) {
    size_t n = 0;
    for (size_t i = 0; i < used && n < cap; ++i) {
      KC_HIP(hipEventSynchronize(pool[i].b));
      float t = 0.f;
      KC_HIP(hipEventElapsedTime(&t, pool[i].a, pool[i].b));
      if (names) names[n] = pool[i].name;
      if (ms) ms[n] = t;
      n++;
    }
    for (size_t i = 0; i < host.size() && n < cap; ++i) {
      if (names) names[n] = host[i].name;
      if (ms) ms[n] = static_cast<float>(host[i].ms);
      n++;
    }
    if (count) *count = n;
    return KC_OK;
  }
  void release() {
    for (auto &r : pool) {
      hipError_t e = hipEventDestroy(r.a);
      e = hipEventDestroy(r.b);
      (void)e;
    }
    pool.clear();
    used = 0;
  }
};
static_assert(!std::is_copy_constructible<Timing>::value && std::is_nothrow_move_constructible<Timing>::value,
              "Timing owns its events: move-only");

// ---- plumbing every device context shares (kc_common.hip) -------------------
// Opens a context: `device` must be a visible HIP device (a failing device count is "0 visible": KC_ERR_HIP);
// makes it current and creates the context's own non-blocking stream.
int open_device_stream(int device, hipStream_t *stream);
// Closes it (no-op for a stream never opened): device current, stream synchronised and destroyed.
void close_device_stream(int device, hipStream_t *stream);
// `own` waits for everything queued on `other` so far (a foreign stream of the same process)
int stream_wait_for(int device, hipStream_t own, void *other);
// The same between two contexts' streams through the waiting context's cached event, its device current; the host does
// not wait.  Nothing to do when both are one stream.
int stream_wait_through(OrderEvent &ev, hipStream_t own, hipStream_t producer);
// Memory a caller passes as "on the device" is read by kernels in place: [ptr + lo_bytes, ptr + hi_bytes) must
// lie inside one allocation of `device`'s memory and ptr % align == 0.  KC_ERR_INVALID otherwise, with `what`
// (the noun: "cloud", "grid", "frame") in the message, and before any read.
int check_device_range(int device, const void *ptr, long long lo_bytes, long long hi_bytes, size_t align,
                       const char *what);

// ---- the host side of kc_q16.h's integers, shared by kc_mcl.hip and kc_mppi.hip (kc_common.hip) ----
// libm's separate cos and sin through pointers, so that the compiler cannot fold the pair into one sincos call (whose
// bits differ from theirs in about 0.1 % of arguments where glibc picks its FMA builds: kc_dvz.hip has the story)
extern double (*volatile host_cos)(double);
extern double (*volatile host_sin)(double);
// DESIGN.md 4.11 rule 29: the 65536 (Cq, Sq) pairs, formed once a process; and a context's own device copy of them:
// reserved, uploaded and `s` drained
const int2 *heading_table();
int upload_heading_table(DevBuf<int2> &d, hipStream_t s);
// rule 36's refusals of a weight table that is there, in their order (cap: the caller's KC_*_MAX_TABLE), and those of a
// penalty table of n_pen = c2 + 1 entries against a distance plane's reach (0: no plane to compare with)
int check_weight_table(const uint32_t *wtab, size_t EW, int w_shift, int cap);
int check_reach(size_t n_pen, int reach);
// a penalty and a weight table from the caller's memory into buffers grown to hold them; returns after the drain
int upload_tables(DevBuf<unsigned short> &d_pen, const uint16_t *pen, size_t n_pen, DevBuf<unsigned> &d_wtab, const uint32_t *wtab,
                  size_t n_wtab, hipStream_t s);

// ---- correctly rounded f32 divide / sqrt on the device ----------------------
// HIP's __fsqrt_rn lowers to the *native* (approximate) sqrt unless
// OCML_BASIC_ROUNDED_OPERATIONS is defined; the plain operators are IEEE
// correctly rounded under -fhip-fp32-correctly-rounded-divide-sqrt (on here).
__host__ __device__ inline float div_rn(float a, float b) { return a / b; }
__host__ __device__ inline float sqrt_rn(float a) { return __builtin_sqrtf(a); }
__host__ __device__ inline double dsqrt_rn(double a) { return __builtin_sqrt(a); }

// ---- packed (cost, index) key: signed-comparable int64 ---------------------
// LowestCost::combine (datatypes/trajectory.h:630-636): lower cost wins, ties
// go to the lower index.  key = (sortable_i32(cost) << 32) | u32 index; signed
// int64 comparison reproduces that order.  KEY_NONE = nothing beats FLT_MAX.
constexpr int64_t KEY_NONE = INT64_MAX;

__host__ __device__ inline int32_t float_sortable(float f) {
  f = f + 0.0f;  // -0.0 -> +0.0 so that both compare equal like floats do
  int32_t b;
#if defined(__HIP_DEVICE_COMPILE__)
  b = __float_as_int(f);
#else
  std::memcpy(&b, &f, 4);
#endif
  return b >= 0 ? b : (b ^ 0x7FFFFFFF);
}
__host__ __device__ inline float sortable_float(int32_t s) {
  int32_t b = s >= 0 ? s : (s ^ 0x7FFFFFFF);
  float f;
#if defined(__HIP_DEVICE_COMPILE__)
  f = __int_as_float(b);
#else
  std::memcpy(&f, &b, 4);
#endif
  return f;
}
__host__ __device__ inline int64_t key_pack(float cost, uint32_t index) {
  const uint64_t hi = static_cast<uint64_t>(
      static_cast<uint32_t>(float_sortable(cost)));
  return static_cast<int64_t>((hi << 32) | static_cast<uint64_t>(index));
}

// ---- checksum of the pinned result record ----------------------------------
// The device writes the record as separate 8-byte stores without fences; the
// host accepts it when the sequence word matches and this word over (key,
// packed counts, sequence, row word) does.  Each input goes through a multiply
// / shift mix and a different rotation, so a record that mixes words of two
// cycles cannot pass the way it could with a plain XOR (equal differences
// cancelling).
__host__ __device__ inline unsigned long long rec_mix(unsigned long long x) {
  x *= 0x9E3779B97F4A7C15ull;
  return x ^ (x >> 29);
}
__host__ __device__ inline unsigned long long rec_rot(unsigned long long x, int r) {
  return (x << r) | (x >> (64 - r));
}
__host__ __device__ inline long long record_check(long long w0, long long w1, long long seq,
                                                  long long w4 = 0) {
  const unsigned long long c = rec_mix(static_cast<unsigned long long>(w0) + 0x5bd1e9955bd1e995ull) ^
                               rec_rot(rec_mix(static_cast<unsigned long long>(w1) ^ 0x2545F4914F6CDD1Dull), 21) ^
                               rec_rot(rec_mix(static_cast<unsigned long long>(seq)), 42) ^
                               rec_rot(rec_mix(static_cast<unsigned long long>(w4) + 0x9E37ull), 11);
  return static_cast<long long>(c);
}

// internal view of a mapper context for the grid hand-off (kc_dwa.hip)
struct MapperView {
  const int *grid;
  int H, W, c0, c1;
  float res;
  hipStream_t stream;
  int device;
};
int mapper_view(kc_mapper *m, MapperView *out);

// internal view of a world map for the obstacle hand-off (kc_worldmap.hip owns the planes and the kernel; DESIGN.md
// 4.11 rules 16 to 19)
struct WorldMapView {
  const int8_t *cls;  // [W x H], cell (I, J) at I + J * W
  int W, H;
  float res;
  double ox, oy;      // rule 46's origin at the current offset
  hipStream_t stream;
  int device;
  int OI, OJ;         // rule 46's offset, for whoever keeps cell coordinates across a shift (kc_mcl, rule 50)
};
int worldmap_view(kc_worldmap *m, WorldMapView *out);
// the map's distance plane (rules 42 and 43) for a reader on another stream: reach 0 and a null plane while it is off
struct WorldMapDistance {
  const uint16_t *dist2;  // [W x H] as cls
  int reach;
};
// host only: queues nothing
int worldmap_distance_state(kc_worldmap *m, WorldMapDistance *out);
// queues rule 43's refresh on the map's stream when the dirty box is not empty; the reader then waits for that stream
int worldmap_distance_refresh(kc_worldmap *m);
// the grid planner's kept goal-rooted disc-mode cost field for a reader on another stream (kc_planner.hip owns it;
// DESIGN.md 4.12 rules 19 and 23).  Host only: queues nothing.  KC_ERR_STATE while the planner holds no such field
struct PlannerFieldView {
  const uint32_t *field;  // [W x H], cell (I, J) at I + J * W; 0xFFFFFFFF: no walk reaches the goal
  int W, H;
  hipStream_t stream;
  int device;
};
int planner_field_view(kc_planner *p, PlannerFieldView *out);
// rule 16's window, and the number of map cells inside rule 17's disc: the most points a list of it can hold
struct WorldMapWindow {
  int ic, jc, rc;
  size_t max_points;  // 0: the window misses the map, nothing to launch
};
int worldmap_window(const WorldMapView &v, double x, double y, float max_range, WorldMapWindow *out);
// Queues the extraction on `stream` (the caller's: it orders the launch after the map's writes itself): the points into
// xyz ([max_points][3] floats; nullptr counts only), the count and the index bounds i_min, i_max, j_min, j_max into cnt,
// five words 16 words apart that hold 0, INT_MAX, INT_MIN, INT_MAX, INT_MIN (grid_points_kernel's block, so
// grid_points_publish_kernel serves both).  rearm: another such block the launch puts back to those values, or nullptr.
int worldmap_queue_points(const WorldMapView &v, const WorldMapWindow &w, float *xyz, unsigned int *cnt, unsigned int *rearm,
                          hipStream_t stream);
// ---- the map's virtual laser scan (kc_worldmap.hip (g); DESIGN.md 4.11 rules 20 to 27) ----
// rule 21's table of one angle array, kept by whoever scans with it: ensure() forms and uploads it again only when the
// bytes of `angles` differ from those it was formed from.  The upload is queued on `s`; the pinned copy is rewritten by
// the host, so the owner's entries return with their stream drained (all of them do).
struct ScanTable {
  std::vector<double> angles;  // what the table was formed from
  PinBuf<int32_t> h;           // (ac_k, as_k) pairs
  DevBuf<int32_t> d;
  bool valid = false;
  int ensure(const double *a, size_t n, hipStream_t s);
};
// rule 21 on the host: KC_ERR_INVALID for a non-finite angle, and then nothing is written
int worldmap_scan_table(const double *angles, size_t n, int32_t *ac_as_out);
// the refusals of rules 20, 21 and 25, in that order: counts, range_max, flags
int worldmap_scan_check(float res, size_t n_poses, size_t n_beams, float range_max, unsigned flags, int *rc_out);
// wm_check_pose: what every pose handed to the map must satisfy
int worldmap_check_pose(const kc_worldmap_pose *p);
struct WorldMapScan {
  const int32_t *table;               // the device copy of a ScanTable of n_beams pairs
  const kc_worldmap_pose *dev_poses;  // n_poses poses on the device; nullptr: the one pose below, in the kernel arguments
  kc_worldmap_pose pose;
  size_t n_poses, n_beams;
  int rc;                             // rule 20's Rc, from worldmap_scan_check
  float range_max;
  unsigned flags;
  const double *real;                 // rule 27: n_beams present ranges on the device (one pose only), or nullptr
  double *ranges;                     // [n_poses * n_beams]
  int32_t *cells;                     // the same count, or nullptr
};
// Queues the one launch on `stream` (the caller's: it orders the launch after the map's writes itself).  Every argument
// has been checked by then.
int worldmap_queue_scan(const WorldMapView &v, const WorldMapScan &s, hipStream_t stream);

// rule 18: the coordinate of cell index k along one axis
__host__ __device__ inline float worldmap_cell_coord(double origin, int k, double res) {
  return static_cast<float>(origin + static_cast<double>(k) * res);
}

// kc_comm.hip: all-reduce (min, or sum) of int64 words on a stream; send == recv is allowed
int comm_allreduce_i64(kc_comm *m, const long long *send, long long *recv, size_t count, bool sum,
                       hipStream_t stream);
int comm_world(const kc_comm *m);
int comm_rank(const kc_comm *m);
int comm_device(const kc_comm *m);

}  // namespace kc
