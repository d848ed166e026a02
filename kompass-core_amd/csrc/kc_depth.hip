// DepthDetector on gfx950: 2-D detections -> 3-D boxes (reference:
// vision/depth_detector.cpp:84-178).
//
// The reference collects every kept depth of a box into a vector, sorts it
// twice (median, then MAD) and scans it once more for the band's min / max.
// Here a box is a histogram over the RAW depth values: d -> float(d) * factor
// is non-decreasing for factor > 0, so the kept values are the conversions of
// one raw interval [d_lo, d_lo + nbins) (found once per context on the host,
// exactly, by converting all 65536 values) and the k-th smallest kept depth is
// the conversion of the k-th smallest kept raw value.  Every pixel is read
// ONCE; the median, the MAD (a radix select over the float bits of the per-bin
// deviations) and the band's min / max come from the histogram, at a cost
// that depends on nbins, not on the box size.  DESIGN.md 4.6.
//
// One launch per call.  Each workgroup takes one chunk (<= 32768 pixels) of
// one box and counts it into an LDS histogram of 16-bit counters (two per
// word: a chunk never reaches 65536 of one value).  A box of one chunk is
// finished from LDS by that workgroup; a box of several chunks adds its
// chunks' counts to a global histogram, and the last workgroup of the box
// (ticket counter, agent-scope release / acquire) finishes it from there.
// Per box the result is (count, median, mad, min_d, max_d); the O(1) geometry
// of the kept boxes runs on the host (kc_hostmath.h), as in the reference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "kc_hostmath.h"
#include "kc_internal.h"
#include "kompass_hip.h"

namespace kc {

constexpr int kDepthBlock = 256;
constexpr int kDepthMaxBins = 65536;  // every uint16 value

struct DepthStats {
  unsigned count;
  float median, mad, min_d, max_d;
};

struct DepthArgs {
  const uint16_t *img;  // element (0, 0) of the boxes' coordinates
  long long rs, cs;     // row / column stride in elements
  int inner_cols;       // 1: consecutive pixels of a chunk run along a row (columns), 0: along a column
  int d_lo, nbins;      // kept raw values: [d_lo, d_lo + nbins)
  float factor;
  float min_depth, max_depth;
  int chunk;            // pixels per workgroup
  const int4 *boxes;    // per box: (y0, x0, ny, nx), clipped to the image
  const int4 *work;     // per workgroup: (box, chunk, chunks of the box, global histogram slot)
  unsigned *hist;       // [slots][nbins] (zeroed by the call)
  unsigned *kept;       // [boxes] kept pixels of multi-chunk boxes (zeroed by the call)
  unsigned *span;       // [boxes][2] occupied bins of multi-chunk boxes: nbins - lowest, highest + 1 (zeroed)
  unsigned *ticket;     // [boxes] (zeroed by the call)
  DepthStats *out;      // [boxes]
};

// count of bin k: 16-bit counters in LDS, two per word ...
struct LdsHist {
  const unsigned *w;
  __device__ unsigned operator()(int k) const { return (w[k >> 1] >> ((k & 1) << 4)) & 0xFFFFu; }
};
// ... or 32-bit counters in global memory (read after the hand-off's acquire)
struct GlobalHist {
  const unsigned *g;
  __device__ unsigned operator()(int k) const { return g[k]; }
};

__device__ inline float depth_of(const DepthArgs &a, int k) {
  return static_cast<float>(a.d_lo + k) * a.factor;  // depth_detector.cpp:97-98
}

// Block-wide sum of one value per thread (result in every thread).
__device__ inline unsigned block_sum(unsigned v, unsigned *sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const unsigned s = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return s;
}

// Block-wide maximum of one value per thread (result in every thread).
__device__ inline unsigned block_max(unsigned v, unsigned *sh) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, static_cast<unsigned>(__shfl_xor(v, o)));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const unsigned s = max(max(sh[0], sh[1]), max(sh[2], sh[3]));
  __syncthreads();
  return s;
}

// The element of rank `rank` (0-based, in key order) of the multiset {key(k) x count(k)}, by radix select over
// the key's low `nbits` bits, 8 per pass: `x` is its key.  With want_next, `x_next` is the key of rank + 1: x
// again when x repeats past rank, else the smallest key above x (one more pass).  sh: 256 + 8 words of LDS.
template <class H, class Key>
__device__ void select_rank(const H &h, int k0, int k1, unsigned rank, int nbits, bool want_next, Key key, unsigned *sh,
                            unsigned &x, unsigned &x_next) {
  const int tid = threadIdx.x;
  unsigned prefix = 0, rem = rank, at_x = 0;
  for (int shift = nbits - 8; shift >= 0; shift -= 8) {
    const unsigned hi_mask = shift + 8 >= 32 ? 0u : ~0u << (shift + 8);
    sh[tid] = 0;
    __syncthreads();
    for (int k = k0 + tid; k <= k1; k += kDepthBlock) {
      const unsigned c = h(k);
      if (!c) continue;
      const unsigned kk = key(k);
      if ((kk & hi_mask) == prefix) atomicAdd(&sh[(kk >> shift) & 255u], c);
    }
    __syncthreads();
    if (tid < 64) {  // wave 0: 4 buckets per lane, inclusive scan over the lanes
      const unsigned b0 = sh[4 * tid], b1 = sh[4 * tid + 1], b2 = sh[4 * tid + 2], b3 = sh[4 * tid + 3];
      const unsigned own = b0 + b1 + b2 + b3;
      unsigned inc = own;
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(inc, o);
        if (tid >= o) inc += u;
      }
      const unsigned exc = inc - own;
      if (exc <= rem && rem < inc) {  // exactly one lane
        unsigned r = rem - exc, d = 4 * tid, bd = b0;
        if (r >= b0) {
          r -= b0, ++d, bd = b1;
          if (r >= b1) {
            r -= b1, ++d, bd = b2;
            if (r >= b2) r -= b2, ++d, bd = b3;
          }
        }
        sh[256] = d;
        sh[257] = r;
        sh[258] = bd;
      }
    }
    __syncthreads();
    prefix |= sh[256] << shift;
    rem = sh[257];
    at_x = sh[258];
    __syncthreads();
  }
  x = prefix;
  x_next = x;
  if (!want_next || rem + 1 < at_x) return;  // rank + 1 has the key x too
  if (tid == 0) sh[259] = 0xFFFFFFFFu;
  __syncthreads();
  unsigned m = 0xFFFFFFFFu;
  for (int k = k0 + tid; k <= k1; k += kDepthBlock) {
    if (!h(k)) continue;
    const unsigned kk = key(k);
    if (kk > x && kk < m) m = kk;
  }
  if (m != 0xFFFFFFFFu) atomicMin(&sh[259], m);
  __syncthreads();
  x_next = sh[259];
  __syncthreads();
}

// getMedian / calculateMAD / the band loop (depth_detector.cpp:104-117, 159-178) of one box from its histogram,
// whose occupied bins lie in [k0, k1].
template <class H>
__device__ void depth_finish(const DepthArgs &a, const H &h, unsigned n, int k0, int k1, unsigned *sh,
                             DepthStats *out) {
  DepthStats s{n, 0.0f, 0.0f, 0.0f, 0.0f};
  if (n <= 1) {  // dropped (:100-103)
    if (threadIdx.x == 0) *out = s;
    return;
  }
  const bool even = (n & 1u) == 0;
  const unsigned r = even ? n / 2 - 1 : n / 2;
  unsigned j0, j1;
  select_rank(h, k0, k1, r, 16, even, [](int k) { return static_cast<unsigned>(k); }, sh, j0, j1);
  const float median = even ? 0.5f * (depth_of(a, static_cast<int>(j0)) + depth_of(a, static_cast<int>(j1)))
                            : depth_of(a, static_cast<int>(j0));
  // deviations are non-negative floats: their bit patterns order like their values
  unsigned m0, m1;
  select_rank(h, k0, k1, r, 32, even,
              [&](int k) { return __float_as_uint(fabsf(depth_of(a, k) - median)); }, sh, m0, m1);
  const float mad = even ? 0.5f * (__uint_as_float(m0) + __uint_as_float(m1)) : __uint_as_float(m0);
  // the band tests are double comparisons (the literal 1.5 is a double)
  const double lo = static_cast<double>(median) - 1.5 * static_cast<double>(mad);
  const double hi = static_cast<double>(median) + 1.5 * static_cast<double>(mad);
  if (threadIdx.x == 0) {
    sh[260] = 0xFFFFFFFFu;  // min bits (none)
    sh[261] = 0;            // max bits + 1 (none)
  }
  __syncthreads();
  unsigned vmin = 0xFFFFFFFFu, vmax = 0;
  for (int k = k0 + static_cast<int>(threadIdx.x); k <= k1; k += kDepthBlock) {
    if (!h(k)) continue;
    const float v = depth_of(a, k);
    const unsigned bits = __float_as_uint(v);  // v >= +0: bits order like values
    if (static_cast<double>(v) >= lo) vmin = min(vmin, bits);
    if (static_cast<double>(v) <= hi) vmax = max(vmax, bits + 1u);
  }
  if (vmin != 0xFFFFFFFFu) atomicMin(&sh[260], vmin);
  if (vmax) atomicMax(&sh[261], vmax);
  __syncthreads();
  if (threadIdx.x == 0) {
    // minimum_d starts at maxDepth_, maximum_d at minDepth_; strict updates
    float mn = a.max_depth, mx = a.min_depth;
    if (sh[260] != 0xFFFFFFFFu && __uint_as_float(sh[260]) < mn) mn = __uint_as_float(sh[260]);
    if (sh[261] && __uint_as_float(sh[261] - 1u) > mx) mx = __uint_as_float(sh[261] - 1u);
    s.median = median;
    s.mad = mad;
    s.min_d = mn;
    s.max_d = mx;
    *out = s;
  }
}

__global__ __launch_bounds__(kDepthBlock) void depth_boxes_kernel(DepthArgs a) {
  extern __shared__ unsigned lds_hist[];
  __shared__ unsigned sh[264];
  __shared__ unsigned last;
  const int tid = threadIdx.x;
  const int4 w = a.work[blockIdx.x];
  const int b = w.x;
  const int4 bx = a.boxes[b];  // (y0, x0, ny, nx)
  const int words = (a.nbins + 1) >> 1;
  for (int i = tid; i < words; i += kDepthBlock) lds_hist[i] = 0;
  __syncthreads();
  // pixels of the box in chunk order: the inner axis is the one with the smaller stride (coalesced reads)
  const unsigned inner = static_cast<unsigned>(a.inner_cols ? bx.w : bx.z);
  const unsigned npix = static_cast<unsigned>(bx.z) * static_cast<unsigned>(bx.w);
  const unsigned p0 = static_cast<unsigned>(w.y) * static_cast<unsigned>(a.chunk);
  const unsigned p1 = min(npix, p0 + static_cast<unsigned>(a.chunk));
  unsigned kept = 0, lo_enc = 0, hi_enc = 0;  // nbins - lowest bin, highest bin + 1 (0: none)
  for (unsigned p = p0 + tid; p < p1; p += kDepthBlock) {
    const unsigned o = p / inner, i = p - o * inner;
    const long long row = bx.x + static_cast<long long>(a.inner_cols ? o : i);
    const long long col = bx.y + static_cast<long long>(a.inner_cols ? i : o);
    const unsigned k = static_cast<unsigned>(a.img[row * a.rs + col * a.cs]) - static_cast<unsigned>(a.d_lo);
    if (k < static_cast<unsigned>(a.nbins)) {  // min_depth <= depth <= max_depth
      atomicAdd(&lds_hist[k >> 1], 1u << ((k & 1u) << 4));
      ++kept;
      lo_enc = max(lo_enc, static_cast<unsigned>(a.nbins) - k);
      hi_enc = max(hi_enc, k + 1u);
    }
  }
  kept = block_sum(kept, sh);  // (its barriers also close the histogram)
  lo_enc = block_max(lo_enc, sh);
  hi_enc = block_max(hi_enc, sh);
  if (w.z == 1) {
    depth_finish(a, LdsHist{lds_hist}, kept, a.nbins - static_cast<int>(lo_enc), static_cast<int>(hi_enc) - 1, sh,
                 &a.out[b]);
    return;
  }
  // several chunks: add this chunk's counts to the box's global histogram, then take a ticket
  unsigned *g = a.hist + static_cast<size_t>(w.w) * static_cast<size_t>(a.nbins);
  for (int i = tid; i < words; i += kDepthBlock) {
    const unsigned v = lds_hist[i];
    if (!v) continue;
    if (v & 0xFFFFu) atomicAdd(&g[2 * i], v & 0xFFFFu);
    if (v >> 16) atomicAdd(&g[2 * i + 1], v >> 16);
  }
  if (tid == 0 && kept) {
    atomicAdd(&a.kept[b], kept);
    atomicMax(&a.span[2 * b], lo_enc);
    atomicMax(&a.span[2 * b + 1], hi_enc);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    last = atomicAdd(&a.ticket[b], 1u) == static_cast<unsigned>(w.z - 1);
  }
  __syncthreads();
  if (!last) return;
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    sh[261] = __hip_atomic_load(&a.kept[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh[262] = __hip_atomic_load(&a.span[2 * b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh[263] = __hip_atomic_load(&a.span[2 * b + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const unsigned n = sh[261];
  const int k0 = a.nbins - static_cast<int>(sh[262]), k1 = static_cast<int>(sh[263]) - 1;
  __syncthreads();
  depth_finish(a, GlobalHist{g}, n, k0, k1, sh, &a.out[b]);
}

}  // namespace kc

using namespace kc;

struct kc_depth {
  int device = 0;
  hipStream_t stream = nullptr;  // created by the first compute call (the constructor needs no device)
  float min_depth = 0.f, max_depth = 0.f, factor = 0.f;
  float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f;
  int d_lo = 0, nbins = 0;
  hm::Rigid3f camera_in_body{}, body_in_world{};
  Timing timing;
  bool lds_ok = false;
  size_t last_upload = 0;
  DevBuf<uint16_t> d_img;
  DevBuf<int4> d_boxes, d_work;
  DevBuf<unsigned> d_hist, d_count;  // d_count: kept [n] + ticket [n] + span [2 n]
  DevBuf<DepthStats> d_out;
  PinBuf<int4> h_boxes, h_work;
  PinBuf<DepthStats> h_out;
  PinBuf<uint16_t> h_img;  // staging of frames with no unit stride
  std::vector<DepthStats> stats;
};

namespace {

int depth_ready(kc_depth *c) {
  if (c->stream) return KC_OK;
  KC_TRY(open_device_stream(c->device, &c->stream));
  c->lds_ok = hipFuncSetAttribute(reinterpret_cast<const void *>(depth_boxes_kernel),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kDepthMaxBins * 2) == hipSuccess;
  if (!c->lds_ok) {
    (void)hipGetLastError();
    KC_FAIL(KC_ERR_HIP, "the depth kernel cannot get %d bytes of LDS", kDepthMaxBins * 2);
  }
  return KC_OK;
}

// A frame passed as "on the device" is read by the kernel in place: every element of the rows x cols frame must
// lie in device memory of the context's device, inside one allocation; anything else (a host pointer, another
// GPU's memory, a shape larger than the buffer) is refused here, before any read.
int check_device_frame(const kc_depth *c, const uint16_t *img, long long rows, long long cols, long long rs,
                       long long cs) {
  // the lowest and highest element offsets of the frame, then bytes [2 lo, 2 hi + 2)
  long long lo = 0, hi = 0, t = 0;
  if (__builtin_mul_overflow(rows - 1, rs, &t)) KC_FAIL(KC_ERR_RANGE, "frame row stride out of range");
  (t < 0 ? lo : hi) = t;
  if (__builtin_mul_overflow(cols - 1, cs, &t)) KC_FAIL(KC_ERR_RANGE, "frame column stride out of range");
  long long &end = t < 0 ? lo : hi;
  if (__builtin_add_overflow(end, t, &end) || __builtin_mul_overflow(lo, 2ll, &lo) ||
      __builtin_mul_overflow(hi, 2ll, &hi) || __builtin_add_overflow(hi, 2ll, &hi))
    KC_FAIL(KC_ERR_RANGE, "frame strides out of range");
  return check_device_range(c->device, img, lo, hi, 1, "frame");
}

// The statistics of every box (count = 0 for a box with no pixel in the image).  Box pixels are the inclusive
// limits top .. top + size (getXLimits / getYLimits) in 64-bit, clipped to the image.
int depth_stats(kc_depth *c, const uint16_t *img, int on_device, long long rows, long long cols, long long rs,
                long long cs, const int32_t *boxes, size_t n) {
  c->stats.assign(n, DepthStats{0, 0.f, 0.f, 0.f, 0.f});
  c->last_upload = 0;
  if (rows < 0 || cols < 0) KC_FAIL(KC_ERR_INVALID, "negative frame shape %lld x %lld", rows, cols);
  if (rows * cols > 0x7FFFFFFFll) KC_FAIL(KC_ERR_RANGE, "frame of more than 2^31 pixels");
  if (n && !boxes) KC_FAIL(KC_ERR_INVALID, "null boxes");
  if (n > 0x7FFFFFFFull) KC_FAIL(KC_ERR_RANGE, "too many boxes");
  KC_TRY(depth_ready(c));
  if (n == 0) return KC_OK;
  if (rows && cols && !img) KC_FAIL(KC_ERR_INVALID, "null frame");
  if (on_device && rows && cols) KC_TRY(check_device_frame(c, img, rows, cols, rs, cs));
  // clip, and the bounding rectangle of the clipped boxes
  struct Clip {
    long long y0, x0, y1, x1;
  };
  std::vector<Clip> clip(n);
  long long ry0 = rows, rx0 = cols, ry1 = -1, rx1 = -1;
  for (size_t i = 0; i < n; ++i) {
    const long long tx = boxes[4 * i], ty = boxes[4 * i + 1], sx = boxes[4 * i + 2], sy = boxes[4 * i + 3];
    Clip k{std::max(ty, 0ll), std::max(tx, 0ll), std::min(ty + sy, rows - 1), std::min(tx + sx, cols - 1)};
    if (k.y0 > k.y1 || k.x0 > k.x1) k = Clip{0, 0, -1, -1};
    clip[i] = k;
    if (k.y0 <= k.y1) {
      ry0 = std::min(ry0, k.y0);
      rx0 = std::min(rx0, k.x0);
      ry1 = std::max(ry1, k.y1);
      rx1 = std::max(rx1, k.x1);
    }
  }
  if (ry1 < 0 || c->nbins == 0) return KC_OK;  // no pixel of any box, or no depth can be kept
  KC_HIP(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  c->timing.begin_cycle();
  // the frame: a host frame uploads the bounding rectangle only; a device frame is read where it lies
  const long long nr = ry1 - ry0 + 1, nc = rx1 - rx0 + 1;
  const uint16_t *dimg = img;
  long long drs = rs, dcs = cs, oy = 0, ox = 0;
  if (!on_device) {
    const size_t bytes = static_cast<size_t>(nr * nc) * sizeof(uint16_t);
    KC_TRY(c->d_img.reserve(static_cast<size_t>(nr * nc)));
    const uint16_t *src = img + ry0 * rs + rx0 * cs;
    // the rectangle is packed into pinned staging on the host (a contiguous run per row or column where the frame
    // has one), then ONE copy: a pitched 2-D copy from pageable memory was 30x slower for narrow rectangles
    KC_HIP(hipStreamSynchronize(s));  // (the staging buffer may still feed the previous call's copy)
    KC_TRY(c->h_img.reserve(static_cast<size_t>(nr * nc)));
    const bool by_rows = std::llabs(cs) <= std::llabs(rs);
    uint16_t *dst = c->h_img.p;
    if (by_rows && cs == 1) {
      for (long long y = 0; y < nr; ++y, dst += nc) std::memcpy(dst, src + y * rs, static_cast<size_t>(nc) * 2);
    } else if (!by_rows && rs == 1) {
      for (long long x = 0; x < nc; ++x, dst += nr) std::memcpy(dst, src + x * cs, static_cast<size_t>(nr) * 2);
    } else if (by_rows) {
      for (long long y = 0; y < nr; ++y)
        for (long long x = 0; x < nc; ++x) *dst++ = src[y * rs + x * cs];
    } else {
      for (long long x = 0; x < nc; ++x)
        for (long long y = 0; y < nr; ++y) *dst++ = src[y * rs + x * cs];
    }
    KC_TRY(c->timing.start("upload", s));
    KC_HIP(hipMemcpyAsync(c->d_img.p, c->h_img.p, bytes, hipMemcpyHostToDevice, s));
    drs = by_rows ? nc : 1;
    dcs = by_rows ? 1 : nr;
    KC_TRY(c->timing.stop(s));
    c->last_upload = bytes;
    dimg = c->d_img.p;
    oy = ry0;
    ox = rx0;
  }
  // boxes and the work list: one workgroup per chunk
  const int chunk = c->nbins > 16384 ? 32768 : 8192;
  KC_TRY(c->h_boxes.reserve(n));
  std::vector<int4> work;
  int slots = 0;
  for (size_t i = 0; i < n; ++i) {
    const Clip &k = clip[i];
    const long long ny = k.y1 - k.y0 + 1, nx = k.x1 - k.x0 + 1;
    c->h_boxes.p[i] = make_int4(static_cast<int>(k.y0 - oy), static_cast<int>(k.x0 - ox), static_cast<int>(ny),
                                static_cast<int>(nx));
    if (ny <= 0) continue;
    const int chunks = static_cast<int>((ny * nx + chunk - 1) / chunk);
    const int slot = chunks > 1 ? slots++ : 0;
    for (int j = 0; j < chunks; ++j) work.push_back(make_int4(static_cast<int>(i), j, chunks, slot));
  }
  KC_TRY(c->h_work.reserve(work.size()));
  std::memcpy(c->h_work.p, work.data(), work.size() * sizeof(int4));
  KC_TRY(c->d_boxes.reserve(n));
  KC_TRY(c->d_work.reserve(work.size()));
  KC_TRY(c->d_count.reserve(4 * n));
  KC_TRY(c->d_out.reserve(n));
  KC_TRY(c->h_out.reserve(n));
  const size_t hist_words = static_cast<size_t>(slots) * static_cast<size_t>(c->nbins);
  if (slots) KC_TRY(c->d_hist.reserve(hist_words));
  KC_HIP(hipMemcpyAsync(c->d_boxes.p, c->h_boxes.p, n * sizeof(int4), hipMemcpyHostToDevice, s));
  KC_HIP(hipMemcpyAsync(c->d_work.p, c->h_work.p, work.size() * sizeof(int4), hipMemcpyHostToDevice, s));
  KC_HIP(hipMemsetAsync(c->d_count.p, 0, 4 * n * sizeof(unsigned), s));
  KC_HIP(hipMemsetAsync(c->d_out.p, 0, n * sizeof(DepthStats), s));
  if (slots) KC_HIP(hipMemsetAsync(c->d_hist.p, 0, hist_words * sizeof(unsigned), s));
  DepthArgs a{};
  a.img = dimg;
  a.rs = drs;
  a.cs = dcs;
  a.inner_cols = std::llabs(dcs) <= std::llabs(drs) ? 1 : 0;
  a.d_lo = c->d_lo;
  a.nbins = c->nbins;
  a.factor = c->factor;
  a.min_depth = c->min_depth;
  a.max_depth = c->max_depth;
  a.chunk = chunk;
  a.boxes = c->d_boxes.p;
  a.work = c->d_work.p;
  a.hist = c->d_hist.p;
  a.kept = c->d_count.p;
  a.ticket = c->d_count.p + n;
  a.span = c->d_count.p + 2 * n;
  a.out = c->d_out.p;
  const size_t lds = static_cast<size_t>((c->nbins + 1) / 2) * sizeof(unsigned);
  KC_TRY(c->timing.start("depth_boxes_kernel", s));
  hipLaunchKernelGGL(depth_boxes_kernel, dim3(static_cast<unsigned>(work.size())), dim3(kDepthBlock), lds, s, a);
  KC_HIP(hipGetLastError());
  KC_TRY(c->timing.stop(s));
  KC_HIP(hipMemcpyAsync(c->h_out.p, c->d_out.p, n * sizeof(DepthStats), hipMemcpyDeviceToHost, s));
  KC_HIP(hipStreamSynchronize(s));
  std::memcpy(c->stats.data(), c->h_out.p, n * sizeof(DepthStats));
  c->timing.mark("host:depth_stats");
  return KC_OK;
}

}  // namespace

extern "C" {

int kc_depth_create(const float depth_range[2], const float cam_pos[3], const float cam_rot_xyzw[4],
                    const float focal[2], const float principal[2], float factor, int device, kc_depth **out) {
  if (!out || !depth_range || !cam_pos || !cam_rot_xyzw || !focal || !principal)
    KC_FAIL(KC_ERR_INVALID, "null argument");
  *out = nullptr;
  // every converted depth must be finite: no NaN can reach a median
  if (!std::isfinite(factor) || !(factor > 0.0f) || !std::isfinite(65535.0f * factor))
    KC_FAIL(KC_ERR_INVALID, "depth conversion factor %g must be finite, > 0, with 65535 * factor finite",
            static_cast<double>(factor));
  auto *c = new kc_depth();
  c->device = device;
  c->min_depth = depth_range[0];
  c->max_depth = depth_range[1];
  c->factor = factor;
  c->fx = focal[0];
  c->fy = focal[1];
  c->cx = principal[0];
  c->cy = principal[1];
  // Eigen::Quaternionf from the (x, y, z, w) vector; getTransformation(q, t) (transformation.h:19-33)
  const hm::Quat q{cam_rot_xyzw[3], cam_rot_xyzw[0], cam_rot_xyzw[1], cam_rot_xyzw[2]};
  c->camera_in_body = hm::Rigid3f::from_quat(q, cam_pos);
  c->body_in_world = hm::Rigid3f::identity();
  // the kept raw values: one interval, since float(d) * factor is non-decreasing in d
  int lo = -1, hi = -2;
  for (int d = 0; d < kDepthMaxBins; ++d) {
    const float v = static_cast<float>(d) * factor;
    if (v <= c->max_depth && v >= c->min_depth) {
      if (lo < 0) lo = d;
      hi = d;
    }
  }
  c->d_lo = lo < 0 ? 0 : lo;
  c->nbins = lo < 0 ? 0 : hi - lo + 1;
  *out = c;
  return KC_OK;
}

void kc_depth_destroy(kc_depth *c) {
  if (!c) return;
  close_device_stream(c->device, &c->stream);
  delete c;
}

int kc_depth_box_stats(kc_depth *c, const uint16_t *img, int data_on_device, int64_t rows, int64_t cols,
                       int64_t row_stride, int64_t col_stride, const int32_t *boxes, size_t n, int64_t *count_out,
                       float *stats_out) {
  if (!c || (n && (!count_out || !stats_out))) KC_FAIL(KC_ERR_INVALID, "null argument");
  KC_TRY(depth_stats(c, img, data_on_device, rows, cols, row_stride, col_stride, boxes, n));
  for (size_t i = 0; i < n; ++i) {
    const DepthStats &s = c->stats[i];
    count_out[i] = s.count;
    stats_out[4 * i] = s.median;
    stats_out[4 * i + 1] = s.mad;
    stats_out[4 * i + 2] = s.min_d;
    stats_out[4 * i + 3] = s.max_d;
  }
  return KC_OK;
}

int kc_depth_boxes(kc_depth *c, const uint16_t *img, int data_on_device, int64_t rows, int64_t cols,
                   int64_t row_stride, int64_t col_stride, const int32_t *boxes, size_t n, const double *state,
                   float *out, int32_t *kept_index, size_t cap, size_t *count_out) {
  if (!c || !count_out || (n && (!out || !kept_index))) KC_FAIL(KC_ERR_INVALID, "null argument");
  *count_out = 0;
  if (cap < n) KC_FAIL(KC_ERR_RANGE, "room for %zu boxes, %zu given", cap, n);
  // updateBoxes: a state replaces body_in_world, none keeps it (depth_detector.cpp:54-56)
  if (state) c->body_in_world = hm::Rigid3f::from_pose2d(state[0], state[1], state[2]);
  KC_TRY(depth_stats(c, img, data_on_device, rows, cols, row_stride, col_stride, boxes, n));
  const hm::Rigid3f cam = c->body_in_world * c->camera_in_body;
  size_t m = 0;
  for (size_t i = 0; i < n; ++i) {
    const DepthStats &s = c->stats[i];
    if (s.count <= 1) continue;  // LOG_WARNING + dropped (:100-103): the host surface logs it
    const int32_t tx = boxes[4 * i], ty = boxes[4 * i + 1], sx = boxes[4 * i + 2], sy = boxes[4 * i + 3];
    const float med = s.median;
    // :119-150, expression by expression
    const float x_opt = (static_cast<float>(tx) + 0.5f * static_cast<float>(sx) - c->cx) * med / c->fx;
    const float y_opt = (static_cast<float>(ty) + 0.5f * static_cast<float>(sy) - c->cy) * med / c->fy;
    const float z_opt = med;
    const float size_x_opt = static_cast<float>(sx) * med / c->fx;
    const float size_y_opt = static_cast<float>(sy) * med / c->fy;
    const float sz[3] = {s.max_d - s.min_d, size_x_opt, size_y_opt};
    float *o = out + 6 * m;
    cam.apply(z_opt, -x_opt, -y_opt, o);
    for (int r = 0; r < 3; ++r)
      o[3 + r] = hm::add3(std::fabs(cam.R[r][0]) * sz[0], std::fabs(cam.R[r][1]) * sz[1],
                          std::fabs(cam.R[r][2]) * sz[2]);
    kept_index[m++] = static_cast<int32_t>(i);
  }
  *count_out = m;
  return KC_OK;
}

int kc_depth_after_stream(kc_depth *c, void *stream) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  KC_TRY(depth_ready(c));
  return stream_wait_for(c->device, c->stream, stream);
}

int kc_depth_last_upload(kc_depth *c, size_t *bytes_out) {
  if (!c || !bytes_out) KC_FAIL(KC_ERR_INVALID, "null argument");
  *bytes_out = c->last_upload;
  return KC_OK;
}

int kc_depth_timing_enable(kc_depth *c, int enable) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  c->timing.enabled = enable != 0;
  return KC_OK;
}

int kc_depth_timing_get(kc_depth *c, const char **names, float *ms, size_t cap, size_t *count) {
  if (!c) KC_FAIL(KC_ERR_INVALID, "null context");
  if (!c->stream) {
    if (count) *count = 0;
    return KC_OK;
  }
  KC_HIP(hipSetDevice(c->device));
  return c->timing.get(names, ms, cap, count);
}

}  // extern "C"
