// Error string, device probing and key helpers of libkompass_hip.so, and the host side of kc_q16.h's integers: the
// heading table, the table checks and uploads that the localiser and the MPPI controller share.
#include <cmath>

#include "kc_internal.h"

namespace kc {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int open_device_stream(int device, hipStream_t *stream) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess) {
    (void)hipGetLastError();
    ndev = 0;
  }
  if (device < 0 || device >= ndev) KC_FAIL(KC_ERR_HIP, "HIP device %d not available (%d visible)", device, ndev);
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    *stream = nullptr;
    KC_FAIL(KC_ERR_HIP, "HIP stream creation failed on device %d", device);
  }
  return KC_OK;
}

// Every kc_*_destroy calls this (and ends its other streams) BEFORE it deletes the context: the context's
// DevBuf / PinBuf / OrderEvent / Timing members free themselves in its destructor, with this device current, and
// nothing queued may still read or write them then.
void close_device_stream(int device, hipStream_t *stream) {
  // (a context exists only once its stream is open, so the device is current for whatever its destroy ends next;
  // kc_depth, which opens lazily, has nothing on the device while it has no stream)
  if (!*stream) return;
  hipError_t e = hipSetDevice(device);
  e = hipStreamSynchronize(*stream);
  e = hipStreamDestroy(*stream);
  (void)e;
  *stream = nullptr;
}

int stream_wait_for(int device, hipStream_t own, void *other) {
  KC_HIP(hipSetDevice(device));
  hipEvent_t e = nullptr;
  KC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  hipError_t rc = hipEventRecord(e, static_cast<hipStream_t>(other));
  if (rc == hipSuccess) rc = hipStreamWaitEvent(own, e, 0);
  (void)hipEventDestroy(e);  // released once the wait is satisfied
  KC_HIP(rc);
  return KC_OK;
}

int stream_wait_through(OrderEvent &ev, hipStream_t own, hipStream_t producer) {
  if (own == producer) return KC_OK;
  if (!ev.e) KC_HIP(hipEventCreateWithFlags(&ev.e, hipEventDisableTiming));
  KC_HIP(hipEventRecord(ev.e, producer));
  KC_HIP(hipStreamWaitEvent(own, ev.e, 0));
  return KC_OK;
}

int check_device_range(int device, const void *ptr, long long lo_bytes, long long hi_bytes, size_t align,
                       const char *what) {
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
    (void)hipGetLastError();
    KC_FAIL(KC_ERR_INVALID, "the device %s %p is not memory HIP knows", what, ptr);
  }
  if (at.type != hipMemoryTypeDevice)
    KC_FAIL(KC_ERR_INVALID, "the device %s is not device memory (HIP memory type %d)", what, static_cast<int>(at.type));
  if (at.device != device)
    KC_FAIL(KC_ERR_INVALID, "the device %s lives on device %d, the context reads device %d", what, at.device, device);
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void *>(ptr)) != hipSuccess) {
    (void)hipGetLastError();
    KC_FAIL(KC_ERR_INVALID, "no allocation holds the device %s", what);
  }
  // offsets from the allocation's base, compared without forming an address: nothing here can wrap
  const uintptr_t p = reinterpret_cast<uintptr_t>(ptr), b = reinterpret_cast<uintptr_t>(base);
  const unsigned long long below = 0ull - static_cast<unsigned long long>(lo_bytes);  // |lo_bytes| where lo_bytes <= 0
  if (lo_bytes > 0 || hi_bytes < 0 || p < b || p - b > size || below > p - b ||
      static_cast<unsigned long long>(hi_bytes) > size - (p - b))
    KC_FAIL(KC_ERR_INVALID, "the device %s (bytes %lld to %lld from its pointer) runs outside its %zu-byte allocation", what, lo_bytes,
            hi_bytes, size);
  if (align > 1 && p % align) KC_FAIL(KC_ERR_INVALID, "the device %s is not aligned to %zu bytes", what, align);
  return KC_OK;
}

double (*volatile host_cos)(double) = static_cast<double (*)(double)>(std::cos);
double (*volatile host_sin)(double) = static_cast<double (*)(double)>(std::sin);

const int2 *heading_table() {
  static const std::vector<int2> table = [] {
    std::vector<int2> t(65536);
    for (int h = 0; h < 65536; ++h) {
      const double a = 2.0 * M_PI * static_cast<double>(h) / 65536.0;
      t[h] = make_int2(static_cast<int>(std::lrint(host_cos(a) * 65536.0)), static_cast<int>(std::lrint(host_sin(a) * 65536.0)));
    }
    return t;
  }();
  return table.data();
}

int upload_heading_table(DevBuf<int2> &d, hipStream_t s) {
  KC_TRY(d.reserve(65536));
  hipError_t he = hipMemcpyAsync(d.p, heading_table(), 65536 * sizeof(int2), hipMemcpyHostToDevice, s);
  if (he == hipSuccess) he = hipStreamSynchronize(s);
  if (he != hipSuccess) KC_FAIL(KC_ERR_HIP, "the heading table's upload failed: %s", hipGetErrorString(he));
  return KC_OK;
}

int check_weight_table(const uint32_t *wtab, size_t EW, int w_shift, int cap) {
  if (EW == 0) KC_FAIL(KC_ERR_INVALID, "an empty weight table");
  if (EW > static_cast<size_t>(cap)) KC_FAIL(KC_ERR_RANGE, "%zu weight entries are above the cap of %d", EW, cap);
  if (w_shift < 0 || w_shift > 30) KC_FAIL(KC_ERR_INVALID, "w_shift must be in 0 .. 30, got %d", w_shift);
  if (wtab[0] < 1u || wtab[0] > (1u << 20)) KC_FAIL(KC_ERR_INVALID, "wtab[0] must be in 1 .. 2^20, got %u", wtab[0]);
  for (size_t i = 1; i < EW; ++i)
    if (wtab[i] > wtab[i - 1]) KC_FAIL(KC_ERR_INVALID, "the weight table increases at entry %zu", i);
  return KC_OK;
}

int check_reach(size_t n_pen, int reach) {
  if (reach == 0) return KC_OK;
  if (reach < 1 || reach > KC_WORLDMAP_DIST_MAX_REACH)
    KC_FAIL(KC_ERR_RANGE, "reach must be in 1 .. %d cells, got %d", KC_WORLDMAP_DIST_MAX_REACH, reach);
  if (n_pen - 1 > static_cast<size_t>(reach) * static_cast<size_t>(reach))
    KC_FAIL(KC_ERR_INVALID, "c2 = %zu is above reach^2 = %d", n_pen - 1, reach * reach);
  return KC_OK;
}

int upload_tables(DevBuf<unsigned short> &d_pen, const uint16_t *pen, size_t n_pen, DevBuf<unsigned> &d_wtab, const uint32_t *wtab,
                  size_t n_wtab, hipStream_t s) {
  KC_TRY(d_pen.reserve(n_pen));
  KC_TRY(d_wtab.reserve(n_wtab));
  KC_HIP(hipMemcpyAsync(d_pen.p, pen, n_pen * sizeof(uint16_t), hipMemcpyHostToDevice, s));
  KC_HIP(hipMemcpyAsync(d_wtab.p, wtab, n_wtab * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  KC_HIP(hipStreamSynchronize(s));
  return KC_OK;
}

}  // namespace kc

extern "C" {

const char *kc_last_error(void) { return kc::g_err; }

int kc_abi_version(void) { return KC_ABI_VERSION; }

int kc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

float kc_key_cost(int64_t key) {
  return kc::sortable_float(static_cast<int32_t>(key >> 32));
}
int64_t kc_key_index(int64_t key) {
  return static_cast<int64_t>(static_cast<uint32_t>(key & 0xFFFFFFFFll));
}
int64_t kc_key_pack(float cost, int64_t index) {
  if (!(cost < 3.402823466e+38f)) return kc::KEY_NONE;
  return kc::key_pack(cost, static_cast<uint32_t>(index));
}

}  // extern "C"
