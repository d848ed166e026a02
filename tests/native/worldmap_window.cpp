// Stand-alone caller of kc_worldmap_window (DESIGN.md 4.11 rule 16) over its edge cases, for a host-side sanitizer run
// of the quantisation: half-way positions, the 2^20-cell and 2048-cell caps from both sides, non-finite and denormal
// arguments.  Needs no device.  kc_worldmap.hip's other entries reach into the mapper's translation unit; the one
// symbol they need is stubbed here so that two translation units suffice:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined
//         -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Ikompass-core_amd/csrc
//         kompass-core_amd/csrc/kc_worldmap.hip kompass-core_amd/csrc/kc_common.hip tests/native/worldmap_window.cpp
//         -o worldmap_window && ./worldmap_window
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "kc_internal.h"
#include "kompass_hip.h"

namespace kc {
int mapper_view(kc_mapper *, MapperView *) { return KC_ERR_UNSUPPORTED; }
}  // namespace kc

static int failures = 0;

static void expect(int want_rc, float res, double ox, double oy, double x, double y, float range, int ic = 0, int jc = 0,
                   int rc = 0) {
  int32_t gi = -7, gj = -7, gr = -7;
  const int got = kc_worldmap_window(res, ox, oy, x, y, range, &gi, &gj, &gr);
  const bool ok = got == want_rc && (want_rc != KC_OK ? (gi == 0 && gj == 0 && gr == 0) : (gi == ic && gj == jc && gr == rc));
  if (!ok) {
    ++failures;
    std::printf("FAIL res %g origin (%g, %g) at (%g, %g) range %g: rc %d (%d, %d, %d), wanted rc %d (%d, %d, %d)\n",
                static_cast<double>(res), ox, oy, x, y, static_cast<double>(range), got, gi, gj, gr, want_rc, ic, jc, rc);
  }
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  const float finf = std::numeric_limits<float>::infinity(), fnan = std::nanf("");
  // exact arithmetic: resolution 0.25, positions on cell centres and half-way between them
  expect(KC_OK, 0.25f, 0.0, 0.0, 0.0, 0.0, 1.0f, 0, 0, 4);
  expect(KC_OK, 0.25f, 0.0, 0.0, 0.125, -0.125, 1.0f, 1, 0, 4);
  expect(KC_OK, 0.25f, 0.0, 0.0, -0.375, 0.625, 1.0f, -1, 3, 4);
  expect(KC_OK, 0.25f, 1.0, -2.0, 0.0, 0.0, 1.0f, -4, 8, 4);
  expect(KC_OK, 0.25f, 0.0, 0.0, 0.0, 0.0, std::nextafterf(1.0f, 2.0f), 0, 0, 5);
  expect(KC_OK, 0.25f, 0.0, 0.0, 0.0, 0.0, std::nextafterf(1.0f, 0.0f), 0, 0, 4);
  expect(KC_OK, 0.25f, 0.0, 0.0, 0.0, 0.0, FLT_MIN, 0, 0, 1);
  expect(KC_OK, 0.25f, 0.0, 0.0, 0.0, 0.0, std::numeric_limits<float>::denorm_min(), 0, 0, 1);
  // the caps, from both sides
  expect(KC_OK, 0.25f, 0.0, 0.0, 0.0, 0.0, 512.0f, 0, 0, 2048);
  expect(KC_ERR_RANGE, 0.25f, 0.0, 0.0, 0.0, 0.0, std::nextafterf(512.0f, 600.0f));
  expect(KC_ERR_RANGE, 0.25f, 0.0, 0.0, 0.0, 0.0, FLT_MAX);
  expect(KC_ERR_RANGE, FLT_MIN, 0.0, 0.0, 0.0, 0.0, FLT_MAX);  // the quotient overflows to infinity
  expect(KC_OK, 0.25f, 0.0, 0.0, 262144.0, -262144.0, 1.0f, 1 << 20, -(1 << 20), 4);
  expect(KC_ERR_RANGE, 0.25f, 0.0, 0.0, 262144.25, 0.0, 1.0f);
  expect(KC_ERR_RANGE, 0.25f, 0.0, 0.0, 0.0, -262144.25, 1.0f);
  expect(KC_ERR_RANGE, 0.25f, 0.0, 0.0, 1e300, 0.0, 1.0f);
  expect(KC_ERR_RANGE, FLT_MIN, 0.0, 0.0, 1.0, 0.0, FLT_MIN);   // (x - origin) / resolution overflows
  // refusals
  expect(KC_ERR_INVALID, 0.25f, 0.0, 0.0, 0.0, 0.0, 0.0f);
  expect(KC_ERR_INVALID, 0.25f, 0.0, 0.0, 0.0, 0.0, -1.0f);
  expect(KC_ERR_INVALID, 0.25f, 0.0, 0.0, 0.0, 0.0, fnan);
  expect(KC_ERR_INVALID, 0.25f, 0.0, 0.0, 0.0, 0.0, finf);
  expect(KC_ERR_INVALID, 0.25f, 0.0, 0.0, nan, 0.0, 1.0f);
  expect(KC_ERR_INVALID, 0.25f, 0.0, 0.0, 0.0, inf, 1.0f);
  expect(KC_ERR_INVALID, 0.25f, -inf, 0.0, 0.0, 0.0, 1.0f);
  expect(KC_ERR_INVALID, 0.0f, 0.0, 0.0, 0.0, 0.0, 1.0f);
  expect(KC_ERR_INVALID, -0.25f, 0.0, 0.0, 0.0, 0.0, 1.0f);
  expect(KC_ERR_INVALID, fnan, 0.0, 0.0, 0.0, 0.0, 1.0f);
  if (kc_worldmap_window(0.25f, 0.0, 0.0, 0.0, 0.0, 1.0f, nullptr, nullptr, nullptr) != KC_ERR_INVALID) ++failures;
  // a sweep across many half-way points either side of the origin: the shift must floor, never trap
  for (int k = -4000; k <= 4000; ++k) {
    const double x = 0.125 * k;  // every half cell
    int32_t gi = 0, gj = 0, gr = 0;
    if (kc_worldmap_window(0.25f, 0.0, 0.0, x, -x, 1.0f, &gi, &gj, &gr) != KC_OK) ++failures;
    const int want_i = static_cast<int>(std::floor(x / 0.25 + 0.5)), want_j = static_cast<int>(std::floor(-x / 0.25 + 0.5));
    if (gi != want_i || gj != want_j || gr != 4) ++failures;
  }
  std::printf("worldmap_window: %d failure(s)\n", failures);
  return failures ? 1 : 0;
}
