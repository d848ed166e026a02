// CPU check of csrc/kc_scan_tables.h: the four-beams-at-a-time forms of kc_dwa_set_scan's host loops give the
// bits of the scalar forms (which restate collision_check.h:110-115 and cost_evaluator.h:174-193), for every
// list length around the vector width, with non-finite ranges, zero ranges and signed zeros, and with finite ranges
// too large for a float.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "kc_scan_tables.h"

using namespace kc;

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

int main() {
  if (!segtab::cpu_has_avx2()) {
    std::printf("no AVX2 on this CPU: nothing to compare, 0 bad\n");
    return 0;
  }
  std::mt19937_64 g(7);
  std::uniform_real_distribution<double> ur(0.0, 12.0), ua(-3.2, 3.2);
  int bad = 0, cases = 0;
  for (int rep = 0; rep < 400; ++rep) {
    const size_t n = rep < 40 ? static_cast<size_t>(rep) : 1 + g() % 5000;
    std::vector<double> r(n), c(n), s(n);
    for (size_t i = 0; i < n; ++i) {
      const double a = ua(g);
      r[i] = ur(g);
      c[i] = std::cos(a);
      s[i] = std::sin(a);
    }
    if (n > 3 && rep % 3 == 0) r[g() % n] = 0.0;
    if (n > 3 && rep % 5 == 0) r[g() % n] = -0.0;
    const bool poison = n > 0 && rep % 7 == 0;
    if (poison) r[g() % n] = (rep % 14 == 0) ? std::numeric_limits<double>::infinity() : std::nan("");
    scantab::Place p{};
    const float yaw = static_cast<float>(ua(g));
    p.r00 = std::cos(yaw); p.r01 = -std::sin(yaw); p.r10 = std::sin(yaw); p.r11 = std::cos(yaw);
    p.z0 = (rep % 2 ? 0.0f : -0.0f); p.z1 = 0.0f * p.r10;
    p.t0 = static_cast<float>(ua(g)); p.t1 = static_cast<float>(ua(g));
    const float hz = -0.125f;
    std::vector<float> xa(3 * n + 4, 7.f), xb(3 * n + 4, 7.f), hxa(n + 4, 7.f), hxb(n + 4, 7.f), hya(n + 4, 7.f), hyb(n + 4, 7.f);
    const bool fa = scantab::points_avx2(r.data(), c.data(), s.data(), n, hz, p, xa.data(), hxa.data(), hya.data());
    const bool fb = scantab::points_scalar(r.data(), c.data(), s.data(), 0, n, hz, p, xb.data(), hxb.data(), hyb.data());
    ++cases;
    if (fa != fb || fa == poison || !same_bits(xa, xb) || !same_bits(hxa, hxb) || !same_bits(hya, hyb)) {
      ++bad;
      std::printf("points differ at n = %zu (finite %d / %d)\n", n, fa, fb);
    }
    if (n > 0) {  // the boxes over the finite obstacles only (beams without a return), poisoned lists included
      std::vector<float> px(hxb), py(hyb);
      for (size_t i = 0; i < n; ++i)
        if (g() % 9 == 0) (g() % 2 ? px : py)[i] = (g() % 2) ? std::numeric_limits<float>::infinity() : std::nanf("");
      for (int k = 0; k < 20; ++k) {
        const size_t j0 = g() % n, j1 = j0 + g() % (n - j0 + 1);
        const scantab::Box a = scantab::box_finite_avx2(px.data(), py.data(), j0, j1);
        const scantab::Box b = scantab::box_finite_scalar(px.data(), py.data(), j0, j1, scantab::box_empty());
        ++cases;
        if (std::memcmp(&a, &b, sizeof(a)) != 0) {
          ++bad;
          std::printf("finite box differs at [%zu, %zu)\n", j0, j1);
        }
      }
    }
    if (!poison && n > 0) {
      for (int k = 0; k < 20; ++k) {
        const size_t j0 = g() % n, j1 = j0 + g() % (n - j0 + 1);
        const scantab::Box a = scantab::box_avx2(hxb.data(), hyb.data(), j0, j1);
        const scantab::Box b = scantab::box_scalar(hxb.data(), hyb.data(), j0, j1, scantab::box_empty());
        ++cases;
        if (std::memcmp(&a, &b, sizeof(a)) != 0) {
          ++bad;
          std::printf("box differs at [%zu, %zu)\n", j0, j1);
        }
      }
    }
  }
  // Finite ranges whose obstacles are not finite floats: 1e39 and DBL_MAX round to inf as floats, and a rotation
  // that adds +inf and -inf gives NaN.  (3e38 stays a finite float, and so does its rotated obstacle: it is a finite
  // obstacle among the others.)  The "every obstacle finite" flag must see the non-finite ones, in both forms, so that
  // the chunk boxes kc_dwa_set_scan builds (box_of when the flag is set, box_of_finite otherwise) hold every finite
  // obstacle of their chunk: a box that lost one would prune the chunk that holds the nearest obstacle.
  {
    const double huge[3] = {1e39, std::numeric_limits<double>::max(), 3e38};
    const double pi = std::acos(-1.0);
    for (int rep = 0; rep < 60; ++rep) {
      const size_t n = 64 + static_cast<size_t>(rep) * 37 % 900;
      std::vector<double> r(n), c(n), s(n);
      for (size_t i = 0; i < n; ++i) {
        const double a = -pi + 2.0 * pi * static_cast<double>(i) / static_cast<double>(n);
        r[i] = 0.5 + ur(g);
        c[i] = std::cos(a);
        s[i] = std::sin(a);
      }
      // a few huge beams, one of them at -45 degrees: x = +big, y = -big
      for (int k = 0; k < 3; ++k) r[g() % n] = huge[(rep + k) % 3];
      const size_t q = (3 * n) / 8;  // angle ~ -pi / 4
      r[q] = huge[rep % 3];
      scantab::Place p{};
      const float yaw = static_cast<float>(-pi / 6 + 0.01 * (rep % 7));  // r00, r01 > 0: +inf + -inf = NaN
      p.r00 = std::cos(yaw); p.r01 = -std::sin(yaw); p.r10 = std::sin(yaw); p.r11 = std::cos(yaw);
      p.z0 = 0.0f; p.z1 = 0.0f;
      p.t0 = 0.25f; p.t1 = -0.5f;
      std::vector<float> xa(3 * n), xb(3 * n), hxa(n), hxb(n), hya(n), hyb(n);
      const bool fa = scantab::points_avx2(r.data(), c.data(), s.data(), n, 0.0f, p, xa.data(), hxa.data(), hya.data());
      const bool fb = scantab::points_scalar(r.data(), c.data(), s.data(), 0, n, 0.0f, p, xb.data(), hxb.data(), hyb.data());
      ++cases;
      bool any_bad_float = false;
      for (size_t i = 0; i < n; ++i) any_bad_float |= !std::isfinite(hxb[i]) || !std::isfinite(hyb[i]);
      if (fa != fb || fa == any_bad_float || !any_bad_float || !same_bits(xa, xb) || !same_bits(hxa, hxb) ||
          !same_bits(hya, hyb)) {
        ++bad;
        std::printf("huge ranges: points differ at n = %zu (finite %d / %d, non-finite obstacle %d)\n", n, fa, fb,
                    any_bad_float);
      }
      const size_t cs = (n + 63) / 64;  // the chunks of kc_dwa_set_scan
      for (size_t j0 = 0; j0 < n; j0 += cs) {
        const size_t j1 = std::min(n, j0 + cs);
        const scantab::Box va = fa ? scantab::box_of(hxa.data(), hya.data(), j0, j1)
                                   : scantab::box_of_finite(hxa.data(), hya.data(), j0, j1);
        const scantab::Box vb = fb ? scantab::box_scalar(hxb.data(), hyb.data(), j0, j1, scantab::box_empty())
                                   : scantab::box_finite_scalar(hxb.data(), hyb.data(), j0, j1, scantab::box_empty());
        ++cases;
        bool holds = std::memcmp(&va, &vb, sizeof(va)) == 0;
        for (size_t j = j0; j < j1; ++j)
          if (std::isfinite(hxb[j]) && std::isfinite(hyb[j]))
            holds = holds && hxb[j] >= va.x0 && hxb[j] <= va.x1 && hyb[j] >= va.y0 && hyb[j] <= va.y1;
        if (!holds) {
          ++bad;
          std::printf("huge ranges: the box of chunk [%zu, %zu) misses a finite obstacle (n = %zu)\n", j0, j1, n);
        }
      }
    }
  }
  // The consequence itself, pinned: one chunk of 64 beams (4096 beams, kc_dwa_set_scan's chunking), the nearest
  // obstacle in lane 1 of the first eight-wide batch, NaN obstacles in lane 1 of every later batch.  _mm256_min_ps
  // returns its second operand when either is NaN, so box_avx2 fed NaN would forget the near obstacle.
  for (const double big : {1e39, std::numeric_limits<double>::max()}) {
    const size_t n = 4096, cs = 64, q = 1536;  // chunk 24: beams at -pi / 4 .. -pi / 4 + 5.6 degrees
    const double pi = std::acos(-1.0);
    std::vector<double> r(n, 1.0), c(n), s(n);
    for (size_t i = 0; i < n; ++i) {
      const double a = -pi + 2.0 * pi * static_cast<double>(i) / static_cast<double>(n);
      c[i] = std::cos(a);
      s[i] = std::sin(a);
    }
    for (size_t i = q; i < q + cs; ++i) r[i] = 3.0;
    r[q + 1] = 0.4;
    for (size_t i = q + 9; i < q + cs; i += 8) r[i] = big;
    scantab::Place p{};
    const float yaw = -0.5f;  // r00, r01 > 0: x = +inf, y = -inf gives hx = NaN
    p.r00 = std::cos(yaw); p.r01 = -std::sin(yaw); p.r10 = std::sin(yaw); p.r11 = std::cos(yaw);
    p.t0 = 0.05f; p.t1 = -0.02f;
    std::vector<float> xyz(3 * n), hx(n), hy(n);
    const bool f = scantab::points(r.data(), c.data(), s.data(), n, 0.0f, p, xyz.data(), hx.data(), hy.data());
    const scantab::Box b = f ? scantab::box_of(hx.data(), hy.data(), q, q + cs) : scantab::box_of_finite(hx.data(), hy.data(), q, q + cs);
    ++cases;
    if (!std::isnan(hx[q + 9]) || !(hx[q + 1] >= b.x0 && hx[q + 1] <= b.x1 && hy[q + 1] >= b.y0 && hy[q + 1] <= b.y1)) {
      ++bad;
      std::printf("range %g: the box of the chunk loses its nearest obstacle (%g, %g): [%g, %g] x [%g, %g]\n", big,
                  hx[q + 1], hy[q + 1], b.x0, b.x1, b.y0, b.y1);
    }
  }
  std::printf("%d cases, %d bad\n", cases, bad);
  return bad ? 1 : 0;
}
