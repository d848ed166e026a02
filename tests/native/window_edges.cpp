// CPU check of hm::build_window_lattice (csrc/kc_hostmath.h) against the oracle's ko_sample_velocities
// (oracle/kompass_oracle.c) at the edges of the velocity window: every case and all three control types, the lattice
// expanded to its (vx, vy, omega) list, count and every value compared as bit patterns, the index tables checked
// against the value tables -- once into a fresh lattice and once into one that still holds the previous case (the
// reuse path: value tables rewritten, index tables kept while the signature stays).  Where a case has a count that
// follows from the rules by hand (a zero window, an empty axis, |v| = kMinVel kept, the value below it dropped) that
// count is required of the oracle's list too, so a case cannot drift away from the edge it is named after.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "kc_hostmath.h"
#include "kompass_oracle.h"

using namespace kc;

static long checks = 0, bad = 0;

static void fail(const std::string &what, int ctr, const char *how, const char *detail) {
  ++bad;
  if (bad <= 20) std::printf("%s, ctr %d, %s: %s\n", what.c_str(), ctr, how, detail);
}

struct Window {
  double lim[10];  // vx max / acc / dec, vy max / acc / dec, omega max angle / max / acc / dec
  double cvx, cvy, com, dt;
  int max_lin, max_ang;
};

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

static kc_limits kc_of(const Window &w) {
  kc_limits L{};
  L.vx_max = w.lim[0]; L.vx_acc = w.lim[1]; L.vx_dec = w.lim[2];
  L.vy_max = w.lim[3]; L.vy_acc = w.lim[4]; L.vy_dec = w.lim[5];
  L.omega_max_angle = w.lim[6]; L.omega_max = w.lim[7]; L.omega_acc = w.lim[8]; L.omega_dec = w.lim[9];
  return L;
}
static ko_limits ko_of(const Window &w) {
  ko_limits L{};
  L.vx_max = w.lim[0]; L.vx_acc = w.lim[1]; L.vx_dec = w.lim[2];
  L.vy_max = w.lim[3]; L.vy_acc = w.lim[4]; L.vy_dec = w.lim[5];
  L.omega_max_angle = w.lim[6]; L.omega_max = w.lim[7]; L.omega_acc = w.lim[8]; L.omega_dec = w.lim[9];
  return L;
}

struct OracleList {
  std::vector<double> vx, vy, om;
  long n = 0;
};
static OracleList oracle_list(int ctr, const Window &w) {
  OracleList o;
  const size_t cap = size_t(1) << 18;
  o.vx.resize(cap); o.vy.resize(cap); o.om.resize(cap);
  const ko_limits L = ko_of(w);
  o.n = ko_sample_velocities(ctr, &L, w.cvx, w.cvy, w.com, w.dt, w.max_lin, w.max_ang, o.vx.data(), o.vy.data(), o.om.data(), cap);
  return o;
}

// one lattice against the oracle's list: count, every value as bits, every index inside its table
static void compare(const std::string &what, int ctr, const char *how, const hm::VelocityLattice &lat, const OracleList &o) {
  ++checks;
  char buf[200];
  if (o.n < 0) return fail(what, ctr, how, "the oracle's buffer overflowed");
  const size_t n = lat.size();
  if (lat.ix.size() != n || lat.iy.size() != n) return fail(what, ctr, how, "ix / iy / row differ in length");
  if (n != static_cast<size_t>(o.n)) {
    std::snprintf(buf, sizeof buf, "%zu samples, the oracle has %ld", n, o.n);
    return fail(what, ctr, how, buf);
  }
  if (n > 0 && lat.signature == 0) return fail(what, ctr, how, "a window lattice with samples and no signature");
  for (size_t i = 0; i < n; ++i) {
    if (lat.ix[i] >= lat.vx_values.size() || lat.iy[i] >= lat.vy_values.size() || lat.row[i] < 0 ||
        static_cast<size_t>(lat.row[i]) >= lat.omega_values.size()) {
      std::snprintf(buf, sizeof buf, "sample %zu indexes outside its tables (%u / %zu, %u / %zu, %d / %zu)", i, unsigned(lat.ix[i]),
                    lat.vx_values.size(), unsigned(lat.iy[i]), lat.vy_values.size(), int(lat.row[i]), lat.omega_values.size());
      return fail(what, ctr, how, buf);
    }
    if (!same_bits(lat.vx(i), o.vx[i]) || !same_bits(lat.vy(i), o.vy[i]) || !same_bits(lat.omega(i), o.om[i])) {
      std::snprintf(buf, sizeof buf, "sample %zu is (%.17g, %.17g, %.17g), the oracle's (%.17g, %.17g, %.17g)", i, lat.vx(i), lat.vy(i),
                    lat.omega(i), o.vx[i], o.vy[i], o.om[i]);
      return fail(what, ctr, how, buf);
    }
  }
}

static hm::VelocityLattice reused;  // holds the previous case, whatever its control type was

// -> the oracle's sample count; expect >= 0: the count the rules give by hand
static long run(const std::string &what, int ctr, const Window &w, long expect = -1) {
  const OracleList o = oracle_list(ctr, w);
  const kc_limits L = kc_of(w);
  hm::VelocityLattice fresh;
  hm::build_window_lattice(ctr, L, w.cvx, w.cvy, w.com, w.dt, w.max_lin, w.max_ang, fresh);
  compare(what, ctr, "fresh", fresh, o);
  hm::build_window_lattice(ctr, L, w.cvx, w.cvy, w.com, w.dt, w.max_lin, w.max_ang, reused);
  compare(what, ctr, "reused", reused, o);
  ++checks;
  if (reused.signature != fresh.signature || reused.ix != fresh.ix || reused.iy != fresh.iy || reused.row != fresh.row)
    fail(what, ctr, "reused", "signature or index tables differ from the fresh lattice's");
  if (expect >= 0) {
    ++checks;
    if (o.n != expect) {
      char buf[100];
      std::snprintf(buf, sizeof buf, "the oracle has %ld samples, the rules give %ld", o.n, expect);
      fail(what, ctr, "case", buf);
    }
  }
  return o.n;
}

static size_t distinct(const std::vector<double> &v, long n) {
  std::vector<double> seen;
  for (long i = 0; i < n; ++i) {
    bool have = false;
    for (double s : seen) have = have || same_bits(s, v[i]);
    if (!have) seen.push_back(v[i]);
  }
  return seen.size();
}

int main() {
  const int ACK = KO_ACKERMANN, DIFF = KO_DIFFERENTIAL_DRIVE, OMNI = KO_OMNI;
  // vx (1, 2, 2), vy (1, 2, 2), omega (2, 2, 3, 3), dt 0.1: a window of +-0.2 m/s and +-0.3 rad/s
  const Window base{{1.0, 2.0, 2.0, 1.0, 2.0, 2.0, 2.0, 2.0, 3.0, 3.0}, 0.5, 0.1, 0.2, 0.1, 7, 5};
  auto all = [&](const std::string &what, const Window &w, long e_ack = -1, long e_diff = -1, long e_omni = -1) {
    run(what, ACK, w, e_ack);
    run(what, DIFF, w, e_diff);
    run(what, OMNI, w, e_omni);
  };
  all("plain window", base, 7 * 5, 7 * 5);

  {  // no acceleration at all: ranges of zero, steps clamped at 0.001, one value an axis
    Window w = base;
    w.lim[1] = w.lim[2] = w.lim[4] = w.lim[5] = w.lim[8] = w.lim[9] = 0.0;
    all("zero window", w, 1, 1, 2);          // omni: (vx, vy, 0) and (vx, 0, omega)
    w.cvx = 0.0;                                   // ... around a standing robot: vx = 0 is "zero"
    all("zero window at rest", w, 0, 0, 1);  // omni: (0, 0.1, 0) stays, vy is not small
    w.cvy = 0.0;
    all("zero window, all three zero", w, 0, 0, 0);
  }
  {  // the velocity outside the limits by more than the window: min > max, an empty axis
    Window w = base;
    w.cvx = 1.5;
    all("vx above the limit", w, 0, 0, 0);
    w.cvx = -1.5;
    all("vx below the limit", w, 0, 0, 0);
    w = base;
    w.com = 3.0;
    all("omega above the limit", w, 0, 0);  // (omni keeps its (vx, vy, 0) samples)
    w.com = -3.0;
    all("omega below the limit", w, 0, 0);
    w = base;
    w.cvy = 1.5;
    all("vy above the limit", w, 7 * 5, 7 * 5);  // (only omni has a vy axis)
  }
  {  // clipped by +max and by -max, every axis
    Window w = base;
    w.cvx = 0.95; w.cvy = 0.9; w.com = 1.9;
    all("clipped by +max", w);
    w.cvx = -0.95; w.cvy = -0.9; w.com = -1.9;
    all("clipped by -max", w);
    w.cvx = 1.0; w.cvy = 1.0; w.com = 2.0;  // exactly on the limit
    all("on +max", w);
    w.cvx = 1.1; w.cvy = 1.1; w.com = 2.2;  // outside by less than the window
    all("outside by less than the window", w);
  }
  {  // one omega: ang_n = 1, the step is x / 0
    Window w = base;
    w.max_ang = 1;
    all("single omega, inf step", w, 7, 7);
    w.lim[8] = w.lim[9] = 0.0;  // 0 / 0: a NaN step, which the clamp at 0.001 lets through
    all("single omega, NaN step", w, 7, 7);
    w.com = 0.0;  // ... and the one omega is zero
    all("single omega of zero, NaN step", w, 7, 7);
    for (int ctr = 0; ctr < 3; ++ctr) {
      const OracleList o = oracle_list(ctr, w);
      ++checks;
      if (distinct(o.om, o.n) != 1) fail("single omega of zero", ctr, "case", "more than one omega in the oracle's list");
    }
  }
  // the smallest counts (max(3, ...)), even counts (the odd rule), the omni 3/4 to 1/4 split
  for (int ml : {1, 2, 3, 4, 5, 6, 8, 9, 12, 16})
    for (int ma : {1, 2, 3, 4}) {
      Window w = base;
      w.max_lin = ml;
      w.max_ang = ma;
      const std::string what = "counts " + std::to_string(ml) + " x " + std::to_string(ma);
      all(what, w);
      // by hand: an axis of k values takes k - 1 steps of range / (k - 1); the repeated addition of that rounded step may
      // pass the upper limit by an ulp, so the axis holds k values or k - 1, never another number.  No value of this
      // window is small, so the list is the full product.
      const size_t nx = static_cast<size_t>(std::max(3, ml) | 1), na = static_cast<size_t>(ma | 1);
      for (int ctr : {ACK, DIFF}) {
        const OracleList o = oracle_list(ctr, w);
        const size_t dx = distinct(o.vx, o.n), da = distinct(o.om, o.n);
        ++checks;
        if (!(dx == nx || dx + 1 == nx) || !(da == na || da + 1 == na) || static_cast<size_t>(o.n) != dx * da)
          fail(what, ctr, "case", "axis counts outside what the split and odd rules give");
      }
    }
  {
    // omni by hand: max_lin 3 -> (2 -> 3, 0 -> 3), 4 -> (3, 1 -> 3), 5 -> (3, 1 -> 3), 16 -> (12 -> 13, 4 -> 5); the window
    // [0.3, 0.7] x [-0.07, 0.33] holds no small vx and no vy of exactly zero
    for (int ml : {3, 4, 5, 16}) {
      Window w = base;
      w.cvy = 0.13;
      w.max_lin = ml;
      w.max_ang = 3;
      const OracleList o = oracle_list(OMNI, w);
      const size_t nx = ml == 16 ? 13 : 3, ny = (ml == 16 ? 5 : 3) + 1;  // (+ the 0.0 of the (vx, 0, omega) samples)
      ++checks;
      if (distinct(o.vx, o.n) != nx || distinct(o.vy, o.n) != ny) fail("omni split " + std::to_string(ml), OMNI, "case", "axis counts");
    }
  }
  {  // vx_max at kMinVel: the axis ends at exactly +-0.01, which is kept (|v| < kMinVel is false) ...
    Window w = base;
    w.cvx = 0.0; w.cvy = 0.0; w.com = 0.0;
    w.lim[0] = 0.01;
    w.max_lin = 3;
    all("vx_max = kMinVel", w, 2 * 5, 2 * 5);  // -0.01 and 0.01 with 5 omegas each; 0 has no omega block
    w.lim[0] = std::nextafter(0.01, 0.0);  // ... and one value below it is dropped
    all("vx_max below kMinVel", w, 0, 0);
    w.lim[0] = std::nextafter(0.01, 1.0);
    all("vx_max above kMinVel", w, 2 * 5, 2 * 5);
    w.lim[0] = 1.0;  // the same three on the vy axis
    w.lim[3] = 0.01;
    w.max_lin = 4;  // omni: 3 x 3
    all("vy_max = kMinVel", w);
    w.lim[3] = std::nextafter(0.01, 0.0);
    all("vy_max below kMinVel", w);
    w.lim[7] = 0.01;  // and on omega, where "small" never drops a sample of a non-small vx
    all("omega_max = kMinVel", w);
  }
  {  // omni axes near zero: both hold several values below kMinVel; (v, w, 0) goes only where both are small
    Window w = base;
    w.cvx = 0.0; w.cvy = 0.0; w.com = 0.0;
    w.lim[1] = w.lim[2] = w.lim[4] = w.lim[5] = 0.2;  // +-0.02 m/s
    w.max_lin = 16;  // 13 x 5
    all("omni axes near zero", w);
    const OracleList o = oracle_list(OMNI, w);
    // by hand: x = -0.02 + k / 300 (k < 13) is small for k = 4 .. 8, y = -0.02 + 0.01 k (k < 5) for k = 2 and perhaps 1, 3
    // (repeated addition decides): small x values appear with the large y values only, large x values with every y
    long sx = 0, sy = 0, both = 0;
    for (long i = 0; i < o.n; ++i) {
      sx += std::fabs(o.vx[i]) < 0.01;
      sy += std::fabs(o.vx[i]) >= 0.01 && std::fabs(o.vy[i]) < 0.01 && o.om[i] == 0.0;
      both += std::fabs(o.vx[i]) < 0.01 && std::fabs(o.vy[i]) < 0.01;
    }
    ++checks;
    if (sx < 5 * 2 || sy < 6 || both != 0) fail("omni axes near zero", OMNI, "case", "the window was meant to hold small values on both axes");
    w.cvx = 0.004; w.cvy = -0.003;
    all("omni axes near zero, off centre", w);
    w.max_lin = 40;  // 31 x 11
    all("omni axes near zero, fine", w);
  }
  // a sweep of vx through zero: values cross |v| = kMinVel, the count changes
  for (int ctr = 0; ctr < 3; ++ctr) {
    Window w = base;
    w.max_lin = 31;
    w.max_ang = 3;
    w.cvy = 0.0;
    long last = -1;
    int changes = 0;
    for (int k = -50; k <= 50; ++k) {
      w.cvx = k * 1e-3;
      const long n = run("sweep through zero, k = " + std::to_string(k), ctr, w);
      changes += last >= 0 && n != last;
      last = n;
    }
    ++checks;
    if (changes < 4) fail("sweep through zero", ctr, "case", "the sample count changed fewer than four times");
    std::printf("sweep through zero, ctr %d: %d changes of the count\n", ctr, changes);
  }
  {  // limits with -0.0: -(-0.0) = +0.0 is the lower limit
    Window w = base;
    w.cvx = 0.0; w.cvy = 0.0; w.com = 0.0;
    w.lim[0] = -0.0;
    all("vx_max = -0.0", w, 0, 0);
    w.lim[3] = -0.0;
    all("vx_max = vy_max = -0.0", w, 0, 0, 0);
    w = base;
    w.lim[7] = -0.0;
    w.com = 0.0;
    all("omega_max = -0.0", w, 7, 7);
    w.com = -0.0;
    w.cvx = -0.0;
    all("omega_max = -0.0, velocity -0.0", w);
    w = base;
    w.lim[1] = w.lim[2] = w.lim[4] = w.lim[5] = w.lim[8] = w.lim[9] = -0.0;
    all("accelerations of -0.0", w, 1, 1, 2);
    w.cvx = -0.0; w.cvy = -0.0; w.com = -0.0;
    all("accelerations and velocity of -0.0", w, 0, 0, 0);
  }
  {  // a float-narrowed time step
    Window w = base;
    w.dt = static_cast<double>(0.05f);
    all("dt = 0.05f", w);
    w.cvx = 0.003;
    w.max_lin = 31;
    all("dt = 0.05f through zero", w);
    w.dt = static_cast<double>(0.1f);
    all("dt = 0.1f through zero", w);
  }
  std::printf("window edges: %ld checks, %ld bad\n", checks, bad);
  return bad ? 1 : 0;
}
