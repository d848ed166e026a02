// Sample patterns of the DWA host path: which pattern's tables are active and which are kept (find_pattern), and the two
// orders the roll-out kernels walk a shard in (order_by_row, deal_order) -- plain host arithmetic, carried out by
// upload_samples / build_perm in kc_dwa.hip.  Host-only like kc_launch_plan.h: no HIP include, compiles with plain g++
// (tests/native/sample_pattern.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace kc {

// The host side of a pattern's tables (kc_dwa::PatternTables adds the device buffers).
struct PatternHost {
  uint64_t sig = 0;    // signature / size of the pattern whose index tables the device buffers hold
  size_t n = 0;
  uint64_t stamp = 0;  // last use (of a kept slot)
  std::vector<int32_t> h_perm, h_dealt;  // the two walking orders: by trig row, and dealt for the single-launch cycle
  std::vector<int32_t> rows;             // trig-row pattern the tables were built for
  std::vector<uint16_t> ix, iy;          // ... and the pattern itself for lists without a signature
  bool perm_valid = false, perm_plain_dev = false, perm_dealt_dev = false;  // the host holds the orders / the device holds which
  size_t perm_first = 0, perm_count = 0;  // ... for this shard
  int perm_cs = 0;                        // ... and these samples per workgroup
  void drop_orders() { perm_valid = perm_plain_dev = perm_dealt_dev = false; }
};

// A lattice (sig, n; for one without a signature its rows / ix / iy) arrives.  same: its tables are the active ones.
// hit: they were kept -- the tables of the active pattern change places with them, or, when the active ones are not
// worth keeping (lists without a signature are not kept), move in and leave the slot empty.  miss: the active pattern is
// put away into an empty slot, a new slot (up to `slots`) or the one unused for longest; what comes back is a stale or
// empty set of buffers and no orders: the caller rebuilds into it.  Whole objects change places: nothing is written,
// nothing queued reads these tables between cycles (the sensor kernels do not).
enum class PatternFind { same, hit, miss };
template <typename T>
PatternFind find_pattern(T &active, std::vector<T> &kept, uint64_t &clock, long &hits, uint64_t sig, size_t n,
                         const std::vector<int32_t> &rows, const std::vector<uint16_t> &ix, const std::vector<uint16_t> &iy,
                         size_t slots) {
  if (n == active.n && (sig != 0 ? sig == active.sig : active.sig == 0 && active.rows == rows && active.ix == ix && active.iy == iy))
    return PatternFind::same;
  if (n > 0 && sig != 0) {
    ++clock;
    const bool active_keeps = active.sig != 0 && active.n > 0;
    for (T &t : kept)
      if (t.sig == sig && t.n == n) {
        std::swap(t, active);
        if (!active_keeps) {  // nothing worth keeping went back: the slot empties
          t.sig = 0;
          t.n = 0;
          t.drop_orders();
          t.ix.clear();
          t.iy.clear();
        }
        t.stamp = clock;
        ++hits;
        return PatternFind::hit;
      }
    if (active_keeps) {
      T *slot = nullptr;
      for (T &t : kept)
        if (t.sig == 0) slot = &t;
      if (!slot && kept.size() < slots) {
        kept.emplace_back();
        slot = &kept.back();
      }
      if (!slot) {
        slot = &kept[0];
        for (T &t : kept)
          if (t.stamp < slot->stamp) slot = &t;
      }
      std::swap(*slot, active);
      slot->stamp = clock;
      active.sig = 0;
      active.n = 0;
    }
  }
  active.drop_orders();  // (the orders also belong to one shard)
  return PatternFind::miss;
}

// shard-local sample ids ordered by trig row (stable): consecutive samples of a fused workgroup then share one or two
// rows of the table.  A counting sort (rows are small integers; this runs whenever the window's pattern is new, which a
// robot crossing v = 0 makes a frequent event).  `start` is scratch.
inline void order_by_row(const int32_t *row, size_t n, std::vector<int32_t> &h_perm, std::vector<int32_t> &start) {
  h_perm.resize(n);
  int32_t rmax = 0;
  for (size_t i = 0; i < n; ++i) rmax = std::max(rmax, row[i]);
  start.assign(static_cast<size_t>(rmax) + 2, 0);
  for (size_t i = 0; i < n; ++i) ++start[static_cast<size_t>(row[i]) + 1];
  for (size_t r = 1; r < start.size(); ++r) start[r] += start[r - 1];
  for (size_t i = 0; i < n; ++i) h_perm[static_cast<size_t>(start[static_cast<size_t>(row[i])]++)] = static_cast<int32_t>(i);
}

// The single-launch cycle gets a second order, dealt from the first (cs samples per workgroup): survivors of the
// collision gate cluster (a few adjacent omega rows, the low speeds of each), and a workgroup costs its own survivors,
// so a cluster of any shape has to land on many workgroups instead of a few.
inline void deal_order(const int32_t *row, const std::vector<int32_t> &h_perm, size_t n, size_t cs, std::vector<int32_t> &dealt) {
  dealt.clear();
  dealt.reserve(n);
  // Rectangular lattice (R trig rows of L samples each -- the non-holonomic
  // window is one): a workgroup takes 8 rows, R/8 apart, and 4 samples of each,
  // L/4 apart.  Survivors cluster in adjacent rows and adjacent speeds, so at
  // most a couple land in one workgroup, and a workgroup reads 8 rows of the
  // trig table instead of 32.  Anything else (omni windows, ragged shards): the
  // skewed stride, one sample per row.
  size_t R = 0, L = 0;
  bool rect = true;
  for (size_t i = 0; i < n && rect;) {
    size_t j = i;
    while (j < n && row[h_perm[j]] == row[h_perm[i]]) ++j;
    if (R == 0) L = j - i;
    rect = (j - i) == L;
    ++R;
    i = j;
  }
  const size_t rows_per = cs / 4;  // cs = 32: 8 rows x 4 samples, 16: 4 x 4
  rect = rect && R * L == n && R % rows_per == 0 && L % 4 == 0;
  if (rect) {
    const size_t A = R / rows_per, B = L / 4;
    for (size_t a = 0; a < A; ++a)
      for (size_t b = 0; b < B; ++b)
        for (size_t i = 0; i < rows_per; ++i)
          for (size_t k = 0; k < 4; ++k) dealt.push_back(h_perm[(a + A * i) * L + b + B * k]);
    return;
  }
  // Ragged rows (omni windows, shares dealt by row): quads again -- every row of the sorted order is cut
  // into groups of (up to) four samples a quarter of the row apart, and the quads are dealt with the skewed
  // stride (a workgroup takes its quads from cs / 4 regions of the sorted order: adjacent rows and adjacent
  // speeds go to different workgroups, and the samples of a workgroup share cs / 4 trig rows or a few more
  // instead of cs -- the rows its lanes have to form).  A workgroup is whatever cs consecutive
  // entries of the flat list are: partial quads only shift the boundaries.
  std::vector<int32_t> qstart, qstep, qcount;  // quad = h_perm[qstart + k * qstep], k < qcount
  for (size_t i = 0; i < n;) {
    size_t j = i;
    while (j < n && row[h_perm[j]] == row[h_perm[i]]) ++j;
    const size_t len = j - i, nq = (len + 3) / 4;
    for (size_t q = 0; q < nq; ++q) {
      qstart.push_back(static_cast<int32_t>(i + q));
      qstep.push_back(static_cast<int32_t>(nq));
      qcount.push_back(static_cast<int32_t>((len - q + nq - 1) / nq));  // elements q, q + nq, ... below len
    }
    i = j;
  }
  const size_t Q = qstart.size(), qper = cs / 4;
  const size_t G = (Q + qper - 1) / qper;
  for (size_t g = 0; g < G; ++g)
    for (size_t j = 0; j < qper; ++j) {
      const size_t e = j * G + (g + 37 * j) % G;
      if (e >= Q) continue;
      for (int32_t k = 0; k < qcount[e]; ++k) dealt.push_back(h_perm[static_cast<size_t>(qstart[e] + k * qstep[e])]);
    }
}

}  // namespace kc
