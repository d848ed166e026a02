// The sample-pattern rule and the two walking orders of the DWA host path (csrc/kc_sample_pattern.h) against lists and
// sequences worked out by hand from the rules the header's comments state.  Plain g++, no GPU.
#include <cstdio>
#include <map>
#include <set>

#include "kc_sample_pattern.h"

using namespace kc;

static int checks = 0, bad = 0;
#define CHECK(...)                                                   \
  do {                                                               \
    ++checks;                                                        \
    if (!(__VA_ARGS__)) {                                            \
      ++bad;                                                         \
      std::printf("line %d: %s\n", __LINE__, #__VA_ARGS__);          \
    }                                                                \
  } while (0)

using Ids = std::vector<int32_t>;

static Ids runs(std::initializer_list<std::pair<int32_t, int>> rs) {  // {row, count} ... in list order
  Ids rows;
  for (auto &r : rs) rows.insert(rows.end(), static_cast<size_t>(r.second), r.first);
  return rows;
}
static Ids interleaved(int R, int L) {  // 0 1 .. R-1 0 1 .. (L times)
  Ids rows;
  for (int i = 0; i < R * L; ++i) rows.push_back(i % R);
  return rows;
}
static Ids row_major(int R, int L) {
  Ids rows;
  for (int i = 0; i < R * L; ++i) rows.push_back(i / L);
  return rows;
}

static bool is_permutation_of_iota(const Ids &p, size_t n) {
  if (p.size() != n) return false;
  std::vector<char> seen(n, 0);
  for (int32_t v : p) {
    if (v < 0 || static_cast<size_t>(v) >= n || seen[static_cast<size_t>(v)]) return false;
    seen[static_cast<size_t>(v)] = 1;
  }
  return true;
}

// both orders of `rows` at cs samples per workgroup, with the properties every case must have -> dealt
static Ids orders(const Ids &rows, size_t cs, Ids *perm_out = nullptr) {
  const size_t n = rows.size();
  Ids perm, scratch, dealt;
  order_by_row(rows.data(), n, perm, scratch);
  deal_order(rows.data(), perm, n, cs, dealt);
  CHECK(is_permutation_of_iota(perm, n));
  CHECK(is_permutation_of_iota(dealt, n));
  bool sorted = true;  // by row, ties in list order
  for (size_t i = 0; i + 1 < perm.size(); ++i) {
    const int32_t a = perm[i], b = perm[i + 1];
    sorted = sorted && (rows[a] < rows[b] || (rows[a] == rows[b] && a < b));
  }
  CHECK(sorted);
  if (perm_out) *perm_out = perm;
  return dealt;
}

// the rectangular deal in closed form: workgroup a * B + b holds (row a + A * i, column b + B * k), i-major
static Ids rect_closed_form(size_t R, size_t L, size_t cs) {
  const size_t A = R / (cs / 4), B = L / 4;
  Ids d;
  for (size_t a = 0; a < A; ++a)
    for (size_t b = 0; b < B; ++b)
      for (size_t i = 0; i < cs / 4; ++i)
        for (size_t k = 0; k < 4; ++k) d.push_back(static_cast<int32_t>((a + A * i) * L + b + B * k));
  return d;
}

static void walking_orders() {
  CHECK(orders(runs({{0, 8}, {1, 3}, {2, 6}}), 16) == (Ids{0, 2, 4, 6, 11, 13, 15, 12, 14, 16, 1, 3, 5, 7, 8, 9, 10}));  // ragged, two workgroups
  CHECK(orders(runs({{0, 5}, {1, 1}, {2, 4}}), 16) == (Ids{0, 2, 4, 1, 3, 5, 6, 7, 8, 9}));                               // ragged, one
  {
    const Ids d = orders(row_major(8, 8), 16);  // rectangular, A = 2, B = 2
    const Ids head{0, 2, 4, 6, 16, 18, 20, 22, 32, 34, 36, 38, 48, 50, 52, 54, 1, 3, 5, 7};
    CHECK(d.size() == 64 && Ids(d.begin(), d.begin() + 20) == head);
    CHECK(d == rect_closed_form(8, 8, 16));
    CHECK(orders(row_major(16, 8), 32) == rect_closed_form(16, 8, 32));
  }
  {
    Ids perm;
    const Ids d = orders(interleaved(4, 4), 16, &perm);  // a stable sort, then the rectangular deal
    CHECK(perm == (Ids{0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15}));
    CHECK(d == (Ids{0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15}));
  }
  // six rows are no multiple of eight: the ragged path
  CHECK(orders(interleaved(6, 4), 32) == (Ids{0, 6, 12, 18, 1, 7, 13, 19, 2, 8, 14, 20, 3, 9, 15, 21, 4, 10, 16, 22, 5, 11, 17, 23}));
  uint64_t st = 0x2545F4914F6CDD1Dull;
  auto next = [&st]() { return static_cast<uint32_t>((st = st * 6364136223846793005ull + 1442695040888963407ull) >> 33); };
  for (int t = 0; t < 400; ++t) {
    const size_t n = 1 + next() % 200, R = 1 + next() % 12;
    Ids rows(n);
    for (auto &r : rows) r = static_cast<int32_t>(next() % R);
    orders(rows, t & 1 ? 32 : 16);
  }
}

// A tables type whose swap is visible, and a driver that does what upload_samples / build_perm do around the rule.
struct Tables : PatternHost {
  int id = -1;  // (stands for the device buffers)
};
struct Lattice {
  uint64_t sig;
  size_t n;
  Ids rows;
  std::vector<uint16_t> ix, iy;
};
struct Store {
  Tables active;
  std::vector<Tables> kept;
  uint64_t clock = 0;
  long hits = 0;
  int next_id = 0;
  using Key = std::pair<uint64_t, size_t>;  // a pattern: signature and size
  std::map<Key, int> built;                 // -> id of the tables built for it last
  std::map<Key, PatternHost> away;          // -> the order fields it had when it was active last

  PatternFind step(const Lattice &l) {
    const long hits0 = hits;
    const int id0 = active.id;
    if (active.sig) away[{active.sig, active.n}] = active;  // (if this step puts it away)
    const PatternFind f = find_pattern(active, kept, clock, hits, l.sig, l.n, l.rows, l.ix, l.iy, 3);
    CHECK(hits == hits0 + (f == PatternFind::hit));
    if (f == PatternFind::same) CHECK(active.id == id0);
    if (f == PatternFind::miss) {
      CHECK(!active.perm_valid && !active.perm_plain_dev && !active.perm_dealt_dev);
      if (l.n == 0) return f;  // (nothing is uploaded)
      active.id = next_id++;
      active.sig = l.sig;
      active.n = l.n;
      active.rows = l.rows;
      active.ix = l.sig ? std::vector<uint16_t>{} : l.ix;
      active.iy = l.sig ? std::vector<uint16_t>{} : l.iy;
      build_orders();
      if (l.sig) built[{l.sig, l.n}] = active.id;
    }
    if (l.sig) {  // the active tables are those built for this pattern, with the order fields they were put away with
      CHECK(active.sig == l.sig && active.n == l.n && active.id == built[{l.sig, l.n}]);
      const PatternHost &w = away[{l.sig, l.n}];
      if (f == PatternFind::hit)
        CHECK(active.perm_valid == w.perm_valid && active.perm_plain_dev == w.perm_plain_dev && active.perm_dealt_dev == w.perm_dealt_dev &&
              active.perm_first == w.perm_first && active.perm_count == w.perm_count && active.perm_cs == w.perm_cs);
    }
    for (const Tables &t : kept) {
      CHECK(t.ix.empty() && t.iy.empty());
      if (t.sig) CHECK(t.n > 0 && t.id == built[{t.sig, t.n}]);
      else CHECK(t.n == 0 && !t.perm_valid && !t.perm_plain_dev && !t.perm_dealt_dev);
    }
    return f;
  }
  void build_orders() {  // fields a swap must carry: different for every id
    active.perm_valid = true;
    active.perm_plain_dev = active.id & 1;
    active.perm_dealt_dev = !(active.id & 1);
    active.perm_first = static_cast<size_t>(active.id);
    active.perm_count = active.n;
    active.perm_cs = active.id & 2 ? 16 : 32;
  }
  std::set<uint64_t> kept_sigs() const {
    std::set<uint64_t> s;
    for (const Tables &t : kept)
      if (t.sig) s.insert(t.sig);
    return s;
  }
};

static Lattice window(uint64_t sig, size_t n = 8) { return Lattice{sig, n, {}, {}, {}}; }

static void kept_patterns() {
  using F = PatternFind;
  using S = std::set<uint64_t>;
  {  // five patterns through three slots
    Store s;
    const uint64_t P[5] = {0x101, 0x102, 0x103, 0x104, 0x105};
    const S after1[5] = {{}, {P[0]}, {P[0], P[1]}, {P[0], P[1], P[2]}, {P[1], P[2], P[3]}};
    for (int i = 0; i < 5; ++i) {
      CHECK(s.step(window(P[i])) == F::miss);
      CHECK(s.kept_sigs() == after1[i]);
    }
    // every pattern is evicted just before its turn: the slot put away longest ago goes
    const S after2[5] = {{P[3], P[4], P[2]}, {P[3], P[4], P[0]}, {P[1], P[4], P[0]}, {P[1], P[2], P[0]}, {P[1], P[2], P[3]}};
    for (int i = 0; i < 5; ++i) {
      CHECK(s.step(window(P[i])) == F::miss);
      CHECK(s.kept_sigs() == after2[i]);
    }
    CHECK(s.active.sig == P[4] && s.kept.size() == 3);
    const F want3[5] = {F::same, F::hit, F::hit, F::hit, F::miss};
    const S after3[5] = {{P[1], P[2], P[3]}, {P[1], P[2], P[4]}, {P[1], P[3], P[4]}, {P[2], P[3], P[4]}, {P[2], P[3], P[1]}};
    for (int i = 0; i < 5; ++i) {
      CHECK(s.step(window(P[4 - i])) == want3[i]);
      CHECK(s.kept_sigs() == after3[i]);
    }
    CHECK(s.hits == 3 && s.kept.size() == 3);
  }
  {  // lists without a signature between windows
    Store s;
    const uint64_t X = 0xA1, Y = 0xB1;
    const Lattice E{0, 5, {0, 0, 1, 1, 2}, {0, 1, 0, 1, 2}, {0, 0, 0, 0, 0}};
    const Lattice E2{0, 5, {0, 1, 2, 0, 1}, {0, 1, 0, 1, 2}, {0, 0, 0, 0, 0}};  // the same count, other rows
    const Lattice none{0, 0, {}, {}, {}};
    CHECK(s.step(window(X, 6)) == F::miss);
    CHECK(s.step(E) == F::miss && s.kept.empty());             // overwrites X
    CHECK(s.active.sig == 0 && s.active.ix == E.ix);
    CHECK(s.step(window(X, 6)) == F::miss && s.kept.empty());  // X was not kept, and the list is not
    CHECK(s.step(window(Y, 6)) == F::miss && s.kept_sigs() == S{X});
    CHECK(s.step(E) == F::miss && s.kept_sigs() == S{X});      // overwrites Y
    CHECK(s.step(E) == F::same);
    CHECK(s.step(Lattice(E)) == F::same);                      // an equal list, vector by vector
    CHECK(s.step(E2) == F::miss);
    CHECK(s.step(none) == F::miss && s.active.n == 5);
    CHECK(s.step(E2) == F::same && !s.active.perm_valid);      // the tables of E2 are still there, its orders are not
    s.build_orders();
    CHECK(s.step(none) == F::miss);
    CHECK(s.step(window(X, 6)) == F::hit);                     // nothing worth keeping goes back: the slot empties
    CHECK(s.kept.size() == 1 && s.kept[0].sig == 0 && s.kept[0].n == 0 && !s.kept[0].perm_valid && !s.kept[0].perm_plain_dev &&
          !s.kept[0].perm_dealt_dev);
    CHECK(s.step(window(Y, 6)) == F::miss);                    // Y was overwritten; X goes into the emptied slot
    CHECK(s.kept.size() == 1 && s.kept_sigs() == S{X});
    CHECK(s.step(none) == F::miss && s.active.sig == Y);
    CHECK(s.step(window(Y, 6)) == F::same);
    CHECK(s.step(window(X, 6)) == F::hit && s.kept_sigs() == S{Y});
    CHECK(s.hits == 2);
    CHECK(s.step(window(X, 7)) == F::miss);                    // the same signature with another size
    CHECK(s.kept.size() == 2 && s.kept[1].sig == X && s.kept[1].n == 6);
    CHECK(s.step(window(X, 9)) == F::miss);                    // ... also while that signature is kept with two other sizes
    CHECK(s.kept.size() == 3 && s.kept[2].sig == X && s.kept[2].n == 7);
    CHECK(s.step(E) == F::miss && s.active.perm_valid);        // a list whose orders are valid ...
    CHECK(s.step(window(Y, 6)) == F::hit);                     // ... goes into the slot, which drops them as it empties
    CHECK(s.kept[0].sig == 0 && s.kept[0].n == 0 && !s.kept[0].perm_valid && !s.kept[0].perm_plain_dev && !s.kept[0].perm_dealt_dev);
    CHECK(s.hits == 3);
  }
}

int main() {
  walking_orders();
  kept_patterns();
  std::printf("%d checks, %d bad\n", checks, bad);
  return bad != 0;
}
