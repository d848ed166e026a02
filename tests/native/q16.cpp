// The Q16 pose arithmetic the world map, the localiser and the MPPI controller share (csrc/kc_q16.h) on a fixed list of
// cases: one line a case, its name, its inputs, its results.  tests/test_q16_cpu.py forms every line again from the Python
// statements of the rules and compares.  Plain g++, no GPU.
#include <cstdio>
#include <initializer_list>

#include "kc_q16.h"

using namespace kc;
typedef long long ll;
typedef unsigned long long ull;

static void draw(ull seed, unsigned step, ull i, unsigned c) {
  std::printf("draw %llu %u %llu %u %llu\n", seed, step, i, c, q16_draw(q16_key(seed, step), i, c));
}
// as kc_mppi.hip forms it: int k, t, c
static void mppi_draw(ull seed, unsigned step, int k, int t, int c) {
  std::printf("mppi_draw %llu %u %d %d %d %llu\n", seed, step, k, t, c, q16_draw(q16_key(seed, step), k, 3 * t + c));
}
static void noise(ull v, int s) { std::printf("noise %llu %d %lld\n", v, s, q16_noise(v, s)); }
static void clamp(ll v) { std::printf("clamp %lld %lld\n", v, q16_clamp(v)); }
// (C, S): the heading table's entry h, which the pytest checks
static void move(int h, ll C, ll S, ll tx, ll ty, ll F, ll L) {
  std::printf("move %d %lld %lld %lld %lld %lld %lld %lld %lld\n", h, C, S, tx, ty, F, L, q16_move_x(tx, C, S, F, L), q16_move_y(ty, C, S, F, L));
}
static void turn(int cq, int sq, int ac, int as) {
  std::printf("turn %d %d %d %d %lld %lld\n", cq, sq, ac, as, q16_turn_x(cq, sq, ac, as), q16_turn_y(cq, sq, ac, as));
}
static void weight_bin(unsigned v, unsigned vmin, int w_shift, int EW) {
  std::printf("weight_bin %u %u %d %d %u\n", v, vmin, w_shift, EW, q16_weight_bin(v, vmin, w_shift, EW));
}

int main() {
  const ll B = kQ16MaxOffset;
  std::printf("bound %lld\n", B);
  std::printf("mix64 0 %llu\n", q16_mix64(0));
  std::printf("mix64 %llu %llu\n", ~0ull, q16_mix64(~0ull));
  draw(0, 0, 0, 0);
  draw(5, 3, 7, 2);
  draw(~0ull, 0xFFFFFFFFu, 65535, 255);
  mppi_draw(0x0123456789ABCDEFull, 77, 65535, 63, 2);
  mppi_draw(9, 0xFFFFFFFFu, 1, 0, 0);
  // g = -131070 and +131070, the extremes; s = 0 and 2^31 - 1; g = -131069 with s = 3: -393207 / 65536 rounds to -6
  for (ull v : {0ull, ~0ull, 1ull, 0x8000800080008000ull})
    for (int s : {0, 1, 3, 1000, 0x7FFFFFFF}) noise(v, s);
  for (ll v : {0ll, B - 1, B, B + 1, -B + 1, -B, -B - 1, 1ll << 62, -(1ll << 62)}) clamp(v);
  move(40000, -50404, -41886, 123456789, -987654321, 70000, -30000);  // C and S negative
  move(40000, -50404, -41886, 0, 0, -(1 << 22), 1 << 22);
  move(0, 65536, 0, 1000, -1000, 12345, -54321);                       // the step is (F, L) itself
  move(0, 65536, 0, B - 100, -B + 50, 100, -50);                       // lands exactly on the bound
  move(0, 65536, 0, B - 100, -B + 50, 101, -51);                       // one past it
  move(32768, -65536, 0, -B + 7, B - 7, 1 << 22, 1 << 22);             // far past it, on the other side
  move(16384, 0, 65536, B, -B, 1, 1);                                  // from the bound: x back inside, y stays
  for (int q = 0; q < 4; ++q) {  // (cq, sq) = (65536, 0), (0, 65536), (-65536, 0), (0, -65536) over two table entries
    const int cq = q == 0 ? 65536 : (q == 2 ? -65536 : 0), sq = q == 1 ? 65536 : (q == 3 ? -65536 : 0);
    turn(cq, sq, 759250125, 759250125);
    turn(cq, sq, -536870912, 929887697);
  }
  turn(32768, 0, 3, -3);   // products of exactly 1.5 and -1.5: 2 and -1
  turn(-32768, 0, 3, 3);   // -1.5 twice: -1 and -1
  turn(1, 1, 32768, 0);    // 0.5 twice: 1 and 1
  turn(1, -1, -32768, 0);  // -0.5 and 0.5: 0 and 1
  weight_bin(5, 5, 0, 1);
  weight_bin(1000, 5, 4, 1024);
  weight_bin(1u << 30, 0, 0, 4096);
  weight_bin(1u << 30, 0, 30, 4096);
  weight_bin(4095 << 4, 0, 4, 4096);
  weight_bin((4094 << 4) + 15, 0, 4, 4096);
  return 0;
}
