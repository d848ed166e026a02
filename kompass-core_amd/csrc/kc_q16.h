// The integers the world map's ray walks, the localiser and the MPPI controller share (DESIGN.md 4.11 rules 22, 28 to 31
// and 36, 4.12 rules 3 and 4), stated once for the device library and held bit for bit to tests/worldmap_mcl_ref.py and
// tests/mppi_ref.py by tests/test_q16_cpu.py.  16 fraction bits of a cell.  Values in, values out; no HIP include.
#pragma once

#if defined(__HIPCC__)
#define KC_Q16_HD __host__ __device__ inline
#else
#define KC_Q16_HD inline
#endif

namespace kc {

constexpr long long kQ16MaxOffset = 1ll << 36;  // 2^20 cells in 16 fraction bits

// rule 28: every offset stays within +- 2^36
KC_Q16_HD long long q16_clamp(long long v) { return v < -kQ16MaxOffset ? -kQ16MaxOffset : (v > kQ16MaxOffset ? kQ16MaxOffset : v); }

// rule 30: the mixer, a step's key, the draw of index i and channel c (MPPI: 3 t + c), the noise of a draw at scale s
KC_Q16_HD unsigned long long q16_mix64(unsigned long long x) {
  unsigned long long z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
KC_Q16_HD unsigned long long q16_key(unsigned long long seed, unsigned step) { return q16_mix64(seed ^ (static_cast<unsigned long long>(step) << 32)); }
KC_Q16_HD unsigned long long q16_draw(unsigned long long key, unsigned long long i, unsigned c) { return q16_mix64(key ^ ((i << 8) | c)); }
KC_Q16_HD long long q16_noise(unsigned long long v, int s) {
  const long long g =
      static_cast<long long>((v & 0xFFFF) + ((v >> 16) & 0xFFFF) + ((v >> 32) & 0xFFFF) + (v >> 48)) - 131070ll;
  return (g * s + (1ll << 15)) >> 16;
}

// rule 22: (a, b) turned by the heading pair (c, s), rounded half up.  A beam's direction (dx, dy) from (cq, sq) and the
// table's (ac, as); rule 31's displacement from (C, S) and (F, L)
KC_Q16_HD long long q16_turn_x(long long c, long long s, long long a, long long b) { return (c * a - s * b + (1ll << 15)) >> 16; }
KC_Q16_HD long long q16_turn_y(long long c, long long s, long long a, long long b) { return (s * a + c * b + (1ll << 15)) >> 16; }

// rule 31 and 4.12 rule 4: the motion step, by the heading before the step
KC_Q16_HD long long q16_move_x(long long tx, long long C, long long S, long long F, long long L) { return q16_clamp(tx + q16_turn_x(C, S, F, L)); }
KC_Q16_HD long long q16_move_y(long long ty, long long C, long long S, long long F, long long L) { return q16_clamp(ty + q16_turn_y(C, S, F, L)); }

// rule 36: the weight table's entry for v, the least of all being vmin
KC_Q16_HD unsigned q16_weight_bin(unsigned v, unsigned vmin, int w_shift, int EW) {
  const unsigned bin = (v - vmin) >> w_shift;
  return bin < static_cast<unsigned>(EW - 1) ? bin : static_cast<unsigned>(EW - 1);
}

}  // namespace kc
