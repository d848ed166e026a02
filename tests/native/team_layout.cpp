// The team layout of the cycle kernel's cost phase (csrc/kc_team_layout.h) against the rule as it is stated: a team is
// floor(16 / R) wavefronts (eight at most), its last place forms the obstacle term, the places in front of it hold every
// point at the widest of {8, 4, 2} lanes a point that fits.  Exhaustive over R = 1..4, P = 2..64.  Plain g++, no GPU.
#include <cstdio>
#include <initializer_list>

#include "kc_team_layout.h"

using namespace kc;

static int checks = 0, bad = 0;
#define CHECK(cond)                                  \
  do {                                               \
    ++checks;                                        \
    if (!(cond)) {                                   \
      ++bad;                                         \
      std::printf("line %d: %s\n", __LINE__, #cond); \
    }                                                \
  } while (0)

static bool fits(int P, int kL, int W) { return P * kL <= 64 * (W - 1); }

int main() {
  for (int R = 1; R <= 4; ++R)
    for (int P = 2; P <= 64; ++P) {
      const TeamLayout l = team_layout(R, P);
      const int W = l.waves, kL = l.lanes_per;
      CHECK(W == (16 / R < 8 ? 16 / R : 8));
      CHECK(R * W <= 16);
      CHECK(kL == 8 || kL == 4 || kL == 2);
      CHECK(fits(P, kL, W));
      CHECK((P * kL + 63) / 64 <= W - 1);  // the same in whole wavefronts
      for (int wider = 2 * kL; wider <= 8; wider *= 2) CHECK(!fits(P, wider, W));
      if (!(W == l.waves && fits(P, kL, W))) std::printf("  at R %d P %d: %d x %d\n", R, P, W, kL);
      // the wavefronts 0..15 fall into teams of W, and a team's places are a permutation of 0..W-1
      for (int wave = 0; wave < 16; ++wave) CHECK(team_of_wave(W, wave) == wave / W);
      for (int t = 0; t < R; ++t) {
        unsigned seen = 0;
        for (int k = 0; k < W; ++k) {
          const int r = team_wave_role(W, t, k);
          CHECK(r >= 0 && r < W);
          seen |= 1u << r;
        }
        CHECK(seen == (1u << W) - 1u);
      }
      // no two teams have their obstacle wavefront, or their first search wavefront, on the same SIMD (wave mod 4)
      if (R > 2)
        for (int place : {0, W - 1}) {
          unsigned simds = 0;
          for (int t = 0; t < R; ++t)
            for (int k = 0; k < W; ++k)
              if (team_wave_role(W, t, k) == place) {
                CHECK(!(simds & (1u << ((t * W + k) & 3))));
                simds |= 1u << ((t * W + k) & 3);
              }
        }
    }
  // the horizon of the headline, by value
  for (int R : {1, 2}) CHECK(team_layout(R, 50).waves == 8 && team_layout(R, 50).lanes_per == 8);  // 400 of 448 lanes
  CHECK(team_layout(3, 50).waves == 5 && team_layout(3, 50).lanes_per == 4);                       // 200 of 256
  CHECK(team_layout(4, 50).waves == 4 && team_layout(4, 50).lanes_per == 2);                       // 100 of 192
  // the edges of the rule
  CHECK(team_layout(2, 56).lanes_per == 8 && team_layout(2, 57).lanes_per == 4 && team_layout(1, 64).lanes_per == 4);
  CHECK(team_layout(4, 48).lanes_per == 4 && team_layout(4, 49).lanes_per == 2 && team_layout(4, 64).lanes_per == 2);
  CHECK(team_layout(3, 32).lanes_per == 8 && team_layout(3, 33).lanes_per == 4 && team_layout(3, 64).lanes_per == 4);
  CHECK(team_layout(4, 24).lanes_per == 8 && team_layout(4, 25).lanes_per == 4);
  std::printf("%d checks, %d bad\n", checks, bad);
  return bad ? 1 : 0;
}
