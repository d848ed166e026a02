// How the single-launch cycle kernel lays the few survivors of a workgroup out over its sixteen wavefronts
// (cycle_costs, kc_cycle_dev.h) -- a pure function of (survivors, trajectory points).  No HIP include: the kernel
// evaluates it on wave-uniform values (a constexpr function is callable from device code), plain g++ compiles it
// for tests/native/team_layout.cpp.
#pragma once

namespace kc {

constexpr int kTeamMaxSurvivors = 4;  // up to this many survivors of a workgroup are costed by teams; more: one per wavefront
constexpr int kCycleWaves = 16;       // wavefronts of a cycle workgroup (1024 threads)

// A team is `waves` consecutive wavefronts.  Its LAST wavefront forms only the obstacle term of the sample, a lane a
// point (wave_obstacle_term: P <= 64); the waves - 1 in front of it hold every point of the sample at once,
// `lanes_per` lanes a point -- so no wavefront runs the obstacle term behind a share of the segment search.
//   waves     = floor(16 / R), at most 8 (eight lanes a point is the widest search: more wavefronts have no use);
//   lanes_per = the widest of {8, 4, 2} with ceil(P * lanes_per / 64) <= waves - 1 (two always fit: P <= 64).
// Wavefronts beyond R * waves idle through the phase.
struct TeamLayout {
  int waves, lanes_per;
};
constexpr TeamLayout team_layout(int R, int P) {
  static_assert(kCycleWaves / 3 == 5 && kCycleWaves / 4 == 4 && kTeamMaxSurvivors == 4, "the quotients spelled out below");
  const int waves = R <= 2 ? 8 : R == 3 ? 5 : 4;  // (no division in the kernel)
  int lanes_per = 8;
  while (lanes_per > 2 && P * lanes_per > 64 * (waves - 1)) lanes_per >>= 1;
  return TeamLayout{waves, lanes_per};
}

// wave / waves for the wavefronts 0..15 and the team sizes above, by a multiplication (scalar code, no division)
constexpr int team_of_wave(int waves, int wave) {
  return (wave * (waves == 8 ? 8 : waves == 5 ? 13 : 16)) >> 6;
}

// The place in its team (0 .. waves - 1; waves - 1 forms the obstacle term, the others search from point slot
// 64 * place / lanes_per on) of the team's k-th wavefront.  The wavefronts of a workgroup go round the four SIMDs of
// the CU, so in teams of four the k-th wavefronts of all teams share a SIMD: with k as the place, one SIMD would issue
// four obstacle terms and another four first search wavefronts while a third idles.  The places of team t are therefore
// turned by t: every SIMD gets one wavefront of each place.  (That wavefront i of a workgroup runs on SIMD i mod 4 is
// inferred from the timing, not documented behaviour: four survivors at P = 50 cost 10.0 us unturned, 8.5 turned.  If a
// device places them otherwise the turn costs nothing and gains nothing; no result depends on it.)  Teams of five and the two of eight stay in order (the
// first are spread by their length; the second have one obstacle wavefront apiece among fourteen that search).
constexpr int kCuSimds = 4;
constexpr int team_wave_role(int waves, int team, int k) {
  return waves == kCuSimds ? (k + team) % kCuSimds : k;
}

}  // namespace kc
