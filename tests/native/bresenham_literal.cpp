// bresenhamEnhanced (reference mapping/line_drawing.h:55-124), restated literally for lines a Python loop cannot
// walk: every step from the start cell, the three emit branches in their order, int64 error terms (the reference's
// int overflows from dx >= 2^29 on; in 64 bits the walk is exact for every line of this build).  Shares nothing
// with the oracle's or the kernels' clipped walks.  Used by tests/test_mapper_ref_cpu.py.
//
//   bresenham_literal H W s0 s1 t0 t1 [t0 t1 ...]
//
// prints, for every line from (s0, s1) to (t0, t1), the points that land in the H x W grid, in the order the
// reference appends them: "beam seq i j" per line, then "steps <total steps walked>".
#include <cstdio>
#include <cstdlib>
#include <cstdint>

namespace {

struct Sink {
  long long H, W;
  long long beam;
  long long seq = 0;
  void operator()(long long x, long long y) {
    if (x >= 0 && x < H && y >= 0 && y < W) std::printf("%lld %lld %lld %lld\n", beam, seq, x, y);
    ++seq;
  }
};

long long walk(long long x, long long y, long long x1, long long y1, Sink &emit) {
  long long dx = x1 - x, dy = y1 - y;
  emit(x, y);
  const long long xstep = (dx >= 0) ? 1 : -1, ystep = (dy >= 0) ? 1 : -1;
  dx = std::llabs(dx);
  dy = std::llabs(dy);
  const long long ddy = 2 * dy, ddx = 2 * dx;
  if (ddx >= ddy) {  // first octant
    long long errorprev = dx, error = dx;
    for (long long i = 0; i < dx; i++) {
      x += xstep;
      error += ddy;
      if (error > ddx) {
        y += ystep;
        error -= ddx;
        if (error + errorprev < ddx) {
          emit(x, y - ystep);
        } else if (error + errorprev > ddx) {
          emit(x - xstep, y);
        } else {
          emit(x - xstep, y);
          emit(x, y - ystep);
        }
      }
      emit(x, y);
      errorprev = error;
    }
    return dx;
  }
  long long errorprev = dy, error = dy;  // second octant
  for (long long i = 0; i < dy; i++) {
    y += ystep;
    error += ddx;
    if (error > ddy) {
      x += xstep;
      error -= ddy;
      if (error + errorprev < ddy) {
        emit(x - xstep, y);
      } else if (error + errorprev > ddy) {
        emit(x, y - ystep);
      } else {
        emit(x - xstep, y);
        emit(x, y - ystep);
      }
    }
    emit(x, y);
    errorprev = error;
  }
  return dy;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 5 || (argc - 5) % 2 != 0) {
    std::fprintf(stderr, "usage: %s H W s0 s1 [t0 t1 ...]\n", argv[0]);
    return 2;
  }
  const long long H = std::atoll(argv[1]), W = std::atoll(argv[2]);
  const long long s0 = std::atoll(argv[3]), s1 = std::atoll(argv[4]);
  long long steps = 0;
  for (int k = 5, b = 0; k < argc; k += 2, ++b) {
    Sink emit{H, W, b};
    steps += walk(s0, s1, std::atoll(argv[k]), std::atoll(argv[k + 1]), emit);
  }
  std::printf("steps %lld\n", steps);
  return 0;
}
