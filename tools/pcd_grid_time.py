"""Cloud -> occupancy grid on the MI355X at 10^6, 10^7 and 5 * 10^7 points of the indoor map recipe
(synthetic.pcd_indoor_map) at 0.05 m.  Per size, one JSON line: the kernels' times from the context's timing
hooks, the wall time of the two C-ABI calls with a host array and with a device-resident one, the read bandwidth
of each pass against the point bytes (12 B a point), and a single-thread CPU baseline: the same two loops in C++,
compiled here with the host flags.  Nothing is gated on these numbers.

A/B of the plain load in front of pass 2's atomicOr: build the variant without it and run both,
  bash tools/build_variant.sh grid_no_preload -DKC_GRID_NO_PRELOAD
  KOMPASS_HIP_LIB=kompass-core_amd/lib_ab/grid_no_preload/libkompass_hip.so python tools/pcd_grid_time.py

  python tools/pcd_grid_time.py [--sizes 1000000,10000000] [--reps 5]"""
import argparse
import ctypes as C
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kompass-core_amd")]

import kompass_hip as kh  # noqa: E402
import synthetic as syn  # noqa: E402

BASELINE = r"""
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
extern "C" int grid_cpu(const float *p, long n, float res, float zg, float zr, int8_t *grid, long cap, int *cells) {
  float lo[2] = {FLT_MAX, FLT_MAX}, hi[2] = {-FLT_MAX, -FLT_MAX};
  for (long i = 0; i < n; ++i) {
    const float x = p[3 * i], y = p[3 * i + 1];
    if (!std::isfinite(x) || !std::isfinite(y)) continue;
    lo[0] = std::min(lo[0], x); hi[0] = std::max(hi[0], x);
    lo[1] = std::min(lo[1], y); hi[1] = std::max(hi[1], y);
  }
  const int cx = (int)std::ceil((hi[0] - lo[0]) / res), cy = (int)std::ceil((hi[1] - lo[1]) / res);
  cells[0] = cx; cells[1] = cy;
  if ((long)cx * cy > cap) return 1;
  std::memset(grid, -1, (size_t)cx * cy);
  const float inv = 1.0f / res;
  for (long i = 0; i < n; ++i) {
    const float x = p[3 * i], y = p[3 * i + 1], z = p[3 * i + 2];
    if (!std::isfinite(x) || !std::isfinite(y)) continue;
    const int ix = (int)((x - lo[0]) * inv), iy = (int)((y - lo[1]) * inv);
    if (ix < 0 || ix >= cx || iy < 0 || iy >= cy) continue;
    const int8_t v = (z > zg && z <= zr) ? 100 : (z <= zg ? 0 : -1);
    int8_t &c = grid[ix + (size_t)iy * cx];
    c = std::max(c, v);
  }
  return 0;
}
"""
HOST_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-shared"]


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000,50000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--resolution", type=float, default=0.05)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp()
    (Path(tmp) / "grid_cpu.cpp").write_text(BASELINE)
    subprocess.check_call(["g++", *HOST_FLAGS, str(Path(tmp) / "grid_cpu.cpp"), "-o", str(Path(tmp) / "grid_cpu.so")])
    cpu = C.CDLL(str(Path(tmp) / "grid_cpu.so")).grid_cpu
    cpu.argtypes = [C.c_void_p, C.c_long, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_long, C.c_void_p]
    L = kh.lib()  # the HIP runtime the library is linked to, for the device-resident cloud
    L.hipMalloc.argtypes, L.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    zg, zr, res = 0.1, 1.0, a.resolution
    for n in [int(s) for s in a.sizes.split(",")]:
        pts = syn.pcd_indoor_map(n, seed=1)
        ctx = kh.CloudContext(max_bytes=pts.nbytes)
        grid, origin = ctx.occupancy_grid(pts, res, zg, zr)  # warm-up: allocations
        dev = C.c_void_p()
        assert L.hipMalloc(C.byref(dev), pts.nbytes) == 0
        assert L.hipMemcpy(dev, pts.ctypes.data, pts.nbytes, 1) == 0
        on_dev = lambda: ctx.occupancy_grid(None, res, zg, zr, device_ptr=dev.value, n_points=n)  # noqa: E731
        on_dev_no_d2h = lambda: ctx.occupancy_grid(None, res, zg, zr, device_ptr=dev.value, n_points=n,  # noqa: E731
                                                   to_host=False)
        g2, _ = on_dev()
        assert np.array_equal(g2, grid)
        host_ms = median_ms(lambda: ctx.occupancy_grid(pts, res, zg, zr), a.reps)
        dev_ms = median_ms(on_dev, a.reps)
        dev_no_d2h_ms = median_ms(on_dev_no_d2h, a.reps)
        ctx.timing_enable(True)
        ks = {}
        for _ in range(a.reps):
            on_dev_no_d2h()
            for name, ms in ctx.timings():
                ks.setdefault(name, []).append(ms)
        ctx.timing_enable(False)
        kern = {k: round(float(np.median(v)), 4) for k, v in ks.items()}
        out = np.empty(grid.size, np.int8)
        cells = (C.c_int * 2)()
        cpu_call = lambda: cpu(pts.ctypes.data, n, res, zg, zr, out.ctypes.data, out.size, cells)  # noqa: E731
        assert cpu_call() == 0 and np.array_equal(out.reshape(grid.shape, order="F"), grid)
        cpu_ms = median_ms(cpu_call, max(1, a.reps // 2))
        gbs = lambda ms: round(pts.nbytes / (ms * 1e-3) / 1e9, 1) if ms > 0 else None  # noqa: E731
        print(json.dumps({
            "points": n, "resolution": res, "grid": list(grid.shape), "point_mbytes": round(pts.nbytes / 1e6, 1),
            "cells": {str(v): int((grid == v).sum()) for v in (-1, 0, 100)}, "kernel_ms": kern,
            "extent_read_gbs": gbs(kern.get("cloud_extent_kernel", 0)),
            "scatter_read_gbs": gbs(kern.get("cloud_grid_scatter_kernel", 0)),
            "abi_host_array_ms": round(host_ms, 3), "abi_device_array_ms": round(dev_ms, 3),
            "abi_device_array_grid_on_device_ms": round(dev_no_d2h_ms, 3), "cpu_single_thread_ms": round(cpu_ms, 2),
        }), flush=True)
        L.hipFree(dev)
        ctx.close()


if __name__ == "__main__":
    main()
