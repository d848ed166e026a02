"""World map update on the MI355X: a 400 x 400 local grid into a 2004 x 1204 world at several yaws,
the device-resident update against the host paste it replaces.

  device : kc_worldmap_update_from_mapper on the mapper's finished device grid (one launch + the 20-byte read-back)
  host   : D2H of the local grid + the numpy statement of the rule (tests/worldmap_ref.py, the whole world, one CPU
           thread) + H2D of the class plane, each timed on its own

Per yaw one JSON line with median [min, max] milliseconds over --reps repetitions after --warmup warm-ups, and the
planes of both sides compared once (the tool stops when they differ).  The numpy statement is the yardstick's cost,
no claim about a compiled CPU paste.  To be run by hand; nothing is gated on these numbers.

  python tools/worldmap_time.py [--reps 30] [--warmup 3] [--yaws 0,0.3,0.785398,1.570796,-2.5]"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kompass-core_amd"), str(ROOT / "tests")]

import kompass_hip as kh  # noqa: E402
import synthetic as syn  # noqa: E402
import worldmap_ref as ref  # noqa: E402
from helpers import DeviceArray, hip_runtime  # noqa: E402

W, H, RES, ORIGIN = 2004, 1204, 0.05, (-50.0, -30.0)
GH = GW = 400


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return [round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--yaws", default="0,0.3,0.785398,1.570796,-2.5")
    args = ap.parse_args()
    if kh.device_count() < 1:
        raise SystemExit("needs a HIP device")
    hip = hip_runtime()
    ang, rng = syn.dense_scan(2048, 1.2)                      # ranges 3.6 .. 8.4 m in a 20 m window
    pose_xy = (ORIGIN[0] + 0.5 * W * RES + 0.013, ORIGIN[1] + 0.5 * H * RES - 0.021)
    with kh.MapperContext(GH, GW, RES, (0, 0, 0), 0.0, len(ang)) as mapper, \
            kh.WorldMapContext(W, H, RES, ORIGIN) as ctx, DeviceArray(np.zeros((W, H), np.int8, order="F")) as dev_map:
        mapper.scan_to_grid_device(ang, rng)
        mapper.sync()
        local = np.empty(GH * GW, np.int32)
        grid_ptr = C.c_void_p(mapper.grid_device_ptr())

        def d2h():
            assert hip.hipMemcpy(local.ctypes.data_as(C.c_void_p), grid_ptr, local.nbytes, 2) == 0

        for yaw in [float(v) for v in args.yaws.split(",")]:
            pose = pose_xy + (yaw,)
            want = ref.WorldMapRef(W, H, RES, ORIGIN)
            ctx.clear()
            d2h()
            g = local.reshape(GW, GH).T
            got = ctx.update_from_mapper(mapper, pose)
            assert got == want.update(g, pose), (got, "device and statement disagree")
            cls, ev = ctx.planes()
            assert np.array_equal(cls, want.cls) and np.array_equal(ev, want.evidence), "planes differ"
            host_cls = np.asfortranarray(want.cls)

            def h2d():
                assert hip.hipMemcpy(dev_map.p, host_cls.ctypes.data_as(C.c_void_p), host_cls.nbytes, 1) == 0

            line = {
                "world": [W, H], "local": [GH, GW], "yaw": yaw, "reps": args.reps, "warmup": args.warmup,
                "changed_first_update": got[0], "box_first_update": list(got[1]),
                "device_update_ms": timed(lambda: ctx.update_from_mapper(mapper, pose), args.reps, args.warmup),
                "host_d2h_local_ms": timed(d2h, args.reps, args.warmup),
                "host_numpy_statement_ms": timed(lambda: want.update(g, pose), args.reps, args.warmup),
                "host_h2d_map_ms": timed(h2d, args.reps, args.warmup),
            }
            line["host_total_ms"] = round(line["host_d2h_local_ms"][0] + line["host_numpy_statement_ms"][0] + line["host_h2d_map_ms"][0], 4)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
