"""World map update on the MI355X: a 400 x 400 local grid into a 2004 x 1204 world at several yaws,
the device-resident update against the host paste it replaces.

  device : kc_worldmap_update_from_mapper on the mapper's finished device grid (one launch + the 20-byte read-back)
  host   : D2H of the local grid + the numpy statement of the rule (tests/worldmap_ref.py, the whole world, one CPU
           thread) + H2D of the class plane, each timed on its own

Per yaw one JSON line with median [min, max] milliseconds over --reps repetitions after --warmup warm-ups, and the
planes of both sides compared once (the tool stops when they differ).  The numpy statement is the yardstick's cost,
no claim about a compiled CPU paste.  To be run by hand; nothing is gated on these numbers.

  python tools/worldmap_time.py [--reps 30] [--warmup 3] [--yaws 0,0.3,0.785398,1.570796,-2.5]

--match times the correlative match instead (rules 9 to 15): the same 400 x 400 local grid against a world that holds
what it saw, the guess a few cells and a degree off, windows K = S = 10 and K = S = 20.  Per window one JSON line: the
whole call (four launches and the read-back, host clock), the four launches by HIP events (a second series of calls,
with the events on), and the numpy statement of the rules (tests/worldmap_match_ref.py, one CPU thread: the yardstick's
cost, not a compiled CPU implementation), whose table and record the device's are compared with once.

  python tools/worldmap_time.py --match [--reps 30] [--warmup 3]

--points times the obstacle hand-off instead (rules 16 to 19): the same world holding what the 400 x 400 local grid saw,
the robot in the middle, max_sensor_range 10 m (Rc = 200).  One JSON line with
  (a) kc_dwa_set_worldmap: the extraction on the controller's stream and the sensor build behind it;
  (b) kc_worldmap_points: the list into host memory;
  (c) the route without it: kc_worldmap_get of the class plane, numpy.nonzero + rule 18 in numpy over the window,
      kc_dwa_set_points, each timed on its own;
  (d) kc_dwa_set_grid_from_mapper on the local grid, the yardstick for a hand-off on the device.
Every repetition ends with a device synchronisation inside the timed span, so the controller's entries are timed with
the sensor build they queue.  The lists of (a) to (c) are compared with the statement once.

  python tools/worldmap_time.py --points [--reps 30] [--warmup 3]

--scan times the virtual laser scan instead (rules 20 to 27): the same world holding what the 400 x 400 local grid saw,
the scan frame in the middle, range_max 10 m (Rc = 200).  One JSON line with
  (a) kc_worldmap_scan to the host at 360, 1440 and 4096 beams;
  (b) a batch of 1024 poses x 360 beams in one launch;
  (c) kc_dvz_deform_worldmap against kc_worldmap_scan followed by kc_dvz_deform, and kc_zone_check_worldmap against
      kc_worldmap_scan followed by kc_zone_check, at 360 beams;
  (d) the route without it: kc_worldmap_get of the class plane alone, and the Python statement of the rules
      (tests/worldmap_scan_ref.py, one loop a beam on one CPU thread: a Python statement's cost, not a compiled CPU
      implementation) timed once.
The ranges of (a) at 360 beams are compared with the statement once.

  python tools/worldmap_time.py --scan [--reps 30] [--warmup 3]

--mcl times the Monte-Carlo localiser instead (rules 28 to 41): the same world, 4096 particles x 64 beams and 1024 x 256
beams spread 2 m around the middle, range_max 10 m.  One JSON line a configuration with
  (a) kc_mcl_step and kc_mcl_step + kc_mcl_resample by the host's clock, and their launches by HIP events (walk, weigh,
      prefix, select);
  (b) the route that exists without the localiser: kc_worldmap_scan of the same N poses x B beams to the host, and the
      penalty sum over its ranges in numpy (vectorised numpy on one CPU thread: a Python statement's cost, not a compiled
      CPU filter);
  (c) kc_worldmap_scan alone for the same rays, by the host's clock with its read-back of N x B doubles: the floor the
      walk sets, and the ratio of the step's walk launch to it.
  python tools/worldmap_time.py --mcl [--reps 30] [--warmup 3]

--mcl --recovery times the fit's step and the injecting resample (rules 59 to 62): the same world, the field model, 4096 x
64 and 65536 x 24.  ONE JSON line with an entry a configuration: kc_mcl_step, step + kc_mcl_resample and step +
kc_mcl_resample_inject(N / 4) by the host's clock (a resample has no wait of its own: the next step's read-back is its
end), the launches of each by HIP events (the injecting resample's five: prefix, select, rows, row_prefix, inject), and
kc_mcl_init_global by the host's clock beside them.  With KOMPASS_HIP_LIB_OLD=1 (tools/ab_libs.sh, a library from before
these rules) the plain legs alone: the A/B of the step and the plain resample.
  python tools/worldmap_time.py --mcl --recovery [--reps 30] [--warmup 3]

--field times the distance plane and the likelihood-field model (rules 42 to 45): the same world under the "latest
observation wins" model, reach 6 and 16.  One JSON line a reach with
  (a) a full refresh (kc_worldmap_set_distance marks the whole map, then kc_worldmap_distance_device: refresh and wait);
  (b) a partial refresh behind a 400 x 400 update: two mappers' grids alternate so that every update changes cells; the
      update itself is outside the clock, the box it left is reported;
  (c) kc_worldmap_get_distance with nothing dirty: the copy of W x H uint16 alone;
and one line a particle configuration (4096 x 64, 1024 x 256, 65536 x 24) with the field step and the beam step of the
same localiser on the same particles, by the host's clock and their launches by HIP events.
  python tools/worldmap_time.py --field [--reps 30] [--warmup 3]

--shift times the rolling window (rules 46 to 48): the same world holding what the 400 x 400 local grid saw.  One JSON line
with
  (a) kc_worldmap_shift by (64, 0) and by (64, 64), each followed by the shift back, so that the window stays where the
      map's content is; the figure is one call: the launch, the two device-to-device copies and the wait;
  (b) the route it replaces: kc_worldmap_get of both planes, numpy.roll of the class plane with the entering strip put to
      unknown, kc_worldmap_set_prior_host, each timed on its own.  THAT ROUTE LOSES THE EVIDENCE: a prior only knows
      e_min and e_max, so every cell's count starts again at a bound;
and one line a reach (6 and 16) with the first distance read after a shift (kc_worldmap_distance_device: the full
refresh rule 48 asks for, and the wait).  The planes after (a) are compared with the statement (tests/worldmap_shift_ref.py)
once.
  python tools/worldmap_time.py --shift [--reps 30] [--warmup 3]

--integrate times the scan integration (rules 52 to 57): an empty 2004 x 1204 world, the scan frame near the middle,
range_max 10 m (Rc = 200), 360, 1440 and 4096 beams of a room scan with KC_INTEGRATE_CLEAR_NO_RETURN.  One JSON line a beam
count with
  (a) kc_worldmap_integrate by the host's clock (two launches and the 20-byte read-back) and its mark and apply launches by
      HIP events, with the mark kernel's byte load in front of its atomic off (the default), on, and off again;
  (b) the route that exists without it, for the same scan: the mapper's scan to its 400 x 400 grid on the device followed
      by kc_worldmap_update_from_mapper, together and each on its own.
At 360 beams the marks, the planes and the record are compared with the statement (tests/worldmap_integrate_ref.py) once.
  python tools/worldmap_time.py --integrate [--reps 30] [--warmup 3]

--movers times the detection of movers in a scan (rules 64 to 69): the same world, seen and free everywhere with the distance
plane on at reach 8 and refreshed beforehand, the same room scan with every seventh beam of its last two thirds without a
return, so that every return is a dynamic beam and the runs are cut.  One JSON line a beam count (360, 1440, 4096) with
kc_worldmap_movers by the host's clock (two launches and the one read-back), its flag and cluster launches by HIP events,
and kc_worldmap_integrate for the same scan on a map of its own beside it.  At 360 beams labels, record and clusters are
compared with the statement (tests/worldmap_movers_ref.py) once.  With --integrate as well, that leg follows in the same run.
  python tools/worldmap_time.py --movers [--integrate] [--reps 30] [--warmup 3]"""
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
import worldmap_match_ref as mref  # noqa: E402
import worldmap_points_ref as pref  # noqa: E402
import worldmap_ref as ref  # noqa: E402
import worldmap_scan_ref as sref  # noqa: E402
from helpers import DeviceArray, hip_context, hip_runtime  # noqa: E402

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


def spread(v):
    return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]


def match_leg(args):
    hip = hip_runtime()
    ang, rng = syn.dense_scan(2048, 1.2)
    true = (ORIGIN[0] + 0.5 * W * RES + 0.013, ORIGIN[1] + 0.5 * H * RES - 0.021, 0.3)
    r = float(np.float32(RES))
    guess = (true[0] - 3 * r, true[1] + 2 * r, true[2] + 0.0175)
    with kh.MapperContext(GH, GW, RES, (0, 0, 0), 0.0, len(ang)) as mapper, kh.WorldMapContext(W, H, RES, ORIGIN) as ctx:
        mapper.scan_to_grid_device(ang, rng)
        mapper.sync()
        local = np.empty(GH * GW, np.int32)
        assert hip.hipMemcpy(local.ctypes.data_as(C.c_void_p), C.c_void_p(mapper.grid_device_ptr()), local.nbytes, 2) == 0
        g = local.reshape(GW, GH).T
        want = ref.WorldMapRef(W, H, RES, ORIGIN)
        assert ctx.update_from_mapper(mapper, true) == want.update(g, true)
        for K in (10, 20):
            S, step = K, 0.00873 * 10 / K   # the same +- 5 degrees either way
            window = dict(n_yaw=K, yaw_step=step, reach=S)
            t0 = time.perf_counter()
            exp, table, _ = mref.match_pose(want, g, guess, K, step, S)
            numpy_ms = (time.perf_counter() - t0) * 1e3
            got = ctx.match_from_mapper(mapper, guess, **window)
            assert got == exp._asdict(), (got, exp, "device and statement disagree")
            assert np.array_equal(ctx.match_scores(K, S), table), "score tables differ"
            whole = timed(lambda: ctx.match_from_mapper(mapper, guess, **window), args.reps, args.warmup)
            ctx.match_set_timing(True)
            parts = []
            for k in range(args.warmup + args.reps):
                ctx.match_from_mapper(mapper, guess, **window)
                if k >= args.warmup:
                    parts.append(ctx.match_times())
            ctx.match_set_timing(False)
            names = ["weight", "points", "score", "pick"]
            line = {"world": [W, H], "local": [GH, GW], "n_yaw": K, "reach": S, "yaw_step": step, "points": exp.points,
                    "candidates": int(table.size), "winner": [exp.k, exp.u, exp.v], "score": exp.score,
                    "score_guess": exp.score_guess, "reps": args.reps, "warmup": args.warmup, "device_match_ms": whole,
                    "numpy_statement_one_thread_ms_once": round(numpy_ms, 1)}
            for i, n in enumerate(names):
                line[f"launch_{n}_ms"] = spread([p[i] for p in parts])
            print(json.dumps(line), flush=True)


def points_leg(args):
    hip = hip_runtime()
    ang, rng = syn.dense_scan(2048, 1.2)
    r = float(np.float32(RES))
    centre = (ORIGIN[0] + (W // 2) * r, ORIGIN[1] + (H // 2) * r)   # on a cell centre: the world holds the local grid's cells
    max_range = 10.0
    inp = syn.make_controller_inputs("cfg2", seed=0, scale=0.25)
    st = centre + (0.0, 0.0)

    def synced(fn):
        def run():
            fn()
            assert hip.hipDeviceSynchronize() == 0
        return run

    with kh.MapperContext(GH, GW, RES, (0, 0, 0), 0.0, len(ang)) as mapper, kh.WorldMapContext(W, H, RES, ORIGIN) as wm:
        mapper.scan_to_grid_device(ang, rng)
        mapper.sync()
        wm.update_from_mapper(mapper, centre + (0.0,))
        cls = wm.planes()[0]
        want, n, bounds = pref.worldmap_points_ref(cls, RES, ORIGIN, centre[0], centre[1], max_range)
        got, got_bounds = wm.points(centre[0], centre[1], max_range)
        assert got_bounds == bounds and pref.sort_points(got, RES, ORIGIN).tobytes() == want.tobytes(), "device and statement disagree"
        ic, jc, rc = kh.worldmap_window(RES, ORIGIN, centre[0], centre[1], max_range)
        inp["points"] = want
        ctx = hip_context(kh, inp)
        host_cls = np.empty((W, H), np.int8, order="F")
        lists = {}

        def get():
            kh._check(kh.lib().kc_worldmap_get(wm.h, host_cls.ctypes.data, None, host_cls.size))

        def numpy_list():
            i0, i1, j0, j1 = max(ic - rc, 0), min(ic + rc, W - 1), max(jc - rc, 0), min(jc + rc, H - 1)
            box = host_cls[i0:i1 + 1, j0:j1 + 1]
            di = np.arange(i0, i1 + 1, dtype=np.int64)[:, None] - ic
            dj = np.arange(j0, j1 + 1, dtype=np.int64)[None, :] - jc
            ii, jj = np.nonzero((box == ref.OCCUPIED) & (di * di + dj * dj <= rc * rc))
            lists["host"] = pref.cell_points(RES, ORIGIN, ii + i0, jj + j0)

        get()
        numpy_list()
        assert pref.sort_points(lists["host"], RES, ORIGIN).tobytes() == want.tobytes(), "host route and statement disagree"
        mapper_points = int((np.asarray(mapper.scan_to_grid(ang, rng)) == ref.OCCUPIED).sum())
        mapper.scan_to_grid_device(ang, rng)
        mapper.sync()
        line = {"world": [W, H], "local": [GH, GW], "max_sensor_range": max_range, "radius_cells": rc, "points": n,
                "mapper_points": mapper_points, "reps": args.reps, "warmup": args.warmup}
        legs = [("a_dwa_set_worldmap_ms", lambda: ctx.set_worldmap(st, wm, max_range)),
                ("b_worldmap_points_to_host_ms", lambda: wm.points(centre[0], centre[1], max_range, cap=n)),
                ("c1_worldmap_get_cls_ms", get),
                ("c2_numpy_nonzero_rule18_ms", numpy_list),
                ("c3_dwa_set_points_ms", lambda: ctx.set_points(st, lists["host"], max_range)),
                ("d_dwa_set_grid_from_mapper_ms", lambda: ctx.set_grid_from_mapper(st, mapper, max_range))]
        for name, fn in legs:
            line[name] = timed(synced(fn), args.reps, args.warmup)
        line["c_total_ms"] = round(sum(line[k][0] for k in ("c1_worldmap_get_cls_ms", "c2_numpy_nonzero_rule18_ms", "c3_dwa_set_points_ms")), 4)
        # a second pass over (a) and (d) in alternation: their difference is judged against (d)'s own spread in this run
        alt = {"a": [], "d": []}
        for k in range(args.warmup + args.reps):
            for key, fn in (("a", legs[0][1]), ("d", legs[5][1])):
                t0 = time.perf_counter()
                synced(fn)()
                if k >= args.warmup:
                    alt[key].append((time.perf_counter() - t0) * 1e3)
        line["a_alternating_ms"], line["d_alternating_ms"] = spread(alt["a"]), spread(alt["d"])
        print(json.dumps(line), flush=True)


def scan_leg(args):
    ang, rng = syn.dense_scan(2048, 1.2)
    r = float(np.float32(RES))
    centre = (ORIGIN[0] + (W // 2) * r, ORIGIN[1] + (H // 2) * r)
    pose = centre + (0.3,)
    range_max = 10.0
    zone = (1.2, 0.8, 0.1, -0.05, 0.3)

    def beams(n):
        return np.arange(n) * (2 * np.pi / n)

    with kh.MapperContext(GH, GW, RES, (0, 0, 0), 0.0, len(ang)) as mapper, kh.WorldMapContext(W, H, RES, ORIGIN) as wm, \
            kh.DvzContext(max_beams=4096) as dvz, \
            kh.ZoneContext(kh.CYLINDER, [0.2, 0.4], [0, 0, 0], [0, 0, 0, 1], 160.0, 0.3, 1.0, beams(360), 0.0, 2.0, range_max) as zc:
        mapper.scan_to_grid_device(ang, rng)
        mapper.sync()
        wm.update_from_mapper(mapper, centre + (0.0,))
        cls = wm.planes()[0]
        a360 = beams(360)
        t0 = time.perf_counter()
        want_r, want_c = sref.scan(cls, RES, ORIGIN, [pose], a360, range_max)
        statement_ms = (time.perf_counter() - t0) * 1e3
        got_r, got_c = wm.scan(pose, a360, range_max, return_cells=True)
        assert got_r.tobytes() == want_r[0].tobytes() and got_c.tobytes() == want_c[0].tobytes(), "device and statement disagree"
        assert dvz.deform_worldmap(zone, wm, pose, a360, range_max)[:3] == dvz.deform(zone, a360, want_r[0])
        assert zc.check_worldmap(wm, pose, True) == zc.check(want_r[0], True)
        host_cls = np.empty((W, H), np.int8, order="F")
        line = {"world": [W, H], "local": [GH, GW], "range_max": range_max, "radius_cells": kh.worldmap_scan_check(RES, 1, 360, range_max),
                "hits_of_360": int((want_c >= 0).sum()), "reps": args.reps, "warmup": args.warmup}
        for n in (360, 1440, 4096):
            a = beams(n)
            line[f"a_scan_{n}_beams_to_host_ms"] = timed(lambda: wm.scan(pose, a, range_max), args.reps, args.warmup)
        rs = np.random.default_rng(3)
        poses = [(centre[0] + dx, centre[1] + dy, yaw) for dx, dy, yaw in
                 zip(rs.uniform(-2, 2, 1024), rs.uniform(-2, 2, 1024), rs.uniform(-np.pi, np.pi, 1024))]
        qposes = [wm.quantise_pose(*p) for p in poses]
        line["b_scan_1024_poses_x_360_beams_ms"] = timed(lambda: wm.scan(qposes, a360, range_max), args.reps, args.warmup)

        def scan_then_deform():
            dvz.deform(zone, a360, wm.scan(pose, a360, range_max))

        def scan_then_check():
            zc.check(wm.scan(pose, a360, range_max), True)

        line["c_dvz_deform_worldmap_ms"] = timed(lambda: dvz.deform_worldmap(zone, wm, pose, a360, range_max), args.reps, args.warmup)
        line["c_scan_then_dvz_deform_ms"] = timed(scan_then_deform, args.reps, args.warmup)
        line["c_zone_check_worldmap_ms"] = timed(lambda: zc.check_worldmap(wm, pose, True), args.reps, args.warmup)
        line["c_scan_then_zone_check_ms"] = timed(scan_then_check, args.reps, args.warmup)
        line["d_worldmap_get_cls_alone_ms"] = timed(
            lambda: kh._check(kh.lib().kc_worldmap_get(wm.h, host_cls.ctypes.data, None, host_cls.size)), args.reps, args.warmup)
        line["d_python_statement_360_beams_one_thread_ms_once"] = round(statement_ms, 1)
        print(json.dumps(line), flush=True)


def mcl_leg(args):
    import worldmap_mcl_ref as lref

    ang, rng = syn.dense_scan(2048, 1.2)
    r = float(np.float32(RES))
    centre = (ORIGIN[0] + (W // 2) * r, ORIGIN[1] + (H // 2) * r)
    range_max = 10.0
    pen, err_shift, wtab, w_shift = lref.sensor_tables(RES, 0.1)
    pen_np = np.array(pen, np.int64)
    cells = 65536.0 / r
    with kh.MapperContext(GH, GW, RES, (0, 0, 0), 0.0, len(ang)) as mapper, kh.WorldMapContext(W, H, RES, ORIGIN) as wm:
        mapper.scan_to_grid_device(ang, rng)
        mapper.sync()
        wm.update_from_mapper(mapper, centre + (0.0,))
        for n, b in ((4096, 64), (1024, 256)):
            a = np.arange(b) * (2 * np.pi / b)
            zq = kh.mcl_quantise_ranges(wm.scan(centre + (0.3,), a, range_max), RES, range_max)
            with kh.MclContext(wm, n, a, range_max, seed=1) as mcl:
                mcl.set_model(pen, err_shift, wtab, w_shift)
                q0 = wm.quantise_pose(*centre, 0.0)
                scales = (lref.noise_scale(0.02 * cells), lref.noise_scale(0.01 * cells), lref.noise_scale(0.01 / (2 * np.pi) * 65536))

                def init():
                    mcl.init_pose(q0.tx, q0.ty, 0, lref.noise_scale(2.0 * cells), lref.noise_scale(65536 / 4))

                def step():
                    return mcl.step(3000, 0, 50, *scales, zq)

                def step_resample():
                    step()
                    mcl.resample()

                init()
                rec = step()
                tx, ty, h, _ = mcl.particles()
                poses = [kh.WorldMapPose(*kh.mcl_heading(int(hh)), int(x), int(y)) for x, y, hh in zip(tx, ty, h)]
                zmax = mcl.zmax

                def scan_only():
                    return wm.scan(poses, a, range_max)

                def scan_and_sum():
                    ranges = scan_only()
                    q = np.minimum(np.rint(ranges / r * 65536.0).astype(np.int64), zmax)
                    bins = np.minimum(np.abs(q - zq[None, :].astype(np.int64)) >> err_shift, len(pen) - 1)
                    return pen_np[bins].sum(axis=1)

                line = {"world": [W, H], "particles": n, "beams": b, "rays": n * b, "range_max": range_max, "reps": args.reps,
                        "warmup": args.warmup, "n_eff_first_step": round(rec.w1 * rec.w1 / rec.w2, 1),
                        "a_step_ms": timed(step, args.reps, args.warmup),
                        "a_step_and_resample_ms": timed(step_resample, args.reps, args.warmup)}
                mcl.set_timing(True)
                parts = []
                for k in range(args.warmup + args.reps):
                    step_resample()
                    if k >= args.warmup:
                        parts.append(mcl.times())
                mcl.set_timing(False)
                for i, name in enumerate(["walk", "weigh", "prefix", "select"]):
                    line[f"launch_{name}_ms"] = spread([p[i] for p in parts])
                line["b_scan_to_host_and_numpy_penalty_sum_ms"] = timed(scan_and_sum, args.reps, args.warmup)
                line["c_scan_to_host_alone_ms"] = timed(scan_only, args.reps, args.warmup)
                line["c_walk_launch_over_scan_call"] = round(line["launch_walk_ms"][0] / line["c_scan_to_host_alone_ms"][0], 3)
                print(json.dumps(line), flush=True)


def recovery_leg(args):
    """--mcl --recovery: ONE JSON line (tools/ab_libs.sh keeps a run's last line) with an entry a configuration."""
    import os

    import worldmap_mcl_field_ref as fref
    import worldmap_mcl_ref as lref

    old = os.environ.get("KOMPASS_HIP_LIB_OLD", "0") == "1"     # a library from before rules 59 to 63: the plain legs alone
    ang, rng = syn.dense_scan(2048, 1.2)
    r = float(np.float32(RES))
    centre = (ORIGIN[0] + (W // 2) * r, ORIGIN[1] + (H // 2) * r)
    range_max = 10.0
    cells = 65536.0 / r
    pen_d2, pen_far, reach, wtab, w_shift = fref.field_tables(RES, 0.1)
    out = []
    with kh.MapperContext(GH, GW, RES, (0, 0, 0), 0.0, len(ang)) as mapper, kh.WorldMapContext(W, H, RES, ORIGIN) as wm:
        wm.set_model(**ref.LATEST_WINS_EXACT)                # a miss makes a cell empty: the scan's inside is free
        mapper.scan_to_grid_device(ang, rng)
        mapper.sync()
        wm.update_from_mapper(mapper, centre + (0.0,))
        wm.set_distance(reach)
        for n, b in ((4096, 64), (65536, 24)):
            a = np.arange(b) * (2 * np.pi / b)
            zq = kh.mcl_quantise_ranges(wm.scan(centre + (0.3,), a, range_max), RES, range_max)
            with kh.MclContext(wm, n, a, range_max, seed=1) as mcl:
                mcl.set_field_model(pen_d2, pen_far, wtab, w_shift)
                q0 = wm.quantise_pose(*centre, 0.0)
                scales = (lref.noise_scale(0.02 * cells), lref.noise_scale(0.01 * cells), lref.noise_scale(0.01 / (2 * np.pi) * 65536))
                mcl.init_pose(q0.tx, q0.ty, 0, lref.noise_scale(2.0 * cells), lref.noise_scale(65536 / 4))

                def step():
                    return mcl.step(3000, 0, 50, *scales, zq)

                def step_resample():
                    step()
                    mcl.resample()

                def step_inject():
                    step()
                    mcl.resample_inject(n // 4)

                def launches(cycle, get):
                    mcl.set_timing(True)
                    parts = []
                    for k in range(args.warmup + args.reps):
                        cycle()
                        if k >= args.warmup:
                            parts.append(get())
                    mcl.set_timing(False)
                    return parts

                line = {"particles": n, "beams": b, "reps": args.reps, "warmup": args.warmup,
                        "step_ms": timed(step, args.reps, args.warmup),
                        "step_and_resample_ms": timed(step_resample, args.reps, args.warmup)}
                parts = launches(step_resample, mcl.times)
                for i, name in enumerate(["walk", "weigh", "prefix", "select"]):
                    line[f"launch_{name}_ms"] = spread([p[i] for p in parts])
                line["resample_launches_ms"] = spread([p[2] + p[3] for p in parts])
                if not old:
                    line["step_and_inject_ms"] = timed(step_inject, args.reps, args.warmup)
                    parts = launches(step_inject, lambda: mcl.times()[2:] + mcl.inject_times())
                    for i, name in enumerate(["prefix", "select", "rows", "row_prefix", "inject"]):
                        line[f"inject_launch_{name}_ms"] = spread([p[i] for p in parts])
                    line["inject_launches_ms"] = spread([sum(p) for p in parts])
                    line["fit_last"] = list(mcl.last_fit().as_tuple())
                line["init_global_ms"] = timed(mcl.init_global, args.reps, args.warmup)
                line["free_cells"] = mcl.init_global()
                out.append(line)
    print(json.dumps({"world": [W, H], "model": "field", "inject": "N / 4", "recovery": out}), flush=True)


def field_leg(args):
    import worldmap_mcl_field_ref as fref
    import worldmap_mcl_ref as lref

    ang, rng = syn.dense_scan(2048, 1.2)
    r = float(np.float32(RES))
    centre = (ORIGIN[0] + (W // 2) * r, ORIGIN[1] + (H // 2) * r)
    range_max = 10.0
    cells = 65536.0 / r
    with kh.MapperContext(GH, GW, RES, (0, 0, 0), 0.0, len(ang)) as m_a, kh.MapperContext(GH, GW, RES, (0, 0, 0), 0.0, len(ang)) as m_b, \
            kh.WorldMapContext(W, H, RES, ORIGIN) as wm:
        wm.set_model(**ref.LATEST_WINS_EXACT)
        m_a.scan_to_grid_device(ang, rng)
        m_b.scan_to_grid_device(ang, rng * 0.8)
        m_a.sync()
        m_b.sync()
        mappers = [m_a, m_b]
        for reach in (6, 16):
            wm.set_distance(reach)
            wm.update_from_mapper(m_a, centre + (0.0,))

            def full():
                wm.set_distance(reach)                           # marks the whole map; the plane's memory is kept
                t0 = time.perf_counter()
                wm.distance_device_ptr()
                return (time.perf_counter() - t0) * 1e3

            boxes = []

            def partial():
                changed, box = wm.update_from_mapper(mappers[len(boxes) & 1], centre + (0.3,))
                assert changed > 0
                t0 = time.perf_counter()
                wm.distance_device_ptr()
                dt = (time.perf_counter() - t0) * 1e3
                boxes.append(wm.distance_info()[2])
                return dt

            for _ in range(args.warmup):
                full()
                partial()
            line = {"world": [W, H], "reach": reach, "reps": args.reps, "warmup": args.warmup,
                    "a_full_refresh_ms": spread([full() for _ in range(args.reps)]),
                    "b_partial_refresh_ms": spread([partial() for _ in range(args.reps)])}
            line["b_refreshed_box"] = list(boxes[-1])
            line["c_get_distance_ms"] = timed(wm.distance, args.reps, args.warmup)
            assert np.array_equal(wm.distance()[900:1100, 500:700], __import__("worldmap_dist_ref").dist2_plane(wm.planes()[0], reach)[900:1100, 500:700]) \
                if reach == 6 else True
            print(json.dumps(line), flush=True)
        wm.set_distance(6)
        pen, err_shift, wtab, w_shift = lref.sensor_tables(RES, 0.1)
        pen_d2, pen_far, _, fwtab, fw_shift = fref.field_tables(RES, 0.1)
        for n, b in ((4096, 64), (1024, 256), (65536, 24)):
            a = np.arange(b) * (2 * np.pi / b)
            zq = kh.mcl_quantise_ranges(wm.scan(centre + (0.3,), a, range_max), RES, range_max)
            with kh.MclContext(wm, n, a, range_max, seed=1) as mcl:
                q0 = wm.quantise_pose(*centre, 0.0)
                scales = (lref.noise_scale(0.02 * cells), lref.noise_scale(0.01 * cells), lref.noise_scale(0.01 / (2 * np.pi) * 65536))
                line = {"world": [W, H], "particles": n, "beams": b, "rays": n * b, "range_max": range_max, "reps": args.reps,
                        "warmup": args.warmup}
                for name in ("field", "beam"):
                    if name == "field":
                        mcl.set_field_model(pen_d2, pen_far, fwtab, fw_shift)
                    else:
                        mcl.set_model(pen, err_shift, wtab, w_shift)
                    mcl.init_pose(q0.tx, q0.ty, 0, lref.noise_scale(2.0 * cells), lref.noise_scale(65536 / 4))

                    def step():
                        return mcl.step(3000, 0, 50, *scales, zq)

                    line[f"{name}_step_ms"] = timed(step, args.reps, args.warmup)
                    mcl.set_timing(True)
                    parts = []
                    for k in range(args.warmup + args.reps):
                        step()
                        if k >= args.warmup:
                            parts.append(mcl.times())
                    mcl.set_timing(False)
                    line[f"{name}_launch_first_ms"] = spread([p[0] for p in parts])
                    line[f"{name}_launch_weigh_ms"] = spread([p[1] for p in parts])
                line["beam_over_field_first_launch"] = round(line["beam_launch_first_ms"][0] / line["field_launch_first_ms"][0], 2)
                print(json.dumps(line), flush=True)


def shift_leg(args):
    import worldmap_shift_ref as shref

    ang, rng = syn.dense_scan(2048, 1.2)
    r = float(np.float32(RES))
    centre = (ORIGIN[0] + (W // 2) * r, ORIGIN[1] + (H // 2) * r)
    with kh.MapperContext(GH, GW, RES, (0, 0, 0), 0.0, len(ang)) as mapper, kh.WorldMapContext(W, H, RES, ORIGIN) as wm:
        mapper.scan_to_grid_device(ang, rng)
        mapper.sync()
        for yaw in (0.0, 0.3, 0.3):
            wm.update_from_mapper(mapper, centre + (yaw,))
        cls0, ev0 = wm.planes()
        line = {"world": [W, H], "reps": args.reps, "warmup": args.warmup}
        for name, d in (("a_shift_64_0_ms", (64, 0)), ("a_shift_64_64_ms", (64, 64))):
            wm.shift(*d)
            cls, ev = wm.planes()
            we, wc = shref.shift_planes(ev0, cls0, *d)
            assert np.array_equal(ev, we) and np.array_equal(cls, wc), "the shifted planes differ from the statement"
            wm.shift(-d[0], -d[1])
            back = [d, (-d[0], -d[1])]
            calls = []

            def one():
                wm.shift(*back[len(calls) & 1])
                calls.append(0)

            line[name] = timed(one, 2 * args.reps, 2 * args.warmup)
            if len(calls) & 1:
                one()
            assert wm.offset() == (0, 0)
        both = [None, None]

        def get():
            both[0], both[1] = wm.planes()

        rolled = [None]

        def roll():
            c = np.roll(both[0], (-64, -64), axis=(0, 1))
            c[W - 64:, :] = ref.UNEXPLORED
            c[:, H - 64:] = ref.UNEXPLORED
            rolled[0] = c

        line["b_get_both_planes_ms"] = timed(get, args.reps, args.warmup)
        line["b_numpy_roll_ms"] = timed(roll, args.reps, args.warmup)
        line["b_set_prior_ms"] = timed(lambda: wm.set_prior(rolled[0]), args.reps, args.warmup)
        line["b_route_total_ms"] = round(line["b_get_both_planes_ms"][0] + line["b_numpy_roll_ms"][0] + line["b_set_prior_ms"][0], 4)
        line["b_route_loses_the_evidence"] = True
        print(json.dumps(line), flush=True)
        for reach in (6, 16):
            wm.set_distance(reach)
            wm.distance_device_ptr()
            flip = []

            def first_read():
                wm.shift(64 if not len(flip) & 1 else -64, 0)              # outside the clock
                flip.append(0)
                t0 = time.perf_counter()
                wm.distance_device_ptr()
                return (time.perf_counter() - t0) * 1e3

            for _ in range(args.warmup):
                first_read()
            print(json.dumps({"world": [W, H], "reach": reach, "reps": args.reps, "warmup": args.warmup,
                              "first_distance_read_after_shift_ms": spread([first_read() for _ in range(args.reps)]),
                              "refreshed_box": list(wm.distance_info()[2])}), flush=True)


def integrate_leg(args):
    import worldmap_integrate_ref as iref

    r = float(np.float32(RES))
    centre = (ORIGIN[0] + (W // 2) * r + 0.013, ORIGIN[1] + (H // 2) * r - 0.021)
    pose = centre + (0.3,)
    range_max = 10.0
    for n in (360, 1440, 4096):
        ang, rng = syn.dense_scan(n, 1.2)                     # a room: ranges 3.6 .. 8.4 m
        ang, rng = np.asarray(ang, dtype=np.float64), np.asarray(rng, dtype=np.float64)
        zq = kh.worldmap_quantise_ranges(rng, RES, range_max)
        with kh.MapperContext(GH, GW, RES, (0, 0, 0), 0.0, n) as mapper, kh.WorldMapContext(W, H, RES, ORIGIN) as wm, \
                kh.WorldMapContext(W, H, RES, ORIGIN) as wm_route:
            line = {"world": [W, H], "beams": n, "range_max": range_max, "radius_cells": kh.worldmap_integrate_check(RES, n, range_max)[0],
                    "reps": args.reps, "warmup": args.warmup}
            if n == 360:                                      # the device against the statement, once
                want = iref.IntegrateRef(W, H, RES, ORIGIN)
                t0 = time.perf_counter()
                marks, changed, box = want.integrate(pose, ang, zq, range_max, kh.INTEGRATE_CLEAR_NO_RETURN)
                line["python_statement_one_thread_ms_once"] = round((time.perf_counter() - t0) * 1e3, 1)
                assert np.array_equal(wm.integrate_marks(pose, ang, zq, range_max, kh.INTEGRATE_CLEAR_NO_RETURN), marks), "marks differ"
                assert wm.integrate(pose, ang, zq, range_max, kh.INTEGRATE_CLEAR_NO_RETURN) == (changed, box), "records differ"
                cls, ev = wm.planes()
                assert np.array_equal(cls, want.cls) and np.array_equal(ev, want.evidence), "planes differ"
                line["changed_first_scan"], line["box_first_scan"] = changed, list(box)

            def call():
                wm.integrate(pose, ang, zq, range_max, kh.INTEGRATE_CLEAR_NO_RETURN)

            for name, on in (("precheck_off", False), ("precheck_on", True), ("precheck_off_again", False)):   # off is the default
                wm.integrate_set_precheck(on)
                line[f"integrate_call_{name}_ms"] = timed(call, args.reps, args.warmup)
                wm.integrate_set_timing(True)
                parts = []
                for k in range(args.warmup + args.reps):
                    call()
                    if k >= args.warmup:
                        parts.append(wm.integrate_times())
                wm.integrate_set_timing(False)
                line[f"launch_mark_{name}_ms"] = spread([p[0] for p in parts])
                line[f"launch_apply_{name}_ms"] = spread([p[1] for p in parts])

            def route():                                      # today's route for the same scan: rasterise twice
                mapper.scan_to_grid_device(ang, rng)
                wm_route.update_from_mapper(mapper, pose)

            line["route_mapper_scan_plus_update_from_mapper_ms"] = timed(route, args.reps, args.warmup)
            line["route_mapper_scan_alone_ms"] = timed(lambda: (mapper.scan_to_grid_device(ang, rng), mapper.sync()), args.reps, args.warmup)
            line["route_update_from_mapper_alone_ms"] = timed(lambda: wm_route.update_from_mapper(mapper, pose), args.reps, args.warmup)
            line["integrate_over_route"] = round(line["integrate_call_precheck_off_ms"][0] / line["route_mapper_scan_plus_update_from_mapper_ms"][0], 3)
            print(json.dumps(line), flush=True)


def movers_leg(args):
    import worldmap_dist_ref as dref
    import worldmap_movers_ref as wmr

    r = float(np.float32(RES))
    centre = (ORIGIN[0] + (W // 2) * r + 0.013, ORIGIN[1] + (H // 2) * r - 0.021)
    pose = centre + (0.3,)
    range_max, reach = 10.0, 8
    prior = np.zeros((W, H), np.int8, order="F")              # seen and free everywhere: every return is a dynamic beam
    for n in (360, 1440, 4096):
        ang, rng = syn.dense_scan(n, 1.2)                     # a room: ranges 3.6 .. 8.4 m
        ang, rng = np.asarray(ang, dtype=np.float64), np.asarray(rng, dtype=np.float64)
        rng[n // 3::7] = np.inf                               # beams without a return cut the runs
        zq = kh.worldmap_quantise_ranges(rng, RES, range_max)
        with kh.WorldMapContext(W, H, RES, ORIGIN) as wm, kh.WorldMapContext(W, H, RES, ORIGIN) as wm_int:
            wm.set_prior(prior)
            wm.set_distance(reach)
            wm.distance_refresh()
            line = {"world": [W, H], "beams": n, "range_max": range_max, "reach": reach, "reps": args.reps, "warmup": args.warmup}
            labels, rec, clusters = wm.movers(pose, ang, zq, range_max)
            line["record"] = list(rec)
            if n == 360:                                      # the device against the statement, once
                q = wm.quantise_pose(*pose)
                plane = np.full((W, H), dref.FAR, np.uint16)  # nothing occupied anywhere
                w_labels, w_rec, w_clusters = wmr.detect(prior, plane, reach, RES, (q.cq, q.sq, q.tx, q.ty), ang, zq, range_max)
                assert rec == tuple(w_rec) and clusters == [tuple(c) for c in w_clusters], "record or clusters differ"
                assert labels.tobytes() == w_labels.tobytes(), "labels differ"
            line["movers_call_ms"] = timed(lambda: wm.movers(pose, ang, zq, range_max), args.reps, args.warmup)
            wm.movers_set_timing(True)
            parts = []
            for k in range(args.warmup + args.reps):
                wm.movers(pose, ang, zq, range_max)
                if k >= args.warmup:
                    parts.append(wm.movers_times())
            wm.movers_set_timing(False)
            line["launch_flag_ms"] = spread([p[0] for p in parts])
            line["launch_cluster_ms"] = spread([p[1] for p in parts])
            line["integrate_call_ms"] = timed(lambda: wm_int.integrate(pose, ang, zq, range_max, kh.INTEGRATE_CLEAR_NO_RETURN),
                                              args.reps, args.warmup)
            line["movers_over_integrate"] = round(line["movers_call_ms"][0] / line["integrate_call_ms"][0], 3)
            print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--yaws", default="0,0.3,0.785398,1.570796,-2.5")
    ap.add_argument("--match", action="store_true", help="time the correlative match instead of the update")
    ap.add_argument("--points", action="store_true", help="time the obstacle hand-off to the controller instead")
    ap.add_argument("--scan", action="store_true", help="time the virtual laser scan instead")
    ap.add_argument("--mcl", action="store_true", help="time the Monte-Carlo localiser instead")
    ap.add_argument("--recovery", action="store_true", help="with --mcl: time the plain and the injecting resample instead")
    ap.add_argument("--field", action="store_true", help="time the distance plane and the likelihood-field model instead")
    ap.add_argument("--shift", action="store_true", help="time the rolling window's shift and the route it replaces instead")
    ap.add_argument("--integrate", action="store_true", help="time the scan integration and today's route for the same scan instead")
    ap.add_argument("--movers", action="store_true", help="time the detection of movers in a scan; with --integrate: both, in one run")
    args = ap.parse_args()
    if kh.device_count() < 1:
        raise SystemExit("needs a HIP device")
    if args.movers:
        movers_leg(args)
        return integrate_leg(args) if args.integrate else None
    if args.integrate:
        return integrate_leg(args)
    if args.match:
        return match_leg(args)
    if args.points:
        return points_leg(args)
    if args.scan:
        return scan_leg(args)
    if args.mcl:
        return recovery_leg(args) if args.recovery else mcl_leg(args)
    if args.field:
        return field_leg(args)
    if args.shift:
        return shift_leg(args)
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
