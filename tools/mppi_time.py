"""MPPI step on the MI355X: kc_mppi_step over a 2004 x 1204 world at two shapes,
K = 1024, T = 32, M = 96 and K = 8192, T = 64, M = 256, with 1, 4 and 8 lanes a sample in the roll-out.

For every shape and variant: the wall time of the whole step (upload, plane check, two launches, read-back; the median
of --reps after --warmup) and the HIP-event times of the two launches (rollout, update).  The variants are timed
interleaved in one run, so their order in time cannot favour one.  Every variant's result is compared with the first's:
a difference is an error, not a timing.

Beside them, as yardsticks only:
  * the statement tests/mppi_ref.py on the same inputs, labelled as what it is: a Python statement's cost on one CPU;
  * the class-level DWA call of tools/class_cycle.py (kompass_cpp.control.DWA.compute_velocity_commands, 91 x 91
    lattice, the "mid" scene), timed in this run.

--movers 0,8,64 adds a leg a count: that many moving obstacles (rules 13 to 18) walking across the path ahead of the
robot, their soft rings over the first states, so that the term is computed and few samples are ended early.  The leg
with 0 movers is the step as it was (the roll-out without the term runs) and needs no entry an older build of the
library lacks.  With movers the statement compared against is tests/mppi_movers_ref.py.  Without --movers: the one leg
with none.

--field adds, beside every leg, the same leg in field mode (rules 19 to 24): a grid planner solves on the world for a goal
beyond the door (cell 1500, 602; r2 = 9), the controller is attached to its kept cost field with MPPIConfig's default
weights (fcap 2^20, w_run 32, w_term 2) and is given no path.  The statement compared against is tests/mppi_field_ref.py,
handed the planner's own field as read back from the device (tests/test_mppi_field_gpu.py shows that field equal to
tests/planner_ref.py's; the Python Dijkstra over 2.4 million cells would only add minutes here).

--rates adds, beside every leg, the same leg with acceleration limits inside the roll-out (rules 25 to 29): the rates of the
closed-loop scene of DESIGN.md 4.12 (F 4096 a step both ways, H 50) from a start velocity of 60000, so that the limiter
binds on the way up to the nominal sequence's 80000 and on most samples' noise after it.  The statement compared against
is tests/mppi_rates_ref.py.  The legs without it set no rates and need no entry an older build of the library lacks.

--box N adds, beside every leg, the same leg with a box footprint of N discs (rules 30 to 36): rule 36's cover of a box N
links of 3.75 cells long and 4 cells wide (N = 8: the 1.5 x 0.2 m robot at 0.05 m), its r2 in the place of the costs' r2.
The statement compared against is tests/mppi_box_ref.py.  The legs without it set no footprint and need no entry an older
build of the library lacks.

The world: a border, a wall with a door and scattered pillars; the robot in free space, the path a straight line
through the door.  One JSON line a shape on stdout."""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kompass-core_amd"), str(ROOT / "tests")]

import kompass_hip as kh  # noqa: E402
import mppi_box_ref as mb  # noqa: E402
import mppi_field_ref as mf  # noqa: E402
import mppi_movers_ref as mm  # noqa: E402
import mppi_rates_ref as mr  # noqa: E402
import mppi_ref as mp  # noqa: E402
import worldmap_mcl_ref as mref  # noqa: E402
from worldmap_ref import EMPTY, OCCUPIED  # noqa: E402

W, H, RES, ORIGIN, REACH = 2004, 1204, 0.05, (-50.0, -30.0), 8
ONE = 1 << 16
SHAPES = ((1024, 32, 96), (8192, 64, 256))
TEAMS = (1, 4, 8)
FIELD_GOAL, FIELD_R2, FIELD_WEIGHTS = (1500, 602), 9, (1 << 20, 32, 2)
RATES, RATES_V0 = mr.Rates(4096, 4096, 1, 1, 50, 50), (60000, 0, 0)


def world():
    rng = np.random.default_rng(3)
    c = np.full((W, H), EMPTY, np.int8)
    c[0, :] = c[-1, :] = OCCUPIED
    c[:, 0] = c[:, -1] = OCCUPIED
    c[1060, :] = OCCUPIED
    c[1060, 596:608] = EMPTY
    for _ in range(400):
        i, j = int(rng.integers(20, W - 20)), int(rng.integers(20, H - 20))
        if abs(j - 602) > 12:                                              # keep the corridor along the path free
            c[i:i + 4, j:j + 4] = OCCUPIED
    return c


def median(v):
    return round(statistics.median(v), 4)


def mover_list(n, pose):
    """n movers in a fan 6 to 20 cells ahead of the robot and 3 to 9 cells beside its path, drifting towards it at about
    0.14 cells a step: hit distance half a cell, so that few samples are ended early and the term is paid in full; soft
    from 9 cells, top 200."""
    hq, sq = 1 << 14, 81 << 16
    g = (200 * 65536) // (((sq - hq) >> 16) + 1)
    rows = []
    for i in range(n):
        ahead, side = 6 + (i * 14) // max(n, 1), (-1) ** i * (3 + i % 7)
        rows.append((pose[0] + ahead * ONE, pose[1] + side * ONE, (i % 5 - 2) * 3000, -(side // abs(side)) * (9000 + 300 * (i % 11)), hq, sq, g))
    return mm.movers(rows, 4000)


def dwa_yardstick(reps, warmup):
    import synthetic as syn
    from kompass_cpp.control import (DWA, AngularVelocityControlParams, ControlLimitsParams, ControlType,
                                     LinearVelocityControlParams, TrajectoryCostWeights)
    from kompass_cpp.types import Path as CppPath, RobotGeometry, Velocity2D
    lim = ControlLimitsParams(LinearVelocityControlParams(1.0, 2.0, 2.0), LinearVelocityControlParams(0.0, 0.0, 0.0),
                              AngularVelocityControlParams(2.0, 2.0, 3.0, 3.0))
    w = TrajectoryCostWeights()
    w.from_dict(dict(reference_path_distance_weight=1.0, goal_distance_weight=1.0, obstacles_distance_weight=1.0,
                     smoothness_weight=0.0, jerk_weight=0.0))
    d = DWA(lim, ControlType.DIFFERENTIAL_DRIVE, 0.1, 5.0, 0.2, 91, 91, RobotGeometry.get("CYLINDER"), [0.1, 0.4],
            [0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], 0.05, w, 1)
    d.set_current_path(CppPath([[x, 0.0, 0.0] for x in np.arange(0.0, 12.01, 1.0)]))
    pts = syn.scene_points("cfg2", "mid")
    ts = []
    for i in range(reps + warmup):
        d.set_current_state(0.001 * (i % 7), 0.0, 0.0, 0.5)
        t0 = time.perf_counter()
        d.compute_velocity_commands(Velocity2D(0.5, 0.0, 0.001 * (i % 5), 0.0), pts)
        ts.append((time.perf_counter() - t0) * 1e3)
    return median(ts[warmup:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--movers", default="0", help="comma-separated counts of moving obstacles, a leg each, e.g. 0,8,64")
    ap.add_argument("--field", action="store_true", help="beside every leg, the same leg steered by the grid planner's cost field")
    ap.add_argument("--rates", action="store_true", help="beside every leg, the same leg with acceleration limits inside the roll-out")
    ap.add_argument("--box", type=int, default=0, help="beside every leg, the same leg with a box footprint of this many discs (1 to 8)")
    ap.add_argument("--no-statement", action="store_true", help="skip the Python statement's timing")
    ap.add_argument("--no-dwa", action="store_true", help="skip the class-level DWA yardstick")
    args = ap.parse_args()
    counts = [int(v) for v in args.movers.split(",")]
    if not 0 <= args.box <= 8:
        raise SystemExit("--box takes 1 to 8 discs")
    boxes = (None, mb.cover(args.box * 1.875, 2.0)[:2]) if args.box else (None,)
    if kh.device_count() < 1:
        raise SystemExit("no HIP device visible")
    cls = world()
    model = mp.Model(0, 2 * ONE, 0, 1565, 0, (mref.noise_scale(0.5 * ONE), 0, mref.noise_scale(500.0)))
    costs = mp.scene_costs()
    dwa_ms = None if args.no_dwa else dwa_yardstick(args.reps, args.warmup)
    with kh.WorldMapContext(W, H, RES, ORIGIN) as m:
        m.set_prior(cls)
        m.set_distance(REACH)
        plane = None if args.no_statement else np.ascontiguousarray(m.distance())
        planner = fplane = None
        if args.field:
            planner = kh.PlannerContext()
            planner.set_grid(cls)
            t0 = time.perf_counter()
            status, cost, passes = planner.solve((1000, 601), FIELD_GOAL, FIELD_R2)
            print(json.dumps(dict(planner_solve_ms=round((time.perf_counter() - t0) * 1e3, 3), status=status, cost=cost, passes=passes)),
                  flush=True)
            fplane = None if args.no_statement else np.ascontiguousarray(planner.field()[0])
        for K, T, M in SHAPES:
            px = [(1000 + j) * ONE for j in range(M)]
            py = [602 * ONE] * M
            pose = (1000 * ONE + 300, 601 * ONE, 700)
            U = [(80000, 0, 20)] * T
            for n_mv in counts:
                for rates in (None, RATES) if args.rates else (None,):
                    for box in boxes:
                        time_leg(args, m, plane, model, costs, K, T, M, px, py, pose, U, n_mv, dwa_ms, rates=rates, box=box)
                        if planner is not None:
                            time_leg(args, m, plane, model, costs, K, T, M, px, py, pose, U, n_mv, dwa_ms, planner, fplane, rates, box)
        if planner is not None:
            planner.close()


def time_leg(args, m, plane, model, costs, K, T, M, px, py, pose, U, n_mv, dwa_ms, planner=None, fplane=None, rates=None, box=None):
    mv = mover_list(n_mv, pose)
    if box is not None:
        costs = costs._replace(r2=box[1])
    line = dict(mode="field" if planner is not None else "path", shape=dict(K=K, T=T, M=M), movers=n_mv, world=[W, H], reps=args.reps,
                warmup=args.warmup, rates=None if rates is None else list(rates), box=None if box is None else len(box[0]))
    with kh.MppiContext(m, K, T, 1) as dev:
        dev.set_model(model.f_lo, model.f_hi, model.l_hi, model.h_hi, model.kq, model.s)
        dev.set_costs(costs.r2, costs.pen_d2, costs.pen_far, costs.pen_hit, costs.w_path, costs.qcap, costs.w_goal, costs.wtab,
                      costs.w_shift)
        if planner is not None:
            dev.set_field(planner, *FIELD_WEIGHTS)                 # and no path: rule 20
        else:
            dev.set_path(px, py)
        if n_mv:
            dev.set_movers(*mv[:7], mv.pen_hit)
        if rates is not None:
            dev.set_rates(rates)
            dev.set_velocity(RATES_V0)
        if box is not None:
            dev.set_footprint(box[0])
        dev.set_timing(True)
        wall = {t: [] for t in TEAMS}
        roll = {t: [] for t in TEAMS}
        upd = {t: [] for t in TEAMS}
        first = None
        for n in range(args.reps + args.warmup):
            for team in TEAMS:                                     # interleaved
                dev.set_team(team)
                t0 = time.perf_counter()
                out, rec = dev.step(*pose, U, n)
                dt = (time.perf_counter() - t0) * 1e3
                words = dev.last_field() if planner is not None else None
                if team == TEAMS[0]:
                    first = (out.tolist(), rec.as_tuple(), words)
                elif (out.tolist(), rec.as_tuple(), words) != first:
                    raise SystemExit(f"{team} lanes a sample differ from {TEAMS[0]} at step {n}")
                if n >= args.warmup:
                    r, u = dev.times()
                    wall[team].append(dt)
                    roll[team].append(r)
                    upd[team].append(u)
        for team in TEAMS:
            line[f"team{team}"] = dict(step_ms=median(wall[team]), rollout_ms=median(roll[team]), update_ms=median(upd[team]))
        line["n_hit"], line["s_min"], line["n_hit_moving"] = first[1][4], first[1][0], int(rec.n_hit_moving) if n_mv else 0
        if plane is not None:
            ts = []
            for n in range(1 if box is not None else 3):           # (a box leg's statement is compared, hardly timed)
                t0 = time.perf_counter()
                if box is not None:
                    fld = None if planner is None else mf.Field(fplane, *FIELD_WEIGHTS)
                    want = mb.step(plane, K, 1, model, costs, *pose, U, args.reps + args.warmup - 1, box[0], rates, RATES_V0, fld, mv, px, py)
                    want = want[:3] + (want[3] if planner is not None else None,)
                elif rates is not None:
                    fld = None if planner is None else mf.Field(fplane, *FIELD_WEIGHTS)
                    want = mr.step(plane, K, 1, model, costs, *pose, U, args.reps + args.warmup - 1, rates, RATES_V0, fld, mv, px, py)
                    want = want[:3] + (want[3] if planner is not None else None,)
                elif planner is not None:
                    want = mf.step(plane, K, 1, model, costs, *pose, U, args.reps + args.warmup - 1, mf.Field(fplane, *FIELD_WEIGHTS), mv)
                else:
                    want = mm.step(plane, K, 1, model, costs, px, py, *pose, U, args.reps + args.warmup - 1, mv) + (None,)
                ts.append((time.perf_counter() - t0) * 1e3)
            if (want[0], tuple(want[1]), want[3]) != (first[0] and [tuple(r) for r in first[0]], first[1] + (line["n_hit_moving"],), first[2]):
                raise SystemExit("the device differs from the statement")
            line["python_statement_ms"] = median(ts)
    if dwa_ms is not None:
        line["dwa_class_level_91x91_mid_ms"] = dwa_ms
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
