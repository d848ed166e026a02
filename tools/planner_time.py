#!/usr/bin/env python3
"""Grid planner timing: kc_planner_solve on the PCD benchmark's map (100 x 60 m at 0.05 m = 2004 x
1204 cells, synthetic.pcd_indoor_map_doors, corner to corner) and on a 500 x 500 clutter grid, from a
device-resident grid and from a host array; the path walk on its own; and the one-thread CPU baseline, the heap
Dijkstra of tests/planner_ref.py.  Warm-up, then --reps repetitions: median and min .. max, the device named.
--clearance REACH_CELLS,WEIGHT10 adds a leg with the clearance cost on (rules 6 to 8): C2 = (sqrt(R2) + REACH_CELLS)^2,
the table of tests/planner_clearance_ref.py; the solve with the clearance pass, the field alone, the walk, the passes.
--shortcut W adds the any-angle path (rules 9 to 12) of span W: the walk call and the shortcut call behind it, each
timed on its own after an untimed solve, the waypoints and the any-angle length against the walk's; with --clearance
the same on the penalised path.
--oriented X,Y[,TURN] adds a leg with the oriented box footprint (rules 13 to 18) of an X x Y m box at 0.05 m, start
class 0, TURN straight-cell lengths a turn (default 1): classification + validity + field, the field alone, their
difference as the validity's share, the state walk on its own after an untimed solve, the passes, and the CPU statement
of tests/planner_oriented_ref.py (validity by masks, heap Dijkstra over the states), beside the disc figures of the run.
--replan adds the replan (rules 19 and 20) on both scenes, from host arrays, alternating in one process: (a) a full
solve of the changed grid, (b) kc_planner_replan of the same grid behind an untimed solve of the unchanged one, the
change a 5 x 5 blocked patch on the path 10 %, 50 % and 90 % of the way from the start, and (c) the replan with only
the start moved (no grid set); milliseconds, passes, the threshold, the touched cells and the tiles relaxed; with
--clearance the same with the cost on.
--frontiers adds the exploration (rules 21 to 26) on both scenes: the part of the map farther than --frontier-radius
cells from the robot (the scene's start) is turned to unknown; kc_planner_explore (r2 of the scene, min_cost 0, min_size
8) on the resident grid, the whole call and its three phases by the library's own host clock (validity + field, mark +
label, sizes + records), the field and label passes, the tiles labelled of all tiles, the frontiers kept of the
components, the path to the first; and the Python statement of tests/planner_frontier_ref.py on one CPU thread (numpy,
a heap Dijkstra and a flood fill in the interpreter: not a compiled CPU implementation).

--car R_MIN[,RW] adds a leg with car motion (rules 27 to 36) on the disc footprint of the scene: turn cells n from R_MIN
metres at 0.05 m, reverse weight RW (none without it), start heading 0, any goal heading: classification + validity +
moves + field, the field alone, the phases by the library's own host clock (maps + moves + init, field), the moves
kernels on their own (steps + moves + init behind a set_car that keeps the validity map, less the init), the walk with
its expansion on its own after an untimed solve, the passes, the states and arcs of the path.  May be given more than once.
The Python statement of tests/planner_car_ref.py is not run here: a heap Dijkstra in the interpreter over eight layers of
these maps takes minutes.

  python tools/planner_time.py [--reps 30] [--cpu-reps 1] [--clearance 20,40] [--shortcut 128] [--oriented 1.5,0.2]
                               [--car 0.5 --car 0.5,2] [--replan] [--frontiers] [--json out.json]
  rocprofv3 --kernel-trace --stats -d out -- python tools/planner_time.py --reps 5 --cpu-reps 0
"""
import argparse
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "kompass-core_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))
import kompass_hip as kh  # noqa: E402
import planner_car_ref as carref  # noqa: E402
import planner_clearance_ref as cref  # noqa: E402
import planner_frontier_ref as fref  # noqa: E402
import planner_oriented_ref as oref  # noqa: E402
import planner_ref as ref  # noqa: E402
import planner_shortcut_ref as sref  # noqa: E402
import synthetic as syn  # noqa: E402


def stats_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)), reps=reps)


def shortcut_leg(ctx, start, goal, r2, a):
    """The walk and the shortcut behind a solve of the resident grid, each call timed on its own."""
    span = a.shortcut
    walk_ms, short_ms = [], []
    for k in range(3 + a.reps):
        ctx.solve(start, goal, r2)
        t0 = time.perf_counter()
        walk = ctx.path()
        t1 = time.perf_counter()
        cells, idx, min_clear2 = ctx.shortcut(span)
        t2 = time.perf_counter()
        if k >= 3:
            walk_ms.append((t1 - t0) * 1e3)
            short_ms.append((t2 - t1) * 1e3)
    st = lambda t: dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)), reps=len(t))  # noqa: E731
    return dict(span=span, walk_ms=st(walk_ms), shortcut_ms=st(short_ms), path_cells=int(len(walk)), waypoints=int(len(idx)),
                longest_span=int(np.diff(idx).max()) if len(idx) > 1 else 0, walk_length_cells=sref.length_cells(walk),
                any_angle_length_cells=sref.length_cells(cells), min_clear2=int(min_clear2))


def print_shortcut(c, indent):
    print(f"{indent}shortcut span {c['span']}: {c['path_cells']} path cells -> {c['waypoints']} waypoints (longest span "
          f"{c['longest_span']}), length {c['walk_length_cells']:.1f} -> {c['any_angle_length_cells']:.1f} cells, smallest touched "
          f"clear2 {c['min_clear2']}")
    for k in ("walk_ms", "shortcut_ms"):
        v = c[k]
        print(f"{indent}  {k:22s} median {v['median']:10.3f}  min {v['min']:10.3f}  max {v['max']:10.3f}  ({v['reps']} reps)")


def replan_leg(ctx, host_grid, start, goal, r2, a):
    """(a), (b) and (c) of the module's text on the grid and cost the context holds."""
    ctx.set_grid(host_grid)
    ctx.solve(start, goal, r2)
    path = ctx.path()
    out = dict(legs=[])
    st = lambda t: dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)), reps=len(t))  # noqa: E731
    for pct in (10, 50, 90):
        ci, cj = (int(v) for v in path[len(path) * pct // 100])
        changed = host_grid.copy()
        changed[max(ci - 2, 0):ci + 3, max(cj - 2, 0):cj + 3] = 100
        full_ms, replan_ms = [], []
        for k in range(3 + a.reps):
            t0 = time.perf_counter()
            ctx.set_grid(changed)
            full = ctx.solve(start, goal, r2)
            t1 = time.perf_counter()
            ctx.set_grid(host_grid)
            ctx.solve(start, goal, r2)
            t2 = time.perf_counter()
            ctx.set_grid(changed)
            got = ctx.replan(start, goal, r2)
            t3 = time.perf_counter()
            if k >= 3:
                full_ms.append((t1 - t0) * 1e3)
                replan_ms.append((t3 - t2) * 1e3)
        kept, T, touched, tiles = ctx.replan_info()
        assert kept and got[:2] == full[:2]
        w, h = host_grid.shape
        out["legs"].append(dict(percent=pct, patch=[ci, cj], status=got[0], cost=got[1], full_solve_ms=st(full_ms), full_passes=full[2],
                                replan_ms=st(replan_ms), replan_passes=got[2], threshold=T, touched=touched, active_tiles=tiles,
                                tiles=-(-w // 64) * -(-h // 64)))
    ctx.set_grid(host_grid)
    ctx.solve(start, goal, r2)
    moved = tuple(int(v) for v in path[len(path) // 10])
    t = []
    for k in range(3 + a.reps):
        t0 = time.perf_counter()
        got = ctx.replan(moved if k % 2 else start, goal, r2)
        if k >= 3:
            t.append((time.perf_counter() - t0) * 1e3)
    assert ctx.replan_info() == (True, 0xFFFFFFFF, 0, 0) and got[2] == 0
    out["start_moved_ms"] = st(t)
    t = []
    for k in range(3 + a.reps):
        ctx.replan(moved if k % 2 else start, goal, r2)
        t0 = time.perf_counter()
        ctx.path()
        if k >= 3:
            t.append((time.perf_counter() - t0) * 1e3)
    out["walk_behind_it_ms"] = st(t)
    return out


def frontier_leg(ctx, host_grid, start, r2, a):
    """The scene's grid with everything beyond a radius of the robot unknown, then the scene's own grid again."""
    w, h = host_grid.shape
    ii, jj = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
    radius = min(a.frontier_radius, max(w, h))
    g = np.asarray(host_grid).copy()
    g[(ii - start[0]) ** 2 + (jj - start[1]) ** 2 > radius * radius] = ref.UNEXPLORED
    ctx.set_grid(g)
    st, comps, kept, passes, lpasses = ctx.explore(start, r2, 0, 8)
    listed, tiles, _ = ctx.explore_info()
    out = dict(radius_cells=radius, status=st, components=comps, kept=kept, passes=passes, label_passes=lpasses, listed_tiles=listed,
               tiles=tiles, first_path_cells=int(len(ctx.frontier_path(0))) if kept else 0)
    whole, phases = [], []
    for k in range(3 + a.reps):
        t0 = time.perf_counter()
        ctx.explore(start, r2, 0, 8)
        t1 = time.perf_counter()
        if k >= 3:
            whole.append((t1 - t0) * 1e3)
            phases.append(ctx.explore_info()[2])
    st_ = lambda t: dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)), reps=len(t))  # noqa: E731
    out["explore_ms"] = st_(whole)
    for k, name in enumerate(("field_ms", "mark_label_ms", "records_ms")):
        out[name] = st_([p[k] for p in phases])
    if kept:
        out["first_path_ms"] = stats_ms(lambda: ctx.frontier_path(0), a.reps)
    if a.cpu_reps > 0:
        t0 = time.perf_counter()
        want = fref.explore(g, start, r2, 0, 8, paths=False)
        dt = (time.perf_counter() - t0) * 1e3
        out["python_statement_one_thread_ms"] = dict(median=dt, min=dt, max=dt, reps=1)
        assert (want["status"], want["components"], len(want["frontiers"])) == (st, comps, kept)
        assert (ctx.frontier_labels() == want["labels"]).all()
    ctx.set_grid(host_grid)
    return out


def print_frontiers(f, indent):
    print(f"{indent}frontiers within {f['radius_cells']} cells: status {f['status']}, {f['kept']} kept of {f['components']} components, "
          f"{f['passes']} field passes, {f['label_passes']} label passes, {f['listed_tiles']} of {f['tiles']} tiles labelled, "
          f"{f['first_path_cells']} cells to the first")
    for k in ("explore_ms", "field_ms", "mark_label_ms", "records_ms", "first_path_ms", "python_statement_one_thread_ms"):
        if k in f:
            v = f[k]
            print(f"{indent}  {k:30s} median {v['median']:10.3f}  min {v['min']:10.3f}  max {v['max']:10.3f}  ({v['reps']} reps)")


def print_replan(r, indent):
    for leg in r["legs"]:
        f, p = leg["full_solve_ms"], leg["replan_ms"]
        print(f"{indent}patch at {leg['percent']} % of the path {leg['patch']}: full solve {f['median']:.3f} ms [{f['min']:.3f}, {f['max']:.3f}] "
              f"{leg['full_passes']} passes; replan {p['median']:.3f} ms [{p['min']:.3f}, {p['max']:.3f}] {leg['replan_passes']} passes, "
              f"{leg['active_tiles']} of {leg['tiles']} tiles, T {leg['threshold']}, {leg['touched']} touched, cost {leg['cost']}")
    for k in ("start_moved_ms", "walk_behind_it_ms"):
        v = r[k]
        print(f"{indent}{k:22s} median {v['median']:10.3f}  min {v['min']:10.3f}  max {v['max']:10.3f}  ({v['reps']} reps)")


def device_name():
    try:
        out = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=30).stdout
        names = [ln.split(":", 1)[1].strip() for ln in out.splitlines() if "Marketing Name" in ln]
        names = [n for n in names if n]
        gpus = [n for n in names if "Instinct" in n or "MI3" in n]
        return gpus[0] if gpus else (names[-1] if names else "unknown")
    except Exception:
        return "unknown"


def scene(name, ctx, host_grid, dev_ptr, elem, start, goal, r2, a):
    w, h = host_grid.shape
    out = dict(scene=name, cells=[w, h], r2=r2)
    # device-resident grid: classification + validity + field, then the same with the validity map kept
    ctx.set_grid_device(dev_ptr, w, h, elem)
    st, cost, passes = ctx.solve(start, goal, r2)
    out.update(status=st, cost=cost, passes=passes, launched=-(-passes // 8) * 8)

    def from_device():
        ctx.set_grid_device(dev_ptr, w, h, elem)
        ctx.solve(start, goal, r2)

    def from_host():
        ctx.set_grid(host_grid)
        ctx.solve(start, goal, r2)

    out["device_grid_ms"] = stats_ms(from_device, a.reps)
    out["host_grid_ms"] = stats_ms(from_host, a.reps)
    out["resolve_ms"] = stats_ms(lambda: ctx.solve(start, goal, r2), a.reps)   # grid and validity resident: field only

    def walk():
        ctx.solve(start, goal, r2)
        ctx.path()

    out["resolve_and_walk_ms"] = stats_ms(walk, a.reps)
    out["path_cells"] = int(len(ctx.path()))
    # what a host walk would have to pay first: the field's way back
    out["field_readback_ms"] = stats_ms(lambda: ctx.field(), max(3, a.reps // 5))
    if a.cpu_reps > 0:
        valid = ref.validity(host_grid, r2)
        out["cpu_validity_ms"] = stats_ms(lambda: ref.validity(host_grid, r2), a.cpu_reps, warm=0)
        out["cpu_dijkstra_ms"] = stats_ms(lambda: ref.cost_field(valid, goal), a.cpu_reps, warm=0)
        f, v = ctx.field()
        assert (f == ref.cost_field(valid, goal)).all() and (v == valid).all()
    if a.shortcut:
        out["shortcut"] = shortcut_leg(ctx, start, goal, r2, a)
    if a.replan:
        out["replan"] = replan_leg(ctx, np.asarray(host_grid), start, goal, r2, a)
    if a.frontiers:
        out["frontiers"] = frontier_leg(ctx, host_grid, start, r2, a)
    if a.clearance:
        out["clearance"] = clearance_leg(ctx, np.asarray(host_grid), start, goal, r2, a)
    if a.oriented:
        out["oriented"] = oriented_leg(ctx, host_grid, dev_ptr, elem, start, goal, a)
    if a.car:
        out["car"] = [car_leg(ctx, host_grid, dev_ptr, elem, start, goal, r2, spec, a) for spec in a.car]
    return out


def car_leg(ctx, host_grid, dev_ptr, elem, start, goal, r2, spec, a):
    """The same grid with car motion on (the scene's disc, start heading 0, any goal heading), then off again."""
    w, h = host_grid.shape
    v = spec.split(",")
    n, rw = carref.turn_cells(float(v[0]), 0.05), int(v[1]) if len(v) > 1 else 0
    ctx.set_car(n, rw)
    ctx.set_grid_device(dev_ptr, w, h, elem)
    try:
        st, cost, passes = ctx.solve_car(start, 0, goal, -1, r2)
    except IndexError as e:   # rule 32's bound: 24 n max(rw, 1) * 8 * cells has to fit 32 bits
        ctx.set_car(0)
        ctx.set_grid_device(dev_ptr, w, h, elem)
        return dict(r_min=float(v[0]), turn_cells=n, reverse_weight=rw, refused=str(e))
    states, prims = ctx.car_path()
    out = dict(r_min=float(v[0]), turn_cells=n, reverse_weight=rw, status=st, cost=cost, passes=passes, launched=-(-passes // 8) * 8,
               states=int(len(states)), arcs=int(np.isin(prims, (carref.L, carref.R, carref.BL, carref.BR)).sum()),
               reverse_primitives=int((prims >= carref.B).sum()), path_cells=int(len(ctx.path())))
    st_ = lambda t: dict(median=float(np.median(t)), min=float(min(t)), max=float(max(t)), reps=len(t))  # noqa: E731

    def timed(before):
        whole, ph0, ph1 = [], [], []
        for k in range(3 + a.reps):
            t0 = time.perf_counter()
            before()
            ctx.solve_car(start, 0, goal, -1, r2)
            t1 = time.perf_counter()
            if k >= 3:
                ms = ctx.car_info()[2]
                whole.append((t1 - t0) * 1e3)
                ph0.append(ms[0])
                ph1.append(ms[1])
        return st_(whole), st_(ph0), st_(ph1)

    # the grid again: forgets the validity map and the moves; set_car again: the moves alone; nothing: the field alone
    out["device_grid_ms"], out["maps_moves_init_ms"], _ = timed(lambda: ctx.set_grid_device(dev_ptr, w, h, elem))
    _, out["moves_init_ms"], _ = timed(lambda: ctx.set_car(n, rw))
    out["resolve_ms"], out["init_ms"], out["field_ms"] = timed(lambda: None)
    out["moves_ms_by_difference"] = out["moves_init_ms"]["median"] - out["init_ms"]["median"]
    walk_ms = []
    for k in range(3 + a.reps):
        ctx.solve_car(start, 0, goal, -1, r2)
        t0 = time.perf_counter()
        ctx.car_path()
        if k >= 3:
            walk_ms.append((time.perf_counter() - t0) * 1e3)
    out["walk_ms"] = st_(walk_ms)
    ctx.set_car(0)
    ctx.set_grid_device(dev_ptr, w, h, elem)
    return out


def oriented_leg(ctx, host_grid, dev_ptr, elem, start, goal, a):
    """The same grid with the oriented footprint on, then off again."""
    w, h = host_grid.shape
    v = [float(x) for x in a.oriented.split(",")]
    a2, b2 = oref.box_a2_b2((v[0], v[1]), 0.0, 0.05)
    turn10 = int(round((v[2] if len(v) > 2 else 1.0) * 10))
    ctx.set_oriented(a2, b2, turn10)
    ctx.set_grid_device(dev_ptr, w, h, elem)
    st, cost, passes = ctx.solve_oriented(start, 0, goal)
    states = ctx.oriented_path()
    f, valid, turn = ctx.oriented_field()
    out = dict(a2=a2, b2=b2, turn10=turn10, mask_offsets=[len(oref.oriented_mask(k, a2, b2)) for k in range(4)], status=st,
               cost=cost, passes=passes, launched=-(-passes // 8) * 8, states=int(len(states)), path_cells=int(len(ctx.path())),
               turns=int((np.diff(states[:, 2]) != 0).sum()) if len(states) else 0,
               valid_states=[int(x) for x in valid.sum(axis=(1, 2))], turn_valid_cells=int(turn.sum()))

    def from_device():
        ctx.set_grid_device(dev_ptr, w, h, elem)   # forgets the validity maps
        ctx.solve_oriented(start, 0, goal)

    out["device_grid_ms"] = stats_ms(from_device, a.reps)
    out["resolve_ms"] = stats_ms(lambda: ctx.solve_oriented(start, 0, goal), a.reps)   # validity resident: field only
    out["validity_ms_by_difference"] = out["device_grid_ms"]["median"] - out["resolve_ms"]["median"]
    walk_ms = []
    for k in range(3 + a.reps):
        ctx.solve_oriented(start, 0, goal)
        t0 = time.perf_counter()
        ctx.oriented_path()
        if k >= 3:
            walk_ms.append((time.perf_counter() - t0) * 1e3)
    out["walk_ms"] = dict(median=float(np.median(walk_ms)), min=float(min(walk_ms)), max=float(max(walk_ms)), reps=len(walk_ms))
    if a.cpu_reps > 0:
        t0 = time.perf_counter()
        want_valid, want_turn = oref.oriented_validity(host_grid, a2, b2), oref.turn_validity(host_grid, a2, b2)
        t1 = time.perf_counter()
        want = oref.state_field(want_valid, want_turn, goal, turn10)
        t2 = time.perf_counter()
        out["cpu_validity_ms"] = dict(median=(t1 - t0) * 1e3, min=(t1 - t0) * 1e3, max=(t1 - t0) * 1e3, reps=1)
        out["cpu_dijkstra_ms"] = dict(median=(t2 - t1) * 1e3, min=(t2 - t1) * 1e3, max=(t2 - t1) * 1e3, reps=1)
        assert (valid == want_valid).all() and (turn == want_turn).all() and (f == want).all()
    ctx.set_oriented(0)
    ctx.set_grid_device(dev_ptr, w, h, elem)
    return out


def clearance_leg(ctx, host_grid, start, goal, r2, a):
    """The same grid (resident) with the clearance cost on, then off again."""
    reach, wt = (int(v) for v in a.clearance.split(","))
    c2 = min(int((r2 ** 0.5 + reach) ** 2), cref.MAX_C2)
    table = cref.clearance_table(wt, r2, c2)
    ctx.set_clearance_cost(c2, table)
    st, cost, passes = ctx.solve(start, goal, r2)
    cells = ctx.path()
    out = dict(c2=c2, weight10=wt, status=st, cost=cost, passes=passes, launched=-(-passes // 8) * 8,
               path_cells=int(len(cells)), path_length=cref.path_length(cells), min_clear2=ctx.path_clearance())

    def with_clearance_pass():
        ctx.set_clearance_cost(c2, table)   # forgets clear2, the penalty and the validity map
        ctx.solve(start, goal, r2)

    def walk():
        ctx.solve(start, goal, r2)
        ctx.path()

    out["table_clearance_field_ms"] = stats_ms(with_clearance_pass, a.reps)
    out["resolve_ms"] = stats_ms(lambda: ctx.solve(start, goal, r2), a.reps)   # clear2 and penalty resident: field only
    out["resolve_and_walk_ms"] = stats_ms(walk, a.reps)
    if a.shortcut:
        out["shortcut"] = shortcut_leg(ctx, start, goal, r2, a)
    if a.replan:
        out["replan"] = replan_leg(ctx, host_grid, start, goal, r2, a)
    ctx.set_clearance_cost(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--cpu-reps", type=int, default=1)
    ap.add_argument("--clearance", default=None, metavar="REACH_CELLS,WEIGHT10")
    ap.add_argument("--shortcut", type=int, default=0, metavar="W", help="time the any-angle path of span W")
    ap.add_argument("--oriented", default=None, metavar="X,Y[,TURN]", help="time the oriented footprint of an X x Y m box")
    ap.add_argument("--car", action="append", default=None, metavar="R_MIN[,RW]", help="time car motion of R_MIN metres of turning radius")
    ap.add_argument("--replan", action="store_true", help="time the replan against a full solve of the changed grid")
    ap.add_argument("--frontiers", action="store_true", help="time kc_planner_explore with the far part of the map unknown")
    ap.add_argument("--frontier-radius", type=int, default=300, metavar="CELLS", help="what the robot knows, in cells around it")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if kh.device_count() < 1:
        raise SystemExit("needs a HIP device")
    ctx, cloud = kh.PlannerContext(), kh.CloudContext()
    res = []
    # the PCD benchmark's map, the grid where kc_cloud_grid_device leaves it (int8)
    pts = syn.pcd_indoor_map_doors(2_000_000)
    host_grid, origin = cloud.occupancy_grid(pts, 0.05, 0.1, 1.0)
    dev, (cx, cy), _ = cloud.occupancy_grid(pts, 0.05, 0.1, 1.0, to_host=False)
    cell = lambda x, y: (ref.world_to_cell(x, origin[0], 0.05), ref.world_to_cell(y, origin[1], 0.05))  # noqa: E731
    res.append(scene("pcd 2004 x 1204", ctx, host_grid, dev, 1, cell(2.5, 2.5), cell(97.5, 57.5),
                     ref.radius_to_r2(0.2, 0.05), a))
    # 500 x 500 clutter, int32 as the mapper writes it, in a device buffer of the tool's own
    rng = np.random.default_rng(3)
    g = np.asfortranarray(np.where(rng.random((500, 500)) < 0.1, 100, 0).astype(np.int32))
    g[:8, :8] = g[-8:, -8:] = 0
    hip = C.CDLL("libamdhip64.so")
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(g.nbytes)) == 0
    assert hip.hipMemcpy(buf, C.c_void_p(g.ctypes.data), C.c_size_t(g.nbytes), 1) == 0
    res.append(scene("clutter 500 x 500", ctx, g, buf.value, 4, (3, 3), (496, 496), 1, a))
    hip.hipFree(buf)
    out = dict(device=device_name(), date=time.strftime("%Y-%m-%d"), scenes=res)
    for s in res:
        print(f"{s['scene']}: status {s['status']}, cost {s['cost']}, {s['passes']} passes ({s['launched']} launched), "
              f"{s['path_cells']} path cells")
        for k in ("device_grid_ms", "host_grid_ms", "resolve_ms", "resolve_and_walk_ms", "field_readback_ms",
                  "cpu_validity_ms", "cpu_dijkstra_ms"):
            if k in s:
                v = s[k]
                print(f"  {k:22s} median {v['median']:10.3f}  min {v['min']:10.3f}  max {v['max']:10.3f}  ({v['reps']} reps)")
        if "shortcut" in s:
            print_shortcut(s["shortcut"], "  ")
        if "replan" in s:
            print_replan(s["replan"], "  ")
        if "frontiers" in s:
            print_frontiers(s["frontiers"], "  ")
        c = s.get("clearance")
        if c:
            print(f"  clearance cost C2 {c['c2']}, weight {c['weight10']}: status {c['status']}, cost {c['cost']}, length "
                  f"{c['path_length']}, {c['passes']} passes ({c['launched']} launched), {c['path_cells']} path cells, "
                  f"min clear2 {c['min_clear2']}")
            for k in ("table_clearance_field_ms", "resolve_ms", "resolve_and_walk_ms"):
                v = c[k]
                print(f"    {k:24s} median {v['median']:10.3f}  min {v['min']:10.3f}  max {v['max']:10.3f}  ({v['reps']} reps)")
            if "shortcut" in c:
                print_shortcut(c["shortcut"], "    ")
            if "replan" in c:
                print_replan(c["replan"], "    ")
        o = s.get("oriented")
        if o:
            print(f"  oriented footprint A2 {o['a2']}, B2 {o['b2']}, turn {o['turn10']}, offsets {o['mask_offsets']}: status "
                  f"{o['status']}, cost {o['cost']}, {o['passes']} passes ({o['launched']} launched), {o['states']} states, "
                  f"{o['path_cells']} path cells, {o['turns']} turns, valid states {o['valid_states']}, turn-valid cells "
                  f"{o['turn_valid_cells']}")
            for k in ("device_grid_ms", "resolve_ms", "walk_ms", "cpu_validity_ms", "cpu_dijkstra_ms"):
                if k in o:
                    v = o[k]
                    print(f"    {k:24s} median {v['median']:10.3f}  min {v['min']:10.3f}  max {v['max']:10.3f}  ({v['reps']} reps)")
            print(f"    validity, by difference  {o['validity_ms_by_difference']:10.3f} ms")
        for c in s.get("car", []):
            if "refused" in c:
                print(f"  car motion R_min {c['r_min']} m, n {c['turn_cells']}, reverse weight {c['reverse_weight']}: refused: {c['refused']}")
                continue
            print(f"  car motion R_min {c['r_min']} m, n {c['turn_cells']}, reverse weight {c['reverse_weight']}: status {c['status']}, cost "
                  f"{c['cost']}, {c['passes']} passes ({c['launched']} launched), {c['states']} states, {c['arcs']} arcs, "
                  f"{c['reverse_primitives']} reverse primitives, {c['path_cells']} path cells")
            for k in ("device_grid_ms", "resolve_ms", "maps_moves_init_ms", "moves_init_ms", "init_ms", "field_ms", "walk_ms"):
                v = c[k]
                print(f"    {k:24s} median {v['median']:10.3f}  min {v['min']:10.3f}  max {v['max']:10.3f}  ({v['reps']} reps)")
            print(f"    moves, by difference     {c['moves_ms_by_difference']:10.3f} ms")
    print(json.dumps(out))
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1))
    ctx.close()
    cloud.close()


if __name__ == "__main__":
    main()
