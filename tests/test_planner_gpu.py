"""The grid planner on the MI355X (kc_planner_*, kompass_cpp.planning, kompass_core.planning): the
device's validity map and cost field bit for bit against the CPU statement of tests/planner_ref.py, the path
cell for cell against its walk, host and device-resident grids against each other, and the closed loop PCD room ->
grid -> GridPlanner -> Path -> DWA / PurePursuit.  A scene the statement cannot solve is unsolved on both sides, and
every scene with a valid cell has one pair from one connected component of the statement's field, so a path is
compared in each.

Every test runs under a time limit.  A solve that went wrong would not hang, but it would run to its pass cap (cells
+ 1 launches over the whole grid: minutes at 2004 x 1204), and a Python-level limit cannot interrupt a native call;
the thread method ends the process instead, and the device work with it."""
import json
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

TIME_LIMIT_S = 120   # the slowest test takes 2 to 3 s on an MI355X box; a loaded box gets forty times that

# the slowest cases (500 x 500 clutter, 2004 x 1204, the DWA closed loop) spend their seconds in the statement's
# Python Dijkstra and in the oracle, not on the device
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(TIME_LIMIT_S, method="thread")]

import kompass_cpp  # noqa: E402
import kompass_hip as kh  # noqa: E402
import planner_ref as ref  # noqa: E402
import synthetic as syn  # noqa: E402

GOLD = Path(__file__).parent / "golden"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert kh.device_count() >= 1, "no HIP device visible"


@pytest.fixture()
def ctx():
    c = kh.PlannerContext()
    yield c
    c.close()


def compare(ctx, grid, pairs, r2, allow_unknown=True, valid=None):
    """Every (start, goal) pair of `pairs` on the grid the context holds: status, validity, field, cost, path and
    the path's own rules against the statement; the pass cap is not hit (the solve would raise).  -> statuses."""
    w, h = grid.shape
    valid = ref.validity(grid, r2, allow_unknown) if valid is None else valid
    seen = []
    for start, goal in pairs:
        st, cost, passes = ctx.solve(start, goal, r2, allow_unknown)
        f, v = ctx.field()
        np.testing.assert_array_equal(v, valid)
        want = ref.cost_field(valid, goal)
        np.testing.assert_array_equal(f, want)
        wst = ref.status(valid, want, start, goal)
        assert st == wst, (start, goal, st, wst)
        assert 0 <= passes <= w * h + 1
        cells = ctx.path()
        if wst == ref.FOUND:
            assert cost == want[start[0], start[1]] and passes >= 1
            np.testing.assert_array_equal(cells, ref.walk(valid, want, start))
            ref.check_path(valid, cells, start, goal)
        else:
            assert cost == ref.INF and len(cells) == 0
        seen.append(st)
    return seen


def connected_pair(valid, seeds):
    """(start, goal) inside one connected component of the statement's field: the seed that reaches farthest is the
    goal, the cell farthest from it the start.  None when no seed is a valid cell."""
    best = None
    for seed in dict.fromkeys(seeds):
        if not valid[seed]:
            continue
        reach = ref.cost_field(valid, seed)
        reach = np.where(reach == ref.INF, 0, reach)
        far = tuple(int(v) for v in np.unravel_index(np.argmax(reach), reach.shape)) if reach.any() else seed  # alone
        if best is None or reach[far] > best[0]:
            best = (int(reach[far]), far, seed)
    return None if best is None else (best[1], best[2])


def free_cells(valid, rng, n):
    idx = np.argwhere(valid)
    return [tuple(int(v) for v in idx[k]) for k in rng.integers(0, len(idx), n)] if len(idx) else [(0, 0)] * n


@pytest.mark.parametrize("shape", [(130, 97), (64, 64), (257, 63), (65, 300), (1, 90), (500, 500)])
@pytest.mark.parametrize("density", [0.02, 0.15, 0.35])
def test_random_clutter(ctx, shape, density):
    rng = np.random.default_rng(hash((shape, int(density * 100))) % 2 ** 32)
    grid = np.where(rng.random(shape) < density, 100, 0).astype(np.int32)
    grid[rng.random(shape) < 0.05] = -1
    ctx.set_grid(grid)
    for r2, unknown in [(0, True), (1, False), (5, True)] if shape != (500, 500) else [(2, True)]:
        valid = ref.validity(grid, r2, unknown)
        cells = free_cells(valid, rng, 4)
        pairs = [(cells[0], cells[1]), (cells[2], cells[3]), (cells[0], cells[0])]
        # one pair with a blocked end and one with an end outside the grid
        occ = np.argwhere(~valid)
        if len(occ):
            pairs.append((cells[1], tuple(int(v) for v in occ[0])))
        pairs.append(((shape[0], 0), cells[2]))
        compare(ctx, grid, pairs, r2, unknown, valid)
        # one pair the statement solves, wherever a cell is valid at all
        pair = connected_pair(valid, cells)
        assert (pair is None) == (not valid.any())
        if pair is not None:
            assert compare(ctx, grid, [pair], r2, unknown, valid) == [ref.FOUND]
        else:
            assert compare(ctx, grid, [((0, 0), (shape[0] - 1, shape[1] - 1))], r2, unknown, valid) == [ref.START_INVALID]


def maze(cells_w, cells_h, seed, scale=3):
    """A perfect maze by depth-first carving, corridors `scale - 1` cells wide."""
    rng = np.random.default_rng(seed)
    open_ = np.zeros((2 * cells_w + 1, 2 * cells_h + 1), bool)
    stack, seen = [(0, 0)], {(0, 0)}
    open_[1, 1] = True
    while stack:
        x, y = stack[-1]
        nb = [(x + dx, y + dy) for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1))
              if 0 <= x + dx < cells_w and 0 <= y + dy < cells_h and (x + dx, y + dy) not in seen]
        if not nb:
            stack.pop()
            continue
        nx, ny = nb[rng.integers(len(nb))]
        open_[x + nx + 1, y + ny + 1] = open_[2 * nx + 1, 2 * ny + 1] = True
        seen.add((nx, ny))
        stack.append((nx, ny))
    big = np.repeat(np.repeat(open_, scale, axis=0), scale, axis=1)
    return np.where(big, 0, 100).astype(np.int32)


def serpentine(w, h, pitch=4):
    """Walls every `pitch` columns with the gap alternating between the two ends: one long corridor that crosses
    every tile many times."""
    g = np.zeros((w, h), np.int32)
    for k, i in enumerate(range(pitch - 1, w - 1, pitch)):
        g[i, :] = 100
        if k % 2:
            g[i, :2] = 0
        else:
            g[i, -2:] = 0
    return g


def test_mazes(ctx):
    for seed, (cw, ch), scale in [(1, (20, 15), 3), (2, (33, 40), 2), (3, (12, 12), 6)]:
        g = maze(cw, ch, seed, scale)
        ctx.set_grid(g)
        a, b = (scale, scale), (g.shape[0] - scale - 1, g.shape[1] - scale - 1)
        assert compare(ctx, g, [(a, b), (b, a)], 0) == [ref.FOUND, ref.FOUND]
        if scale >= 6:  # room for a one-cell footprint: two cells off the walls
            a2, b2 = (a[0] + 2, a[1] + 2), (b[0] - 2, b[1] - 2)
            assert compare(ctx, g, [(a2, b2)], 1) == [ref.FOUND]
    g = serpentine(150, 140)
    ctx.set_grid(g)
    st, cost, passes = ctx.solve((0, 0), (149, 139), 0)
    assert st == ref.FOUND and cost > 10 * 140 * 30 and passes > 30
    assert compare(ctx, g, [((0, 0), (149, 139)), ((148, 0), (1, 1))], 0) == [ref.FOUND, ref.FOUND]
    # the closed corridor
    g[3, :] = 100
    ctx.set_grid(g)
    assert compare(ctx, g, [((0, 0), (149, 139))], 0) == [ref.UNREACHABLE]


@pytest.mark.parametrize("name", ["pcd_room_ascii.pcd", "pcd_room_binary.pcd"])
def test_pcd_room_device_grid_and_host_grid(ctx, name):
    pts = np.ascontiguousarray(kompass_cpp.utils.read_pcd(str(GOLD / name)))
    cloud = kh.CloudContext()
    for res, rh in [(0.1, 2.5), (0.05, 1.0)]:
        host_grid, origin = cloud.occupancy_grid(pts, res, 0.05, rh)
        dev, (cx, cy), origin_d = cloud.occupancy_grid(pts, res, 0.05, rh, to_host=False)
        assert (cx, cy) == host_grid.shape and dev
        r2 = ref.radius_to_r2(0.2, res)
        valid = ref.validity(host_grid, r2)
        rng = np.random.default_rng(7)
        cells = free_cells(valid, rng, 4)
        pairs = [(cells[0], cells[1]), (cells[2], cells[3]), connected_pair(valid, cells)]
        ctx.set_grid_device(dev, cx, cy, elem_bytes=1)   # the PCD grid where kc_cloud_grid_device left it
        seen = compare(ctx, host_grid, pairs, r2, True, valid)
        assert seen[2] == ref.FOUND
        f_dev, v_dev = ctx.field()
        ctx.set_grid(host_grid)
        assert compare(ctx, host_grid, pairs, r2, True, valid) == seen
        f_host, v_host = ctx.field()
        np.testing.assert_array_equal(f_dev, f_host)
        np.testing.assert_array_equal(v_dev, v_host)
        # unknown cells block: the sparse floor of the room leaves little to walk on, both sides agree on what
        compare(ctx, host_grid, pairs, 0, False)
    cloud.close()


def _scan():
    d = json.loads((GOLD / "laserscan_data.json").read_text())
    rng = np.array(d["ranges"], np.float64)
    ang = d["angle_min"] + d["angle_increment"] * np.arange(len(rng))
    return ang, rng


def test_mapper_grid_where_it_lies(ctx):
    ang, rng = _scan()
    for H, W, res in [(100, 100, 0.1), (150, 90, 0.05)]:
        m = kh.MapperContext(H, W, res, (0.0, 0.0, 0.0), 0.0, len(ang))
        host_grid = np.array(m.scan_to_grid(ang, rng))
        assert (host_grid == 100).any() and (host_grid == 0).any() and (host_grid == -1).any()
        m.scan_to_grid_device(ang, rng)
        m.sync()
        ctx.set_grid_device(m.grid_device_ptr(), H, W, elem_bytes=4)
        c0, c1 = H // 2 - 1, W // 2 - 1
        # the cell the statement finds farthest from the sensor's cell with unknown cells shut
        reach = ref.cost_field(ref.validity(host_grid, 2, False), (c0, c1))
        far = tuple(int(v) for v in np.unravel_index(np.argmax(np.where(reach == ref.INF, 0, reach)), reach.shape))
        assert reach[far] > 100
        pairs = [((c0, c1), far), (far, (c0, c1)), ((0, 0), (c0, c1))]
        for r2, unknown in [(2, False), (2, True), (0, True)]:
            seen = compare(ctx, host_grid, pairs, r2, unknown)
            f_dev, _ = ctx.field()
            assert seen[0] == ref.FOUND
        ctx.set_grid(host_grid)
        compare(ctx, host_grid, pairs, 0, True)
        np.testing.assert_array_equal(ctx.field()[0], f_dev)
        m.close()


def test_pcd_benchmark_grid_2004_x_1204(ctx):
    """The PCD benchmark's map (100 x 60 m at 0.05 m) with doorways, corner to corner, from the device grid."""
    pts = syn.pcd_indoor_map_doors(2_000_000)
    cloud = kh.CloudContext()
    host_grid, origin = cloud.occupancy_grid(pts, 0.05, 0.1, 1.0)
    assert host_grid.shape == (2004, 1204)
    dev, (cx, cy), _ = cloud.occupancy_grid(pts, 0.05, 0.1, 1.0, to_host=False)
    ctx.set_grid_device(dev, cx, cy, elem_bytes=1)
    r2 = ref.radius_to_r2(0.2, 0.05)
    cell = lambda x, y: (ref.world_to_cell(x, origin[0], 0.05), ref.world_to_cell(y, origin[1], 0.05))
    seen = compare(ctx, host_grid, [(cell(2.5, 2.5), cell(97.5, 57.5))], r2)
    assert seen == [ref.FOUND]
    st, cost, passes = ctx.solve(cell(2.5, 2.5), cell(97.5, 57.5), r2)
    print(f"2004 x 1204: cost {cost}, {passes} passes, {len(ctx.path())} path cells")
    cloud.close()


def test_refusals(ctx):
    with pytest.raises(kh.KompassHipError):
        ctx.solve((0, 0), (1, 1))                       # no grid yet
    g = np.zeros((8, 8), np.int32)
    with pytest.raises(ValueError):
        ctx.set_grid_device(g.ctypes.data, 8, 8, 4)     # host memory is not a device grid
    with pytest.raises(ValueError):
        ctx.set_grid(np.zeros((8, 8), np.float32))
    with pytest.raises(ValueError):
        kh._check(kh.lib().kc_planner_set_grid_host(ctx.h, g.ctypes.data, 2, 8, 8))
    with pytest.raises(IndexError):
        kh._check(kh.lib().kc_planner_set_grid_host(ctx.h, g.ctypes.data, 4, 1 << 15, 1 << 14))  # above the cell cap
    ctx.set_grid(g)
    with pytest.raises(IndexError):
        ctx.solve((0, 0), (1, 1), r2=255 * 255)
    assert ctx.solve((0, 0), (7, 7), r2=254 * 254)[0] == ref.FOUND
    with pytest.raises(kh.KompassHipError):
        kh.PlannerContext().field()                     # before any solve


def test_device_tensor_through_the_array_interface():
    """A torch tensor needs torch's HIP runtime to be the process's only one (torch imported before kompass_cpp,
    DESIGN.md 4.8): the check runs in a fresh process, _torch_planner_worker.py, under a limit of its own."""
    worker = Path(__file__).resolve().parent / "_torch_planner_worker.py"
    p = subprocess.run([sys.executable, str(worker)], capture_output=True, text=True, timeout=TIME_LIMIT_S - 30)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]


def test_front_end_says_what_it_lacks():
    from kompass_core.mapping import LocalMapper, MapConfig
    from kompass_core.planning import GridPlanner

    fe = GridPlanner(_robot())
    with pytest.raises(ValueError, match="map_meta_data"):
        fe.setup_problem(None, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0)
    with pytest.raises(ValueError, match="map_meta_data"):
        fe.setup_problem(None, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, grid=np.zeros((8, 8), np.int32))
    with pytest.raises(ValueError, match="resolution"):
        fe.setup_problem(dict(origin_x=0.0, origin_y=0.0, width=8, height=8), 0.0, 0.0, 0.0, 1.0, 1.0, 0.0)
    with pytest.raises(ValueError, match="no grid yet"):
        fe.setup_problem(None, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, grid=LocalMapper(MapConfig()))


def _shape_dims():
    G = kompass_cpp.types.RobotGeometry
    return [(G.CYLINDER, ref.CYLINDER, [0.2, 0.4]), (G.BOX, ref.BOX, [0.5, 0.3, 0.4]), (G.SPHERE, ref.SPHERE, [0.25])]


def test_class_against_the_statement():
    rng = np.random.default_rng(11)
    grid = np.where(rng.random((120, 80)) < 0.03, 100, 0).astype(np.int32)
    grid[rng.random((120, 80)) < 0.1] = -1
    origin, res = (-3.0, 1.5), 0.05
    for shape, rshape, dims in _shape_dims():
        for unknown, margin, simplify in [(True, 0.0, False), (False, 0.05, True)]:
            p = kompass_cpp.planning.GridPlanner(shape, dims, allow_unknown=unknown, margin=margin)
            p.set_space_bounds_from_map(origin[0], origin[1], 120, 80, res)
            p.set_grid(grid if unknown else grid.astype(np.int8))
            radius = ref.footprint_radius(rshape, dims) + float(np.float32(margin))
            assert p.get_footprint_r2() == ref.radius_to_r2(radius, res)
            for sx, sy, gx, gy in [(-2.8, 1.7, 2.7, 5.2), (2.0, 5.0, -2.5, 2.0), (-2.8, 1.7, 9.0, 2.0),
                                   (float("nan"), 0.0, 0.0, 2.0)]:
                want = ref.plan(grid, origin, res, (sx, sy), (gx, gy), radius, unknown, simplify)
                p.setup_problem(sx, sy, 0.0, gx, gy, 0.0)
                ok = p.solve()
                assert ok == (want["status"] == ref.FOUND) and p.get_status() == want["status"]
                assert p.get_cells() == (want["start"], want["goal"])
                path = p.get_solution(simplify)
                if not ok:
                    assert path is None and p.get_cost() == float("inf") and len(p.get_path_cells()) == 0
                    continue
                np.testing.assert_array_equal(p.get_path_cells(simplify), want["cells"])
                np.testing.assert_array_equal(np.asarray(path.x()), want["points"][:, 0])
                np.testing.assert_array_equal(np.asarray(path.y()), want["points"][:, 1])
                assert np.float32(p.get_cost()) == want["cost"]
    with pytest.raises(ValueError):
        p.set_grid(np.zeros((10, 10), np.int32))  # not the announced shape


def _robot(dims=(0.1, 0.4)):
    from kompass_core.models import Robot, RobotGeometry, RobotType
    return Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER,
                 geometry_params=np.array(dims))


def test_front_end_with_a_mapper_and_a_device_grid():
    from kompass_core.planning import GridPlanner

    ang, rng = _scan()
    H, W, res = 120, 120, 0.1
    mapper = kompass_cpp.mapping.LocalMapper(grid_height=H, grid_width=W, resolution=res, laserscan_position=[0.0, 0.0, 0.0],
                                             laserscan_orientation=0.0, is_pointcloud=False, scan_size=len(ang),
                                             angle_step=0.0175, max_height=1.0, min_height=0.0, range_max=20.0)
    grid = np.array(mapper.scan_to_grid(ang, rng))
    fe = GridPlanner(_robot(), allow_unknown=False, margin=0.1)
    c0, c1 = H // 2 - 1, W // 2 - 1
    origin = (np.float32(-c0) * np.float32(res), np.float32(-c1) * np.float32(res))
    radius = ref.footprint_radius(ref.CYLINDER, [0.1, 0.4]) + float(np.float32(0.1))
    reach = ref.cost_field(ref.validity(grid, ref.radius_to_r2(radius, res), False), (c0, c1))
    far = np.unravel_index(np.argmax(np.where(reach == ref.INF, 0, reach)), reach.shape)
    goal = (float(ref.cell_to_world(far[0], origin[0], res)) + 0.01, float(ref.cell_to_world(far[1], origin[1], res)) + 0.01)
    want = ref.plan(grid, origin, res, (0.0, 0.0), goal, radius, False)
    assert want["status"] == ref.FOUND
    fe.setup_problem(None, 0.0, 0.0, 0.0, goal[0], goal[1], 0.0, grid=mapper)   # the mapper's grid on the device
    path = fe.solve()
    np.testing.assert_array_equal(fe.path_cells, want["cells"])
    np.testing.assert_array_equal(np.asarray(path.x()), want["points"][:, 0])
    assert np.float32(fe.get_cost()) == want["cost"]
    # the same map as metadata + host array
    meta = dict(origin_x=float(origin[0]), origin_y=float(origin[1]), width=H, height=W, resolution=res)
    fe.setup_problem(meta, 0.0, 0.0, 0.0, goal[0], goal[1], 0.0, grid=grid)
    assert fe.solve() is not None
    np.testing.assert_array_equal(fe.path_cells, want["cells"])
    # a goal inside a wall: no path, no exception
    occ = np.argwhere(grid == 100)[0]
    fe.setup_problem(meta, 0.0, 0.0, 0.0, float(ref.cell_to_world(occ[0], origin[0], res)) + 0.01,
                     float(ref.cell_to_world(occ[1], origin[1], res)) + 0.01, 0.0)
    assert fe.solve() is None and fe.status == ref.GOAL_INVALID


# ---- closed loop: PCD room -> grid -> GridPlanner -> Path -> followers -------------------------------------------
ROBOT_RADIUS = 0.1


def _room_plan():
    from kompass_core.planning import GridPlanner

    res = 0.1
    grid, origin = kompass_cpp.utils.read_pcd_to_occupancy_grid(str(GOLD / "pcd_room_ascii.pcd"), res, 0.05, 2.5)
    pts = np.asarray(kompass_cpp.utils.read_pcd(str(GOLD / "pcd_room_ascii.pcd")))
    obstacles = np.ascontiguousarray(pts[np.isfinite(pts).all(axis=1) & (pts[:, 2] > 0.05) & (pts[:, 2] <= 2.5)])
    assert len(obstacles) == 15
    fe = GridPlanner(_robot((ROBOT_RADIUS, 0.4)), margin=0.25)
    meta = dict(origin_x=origin[0], origin_y=origin[1], width=grid.shape[0], height=grid.shape[1], resolution=res)
    # along the wall y = -1.5 to the corner it makes with the wall x = 2
    start, goal = (-1.7, -1.0), (1.5, -0.7)
    fe.setup_problem(meta, start[0], start[1], 0.0, goal[0], goal[1], 0.0, grid=grid)
    path = fe.solve()
    want = ref.plan(np.asarray(grid), origin[:2], res, start, goal, ROBOT_RADIUS + float(np.float32(0.25)))
    assert want["status"] == ref.FOUND and path is not None
    np.testing.assert_array_equal(fe.path_cells, want["cells"])
    xy = np.stack([np.asarray(path.x()), np.asarray(path.y())], 1)
    d = np.hypot(xy[:, None, 0] - obstacles[None, :, 0], xy[:, None, 1] - obstacles[None, :, 1]).min()
    assert d >= ROBOT_RADIUS + 0.25 - res * math.sqrt(2) - 1e-6   # a point lies anywhere in its cell
    return xy, obstacles


def test_closed_loop_dwa():
    from kompass_core.control import DWAConfig, TrajectoryCostsWeights
    from kompass_core.models import AngularCtrlLimits, LinearCtrlLimits, RobotGeometry, RobotType
    from test_gpu_controller import lockstep, make_pair

    xy, obstacles = _room_plan()
    cfg = DWAConfig(max_linear_samples=11, max_angular_samples=11, octree_resolution=0.1,
                    costs_weights=TrajectoryCostsWeights(reference_path_distance_weight=1.0, goal_distance_weight=3.0,
                                                         obstacles_distance_weight=1.0, smoothness_weight=0.0,
                                                         jerk_weight=0.0),
                    prediction_horizon=20, control_horizon=2, control_time_step=0.1)
    robot, gpu, cpu = make_pair(RobotType.OMNI, RobotGeometry.Type.CYLINDER, [ROBOT_RADIUS, 0.4],
                                LinearCtrlLimits(max_vel=1.0, max_acc=2.0, max_decel=2.0),
                                AngularCtrlLimits(max_vel=2.0, max_acc=3.0, max_decel=3.0, max_steer=2.0), cfg,
                                vy_lim=LinearCtrlLimits(max_vel=1.0, max_acc=2.0, max_decel=2.0))
    end, n, cycles = lockstep(robot, gpu, cpu, [tuple(p) for p in xy], (float(xy[0, 0]), float(xy[0, 1]), 0.0),
                              cloud=obstacles, max_controls=600, clearance_to=obstacles)
    assert end is True, f"goal not reached after {n} controls"
    assert cycles > 5
    assert lockstep.min_clearance >= ROBOT_RADIUS, f"clearance {lockstep.min_clearance}"


def test_closed_loop_pure_pursuit():
    from kompass_core.control import PurePursuit, PurePursuitConfig
    from kompass_core.models import AngularCtrlLimits, LinearCtrlLimits, RobotCtrlLimits, RobotState

    xy, obstacles = _room_plan()
    robot = _robot((ROBOT_RADIUS, 0.4))
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=0.5, max_acc=2.0, max_decel=2.0),
                          omega_limits=AngularCtrlLimits(max_vel=1.5, max_steer=0.7, max_acc=3.0, max_decel=3.0))
    fe = PurePursuit(robot, lim, config=PurePursuitConfig(wheel_base=robot.wheelbase, lookahead_distance=0.4),
                     control_time_step=0.1)
    fe.set_path(xy)
    heading = math.atan2(xy[3, 1] - xy[0, 1], xy[3, 0] - xy[0, 0])
    state = RobotState(x=float(xy[0, 0]), y=float(xy[0, 1]), yaw=heading, speed=0.0)
    clearance, reached = float("inf"), False
    for _ in range(600):
        ok = fe.loop_step(current_state=state, point_cloud=obstacles)
        if fe.reached_end():
            reached = True
            break
        assert ok
        state.simulate(v_x=fe.linear_x_control[0], v_y=fe.linear_y_control[0], omega=fe.angular_control[0], dt=0.1)
        clearance = min(clearance, float(np.hypot(obstacles[:, 0] - state.x, obstacles[:, 1] - state.y).min()))
    assert reached, f"goal not reached, stopped at ({state.x:.2f}, {state.y:.2f})"
    assert clearance >= ROBOT_RADIUS, f"clearance {clearance}"
