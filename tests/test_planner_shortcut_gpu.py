"""The grid planner's any-angle path on the MI355X (kc_planner_shortcut / kc_planner_get_shortcut, kompass_cpp.planning,
kompass_core.planning; DESIGN.md 4.10 rules 9 to 12): the kept indices, their cells, the count, the smallest touched
clear2 and the float length bit for bit against the CPU statement of tests/planner_shortcut_ref.py, on seeded clutter
with and without the clearance cost, the doorway scene, an empty grid corner to corner; the refusals, the feature
unused, a device-resident grid, the class and the front end, and the closed loop through PurePursuit.

Every test runs under the time limit of test_planner_gpu.py, for its reason: only the thread method ends a native
call that went wrong."""
import ctypes as C
import math

import numpy as np
import pytest

TIME_LIMIT_S = 120

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(TIME_LIMIT_S, method="thread")]

import kompass_cpp  # noqa: E402
import kompass_hip as kh  # noqa: E402
import planner_clearance_ref as cref  # noqa: E402
import planner_ref as ref  # noqa: E402
import planner_shortcut_ref as sref  # noqa: E402
from helpers import DeviceArray  # noqa: E402
from test_planner_gpu import GOLD, ROBOT_RADIUS, _robot, connected_pair, free_cells  # noqa: E402

SPANS = [1, 2, 17, 64, 1024]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert kh.device_count() >= 1, "no HIP device visible"


@pytest.fixture()
def ctx():
    c = kh.PlannerContext()
    yield c
    c.close()


def compare(ctx, valid, spans=SPANS, clear2=None, resolution=0.05):
    """The shortcut of the context's last path for every span against the statement: indices, cells, count, the
    smallest touched clear2 and the float length.  -> the counts."""
    walk = ctx.path()
    assert len(walk) >= 1
    counts = []
    for span in spans:
        want = sref.shortcut(valid, walk, span, clear2)
        cells, idx, mc = ctx.shortcut(span)
        np.testing.assert_array_equal(idx, want["indices"])
        np.testing.assert_array_equal(cells, want["cells"])
        assert len(idx) == want["count"] and cells.dtype == np.int32 and idx.dtype == np.int32
        assert mc == want["min_clear2"], (span, mc, want["min_clear2"])
        assert sref.length_metres(cells, resolution) == sref.length_metres(want["cells"], resolution)
        if clear2 is not None:
            assert mc >= ctx.path_clearance()
        n = C.c_size_t(0)
        kh._check(kh.lib().kc_planner_get_shortcut(ctx.h, None, None, 0, C.byref(n)))   # the count alone
        assert n.value == want["count"]
        counts.append(len(idx))
    np.testing.assert_array_equal(ctx.path(), walk)   # the walk is what it was
    return counts


def clutter(shape, density):
    rng = np.random.default_rng(hash((shape, int(density * 100))) % 2 ** 32)
    grid = np.where(rng.random(shape) < density, 100, 0).astype(np.int32)
    grid[rng.random(shape) < 0.05] = -1
    return grid, rng


@pytest.mark.parametrize("shape", [(64, 64), (130, 97), (257, 63), (65, 300), (1, 90)])
@pytest.mark.parametrize("density", [0.02, 0.15, 0.35])
def test_random_clutter(ctx, shape, density):
    grid, rng = clutter(shape, density)
    ctx.set_grid(grid)
    valid = ref.validity(grid, 0)
    seeds = free_cells(valid, rng, 4)
    start, goal = connected_pair(valid, seeds)
    assert ctx.solve(start, goal, 0)[0] == ref.FOUND
    counts = compare(ctx, valid)
    assert counts[0] == len(ctx.path())              # a span of one cell keeps the walk
    # the path the other way round: the opposite octants
    assert ctx.solve(goal, start, 0)[0] == ref.FOUND
    compare(ctx, valid, [17, 1024])
    # n = 1 (start equal to goal) and n = 2
    assert ctx.solve(goal, goal, 0)[0] == ref.FOUND
    assert compare(ctx, valid) == [1] * len(SPANS)
    walk = ref.walk(valid, ref.cost_field(valid, goal), start)
    if len(walk) >= 2:
        assert ctx.solve(tuple(int(v) for v in walk[-2]), goal, 0)[0] == ref.FOUND
        assert compare(ctx, valid) == [2] * len(SPANS)


@pytest.mark.parametrize("shape", [(130, 97), (65, 300)])
@pytest.mark.parametrize("cost", [(1, 36, 25, False), (4, 100, 3000, True)])
def test_random_clutter_with_the_clearance_cost(ctx, shape, cost):
    r2, c2, wt, unknown = cost
    grid, rng = clutter(shape, 0.02)
    ctx.set_clearance_cost(c2, cref.clearance_table(wt, r2, c2))
    ctx.set_grid(grid)
    valid, clear2 = ref.validity(grid, r2, unknown), cref.clearance2(grid, c2, unknown)
    start, goal = connected_pair(valid, free_cells(valid, rng, 4))
    assert ctx.solve(start, goal, r2, unknown)[0] == ref.FOUND
    assert len(ctx.path()) > 17
    compare(ctx, valid, clear2=clear2)


def test_doorway_scene(ctx):
    grid, start, goal = cref.doorway_scene()
    valid = ref.validity(grid, 4)
    ctx.set_grid(grid)
    assert ctx.solve(start, goal, 4)[0] == ref.FOUND
    assert compare(ctx, valid, [16, 128]) == [10, 5]
    clear2 = cref.clearance2(grid, 100)
    ctx.set_clearance_cost(100, cref.clearance_table(40, 4, 100))
    with pytest.raises(kh.KompassHipError):
        ctx.shortcut(128)                                # the clearance cost forgot the solve
    assert ctx.solve(start, goal, 4)[0] == ref.FOUND
    assert compare(ctx, valid, [16, 128], clear2) == [11, 9]
    assert ctx.shortcut(128)[2] == 81 == ctx.path_clearance()


def test_walk_beyond_the_reach_of_every_blocking_cell(ctx):
    """The walk's own smallest clear2 is CLEAR_FAR, the largest value: a segment may then touch CLEAR_FAR cells only.
    The octile walk goes diagonally, then straight; the straight line between its ends passes the one blocking cell."""
    grid = np.zeros((90, 70), np.int32)
    grid[45, 25] = 100
    c2 = 25
    ctx.set_clearance_cost(c2, cref.clearance_table(30, 1, c2))
    ctx.set_grid(grid)
    valid, clear2 = ref.validity(grid, 1), cref.clearance2(grid, c2)
    assert ctx.solve((10, 10), (80, 40), 1)[0] == ref.FOUND
    assert ctx.path_clearance() == cref.CLEAR_FAR
    compare(ctx, valid, [8, 128], clear2)
    cells, idx, mc = ctx.shortcut(128)
    assert mc == cref.CLEAR_FAR
    # rule 10 binds: on validity alone the shortcut passes within the reach of the blocking cell
    loose = sref.select(valid, ctx.path(), 128)
    assert loose != idx.tolist() and sref.min_touched_clear2(ctx.path(), loose, clear2) < c2


def test_empty_grid_corner_to_corner(ctx):
    grid = np.zeros((300, 200), np.int32)
    ctx.set_grid(grid)
    assert ctx.solve((0, 0), (299, 199), 0)[0] == ref.FOUND
    assert len(ctx.path()) == 300
    assert compare(ctx, np.ones((300, 200), bool), [1024, 128]) == [2, 4]
    cells, idx, mc = ctx.shortcut(1024)
    assert cells.tolist() == [[0, 0], [299, 199]] and idx.tolist() == [0, 299] and mc == cref.CLEAR_FAR


def test_refusals(ctx):
    with pytest.raises(kh.KompassHipError):
        ctx.shortcut(64)                                 # no grid, no solve
    grid = np.zeros((40, 30), np.int32)
    grid[20, :] = 100
    ctx.set_grid(grid)
    with pytest.raises(kh.KompassHipError):
        ctx.shortcut(64)                                 # no solve
    assert ctx.solve((2, 3), (37, 20), 0)[0] == ref.UNREACHABLE
    with pytest.raises(kh.KompassHipError):
        ctx.shortcut(64)                                 # a solve without a path
    n = C.c_size_t(7)
    with pytest.raises(kh.KompassHipError):
        kh._check(kh.lib().kc_planner_get_shortcut(ctx.h, None, None, 0, C.byref(n)))
    assert n.value == 0
    assert ctx.solve((2, 3), (15, 20), 0)[0] == ref.FOUND
    for span in (0, -1, 1025):
        with pytest.raises(IndexError):
            ctx.shortcut(span)
    with pytest.raises(kh.KompassHipError):
        kh._check(kh.lib().kc_planner_get_shortcut(ctx.h, None, None, 0, C.byref(n)))   # refused spans left nothing
    cells, idx, _ = ctx.shortcut(1024)
    assert idx.tolist() == [0, len(ctx.path()) - 1]
    out = np.empty((1, 2), np.int32)
    with pytest.raises(IndexError):
        kh._check(kh.lib().kc_planner_get_shortcut(ctx.h, out.ctypes.data, None, 1, C.byref(n)))   # two cells, room for one
    # a new solve and a new grid forget the result
    assert ctx.solve((2, 3), (15, 20), 0)[0] == ref.FOUND
    with pytest.raises(kh.KompassHipError):
        kh._check(kh.lib().kc_planner_get_shortcut(ctx.h, None, None, 0, C.byref(n)))
    ctx.shortcut(8)
    ctx.set_grid(np.zeros((40, 30), np.int32))
    with pytest.raises(kh.KompassHipError):
        kh._check(kh.lib().kc_planner_get_shortcut(ctx.h, None, None, 0, C.byref(n)))
    with pytest.raises(kh.KompassHipError):
        ctx.shortcut(8)
    assert ctx.solve((2, 3), (37, 20), 0)[0] == ref.FOUND
    assert ctx.shortcut(64)[1].tolist() == [0, 35] and ctx.shortcut(8)[1].tolist() == [0, 8, 16, 24, 32, 35]
    assert ctx.shortcut(64)[1].tolist() == [0, 35]       # the cache is per span


def outputs(ctx, start, goal, r2):
    st, cost, passes = ctx.solve(start, goal, r2)
    f, v = ctx.field()
    return st, cost, passes, f, v, ctx.path()


def test_unused_means_unchanged(ctx):
    rng = np.random.default_rng(41)
    grid = np.where(rng.random((130, 97)) < 0.08, 100, 0).astype(np.int32)
    valid = ref.validity(grid, 2)
    start, goal = connected_pair(valid, free_cells(valid, rng, 4))
    ctx.set_grid(grid)
    first = outputs(ctx, start, goal, 2)
    assert first[0] == ref.FOUND
    np.testing.assert_array_equal(first[3], ref.cost_field(valid, goal))
    np.testing.assert_array_equal(first[5], ref.walk(valid, first[3], start))
    compare(ctx, valid, [64])
    f, v = ctx.field()
    np.testing.assert_array_equal(f, first[3])
    np.testing.assert_array_equal(v, first[4])
    np.testing.assert_array_equal(ctx.path(), first[5])
    second = outputs(ctx, start, goal, 2)                # a solve after a shortcut
    assert second[:3] == first[:3]
    for a, b in zip(second[3:], first[3:]):
        np.testing.assert_array_equal(a, b)
    # the shortcut before the path was asked for walks first
    ctx.solve(start, goal, 2)
    compare(ctx, valid, [64])
    # with the clearance cost: cost and path clearance keep describing the walk
    ctx.set_clearance_cost(64, cref.clearance_table(60, 2, 64))
    third = outputs(ctx, start, goal, 2)
    m = ctx.path_clearance()
    compare(ctx, valid, [64], cref.clearance2(grid, 64))
    assert ctx.path_clearance() == m
    np.testing.assert_array_equal(ctx.path(), third[5])
    np.testing.assert_array_equal(ctx.field()[0], third[3])


def test_device_resident_grid(ctx):
    grid, start, goal = cref.doorway_scene()
    valid, clear2 = ref.validity(grid, 4), cref.clearance2(grid, 100)
    ctx.set_clearance_cost(100, cref.clearance_table(40, 4, 100))
    ctx.set_grid(grid)
    assert ctx.solve(start, goal, 4)[0] == ref.FOUND
    host = [ctx.shortcut(w) for w in (16, 128)]
    for dtype in (np.int32, np.int8):
        g = np.asfortranarray(grid.astype(dtype))
        with DeviceArray(g) as buf:
            ctx.set_grid(np.zeros_like(grid))
            ctx.set_grid_device(buf.ptr, 96, 80, elem_bytes=g.itemsize)
            assert ctx.solve(start, goal, 4)[0] == ref.FOUND
            assert compare(ctx, valid, [16, 128], clear2) == [11, 9]
            dev = [ctx.shortcut(w) for w in (16, 128)]
        for a, b in zip(dev, host):
            np.testing.assert_array_equal(a[0], b[0])
            np.testing.assert_array_equal(a[1], b[1])
            assert a[2] == b[2]


# ---- the class and the front end on the doorway scene at 0.05 m -------------------------------------------------
RES, ORIGIN, DIMS = 0.05, (-1.0, 0.5), [0.1, 0.4]
REACH, WEIGHT = 0.4, 4.0


def _doorway(with_cost):
    grid, start, goal = cref.doorway_scene()
    xy = lambda c: (float(ref.cell_to_world(c[0], ORIGIN[0], RES)) + 0.01, float(ref.cell_to_world(c[1], ORIGIN[1], RES)) + 0.01)  # noqa: E731
    if with_cost:
        p = cref.plan(grid, start, goal, 4, 100, 40)
        return grid, xy(start), xy(goal), p["valid"], p["cells"], p["clear2"]
    valid = ref.validity(grid, 4)
    return grid, xy(start), xy(goal), valid, ref.walk(valid, ref.cost_field(valid, goal), start), None


def _check_any_angle(path, cells, length, want):
    np.testing.assert_array_equal(cells, want["cells"])
    np.testing.assert_array_equal(np.asarray(path.x()), ref.cell_to_world(want["cells"][:, 0], ORIGIN[0], RES))
    np.testing.assert_array_equal(np.asarray(path.y()), ref.cell_to_world(want["cells"][:, 1], ORIGIN[1], RES))
    assert np.float32(length) == sref.length_metres(want["cells"], RES)


@pytest.mark.parametrize("with_cost", [False, True])
def test_class_on_the_doorway_scene(with_cost):
    grid, s, t, valid, walk, clear2 = _doorway(with_cost)
    p = kompass_cpp.planning.GridPlanner(kompass_cpp.types.RobotGeometry.CYLINDER, DIMS)
    if with_cost:
        p.set_clearance_cost(REACH, WEIGHT)
    p.set_space_bounds_from_map(ORIGIN[0], ORIGIN[1], 96, 80, RES)
    p.set_grid(grid)
    assert p.get_any_angle_solution() is None and len(p.get_any_angle_cells()) == 0
    assert p.get_any_angle_length() == float("inf")
    p.setup_problem(s[0], s[1], 0.0, t[0], t[1], 0.0)
    assert p.solve()
    cost, length = p.get_cost(), p.get_path_length()
    for span, count in [(16, 11 if with_cost else 10), (128, 9 if with_cost else 5)]:
        want = sref.shortcut(valid, walk, span, clear2)
        assert want["count"] == count
        _check_any_angle(p.get_any_angle_solution(span), p.get_any_angle_cells(span), p.get_any_angle_length(span), want)
        cells, idx = p.get_any_angle_cells(span, with_indices=True)
        np.testing.assert_array_equal(idx, want["indices"])
        np.testing.assert_array_equal(cells, want["cells"])
    want = sref.shortcut(valid, walk, 128, clear2)
    _check_any_angle(p.get_any_angle_solution(), p.get_any_angle_cells(), p.get_any_angle_length(), want)   # the default span
    assert np.float32(p.get_any_angle_length()) == np.float32(float(np.float32(RES)) * (138.2514538611667 if with_cost else 108.39283822378206))
    # cost, length and the walk keep describing the walk
    assert p.get_cost() == cost and p.get_path_length() == length
    np.testing.assert_array_equal(p.get_path_cells(), walk)
    if with_cost:
        assert np.float32(p.get_any_angle_min_clearance()) == np.sqrt(np.float32(81)) * np.float32(RES)
        assert p.get_any_angle_min_clearance() >= p.get_path_min_clearance()
    else:
        assert p.get_any_angle_min_clearance() == float("inf")
    for span in (0, 1025):
        with pytest.raises(IndexError):
            p.get_any_angle_solution(span)


def test_front_end_on_the_doorway_scene():
    from kompass_core.planning import GridPlanner

    grid, s, t, valid, walk, clear2 = _doorway(True)
    meta = dict(origin_x=ORIGIN[0], origin_y=ORIGIN[1], width=96, height=80, resolution=RES)
    fe = GridPlanner(_robot(tuple(DIMS)), clearance_reach=REACH, clearance_weight=WEIGHT, any_angle=True, simplify=True)
    fe.setup_problem(meta, s[0], s[1], 0.0, t[0], t[1], 0.0, grid=grid)
    path = fe.solve()
    assert path is not None and fe.solution is path and fe.status == ref.FOUND
    want = sref.shortcut(valid, walk, 128, clear2)
    assert want["count"] == 9
    _check_any_angle(path, fe.path_cells, fe.any_angle_length, want)
    assert np.float32(fe.path_length) == ref.cost_in_metres(cref.path_length(walk), RES)       # the walk's
    assert np.float32(fe.min_clearance) == np.float32(fe.any_angle_min_clearance) == np.sqrt(np.float32(81)) * np.float32(RES)
    short = GridPlanner(_robot(tuple(DIMS)), clearance_reach=REACH, clearance_weight=WEIGHT, any_angle=True, max_span=16)
    short.setup_problem(meta, s[0], s[1], 0.0, t[0], t[1], 0.0, grid=grid)
    _check_any_angle(short.solve(), short.path_cells, short.any_angle_length, sref.shortcut(valid, walk, 16, clear2))
    # off by default: the walk as before
    plain = GridPlanner(_robot(tuple(DIMS)), clearance_reach=REACH, clearance_weight=WEIGHT)
    plain.setup_problem(meta, s[0], s[1], 0.0, t[0], t[1], 0.0, grid=grid)
    assert len(np.asarray(plain.solve().x())) == len(walk)
    np.testing.assert_array_equal(plain.path_cells, walk)
    # no path: None, as without the option
    fe.setup_problem(meta, s[0], s[1], 0.0, float(ref.cell_to_world(48, ORIGIN[0], RES)) + 0.01,
                     float(ref.cell_to_world(10, ORIGIN[1], RES)) + 0.01, 0.0)
    assert fe.solve() is None and fe.status == ref.GOAL_INVALID and len(fe.path_cells) == 0
    with pytest.raises(ValueError):
        GridPlanner(_robot(tuple(DIMS)), any_angle=True, max_span=0)


# ---- closed loop: PCD room -> grid -> GridPlanner(any_angle) -> Path -> PurePursuit ------------------------------
def _room_plan_any_angle():
    from kompass_core.planning import GridPlanner

    res = 0.1
    grid, origin = kompass_cpp.utils.read_pcd_to_occupancy_grid(str(GOLD / "pcd_room_ascii.pcd"), res, 0.05, 2.5)
    pts = np.asarray(kompass_cpp.utils.read_pcd(str(GOLD / "pcd_room_ascii.pcd")))
    obstacles = np.ascontiguousarray(pts[np.isfinite(pts).all(axis=1) & (pts[:, 2] > 0.05) & (pts[:, 2] <= 2.5)])
    assert len(obstacles) == 15
    fe = GridPlanner(_robot((ROBOT_RADIUS, 0.4)), margin=0.25, any_angle=True)
    meta = dict(origin_x=origin[0], origin_y=origin[1], width=grid.shape[0], height=grid.shape[1], resolution=res)
    start, goal = (-1.7, -1.0), (1.5, -0.7)
    fe.setup_problem(meta, start[0], start[1], 0.0, goal[0], goal[1], 0.0, grid=grid)
    path = fe.solve()
    want = ref.plan(np.asarray(grid), origin[:2], res, start, goal, ROBOT_RADIUS + float(np.float32(0.25)))
    assert want["status"] == ref.FOUND and path is not None
    short = sref.shortcut(want["valid"], want["cells"], 128)
    np.testing.assert_array_equal(fe.path_cells, short["cells"])
    assert 2 <= short["count"] < len(want["cells"])
    xy = np.stack([np.asarray(path.x()), np.asarray(path.y())], 1)
    # along the segments too, not at the waypoints alone
    dense = np.concatenate([np.linspace(xy[k], xy[k + 1], 50) for k in range(len(xy) - 1)])
    d = np.hypot(dense[:, None, 0] - obstacles[None, :, 0], dense[:, None, 1] - obstacles[None, :, 1]).min()
    # an obstacle point lies anywhere in its cell, and a point of a segment within half a cell's diagonal of the
    # position of a valid cell it touches
    assert d >= ROBOT_RADIUS + 0.25 - res * math.sqrt(2) - res * math.sqrt(0.5) - 1e-6
    return xy, obstacles


def test_closed_loop_pure_pursuit():
    from kompass_core.control import PurePursuit, PurePursuitConfig
    from kompass_core.models import AngularCtrlLimits, LinearCtrlLimits, RobotCtrlLimits, RobotState

    xy, obstacles = _room_plan_any_angle()
    robot = _robot((ROBOT_RADIUS, 0.4))
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=0.5, max_acc=2.0, max_decel=2.0),
                          omega_limits=AngularCtrlLimits(max_vel=1.5, max_steer=0.7, max_acc=3.0, max_decel=3.0))
    fe = PurePursuit(robot, lim, config=PurePursuitConfig(wheel_base=robot.wheelbase, lookahead_distance=0.4),
                     control_time_step=0.1)
    fe.set_path(xy)
    heading = math.atan2(xy[1, 1] - xy[0, 1], xy[1, 0] - xy[0, 0])
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
