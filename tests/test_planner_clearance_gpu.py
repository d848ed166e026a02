"""The grid planner's clearance cost on the MI355X (kc_planner_set_clearance_cost / get_clearance / path_clearance,
kompass_cpp.planning, kompass_core.planning; DESIGN.md 4.10 rules 6 to 8): the device's clearance field, penalty,
validity map and penalised cost field bit for bit against the CPU statement of tests/planner_clearance_ref.py, the
path cell for cell against its rule-8 walk, the cost off against the planner without it, host against
device-resident grids, and the class and the front end on the doorway scene.

Every test runs under the time limit of test_planner_gpu.py, for its reason: a solve that went wrong would run to
its pass cap, and only the thread method ends a native call."""

import numpy as np
import pytest

TIME_LIMIT_S = 120

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(TIME_LIMIT_S, method="thread")]

import kompass_cpp  # noqa: E402
import kompass_hip as kh  # noqa: E402
import planner_clearance_ref as cref  # noqa: E402
import planner_ref as ref  # noqa: E402
from helpers import DeviceArray  # noqa: E402
from test_planner_gpu import connected_pair, free_cells  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert kh.device_count() >= 1, "no HIP device visible"


@pytest.fixture()
def ctx():
    c = kh.PlannerContext()
    yield c
    c.close()


def compare(ctx, grid, pairs, r2, c2, table, allow_unknown=True, maps=None):
    """Every (start, goal) pair on the grid and clearance cost the context holds: clear2, penalty, validity, field,
    status, cost, path and the path's smallest clear2 against the statement; the pass cap is not hit.  -> statuses."""
    w, h = grid.shape
    if maps is None:
        maps = (ref.validity(grid, r2, allow_unknown), cref.clearance2(grid, c2, allow_unknown))
    valid, clear2 = maps
    pen = cref.penalty(clear2, table)
    seen = []
    for start, goal in pairs:
        st, cost, passes = ctx.solve(start, goal, r2, allow_unknown)
        f, v = ctx.field()
        c, p = ctx.clearance()
        np.testing.assert_array_equal(c, clear2)
        np.testing.assert_array_equal(p, pen)
        np.testing.assert_array_equal(v, valid)
        want = cref.cost_field(valid, pen, goal)
        np.testing.assert_array_equal(f, want)
        wst = ref.status(valid, want, start, goal)
        assert st == wst, (start, goal, st, wst)
        assert 0 <= passes <= w * h + 1
        cells = ctx.path()
        if wst == ref.FOUND:
            assert cost == want[start[0], start[1]] and passes >= 1
            np.testing.assert_array_equal(cells, cref.walk(valid, want, pen, start))
            ref.check_path(valid, cells, start, goal)
            assert cref.path_cost(cells, pen) == cost           # rule 8: the path pays what the field says
            assert len(cells) <= cost // 10 + 2
            assert ctx.path_clearance() == cref.path_clearance(cells, clear2)
        else:
            assert cost == ref.INF and len(cells) == 0
            with pytest.raises(kh.KompassHipError):
                ctx.path_clearance()
        seen.append(st)
    return seen


# one tile, tile edges in both directions, a grid one cell wide
SHAPES = [(64, 64), (130, 97), (65, 300), (257, 63), (1, 90)]
# (r2, c2, weight10, allow_unknown): reach beyond the footprint, unknown cells blocking, reach == footprint (an
# all-zero table), and penalties far above the step costs
COSTS = [(0, 9, 10, True), (1, 36, 25, False), (5, 5, 40, True), (4, 100, 3000, True)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("density", [0.03, 0.15])
@pytest.mark.parametrize("cost", COSTS)
def test_random_clutter(ctx, shape, density, cost):
    r2, c2, wt, unknown = cost
    rng = np.random.default_rng(hash((shape, int(density * 100))) % 2 ** 32)
    grid = np.where(rng.random(shape) < density, 100, 0).astype(np.int32)
    grid[rng.random(shape) < 0.05] = -1
    table = cref.clearance_table(wt, r2, c2)
    ctx.set_clearance_cost(c2, table)
    ctx.set_grid(grid)
    maps = (ref.validity(grid, r2, unknown), cref.clearance2(grid, c2, unknown))
    valid = maps[0]
    np.testing.assert_array_equal(maps[1] <= r2, ~valid)
    cells = free_cells(valid, rng, 4)
    pairs = [(cells[0], cells[1]), (cells[2], cells[3]), (cells[0], cells[0])]
    occ = np.argwhere(~valid)
    if len(occ):
        pairs.append((cells[1], tuple(int(v) for v in occ[0])))   # an invalid end
    pairs.append(((shape[0], 0), cells[2]))                       # an end outside the grid
    pair = connected_pair(valid, cells)
    assert (pair is None) == (not valid.any())
    seen = compare(ctx, grid, pairs + ([pair] if pair is not None else []), r2, c2, table, unknown, maps)
    if pair is not None:
        assert seen[-1] == ref.FOUND


def test_reach_at_the_cap(ctx):
    """One occupied cell and the widest reach: clear2 runs from 0 to 254^2 = 64516 and is 0xFFFF beyond, the edge of
    the uint16 field.  The expected field is the rule in closed form."""
    w, h, c2 = 300, 70, cref.MAX_C2
    grid = np.zeros((w, h), np.int32)
    grid[2, 35] = 100
    d2 = (np.arange(w)[:, None] - 2) ** 2 + (np.arange(h)[None, :] - 35) ** 2
    clear2 = np.where(d2 <= c2, d2, cref.CLEAR_FAR).astype(np.uint16)
    assert clear2[256, 35] == 64516 and clear2[257, 35] == cref.CLEAR_FAR and clear2[256, 36] == cref.CLEAR_FAR
    assert (clear2 == cref.CLEAR_FAR).sum() > 1000 and clear2[2, 35] == 0
    small = np.zeros((40, 30), np.int32)
    small[2, 15] = 100
    np.testing.assert_array_equal(cref.clearance2(small, 400), np.where(d2[:40, 20:50] <= 400, d2[:40, 20:50], cref.CLEAR_FAR))
    table = cref.clearance_table(200, 1, c2)
    ctx.set_clearance_cost(c2, table)
    ctx.set_grid(grid)
    maps = (ref.validity(grid, 1), clear2)
    assert compare(ctx, grid, [((299, 3), (5, 35)), ((5, 35), (299, 69))], 1, c2, table, True, maps) == [ref.FOUND] * 2
    with pytest.raises(IndexError):
        ctx.set_clearance_cost(c2 + 1, np.zeros(c2 + 2, np.uint32))


def outputs(ctx, start, goal, r2):
    st, cost, passes = ctx.solve(start, goal, r2)
    f, v = ctx.field()
    return st, cost, passes, f, v, ctx.path()


def test_off_means_off(ctx):
    rng = np.random.default_rng(41)
    grid = np.where(rng.random((130, 97)) < 0.08, 100, 0).astype(np.int32)
    valid = ref.validity(grid, 2)
    start, goal = connected_pair(valid, free_cells(valid, rng, 4))
    ctx.set_grid(grid)
    first = outputs(ctx, start, goal, 2)
    assert first[0] == ref.FOUND
    np.testing.assert_array_equal(first[3], ref.cost_field(valid, goal))
    np.testing.assert_array_equal(first[5], ref.walk(valid, first[3], start))
    with pytest.raises(kh.KompassHipError):
        ctx.clearance()
    with pytest.raises(kh.KompassHipError):
        ctx.path_clearance()
    ctx.set_clearance_cost(64, cref.clearance_table(60, 2, 64))
    with pytest.raises(kh.KompassHipError):
        ctx.field()                       # the last solve is forgotten
    second = outputs(ctx, start, goal, 2)
    assert second[0] == ref.FOUND and second[1] > first[1]
    np.testing.assert_array_equal(second[4], first[4])
    ctx.clearance()
    ctx.set_clearance_cost(0)
    third = outputs(ctx, start, goal, 2)
    assert third[:3] == first[:3]
    for a, b in zip(third[3:], first[3:]):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(kh.KompassHipError):
        ctx.clearance()
    # a NULL table switches it off as well
    ctx.set_clearance_cost(64, cref.clearance_table(60, 2, 64))
    ctx.set_clearance_cost(64, None)
    assert outputs(ctx, start, goal, 2)[:3] == first[:3]


def test_zero_table(ctx):
    rng = np.random.default_rng(43)
    grid = np.where(rng.random((130, 97)) < 0.1, 100, 0).astype(np.int32)
    valid = ref.validity(grid, 1)
    start, goal = connected_pair(valid, free_cells(valid, rng, 4))
    table = np.zeros(10, np.uint32)
    ctx.set_clearance_cost(9, table)
    ctx.set_grid(grid)
    assert compare(ctx, grid, [(start, goal)], 1, 9, table) == [ref.FOUND]
    f, _ = ctx.field()
    np.testing.assert_array_equal(f, ref.cost_field(valid, goal))
    cells = ctx.path()
    assert cref.path_length(cells) == f[start]   # the rule-8 walk realises the field, the rule-4 walk need not


def test_range(ctx):
    grid = np.zeros((64, 64), np.int32)
    ctx.set_grid(grid)
    cells = 64 * 64
    most = 0xFFFFFFFE // cells - 14              # the largest penalty whose sums cannot wrap
    assert (14 + most) * cells <= 0xFFFFFFFE < (14 + most + 1) * cells
    table = np.zeros(10, np.uint32)
    table[3] = most + 1                          # no cell of this grid carries it: the bound is the table's
    ctx.set_clearance_cost(9, table)
    with pytest.raises(IndexError):
        ctx.solve((0, 0), (63, 63))
    table[3] = most
    ctx.set_clearance_cost(9, table)
    assert ctx.solve((0, 0), (63, 63))[:2] == (ref.FOUND, 63 * 14)
    with pytest.raises(IndexError):
        ctx.set_clearance_cost(64517, np.zeros(64518, np.uint32))
    with pytest.raises(ValueError):
        ctx.set_clearance_cost(9, np.zeros(9, np.uint32))
    with pytest.raises(ValueError):
        ctx.set_clearance_cost(9, np.zeros(11, np.uint32))
    assert ctx.solve((0, 0), (63, 63))[:2] == (ref.FOUND, 63 * 14)   # a refused table leaves the one before


def test_device_resident_grid(ctx):
    grid, start, goal = cref.doorway_scene()
    r2, c2, wt = 4, 100, 40
    table = cref.clearance_table(wt, r2, c2)
    ctx.set_clearance_cost(c2, table)
    ctx.set_grid(grid)
    assert compare(ctx, grid, [(start, goal)], r2, c2, table) == [ref.FOUND]
    host = outputs(ctx, start, goal, r2) + ctx.clearance() + (ctx.path_clearance(),)
    assert host[1] == 1524 and host[-1] == 81
    for dtype in (np.int32, np.int8):
        g = np.asfortranarray(grid.astype(dtype))
        with DeviceArray(g) as buf:
            ctx.set_grid(np.zeros_like(grid))
            ctx.set_grid_device(buf.ptr, 96, 80, elem_bytes=g.itemsize)
            dev = outputs(ctx, start, goal, r2) + ctx.clearance() + (ctx.path_clearance(),)
        assert dev[:3] == host[:3] and dev[-1] == host[-1]
        for a, b in zip(dev[3:-1], host[3:-1]):
            np.testing.assert_array_equal(a, b)


# ---- the class and the front end on the doorway scene at 0.05 m -------------------------------------------------
RES, ORIGIN, DIMS = 0.05, (-1.0, 0.5), [0.1, 0.4]
REACH, WEIGHT = 0.4, 4.0


def _doorway_statement():
    grid, start, goal = cref.doorway_scene()
    radius = ref.footprint_radius(ref.CYLINDER, DIMS)
    r2 = ref.radius_to_r2(radius, RES)
    c2 = ref.radius_to_r2(radius + float(np.float32(REACH)), RES)
    wt = int(round(float(np.float32(WEIGHT)) * 10))
    assert (r2, c2, wt) == (4, 100, 40)
    want = cref.plan(grid, start, goal, r2, c2, wt)
    assert (want["status"], want["cost"], want["length"], want["min_clear2"]) == (ref.FOUND, 1524, 1418, 81)
    xy = lambda c: (float(ref.cell_to_world(c[0], ORIGIN[0], RES)) + 0.01, float(ref.cell_to_world(c[1], ORIGIN[1], RES)) + 0.01)  # noqa: E731
    return grid, xy(start), xy(goal), want


def _check_solution(path, cells, cost, length, min_clearance, want):
    np.testing.assert_array_equal(cells, want["cells"])
    np.testing.assert_array_equal(np.asarray(path.x()), ref.cell_to_world(want["cells"][:, 0], ORIGIN[0], RES))
    np.testing.assert_array_equal(np.asarray(path.y()), ref.cell_to_world(want["cells"][:, 1], ORIGIN[1], RES))
    assert np.float32(cost) == ref.cost_in_metres(want["cost"], RES)
    assert np.float32(length) == ref.cost_in_metres(want["length"], RES)
    assert np.float32(min_clearance) == np.sqrt(np.float32(want["min_clear2"])) * np.float32(RES)
    assert np.float32(min_clearance) == np.sqrt(np.float32(81)) * np.float32(0.05)


def test_class_on_the_doorway_scene():
    grid, s, t, want = _doorway_statement()
    p = kompass_cpp.planning.GridPlanner(kompass_cpp.types.RobotGeometry.CYLINDER, DIMS)
    p.set_clearance_cost(REACH, WEIGHT)               # before the bounds: evaluated once they are known
    p.set_space_bounds_from_map(ORIGIN[0], ORIGIN[1], 96, 80, RES)
    assert (p.get_footprint_r2(), p.get_clearance_c2(), p.get_clearance_weight10()) == (4, 100, 40)
    p.set_grid(grid)
    p.setup_problem(s[0], s[1], 0.0, t[0], t[1], 0.0)
    assert p.solve() and p.get_status() == ref.FOUND
    _check_solution(p.get_solution(), p.get_path_cells(), p.get_cost(), p.get_path_length(), p.get_path_min_clearance(), want)
    c, pen = p.get_clearance()
    np.testing.assert_array_equal(c, want["clear2"])
    np.testing.assert_array_equal(pen, want["pen"])
    f, v = p.get_field()
    np.testing.assert_array_equal(f, want["field"])
    np.testing.assert_array_equal(np.asarray(v).astype(bool), want["valid"])
    # the same bounds again keep the table; off is the plain planner
    p.set_space_bounds_from_map(ORIGIN[0], ORIGIN[1], 96, 80, RES)
    p.setup_problem(s[0], s[1], 0.0, t[0], t[1], 0.0)
    assert p.solve() and np.float32(p.get_cost()) == ref.cost_in_metres(1524, RES)
    p.set_clearance_cost(0.0, WEIGHT)
    assert p.get_solution() is None and p.get_clearance_c2() == 0
    assert p.solve() and np.float32(p.get_cost()) == ref.cost_in_metres(1138, RES)
    plain = ref.plan(grid, ORIGIN, RES, s, t, ref.footprint_radius(ref.CYLINDER, DIMS))
    np.testing.assert_array_equal(p.get_path_cells(), plain["cells"])
    assert np.float32(p.get_path_length()) == ref.cost_in_metres(cref.path_length(plain["cells"]), RES)
    with pytest.raises(RuntimeError):
        p.get_clearance()
    with pytest.raises(RuntimeError):
        p.get_path_min_clearance()
    with pytest.raises(IndexError):
        p.set_clearance_cost(254 * RES, 1.0)          # 256 cells with the footprint: wider than the cap


def test_front_end_on_the_doorway_scene():
    from kompass_core.control import DWA, DWAConfig
    from kompass_core.models import AngularCtrlLimits, LinearCtrlLimits, RobotCtrlLimits
    from kompass_core.planning import GridPlanner
    from test_planner_gpu import _robot

    grid, s, t, want = _doorway_statement()
    meta = dict(origin_x=ORIGIN[0], origin_y=ORIGIN[1], width=96, height=80, resolution=RES)
    fe = GridPlanner(_robot(tuple(DIMS)), clearance_reach=REACH, clearance_weight=WEIGHT)
    fe.setup_problem(meta, s[0], s[1], 0.0, t[0], t[1], 0.0, grid=grid)
    path = fe.solve()
    assert path is not None and fe.status == ref.FOUND
    _check_solution(path, fe.path_cells, fe.get_cost(), fe.path_length, fe.min_clearance, want)
    c, pen = fe.clearance_field()
    np.testing.assert_array_equal(c, want["clear2"])
    np.testing.assert_array_equal(pen, want["pen"])
    # the defaults leave it off; set_clearance_cost switches it on afterwards
    plain = GridPlanner(_robot(tuple(DIMS)))
    plain.setup_problem(meta, s[0], s[1], 0.0, t[0], t[1], 0.0, grid=grid)
    assert plain.solve() is not None and np.float32(plain.get_cost()) == ref.cost_in_metres(1138, RES)
    plain.set_clearance_cost(REACH, WEIGHT)
    assert plain.solution is None
    plain.setup_problem(meta, s[0], s[1], 0.0, t[0], t[1], 0.0)          # the grid of the last call
    assert plain.solve() is not None
    np.testing.assert_array_equal(plain.path_cells, want["cells"])
    # a follower takes the path as it is
    limits = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=2.0, max_decel=2.0),
                             omega_limits=AngularCtrlLimits(max_vel=2.0, max_acc=3.0, max_decel=3.0, max_steer=2.0))
    dwa = DWA(robot=_robot(tuple(DIMS)), ctrl_limits=limits,
              config=DWAConfig(max_linear_samples=4, max_angular_samples=4, prediction_horizon=4, control_horizon=2))
    dwa.planner.set_current_path(path)
    dwa.set_path(np.stack([np.asarray(path.x()), np.asarray(path.y())], 1))
