"""The grid planner's oriented box footprint on the MI355X (kc_planner_set_oriented / solve_oriented /
get_oriented_field / get_oriented_path, kompass_cpp.planning, kompass_core.planning; DESIGN.md 4.10 rules 13 to 18):
the four validity layers, the turn-valid map, the four field layers, status, cost and the state walk bit for bit
against the CPU statement of tests/planner_oriented_ref.py, on the corridor a disc cannot enter, the L with a turning
bay, seeded clutter and degenerate shapes; host against device-resident grids; off means off; the exclusions.

Every grid is at most 130 cells a side.  Every test runs under the time limit of test_planner_gpu.py, for its reason:
a solve that went wrong would run to its pass cap, and only the thread method ends a native call."""

import numpy as np
import pytest

TIME_LIMIT_S = 120

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(TIME_LIMIT_S, method="thread")]

import kompass_cpp  # noqa: E402
import kompass_hip as kh  # noqa: E402
import planner_oriented_ref as oref  # noqa: E402
import planner_ref as ref  # noqa: E402
from helpers import DeviceArray  # noqa: E402

BIG, SMALL = (225, 4), (9, 1)   # A2, B2 of the 1.5 x 0.2 m and the 0.3 x 0.1 m box at 0.05 m


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert kh.device_count() >= 1, "no HIP device visible"


@pytest.fixture()
def ctx():
    c = kh.PlannerContext()
    yield c
    c.close()


def compare(ctx, grid, start, k0, goal, a2, b2, turn10, allow_unknown=True):
    """One solve on the grid and box the context holds against the statement: validity by class, turn validity, the
    four field layers, status, cost, the state walk and its collapsed cells.  -> the statement's plan."""
    w, h = grid.shape
    want = oref.plan(grid, start, k0, goal, a2, b2, turn10, allow_unknown)
    st, cost, passes = ctx.solve_oriented(start, k0, goal, allow_unknown)
    f, v, t = ctx.oriented_field()
    np.testing.assert_array_equal(v, want["valid"])
    np.testing.assert_array_equal(t, want["turn"])
    np.testing.assert_array_equal(f, want["field"])
    assert st == want["status"], (st, want["status"])
    assert cost == want["cost"]
    assert 0 <= passes <= 4 * w * h + 1
    states, cells = ctx.oriented_path(), ctx.path()
    if st == ref.FOUND:
        np.testing.assert_array_equal(states, want["states"])
        np.testing.assert_array_equal(cells, want["cells"])
        assert sum(want["step_costs"]) == cost          # rule 17: the walk pays what the field says
    else:
        assert len(states) == 0 and len(cells) == 0
    return want


def test_corridor_a_disc_cannot_enter(ctx):
    grid, start, goal = oref.corridor_scene()
    ctx.set_grid(grid)
    ctx.set_oriented(*BIG, 10)
    want = compare(ctx, grid, start, 0, goal, *BIG, 10)
    st, cost, _ = ctx.solve_oriented(start, 0, goal)
    assert (st, cost) == (kh.PLAN_FOUND, 670)
    _, v, t = ctx.oriented_field()
    assert v.sum(axis=(1, 2)).tolist() == [216, 0, 0, 0] and not t.any()
    states = ctx.oriented_path()
    assert len(states) == 68 and (states[:, 2] == 0).all() and (states[:, 1] == 33).all()
    assert want["cost"] == 670
    # the same scene in disc mode: the circumscribed disc fits nowhere in the corridor
    ctx.set_oriented(0)
    r2 = ref.radius_to_r2(ref.footprint_radius(ref.BOX, oref.BIG_BOX), oref.RES)
    st, cost, _ = ctx.solve(start, goal, r2)
    assert (st, cost) == (kh.PLAN_START_INVALID, kh.PLAN_INF)
    assert not ctx.field()[1].any()


def test_l_with_a_turning_bay(ctx):
    grid, start, goal = oref.l_scene()
    ctx.set_grid(grid)
    ctx.set_oriented(*BIG, 10)
    want = compare(ctx, grid, start, 0, goal, *BIG, 10)
    assert (want["status"], want["cost"], int(want["turn"].sum())) == (ref.FOUND, 782, 31)
    states = ctx.oriented_path()
    ks = states[:, 2]
    assert ks[np.r_[True, ks[1:] != ks[:-1]]].tolist() == [0, 1, 2]
    steps = np.abs(np.diff(states[:, :2], axis=0)).sum(axis=1)       # 0 a turn, 1 straight, 2 diagonal
    assert int((steps == 0).sum() * 10 + (steps == 1).sum() * 10 + (steps == 2).sum() * 14) == 782
    # without the bay there is nowhere to turn
    grid, start, goal = oref.l_scene(bay=False)
    ctx.set_grid(grid)
    want = compare(ctx, grid, start, 0, goal, *BIG, 10)
    assert want["status"] == ref.UNREACHABLE and not want["turn"].any()


@pytest.mark.parametrize("allow_unknown", [True, False])
def test_seeded_clutter(ctx, allow_unknown):
    grid, start, goal = oref.clutter_scene(unknown=True)
    assert (grid == -1).sum() > 10
    ctx.set_grid(grid)
    ctx.set_oriented(*SMALL, 7)
    for k0 in range(4):
        want = compare(ctx, grid, start, k0, goal, *SMALL, 7, allow_unknown)
        assert want["status"] == ref.FOUND
    if allow_unknown:   # unknown cells pass: the grid of the issue's prototype
        assert want["field"][:, start[0], start[1]].tolist() == [922, 929, 928, 929]
    # the way back, and a turn cost above a step's
    ctx.set_oriented(*SMALL, 25)
    compare(ctx, grid, goal, 1, start, *SMALL, 25, allow_unknown)


@pytest.mark.parametrize("shape", [(1, 40), (40, 1), (130, 3)])
def test_degenerate_shapes(ctx, shape):
    grid = np.zeros(shape, np.int32)
    c = (shape[0] // 2, shape[1] // 2)
    ctx.set_grid(grid)
    ctx.set_oriented(*SMALL, 10)
    for k0 in range(4):
        want = compare(ctx, grid, c, k0, c, *SMALL, 10)          # goal = start
        assert want["status"] == ref.FOUND and want["cost"] == 0 and len(want["states"]) == 1
    far = (shape[0] - 1, shape[1] - 1)
    compare(ctx, grid, (0, 0), 0, far, *SMALL, 10)
    ctx.set_oriented(*BIG, 10)                                   # a box longer than the grid is wide
    compare(ctx, grid, (0, 0), 2, far, *BIG, 10)
    # start or goal outside the grid
    ctx.set_oriented(*SMALL, 10)
    assert compare(ctx, grid, (-1, 0), 0, c, *SMALL, 10)["status"] == ref.START_OUTSIDE
    assert compare(ctx, grid, c, 0, (shape[0], 0), *SMALL, 10)["status"] == ref.GOAL_OUTSIDE


def test_invalid_goal_and_start_valid_in_another_class_only(ctx):
    grid, start, goal = oref.corridor_scene()
    ctx.set_grid(grid)
    ctx.set_oriented(*BIG, 10)
    # the start fits lengthwise only: class 2 there is START_INVALID although the cell has a valid class
    assert compare(ctx, grid, start, 2, goal, *BIG, 10)["status"] == ref.START_INVALID
    assert compare(ctx, grid, start, 1, goal, *BIG, 10)["status"] == ref.START_INVALID
    # a goal with no valid class: next to the wall
    assert compare(ctx, grid, start, 0, (69, 31), *BIG, 10)["status"] == ref.GOAL_INVALID
    assert compare(ctx, grid, start, 0, (40, 10), *BIG, 10)["status"] == ref.GOAL_INVALID


def _outputs(ctx, start, k0, goal):
    res = ctx.solve_oriented(start, k0, goal)
    return res, ctx.oriented_field(), ctx.oriented_path(), ctx.path()


def _assert_same(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1], b[1]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_array_equal(a[3], b[3])


def test_int8_int32_host_and_device_grids_agree(ctx):
    grid, start, goal = oref.l_scene()
    ctx.set_oriented(*BIG, 10)
    ctx.set_grid(grid)
    host = _outputs(ctx, start, 0, goal)
    assert host[0][:2] == (kh.PLAN_FOUND, 782)
    ctx.set_grid(grid.astype(np.int8))
    _assert_same(_outputs(ctx, start, 0, goal), host)
    for dtype in (np.int32, np.int8):
        g = np.asfortranarray(grid.astype(dtype))
        with DeviceArray(g) as buf:
            ctx.set_grid(np.zeros_like(grid))
            ctx.set_grid_device(buf.ptr, 72, 70, elem_bytes=g.itemsize)
            dev = _outputs(ctx, start, 0, goal)
        _assert_same(dev, host)


def test_disc_mode_is_unchanged_after_on_and_off(ctx):
    grid, start, goal = oref.clutter_scene(unknown=True)

    def disc(c):
        out = []
        for r2, unknown in ((0, True), (2, False)):
            res = c.solve(start, goal, r2, unknown)
            out.append((res, c.field(), c.path()))
        return out

    fresh = kh.PlannerContext()
    try:
        fresh.set_grid(grid)
        want = disc(fresh)
    finally:
        fresh.close()
    assert want[0][0][0] == kh.PLAN_FOUND
    ctx.set_grid(grid)
    ctx.set_oriented(*SMALL, 7)
    assert ctx.solve_oriented(start, 0, goal)[0] == kh.PLAN_FOUND
    assert len(ctx.oriented_path()) > 0
    ctx.set_oriented(0)
    got = disc(ctx)
    for (r0, (f0, v0), p0), (r1, (f1, v1), p1) in zip(want, got):
        assert r0 == r1                                   # status, cost and passes
        assert f0.tobytes() == f1.tobytes() and v0.tobytes() == v1.tobytes() and p0.tobytes() == p1.tobytes()
    with pytest.raises(kh.KompassHipError):               # off again: the oriented calls have nothing to give
        ctx.oriented_field()
    with pytest.raises(kh.KompassHipError):
        ctx.solve_oriented(start, 0, goal)


def test_abi_exclusions_and_range_errors(ctx):
    grid, start, goal = oref.clutter_scene()
    ctx.set_grid(grid)
    with pytest.raises(IndexError):                       # turn10 = 0
        ctx.set_oriented(9, 1, 0)
    with pytest.raises(IndexError):
        ctx.set_oriented(9, 1, 10001)
    with pytest.raises(IndexError):                       # T2 beyond 254 cells
        ctx.set_oriented(254 * 254, 1, 10)
    ctx.set_oriented(254 * 254, 0, 10)
    ctx.set_oriented(*SMALL, 10)
    with pytest.raises(ValueError):
        ctx.solve_oriented(start, 4, goal)
    with pytest.raises(kh.KompassHipError):               # the disc solve belongs to the disc mode
        ctx.solve(start, goal, 1)
    with pytest.raises(kh.KompassHipError, match="clearance"):   # rule 18: set second, refused
        ctx.set_clearance_cost(9, np.zeros(10, np.uint32))
    assert ctx.solve_oriented(start, 0, goal)[0] == kh.PLAN_FOUND
    with pytest.raises(kh.KompassHipError, match="any-angle"):
        ctx.shortcut(16)
    with pytest.raises(kh.KompassHipError):
        ctx.field()
    ctx.set_oriented(0)
    ctx.set_clearance_cost(9, np.zeros(10, np.uint32))
    with pytest.raises(kh.KompassHipError, match="clearance"):   # the other order
        ctx.set_oriented(*SMALL, 10)
    ctx.set_clearance_cost(0)
    ctx.set_oriented(*SMALL, 10)


# ---- the class and the front end at 0.05 m ------------------------------------------------------------------------
ORIGIN = (-1.0, 0.5)


def _world(cell):
    return (float(ref.cell_to_world(cell[0], ORIGIN[0], oref.RES)) + 0.01, float(ref.cell_to_world(cell[1], ORIGIN[1], oref.RES)) + 0.01)


def test_class_on_the_l_scene():
    grid, start, goal = oref.l_scene()
    want = oref.plan(grid, start, 0, goal, *BIG, 10)
    BOX = kompass_cpp.types.RobotGeometry.BOX
    p = kompass_cpp.planning.GridPlanner(BOX, list(oref.BIG_BOX))
    p.set_oriented_footprint(True, 1.0)                   # before the bounds: evaluated once they are known
    assert p.oriented_on() and p.get_oriented_turn10() == 10
    p.set_space_bounds_from_map(ORIGIN[0], ORIGIN[1], 72, 70, oref.RES)
    assert p.get_oriented_a2_b2() == BIG
    p.set_grid(grid)
    s, t = _world(start), _world(goal)
    p.setup_problem(s[0], s[1], 0.1, t[0], t[1], 2.0)     # yaw 0.1 is class 0; goal_yaw is not used
    assert p.get_cells() == (start, goal)
    assert p.solve() and p.get_status() == ref.FOUND
    np.testing.assert_array_equal(p.get_path_states(), want["states"])
    np.testing.assert_array_equal(p.get_path_cells(), want["cells"])
    np.testing.assert_array_equal(p.get_path_cells(True), ref.simplify(want["cells"]))
    f, v, turn = p.get_oriented_field()
    np.testing.assert_array_equal(f, want["field"])
    np.testing.assert_array_equal(np.stack([(v >> k & 1).astype(bool) for k in range(4)]), want["valid"])
    np.testing.assert_array_equal(turn.astype(bool), want["turn"])
    assert np.float32(p.get_cost()) == ref.cost_in_metres(782, oref.RES)          # the turns included
    moved = np.any(want["states"][1:, :2] != want["states"][:-1, :2], axis=1)
    length = sum(c for c, m in zip(want["step_costs"], moved) if m)
    assert length == 782 - 2 * 10                                                 # two turns of 45 degrees
    assert np.float32(p.get_path_length()) == ref.cost_in_metres(length, oref.RES)
    path = p.get_solution()
    np.testing.assert_array_equal(np.asarray(path.x()), ref.cell_to_world(want["cells"][:, 0], ORIGIN[0], oref.RES))
    np.testing.assert_array_equal(np.asarray(path.y()), ref.cell_to_world(want["cells"][:, 1], ORIGIN[1], oref.RES))
    # rule 18's three errors
    with pytest.raises(ValueError, match="any-angle"):
        p.get_any_angle_cells(16)
    with pytest.raises(ValueError, match="any-angle"):
        p.get_any_angle_solution(16)
    with pytest.raises(ValueError, match="clearance"):
        p.set_clearance_cost(0.4, 4.0)
    q = kompass_cpp.planning.GridPlanner(kompass_cpp.types.RobotGeometry.CYLINDER, [0.1, 0.4])
    with pytest.raises(ValueError, match="BOX"):
        q.set_oriented_footprint(True, 1.0)
    r = kompass_cpp.planning.GridPlanner(BOX, list(oref.BIG_BOX))
    r.set_clearance_cost(0.4, 4.0)
    with pytest.raises(ValueError, match="clearance"):
        r.set_oriented_footprint(True, 1.0)
    with pytest.raises(IndexError):
        p.set_oriented_footprint(True, 0.0)
    # another start class: the box does not fit across the corridor
    p.setup_problem(s[0], s[1], 1.6, t[0], t[1], 0.0)
    assert not p.solve() and p.get_status() == ref.START_INVALID and len(p.get_path_states()) == 0
    # off again: the disc planner, which the corridor refuses
    p.set_oriented_footprint(False)
    p.setup_problem(s[0], s[1], 0.0, t[0], t[1], 0.0)
    assert not p.solve() and p.get_status() == ref.START_INVALID


def test_front_end_on_the_corridor():
    from kompass_core.planning import GridPlanner
    from test_planner_oriented_cpu import _box_robot

    grid, start, goal = oref.corridor_scene()
    want = oref.plan(grid, start, 0, goal, *BIG, 10)
    meta = dict(origin_x=ORIGIN[0], origin_y=ORIGIN[1], width=72, height=70, resolution=oref.RES)
    s, t = _world(start), _world(goal)
    fe = GridPlanner(_box_robot(), footprint="oriented", turn_cost=1.0)
    fe.setup_problem(meta, s[0], s[1], 0.0, t[0], t[1], 0.0, grid=grid)
    path = fe.solve()
    assert path is not None and fe.status == ref.FOUND
    np.testing.assert_array_equal(fe.get_path_states(), want["states"])
    np.testing.assert_array_equal(fe.path_cells, want["cells"])
    assert np.float32(fe.get_cost()) == ref.cost_in_metres(670, oref.RES) == np.float32(fe.path_length)
    with pytest.raises(ValueError, match="clearance"):
        fe.set_clearance_cost(0.4, 4.0)
    disc = GridPlanner(_box_robot())
    disc.setup_problem(meta, s[0], s[1], 0.0, t[0], t[1], 0.0, grid=grid)
    assert disc.solve() is None and disc.status == ref.START_INVALID and len(disc.get_path_states()) == 0
