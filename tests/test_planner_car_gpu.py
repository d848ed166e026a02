"""The grid planner's car motion on the MI355X (kc_planner_set_car / solve_car / get_car_field / get_car_path,
kompass_cpp.planning, kompass_core.planning; DESIGN.md 4.10 rules 27 to 36): the moves bytes, the eight field layers,
status, cost, states, primitives and the expanded cells bit for bit against the CPU statement of
tests/planner_car_ref.py, on degenerate shapes, one tile, ragged tiles, the three 72 x 70 scenes and the issue's own;
both footprints; every goal heading; host against device-resident maps; off means off; the exclusions.

Every grid is at most 130 cells a side.  Every test runs under the time limit of test_planner_gpu.py, for its reason:
a solve that went wrong would run to its pass cap, and only the thread method ends a native call."""

import numpy as np
import pytest

TIME_LIMIT_S = 120

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(TIME_LIMIT_S, method="thread")]

import kompass_cpp  # noqa: E402
import kompass_hip as kh  # noqa: E402
import planner_car_ref as cref  # noqa: E402
import planner_oriented_ref as oref  # noqa: E402
import planner_ref as ref  # noqa: E402
from helpers import DeviceArray  # noqa: E402

SMALL = (9, 1)      # A2, B2 of the 0.3 x 0.1 m box at 0.05 m
NMAX = kh.PLAN_MAX_TURN_CELLS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert kh.device_count() >= 1, "no HIP device visible"


@pytest.fixture()
def ctx():
    c = kh.PlannerContext()
    yield c
    c.close()


_MAPS = {}


def statement(grid, start, h0, goal, hg, n, rw, r2=0, box=None, allow_unknown=True):
    """cref.plan with the maps of (grid, footprint, n, rw) made once: they do not depend on the problem."""
    key = (grid.tobytes(), grid.shape, n, rw, r2, box, allow_unknown)
    if key not in _MAPS:
        valid = cref.state_validity(grid, r2, box, allow_unknown)
        _MAPS[key] = (valid, cref.moves_map(valid, box is None, n, rw))
    valid, moves = _MAPS[key]
    field = cref.state_field(valid, moves, goal, hg, n, rw)
    st = cref.status(valid, field, start, h0, goal, hg)
    out = dict(status=st, valid=valid, moves=moves, field=field, states=None, prims=None, cells=None, cost=ref.INF, step_costs=None)
    if st == ref.FOUND:
        out["states"], out["prims"], out["step_costs"] = cref.walk(moves, field, start, h0, n, rw)
        out["cells"], _ = cref.expand(out["states"], out["prims"], n)
        out["cost"] = int(field[h0, start[0], start[1]])
    return out


def compare(ctx, grid, start, h0, goal, hg, n, rw, r2=0, box=None, allow_unknown=True):
    """One solve on the grid and mode the context holds against the statement: validity by heading, the moves bytes, the
    eight field layers, status, cost, passes within the cap, states, primitives and expanded cells."""
    w, h = grid.shape
    want = statement(grid, start, h0, goal, hg, n, rw, r2, box, allow_unknown)
    st, cost, passes = ctx.solve_car(start, h0, goal, hg, r2, allow_unknown)
    f, m, v = ctx.car_field()
    np.testing.assert_array_equal(v, want["valid"])
    np.testing.assert_array_equal(m, want["moves"])
    np.testing.assert_array_equal(f, want["field"])
    assert st == want["status"], (st, want["status"])
    assert cost == want["cost"]
    assert 0 <= passes <= 8 * w * h + 1
    states, prims = ctx.car_path()
    cells = ctx.path()
    if st == ref.FOUND:
        np.testing.assert_array_equal(states, want["states"])
        np.testing.assert_array_equal(prims, want["prims"])
        np.testing.assert_array_equal(cells, want["cells"])
        assert sum(want["step_costs"]) == cost          # rule 33: the walk pays what the field says
    else:
        assert len(states) == 0 and len(prims) == 0 and len(cells) == 0
    return want


def seeded(shape, seed, p=0.02):
    """Bernoulli(p) obstacles with the two corners cleared."""
    w, h = shape
    g = np.where(np.random.default_rng(seed).random(shape) < p, ref.OCCUPIED, 0).astype(np.int32)
    g[:min(w, 10), :min(h, 10)] = 0
    g[max(0, w - 10):, max(0, h - 10):] = 0
    return g


def test_the_issues_scenes(ctx):
    grid, start, goal = cref.dead_end_scene()
    ctx.set_grid(grid)
    for n, rw, status, cost in [(1, 0, ref.UNREACHABLE, ref.INF), (2, 0, ref.UNREACHABLE, ref.INF), (1, 2, ref.FOUND, 274), (2, 2, ref.FOUND, 300)]:
        ctx.set_car(n, rw)
        want = compare(ctx, grid, start, 0, goal, cref.ANY, n, rw, r2=1)
        assert (want["status"], want["cost"]) == (status, cost)
    assert ctx.car_path()[1].tolist() == [cref.B] * 15
    ctx.set_car(1, 2)
    ctx.solve_car(start, 0, goal, cref.ANY, 1)
    assert ctx.car_path()[1].tolist() == [cref.BL, cref.R, cref.BL, cref.R] + [cref.S] * 13
    grid, start, goal = cref.free_scene()
    ctx.set_grid(grid)
    ctx.set_car(2, 0)
    want = compare(ctx, grid, start, 0, goal, 4, 2, 0)
    assert want["cost"] == 410 and want["prims"].tolist() == [cref.S] + [cref.L] * 5 + [cref.S] * 8 + [cref.R]
    # the goal cell is the start cell, in another heading: the path leaves and comes back
    want = compare(ctx, grid, start, 0, start, 4, 2, 0)
    assert want["status"] == ref.FOUND and want["cost"] > 0 and len(want["states"]) > 1
    assert compare(ctx, grid, start, 0, start, 0, 2, 0)["cost"] == 0
    assert compare(ctx, grid, start, 3, start, cref.ANY, 2, 0)["cost"] == 0


@pytest.mark.parametrize("shape", [(1, 1), (1, 40), (40, 1)])
def test_degenerate_shapes(ctx, shape):
    grid = np.zeros(shape, np.int32)
    c = (shape[0] // 2, shape[1] // 2)
    far = (shape[0] - 1, shape[1] - 1)
    ctx.set_grid(grid)
    for n, rw in [(1, 0), (2, 3), (NMAX, 16)]:
        ctx.set_car(n, rw)
        for h0 in range(8):
            want = compare(ctx, grid, c, h0, c, cref.ANY, n, rw)                # goal = start
            assert want["status"] == ref.FOUND and want["cost"] == 0 and len(want["states"]) == 1
        compare(ctx, grid, (0, 0), 0, far, cref.ANY, n, rw)
        compare(ctx, grid, (0, 0), 2, far, 2, n, rw)
        compare(ctx, grid, far, 0, (0, 0), cref.ANY, n, rw)                       # backwards or not at all
        want = compare(ctx, grid, c, 0, c, 4, n, rw)                              # no room to come back in another heading
        assert want["status"] == ref.UNREACHABLE
        assert compare(ctx, grid, (-1, 0), 0, c, cref.ANY, n, rw)["status"] == ref.START_OUTSIDE
        assert compare(ctx, grid, c, 0, (shape[0], 0), cref.ANY, n, rw)["status"] == ref.GOAL_OUTSIDE


@pytest.mark.parametrize("shape", [(64, 64), (65, 63), (130, 70)])
def test_one_tile_and_ragged_tiles(ctx, shape):
    grid = seeded(shape, 11)
    w, h = shape
    start, goal = (3, 3), (w - 4, h - 4)
    ctx.set_grid(grid)
    found = 0
    for n, rw, r2, hg in [(1, 0, 0, cref.ANY), (2, 1, 4, 6), (3, 3, 0, 1), (NMAX, 16, 4, cref.ANY)]:
        ctx.set_car(n, rw)
        found += compare(ctx, grid, start, 1, goal, hg, n, rw, r2)["status"] == ref.FOUND
    assert found >= 2


def test_arcs_across_tile_borders_and_at_the_edges(ctx):
    """A free 130 x 70 grid: every arc at every place is in the moves bytes and the field, which are compared whole.
    On top of that, paths whose arcs cross the tile border at i = 64 and j = 64 on both diagonals, an arc that ends
    in the last row or column, and arcs that would leave the grid."""
    grid = np.zeros((130, 70), np.int32)
    ctx.set_grid(grid)
    n = 3
    ctx.set_car(n, 1)
    crossed = set()
    for start, h0, goal, hg in [((60, 60), 0, (70, 68), 2), ((68, 60), 4, (58, 68), 2), ((60, 68), 0, (70, 58), 6), ((68, 68), 4, (58, 58), 6),
                                ((61, 61), 1, (67, 69), 2), ((67, 61), 3, (61, 69), 2)]:
        want = compare(ctx, grid, start, h0, goal, hg, n, 1)
        assert want["status"] == ref.FOUND
        for a, b, prim in zip(want["states"][:-1], want["states"][1:], want["prims"]):
            if prim in (cref.L, cref.R, cref.BL, cref.BR):
                if min(a[0], b[0]) < 64 <= max(a[0], b[0]):
                    crossed.add(("i", int(a[2]) & 1))
                if min(a[1], b[1]) < 64 <= max(a[1], b[1]):
                    crossed.add(("j", int(a[2]) & 1))
    assert {("i", 0), ("i", 1), ("j", 0), ("j", 1)} <= crossed, crossed
    _, m, _ = ctx.car_field()
    assert m[0, 129 - 2 * n, 30] >> cref.L & 1 and cref.target(129 - 2 * n, 30, 0, cref.L, n)[0] == 129      # ends in the last column
    assert m[2, 30, 69 - 2 * n] >> cref.R & 1 and cref.target(30, 69 - 2 * n, 2, cref.R, n)[1] == 69          # ... the last row
    assert not m[0, 129 - 2 * n + 1, 30] >> cref.L & 1 and not m[2, 30, 69 - 2 * n + 1] >> cref.R & 1         # would leave the grid
    assert not m[4, 2 * n - 1, 30] >> cref.L & 1 and m[4, 2 * n - 1, 30] >> cref.BL & 1
    assert not m[0, 129, 30] & 1 and m[0, 129, 30] >> cref.B & 1
    want = compare(ctx, grid, (129 - 2 * n, 30), 0, (129, 30 + n), 1, n, 1)
    assert want["prims"].tolist() == [cref.L]


@pytest.mark.parametrize("scene", ["corridor", "l", "clutter"])
def test_the_three_scenes_both_footprints(ctx, scene):
    grid, start, goal = {"corridor": oref.corridor_scene, "l": oref.l_scene, "clutter": oref.clutter_scene}[scene]()
    ctx.set_grid(grid)
    found = 0
    for n, rw, r2, box in [(1, 0, 0, None), (2, 1, 4, None), (3, 3, 4, None), (NMAX, 16, 0, None), (1, 1, 0, SMALL), (2, 0, 0, SMALL),
                           (3, 16, 0, SMALL)]:
        ctx.set_car(n, rw, *(box or (0, 0)))
        found += compare(ctx, grid, start, 0, goal, cref.ANY, n, rw, r2, box)["status"] == ref.FOUND
    assert found >= 3


@pytest.mark.parametrize("box", [None, SMALL])
def test_every_goal_heading(ctx, box):
    grid, start, goal = oref.clutter_scene()
    ctx.set_grid(grid)
    ctx.set_car(2, 1, *(box or (0, 0)))
    costs = []
    for hg in (cref.ANY,) + tuple(range(8)):
        want = compare(ctx, grid, start, 1, goal, hg, 2, 1, 1, box)
        assert want["status"] == ref.FOUND and (hg == cref.ANY or want["states"][-1][2] == hg)
        costs.append(want["cost"])
    assert costs[0] == min(costs[1:])
    # a goal heading the box does not fit in at the goal: GOAL_INVALID although the cell has valid headings
    if box:
        g2, s2, t2 = oref.corridor_scene()
        ctx.set_grid(g2)
        ctx.set_car(1, 1, 225, 4)
        assert compare(ctx, g2, s2, 0, t2, 2, 1, 1, 0, (225, 4))["status"] == ref.GOAL_INVALID
        assert compare(ctx, g2, s2, 2, t2, 0, 1, 1, 0, (225, 4))["status"] == ref.START_INVALID
        assert compare(ctx, g2, s2, 4, t2, 0, 1, 1, 0, (225, 4))["status"] == ref.UNREACHABLE    # nowhere to turn round
        want = compare(ctx, g2, s2, 4, t2, 4, 1, 1, 0, (225, 4))                                 # backwards all the way
        assert want["status"] == ref.FOUND and want["prims"].tolist() == [cref.B] * 67


@pytest.mark.parametrize("allow_unknown", [True, False])
def test_unknown_cells(ctx, allow_unknown):
    grid, start, goal = oref.clutter_scene(unknown=True)
    assert (grid == -1).sum() > 10
    ctx.set_grid(grid)
    for box in (None, SMALL):
        ctx.set_car(2, 2, *(box or (0, 0)))
        want = compare(ctx, grid, start, 0, goal, cref.ANY, 2, 2, 2, box, allow_unknown)
        assert want["status"] == ref.FOUND
        compare(ctx, grid, goal, 5, start, 3, 2, 2, 2, box, allow_unknown)               # the way back


def _outputs(ctx, start, h0, goal, hg, r2):
    res = ctx.solve_car(start, h0, goal, hg, r2)
    return res, ctx.car_field(), ctx.car_path(), ctx.path()


def _assert_same(a, b):
    assert a[0] == b[0]
    for x, y in zip(a[1] + a[2], b[1] + b[2]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a[3], b[3])


def test_host_device_and_world_map_grids_agree(ctx):
    from kompass_core.mapping import WorldMap

    grid, start, goal = oref.clutter_scene(unknown=True)
    ctx.set_car(2, 1)
    ctx.set_grid(grid)
    host = _outputs(ctx, start, 0, goal, 4, 1)
    assert host[0][0] == kh.PLAN_FOUND
    ctx.set_grid(grid.astype(np.int8))
    _assert_same(_outputs(ctx, start, 0, goal, 4, 1), host)
    for dtype in (np.int32, np.int8):
        g = np.asfortranarray(grid.astype(dtype))
        with DeviceArray(g) as buf:
            ctx.set_grid(np.zeros_like(grid))
            ctx.set_grid_device(buf.ptr, 72, 70, elem_bytes=g.itemsize)
            dev = _outputs(ctx, start, 0, goal, 4, 1)
        _assert_same(dev, host)
    wm = WorldMap(72, 70, oref.RES, (0.0, 0.0))
    wm.set_prior(grid)
    np.testing.assert_array_equal(np.asarray(wm.occupancy), grid)
    dg = wm.device_grid
    ptr = dg.__cuda_array_interface__["data"][0]
    ctx.set_grid(np.zeros_like(grid))
    ctx.set_grid_device(ptr, 72, 70, elem_bytes=1)
    _assert_same(_outputs(ctx, start, 0, goal, 4, 1), host)


def test_other_modes_are_unchanged_by_default_and_after_on_and_off(ctx):
    grid, start, goal = oref.clutter_scene(unknown=True)

    def others(c):
        out = []
        for r2, unknown in ((0, True), (2, False)):
            res = c.solve(start, goal, r2, unknown)
            out.append((res, c.field(), c.path()))
        c.set_oriented(*SMALL, 7)
        res = c.solve_oriented(start, 1, goal)
        out.append((res, c.oriented_field(), c.oriented_path()))
        c.set_oriented(0)
        return out

    def check(got):
        for k, (r2, unknown) in enumerate(((0, True), (2, False))):
            res, (f, v), p = got[k]
            valid = ref.validity(grid, r2, unknown)
            field = ref.cost_field(valid, goal)
            np.testing.assert_array_equal(v, valid)
            np.testing.assert_array_equal(f, field)
            st = ref.status(valid, field, start, goal)
            assert res[:2] == (st, int(field[start]) if st == ref.FOUND else ref.INF)
            np.testing.assert_array_equal(p, ref.walk(valid, field, start) if st == ref.FOUND else np.zeros((0, 2), np.int32))
        res, (f, v, t), states = got[2]
        want = oref.plan(grid, start, 1, goal, *SMALL, 7)
        np.testing.assert_array_equal(f, want["field"])
        np.testing.assert_array_equal(v, want["valid"])
        np.testing.assert_array_equal(t, want["turn"])
        assert res[:2] == (want["status"], want["cost"])
        np.testing.assert_array_equal(states, want["states"])

    ctx.set_grid(grid)
    fresh = others(ctx)                     # the mode never set
    check(fresh)
    for box in ((0, 0), SMALL):
        ctx.set_car(2, 1, *box)
        assert ctx.solve_car(start, 0, goal, cref.ANY, 1)[0] == kh.PLAN_FOUND
        assert len(ctx.car_path()[0]) > 0
        ctx.set_car(0)
        got = others(ctx)
        check(got)
        for a, b in zip(fresh, got):
            assert a[0] == b[0]             # status, cost and passes
            for x, y in zip(a[1], b[1]):
                assert x.tobytes() == y.tobytes()
            assert a[2].tobytes() == b[2].tobytes()
    with pytest.raises(kh.KompassHipError):                # off again: the car calls have nothing to give
        ctx.car_field()
    with pytest.raises(kh.KompassHipError):
        ctx.solve_car(start, 0, goal)


def test_abi_exclusions_and_range_errors(ctx):
    grid, start, goal = oref.clutter_scene()
    ctx.set_grid(grid)
    with pytest.raises(IndexError):                        # n above the maximum
        ctx.set_car(NMAX + 1, 0)
    with pytest.raises(IndexError):
        ctx.set_car(-1, 0)
    with pytest.raises(IndexError):                        # rw > 16
        ctx.set_car(2, 17)
    with pytest.raises(IndexError):                        # a box beyond 254 cells
        ctx.set_car(2, 0, 254 * 254, 1)
    with pytest.raises(kh.KompassHipError):                # off: the car solve has no mode
        ctx.solve_car(start, 0, goal)
    ctx.set_car(2, 1)
    with pytest.raises(ValueError):
        ctx.solve_car(start, 8, goal)
    with pytest.raises(ValueError):
        ctx.solve_car(start, 0, goal, -2)
    with pytest.raises(kh.KompassHipError):                # the other solves belong to the other modes
        ctx.solve(start, goal, 1)
    with pytest.raises(kh.KompassHipError):
        ctx.solve_oriented(start, 0, goal)
    with pytest.raises(kh.KompassHipError):
        ctx.replan(start, goal, 1)
    with pytest.raises(kh.KompassHipError, match="car"):
        ctx.explore(start, 1)
    with pytest.raises(kh.KompassHipError, match="clearance"):   # set second, refused
        ctx.set_clearance_cost(9, np.zeros(10, np.uint32))
    with pytest.raises(kh.KompassHipError, match="car"):
        ctx.set_oriented(*SMALL, 10)
    assert ctx.solve_car(start, 0, goal, cref.ANY, 1)[0] == kh.PLAN_FOUND
    with pytest.raises(kh.KompassHipError, match="any-angle"):
        ctx.shortcut(16)
    with pytest.raises(kh.KompassHipError):
        ctx.field()
    with pytest.raises(kh.KompassHipError):
        ctx.oriented_field()
    ctx.set_car(0)
    ctx.set_clearance_cost(9, np.zeros(10, np.uint32))
    with pytest.raises(kh.KompassHipError, match="clearance"):   # the other order
        ctx.set_car(2, 1)
    ctx.set_clearance_cost(0)
    ctx.set_oriented(*SMALL, 10)
    with pytest.raises(kh.KompassHipError, match="oriented"):
        ctx.set_car(2, 1)
    ctx.set_oriented(0)
    ctx.set_car(2, 1)
    assert ctx.car_info()[:2] == (2, 1)


def test_rule_32s_bound(ctx):
    """24 n max(rw, 1) 8 cells must fit: the smallest grid that n = 8, rw = 16 is refused on, one cell wide; it passes at
    n = 1 without reverse (the goal heading keeps the field to the cells below the goal: three passes)."""
    cells = 174763
    assert cref.check_range(NMAX, 16, cells - 1)
    grid = np.zeros((1, cells), np.int8)
    assert cref.check_range(1, 0, cells) and not cref.check_range(NMAX, 16, cells)
    ctx.set_grid(grid)
    ctx.set_car(NMAX, 16)
    with pytest.raises(IndexError):
        ctx.solve_car((0, 0), 2, (0, 5))
    ctx.set_car(1, 0)
    st, cost, passes = ctx.solve_car((0, 0), 2, (0, 100), 2)
    assert (st, cost) == (kh.PLAN_FOUND, 1000) and passes <= 8 * cells + 1
    assert ctx.car_path()[1].tolist() == [cref.S] * 100


# ---- the class and the front end at 0.05 m ------------------------------------------------------------------------
ORIGIN = (-1.0, 0.5)


def _world(cell):
    return (float(ref.cell_to_world(cell[0], ORIGIN[0], oref.RES)) + 0.01, float(ref.cell_to_world(cell[1], ORIGIN[1], oref.RES)) + 0.01)


def test_class_on_the_free_scene_and_the_dead_end():
    CYL = kompass_cpp.types.RobotGeometry.CYLINDER
    grid, start, goal = cref.free_scene()
    want = statement(grid, start, 0, goal, 4, 2, 0, r2=1)
    p = kompass_cpp.planning.GridPlanner(CYL, [0.05, 0.4])
    p.set_car_motion(True, 0.2, False, 2, True)               # before the bounds: evaluated once they are known
    assert p.car_on() and p.get_car_reverse_weight() == 0
    p.set_space_bounds_from_map(ORIGIN[0], ORIGIN[1], 40, 30, oref.RES)
    assert p.get_car_turn_cells() == 2 == cref.turn_cells(0.2, oref.RES) and p.get_footprint_r2() == 1
    p.set_grid(grid)
    s, t = _world(start), _world(goal)
    p.setup_problem(s[0], s[1], 0.1, t[0], t[1], 3.1)          # yaw 0.1 is heading 0, 3.1 heading 4
    assert p.get_cells() == (start, goal)
    assert p.solve() and p.get_status() == ref.FOUND
    np.testing.assert_array_equal(p.get_path_states(), want["states"])
    np.testing.assert_array_equal(p.get_path_moves(), want["prims"])
    np.testing.assert_array_equal(p.get_path_cells(), want["cells"])
    np.testing.assert_array_equal(p.get_path_cells(True), ref.simplify(want["cells"]))
    f, m, v = p.get_car_field()
    np.testing.assert_array_equal(f, want["field"])
    np.testing.assert_array_equal(m, want["moves"])
    np.testing.assert_array_equal(np.stack([(v >> h & 1).astype(bool) for h in range(8)]), want["valid"])
    assert want["cost"] == 410 and np.float32(p.get_cost()) == ref.cost_in_metres(410, oref.RES)
    d = np.abs(np.diff(want["cells"], axis=0)).sum(axis=1)
    assert np.float32(p.get_path_length()) == ref.cost_in_metres(int((d == 1).sum() * 10 + (d == 2).sum() * 14), oref.RES)
    path = p.get_solution()
    np.testing.assert_array_equal(np.asarray(path.x()), ref.cell_to_world(want["cells"][:, 0], ORIGIN[0], oref.RES))
    np.testing.assert_array_equal(np.asarray(path.y()), ref.cell_to_world(want["cells"][:, 1], ORIGIN[1], oref.RES))
    assert p.replan() and not p.replanned()                   # rule 35: a full solve
    np.testing.assert_array_equal(p.get_path_states(), want["states"])
    # the goal's yaw not honoured: every heading ends the path
    p.set_car_motion(True, 0.2, False, 2, False)
    assert p.solve()
    np.testing.assert_array_equal(p.get_path_moves(), statement(grid, start, 0, goal, cref.ANY, 2, 0, r2=1)["prims"])
    # rule 35's errors
    with pytest.raises(ValueError, match="any-angle"):
        p.get_any_angle_cells(16)
    with pytest.raises(ValueError, match="clearance"):
        p.set_clearance_cost(0.4, 4.0)
    with pytest.raises(ValueError, match="car"):
        p.explore(s[0], s[1], 0.0, 1)
    with pytest.raises(IndexError):                           # 0.05 m cells: 1.0 m is 9 turn cells
        p.set_car_motion(True, 1.0, False, 2, True)
    assert p.get_car_turn_cells() == 2                        # a refused mode leaves the one before
    with pytest.raises(IndexError):
        p.set_car_motion(True, 0.2, True, 17, True)
    r = kompass_cpp.planning.GridPlanner(CYL, [0.05, 0.4])
    r.set_clearance_cost(0.4, 4.0)
    with pytest.raises(ValueError, match="clearance"):
        r.set_car_motion(True, 0.2, False, 2, True)
    # the dead end: reverse at a price; getPathLength does not weigh it
    grid, start, goal = cref.dead_end_scene()
    s, t = _world(start), _world(goal)
    q = kompass_cpp.planning.GridPlanner(CYL, [0.05, 0.4])
    q.set_space_bounds_from_map(ORIGIN[0], ORIGIN[1], 40, 21, oref.RES)
    q.set_grid(grid)
    q.setup_problem(s[0], s[1], 0.0, t[0], t[1], float("nan"))   # a goal yaw that is no number: any heading
    q.set_car_motion(True, 0.2, False, 2, True)
    assert not q.solve() and q.get_status() == ref.UNREACHABLE and len(q.get_path_states()) == 0 and len(q.get_path_moves()) == 0
    q.set_car_motion(True, 0.2, True, 2, True)
    assert q.get_car_reverse_weight() == 2
    assert q.solve() and q.get_path_moves().tolist() == [cref.B] * 15
    assert np.float32(q.get_cost()) == ref.cost_in_metres(300, oref.RES) and np.float32(q.get_path_length()) == ref.cost_in_metres(150, oref.RES)
    q.set_car_motion(False)                                   # off again: the disc planner, heading-free
    assert q.solve() and len(q.get_path_states()) == 0 and np.float32(q.get_cost()) == ref.cost_in_metres(150, oref.RES)


def test_front_end_both_footprints_and_a_world_map():
    from kompass_core.mapping import WorldMap
    from kompass_core.planning import GridPlanner
    from test_planner_gpu import _robot
    from test_planner_oriented_cpu import _box_robot

    grid, start, goal = oref.clutter_scene()
    origin = (0.0, 0.0)
    meta = dict(origin_x=origin[0], origin_y=origin[1], width=72, height=70, resolution=oref.RES)
    world = lambda c: (c[0] * oref.RES + 0.01, c[1] * oref.RES + 0.01)
    s, t = world(start), world(goal)
    # the disc: a 0.05 m cylinder is R2 = 1; 0.2 m of turning radius is n = 2
    want = statement(grid, start, 1, goal, 2, 2, 3, r2=1)
    fe = GridPlanner(_robot((0.05, 0.4)), motion="car", min_turning_radius=0.2, allow_reverse=True, reverse_weight=3)
    fe.setup_problem(meta, s[0], s[1], 0.8, t[0], t[1], 1.6, grid=grid)
    path = fe.solve()
    assert path is not None and fe.status == ref.FOUND and fe.turn_cells == 2
    np.testing.assert_array_equal(fe.get_path_states(), want["states"])
    np.testing.assert_array_equal(fe.get_path_moves(), want["prims"])
    np.testing.assert_array_equal(fe.path_cells, want["cells"])
    assert np.float32(fe.get_cost()) == ref.cost_in_metres(want["cost"], oref.RES)
    # the same map as a WorldMap, read in place
    wm = WorldMap(72, 70, oref.RES, origin)
    wm.set_prior(grid)
    fw = GridPlanner(_robot((0.05, 0.4)), motion="car", min_turning_radius=0.2, allow_reverse=True, reverse_weight=3)
    fw.setup_problem(None, s[0], s[1], 0.8, t[0], t[1], 1.6, grid=wm)
    assert fw.solve() is not None
    np.testing.assert_array_equal(fw.get_path_states(), want["states"])
    np.testing.assert_array_equal(fw.path_cells, want["cells"])
    assert fw.replan(start=(s[0], s[1], 0.8)) is not None and not fw.replanned
    # goal_heading="any", and the oriented footprint: the 0.3 x 0.1 m box is (A2, B2) = (9, 1)
    want = statement(grid, start, 1, goal, cref.ANY, 2, 0, box=SMALL)
    fo = GridPlanner(_box_robot(oref.SMALL_BOX), footprint="oriented", motion="car", min_turning_radius=0.2, goal_heading="any")
    fo.setup_problem(meta, s[0], s[1], 0.8, t[0], t[1], 1.6, grid=grid)
    assert fo.solve() is not None
    np.testing.assert_array_equal(fo.get_path_states(), want["states"])
    np.testing.assert_array_equal(fo.path_cells, want["cells"])
    # rule 35's errors
    with pytest.raises(ValueError, match="car"):
        fe.find_frontiers(s[0], s[1])
    with pytest.raises(ValueError, match="car"):
        fe.explore(s[0], s[1])
    with pytest.raises(ValueError, match="clearance"):
        fe.set_clearance_cost(0.4, 4.0)
    # the default stays the grid planner
    disc = GridPlanner(_robot((0.05, 0.4)))
    disc.setup_problem(meta, s[0], s[1], 0.8, t[0], t[1], 1.6, grid=grid)
    assert disc.solve() is not None and disc.motion == "grid" and disc.turn_cells == 0
    assert len(disc.get_path_states()) == 0 and len(disc.get_path_moves()) == 0
    np.testing.assert_array_equal(disc.path_cells, ref.walk(ref.validity(grid, 1), ref.cost_field(ref.validity(grid, 1), goal), start))
