"""Exploration on the MI355X (kc_planner_explore and its getters, kompass_cpp.planning, kompass_core.planning; DESIGN.md
4.10 rules 21 to 26) against the CPU statement tests/planner_frontier_ref.py: labels, field, validity, records and their
order, status, components and every path, bit for bit: the outputs are integers, there is no tolerance anywhere.

Every test runs under the time limit of test_planner_gpu.py, for its reason: a solve or a labelling that went wrong
would run to its pass cap, and only the thread method ends a native call."""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

TIME_LIMIT_S = 120

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(TIME_LIMIT_S, method="thread")]

import kompass_hip as kh  # noqa: E402
import planner_frontier_ref as fref  # noqa: E402
import planner_ref as ref  # noqa: E402
from helpers import DeviceArray  # noqa: E402
from test_planner_frontier_cpu import ragged, serpentine, tie_grids  # noqa: E402

INF = ref.INF
U, O = ref.UNEXPLORED, ref.OCCUPIED
STATE = r"\[kc -5\]"
SHAPES = [(1, 1), (1, 70), (70, 1), (5, 3), (37, 29), (63, 64), (64, 64), (65, 65), (129, 67)]
DENSITIES = [0.02, 0.1, 0.3]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert kh.device_count() >= 1, "no HIP device visible"


@pytest.fixture()
def ctx():
    c = kh.PlannerContext()
    yield c
    c.close()


@pytest.fixture()
def other():
    c = kh.PlannerContext()
    yield c
    c.close()


def records_of(ctx):
    return [dict(size=int(r["size"]), sum_i=int(r["sum_i"]), sum_j=int(r["sum_j"]), entry=(int(r["entry_i"]), int(r["entry_j"])),
                 cost=int(r["cost"]), root=int(r["root"])) for r in ctx.frontiers()]


def check_paths(ctx, want, robot):
    """Every kept frontier's path: the statement's, from the robot to the entry, legal, and as long as its cost."""
    for k, (rec, path) in enumerate(zip(want["frontiers"], want["paths"])):
        got = ctx.frontier_path(k)
        np.testing.assert_array_equal(got, path)
        assert tuple(got[0]) == tuple(robot) and tuple(got[-1]) == rec["entry"]
        ref.check_path(want["valid"], got, tuple(robot), rec["entry"])
        assert fref.path_cost(got) == rec["cost"]
    with pytest.raises(IndexError):
        ctx.frontier_path(len(want["frontiers"]))


def explore_and_check(ctx, grid, robot, r2=0, min_cost=0, min_size=1, want=None, paths=True):
    """One explore of the grid the context holds against the statement -> (the statement, label passes)."""
    if want is None:
        want = fref.explore(grid, robot, r2, min_cost, min_size, paths=paths)
    st, comps, kept, passes, lpasses = ctx.explore(robot, r2, min_cost, min_size)
    f, v = ctx.field()
    np.testing.assert_array_equal(v, want["valid"])
    np.testing.assert_array_equal(f, want["field"])
    np.testing.assert_array_equal(ctx.frontier_labels(), want["labels"])
    assert (st, comps, kept) == (want["status"], want["components"], len(want["frontiers"]))
    assert records_of(ctx) == want["frontiers"]
    if paths:
        check_paths(ctx, want, robot)
    listed, tiles, _ = ctx.explore_info()
    w, h = grid.shape
    front = want["labels"] != INF
    tile_has = {(i // 64, j // 64) for i, j in np.argwhere(front)}
    assert tiles == -(-w // 64) * -(-h // 64) and listed == len(tile_has)
    assert (lpasses == 0) == (listed == 0)
    return want, lpasses


def pick_robot(grid, r2, rng):
    free = np.argwhere(fref.explore_validity(grid, r2))
    return tuple(int(v) for v in free[rng.integers(len(free))]) if len(free) else (0, 0)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("density", DENSITIES)
def test_ragged_grids(ctx, shape, density):
    """Seeded grids with blobs of unknown: r2 in {0, 1, 8}, min_cost in {0, 30}, min_size in {1, 3}, from a host array and
    from a grid that lies on the device.  The statement's maps are made once per r2 and shared."""
    seed = shape[0] * 1000 + shape[1] * 10 + int(density * 100)
    rng = np.random.default_rng(seed)
    grid = ragged(shape, density, seed)
    w, h = shape
    with DeviceArray(np.asfortranarray(grid)) as dev:
        for r2 in (0, 1, 8):
            robot = pick_robot(grid, r2, rng)
            valid = fref.explore_validity(grid, r2)
            field = ref.cost_field(valid, robot)
            for min_cost in (0, 30):
                labels = fref.label(fref.frontier_cells(grid, valid, field, min_cost))
                for min_size in (1, 3):
                    comps, kept = fref.records(labels, field, min_size)
                    status = ref.START_INVALID if not valid[robot] else (ref.FOUND if kept else fref.NO_FRONTIER)
                    want = dict(status=status, valid=valid, field=field, labels=labels, components=comps, frontiers=kept,
                                paths=[fref.frontier_path(valid, field, r["entry"]) for r in kept])
                    ctx.set_grid(grid)
                    explore_and_check(ctx, grid, robot, r2, min_cost, min_size, want)
                    ctx.set_grid_device(dev.ptr, w, h, 4)
                    explore_and_check(ctx, grid, robot, r2, min_cost, min_size, want)


def test_component_across_the_corner_of_four_tiles(ctx):
    """(63, 63) and (64, 64) of a 128 x 128 grid touch only by the corner where four tiles meet: one frontier."""
    g = np.full((128, 128), O, np.int32)
    g[63, 63] = g[64, 64] = 0
    g[62, 63] = g[65, 64] = U                       # each free cell's unknown neighbour
    g[63, 64] = 0                                   # the orthogonal cell a diagonal step needs ...
    g[64, 63] = 0                                   # ... both of them
    ctx.set_grid(g)
    want, lpasses = explore_and_check(ctx, g, (63, 63))
    front = want["labels"] != INF
    assert front[63, 63] and front[64, 64] and not front[63, 64] and not front[64, 63]
    assert want["components"] == 1 and want["labels"][64, 64] == 63 + 63 * 128 and lpasses >= 2


def test_serpentine_takes_more_than_one_pass(ctx):
    g = serpentine(64, 64)
    ctx.set_grid(g)
    want, lpasses = explore_and_check(ctx, g, (0, 0), paths=False)
    assert lpasses > 1
    assert want["components"] == 1 and want["frontiers"][0]["root"] == 0 and want["frontiers"][0]["size"] > 2000
    assert (ctx.frontier_labels()[want["labels"] != INF] == 0).all()
    check_paths(ctx, dict(want, paths=[fref.frontier_path(want["valid"], want["field"], want["frontiers"][0]["entry"])]), (0, 0))


def test_wide_component_across_four_tiles(ctx):
    g = serpentine(200, 64)
    ctx.set_grid(g)
    want, lpasses = explore_and_check(ctx, g, (100, 0), paths=False)
    assert want["components"] == 1 and want["frontiers"][0]["root"] == 0 and lpasses > 4


def test_sums_are_64_bit(ctx):
    """32768 x 17, even rows free, odd rows unknown but for a free column at i = 0: one frontier whose sum_i exceeds 2^32.
    Frontier cells, size and sums in closed form from numpy.  Cell (0, 0) has no unknown neighbour (its neighbours are
    the free (1, 0) and the free link (0, 1)), so by rule 23 it is no frontier cell and the label is 1, the flat index
    of (1, 0), not 0."""
    w, h = 32768, 17
    g = np.zeros((w, h), np.int8)
    g[1:, 1::2] = U
    ctx.set_grid(g)
    st, comps, kept, passes, lpasses = ctx.explore((0, 0), 0, 0, 1)
    front = np.zeros((w, h), bool)
    front[1:, 0::2] = True                          # beside the unknown row above or below
    front[0, 1::2] = True                           # the links: beside (1, j)
    ii, jj = np.nonzero(front)
    lab = ctx.frontier_labels()
    np.testing.assert_array_equal(lab != INF, front)
    assert (lab[front] == 1).all()
    assert (st, comps, kept) == (ref.FOUND, 1, 1) and lpasses > 1
    rec = records_of(ctx)[0]
    assert int(ii.sum()) > 2 ** 32
    f, v = ctx.field()
    key = (f[front].astype(np.int64) << 32) | (ii + jj * w)
    e = int(np.argmin(key))
    assert rec == dict(size=int(front.sum()), sum_i=int(ii.sum()), sum_j=int(jj.sum()), entry=(int(ii[e]), int(jj[e])),
                       cost=int(f[front][e]), root=1)
    assert rec["entry"] == (1, 0) and rec["cost"] == 10
    np.testing.assert_array_equal(ctx.frontier_path(0), [[0, 0], [1, 0]])


def test_equal_cost_ties(ctx):
    for grid, robot in tie_grids():
        ctx.set_grid(grid)
        want, _ = explore_and_check(ctx, grid, robot)
        costs = [r["cost"] for r in want["frontiers"]]
        assert costs == [30] * len(costs)
    assert [r["entry"] for r in want["frontiers"]] == [(1, 0)]


def test_checkerboard_and_one_cell_components(ctx):
    """A 65 x 65 checkerboard of free and unknown cells.  No step leaves the robot's cell there (the orthogonal
    neighbours are unknown and a diagonal step needs both of them), so by rules 22 and 23 the statement has one
    component, the robot's own cell: kept with min_size = 1, KC_PLAN_NO_FRONTIER with min_size = 2.  The many one-cell
    components that can be reached come from a board of period 3 under a free row: an unknown cell walled in by three
    occupied ones, its fourth neighbour a frontier of its own: 21 x 21 = 441 of them at 65 x 65 and 66 x 66 = 4356 at
    200 x 200, none kept with min_size = 2, all kept and sorted with min_size = 1."""
    ii, jj = np.meshgrid(np.arange(65), np.arange(65), indexing="ij")
    board = np.where((ii + jj) % 2 == 0, 0, U).astype(np.int32)
    ctx.set_grid(board)
    alone, _ = explore_and_check(ctx, board, (32, 32))
    assert alone["components"] == 1 and alone["frontiers"][0]["size"] == 1 and alone["frontiers"][0]["cost"] == 0
    none, _ = explore_and_check(ctx, board, (32, 32), min_size=2)
    assert none["status"] == fref.NO_FRONTIER and none["components"] == 1
    g = np.zeros((65, 65), np.int32)
    g[1::3, 2::3] = U
    g[1::3, 1::3] = O
    g[1::3, 3::3] = O
    g[0::3, 2::3] = O
    ctx.set_grid(g)
    want = fref.explore(g, (0, 0), 0, 0, 1)
    assert want["components"] == 441 and all(r["size"] == 1 for r in want["frontiers"]) and len(want["frontiers"]) == 441
    explore_and_check(ctx, g, (0, 0), min_size=1, want=want)
    none, _ = explore_and_check(ctx, g, (0, 0), min_size=2, paths=False)
    assert none["status"] == fref.NO_FRONTIER and none["components"] == 441 and none["frontiers"] == []
    # the same board at 200 x 200, sixteen tiles: thousands of them; the paths are left to the board above
    g = np.zeros((200, 200), np.int32)
    g[1::3, 2::3] = U
    g[1::3, 1::3] = O
    g[1::3, 3::3] = O
    g[0::3, 2::3] = O
    ctx.set_grid(g)
    want = fref.explore(g, (0, 0), 0, 0, 1, paths=False)
    assert want["components"] == 66 * 66 and len(want["frontiers"]) == 66 * 66 and all(r["size"] == 1 for r in want["frontiers"])
    explore_and_check(ctx, g, (0, 0), min_size=1, want=want, paths=False)
    none, _ = explore_and_check(ctx, g, (0, 0), min_size=2, paths=False)
    assert none["status"] == fref.NO_FRONTIER and none["components"] == 66 * 66 and none["frontiers"] == []


def test_frontier_behind_a_wall_and_a_door(ctx):
    g = np.zeros((40, 30), np.int32)
    g[20, :] = O                                    # the wall
    g[39, :] = U                                    # the unknown beyond it
    ctx.set_grid(g)
    closed, _ = explore_and_check(ctx, g, (5, 15))
    assert closed["status"] == fref.NO_FRONTIER and closed["components"] == 0
    g[20, 10] = 0                                   # the door
    ctx.set_grid(g)
    opened, _ = explore_and_check(ctx, g, (5, 15))
    assert opened["status"] == ref.FOUND and opened["frontiers"][0]["size"] == 30
    assert (opened["labels"][38, :] != INF).all()


def test_corridor_too_narrow_for_the_disc(ctx):
    g = np.zeros((60, 40), np.int32)
    g[25:35, :] = O
    g[25:35, 19:22] = 0                             # three cells wide: on its centre line the walls are 2 cells off, 4 <= 8
    g[59, :] = U
    ctx.set_grid(g)
    narrow, _ = explore_and_check(ctx, g, (5, 20), r2=8)
    assert narrow["status"] == fref.NO_FRONTIER and narrow["components"] == 0
    point, _ = explore_and_check(ctx, g, (5, 20), r2=0)
    assert point["status"] == ref.FOUND
    g[25:35, 16:25] = 0                             # nine cells wide: the walls are 5 cells off the centre line
    ctx.set_grid(g)
    wide, _ = explore_and_check(ctx, g, (5, 20), r2=8)
    assert wide["status"] == ref.FOUND


def test_no_unknown_and_the_robot_cell_cases(ctx):
    g = np.zeros((30, 20), np.int32)
    g[10, 10] = O
    ctx.set_grid(g)
    known, _ = explore_and_check(ctx, g, (3, 3))
    assert known["status"] == fref.NO_FRONTIER and known["components"] == 0
    g[25:, :] = U
    ctx.set_grid(g)
    for robot, status in [((27, 5), ref.START_INVALID), ((10, 10), ref.START_INVALID), ((-1, 5), ref.START_OUTSIDE),
                          ((30, 5), ref.START_OUTSIDE), ((5, 20), ref.START_OUTSIDE), ((5, 5), ref.FOUND)]:
        out, _ = explore_and_check(ctx, g, robot)
        assert out["status"] == status and (status == ref.FOUND or (out["components"] == 0 and len(ctx.frontiers()) == 0))
    out, _ = explore_and_check(ctx, g, (11, 10), r2=1)           # inside the inflation of (10, 10)
    assert out["status"] == ref.START_INVALID


def test_min_cost_drops_the_frontier_the_robot_stands_beside(ctx):
    g = np.zeros((50, 20), np.int32)
    g[0, :] = U
    g[49, :] = U
    ctx.set_grid(g)
    both, _ = explore_and_check(ctx, g, (2, 10))
    assert [r["entry"] for r in both["frontiers"]] == [(1, 10), (48, 10)]
    far, _ = explore_and_check(ctx, g, (2, 10), min_cost=200)
    assert [r["root"] for r in far["frontiers"]] == [48] and far["frontiers"][0]["cost"] == 460 and far["components"] == 1


# ---- what an explore leaves in the context ------------------------------------------------------------------------
def solve_outputs(c, start, goal, r2, unknown, replan=False):
    out = (c.replan if replan else c.solve)(start, goal, r2, unknown)
    f, v = c.field()
    return out[:2], f, v, c.path()


@pytest.mark.parametrize("unknown", [True, False])
@pytest.mark.parametrize("r2", [0, 8])
def test_a_solve_after_an_explore_is_a_fresh_solve(ctx, other, unknown, r2):
    grid = ragged((129, 67), 0.05, 7)
    rng = np.random.default_rng(5)
    valid = ref.validity(grid, r2, unknown)
    idx = np.argwhere(valid)
    start, goal = (tuple(int(v) for v in idx[k]) for k in rng.integers(0, len(idx), 2))
    other.set_grid(grid)
    fresh = solve_outputs(other, start, goal, r2, unknown)
    for replan in (False, True):
        ctx.set_grid(grid)
        ctx.solve(start, goal, r2, unknown)                      # a kept field and a cached validity map to get wrong
        ctx.explore(start, r2, 0, 1)
        got = solve_outputs(ctx, start, goal, r2, unknown, replan)
        assert got[0] == fresh[0]
        for a, b in zip(got[1:], fresh[1:]):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(got[1], ref.cost_field(valid, goal))
        if replan:
            assert ctx.replan_info()[0] is False                 # a full solve: the explore field is not kept


def test_explore_twice_follows_the_grid(ctx):
    g = ragged((65, 65), 0.05, 11)
    robot = pick_robot(g, 1, np.random.default_rng(1))
    ctx.set_grid(g)
    a, _ = explore_and_check(ctx, g, robot, r2=1)
    g2 = g.copy()
    g2[:, 40:] = U
    g2[robot] = 0
    ctx.set_grid(g2)
    b, _ = explore_and_check(ctx, g2, robot, r2=1)
    assert not np.array_equal(a["labels"], b["labels"])
    explore_and_check(ctx, g2, robot, r2=1, min_size=3)          # and once more without a grid in between


def test_call_order_and_argument_errors(ctx):
    g = np.zeros((20, 20), np.int32)
    g[19, :] = U
    with pytest.raises(kh.KompassHipError, match=STATE):
        ctx.explore((1, 1))                                      # no grid
    ctx.set_grid(g)
    for call in (ctx.frontiers, lambda: ctx.frontier_path(0), ctx.frontier_labels, ctx.explore_info):
        with pytest.raises(kh.KompassHipError, match=STATE):
            call()                                               # before any explore
    with pytest.raises(IndexError):
        ctx.explore((1, 1), r2=255 * 255)
    with pytest.raises(IndexError):
        ctx.explore((1, 1), min_size=0)
    assert ctx.explore((1, 1))[0] == ref.FOUND
    for call in (ctx.path, ctx.shortcut, ctx.path_clearance):
        with pytest.raises(kh.KompassHipError, match=STATE):
            call()                                               # a solve's getters after an explore
    assert len(ctx.frontiers()) == 1 and len(ctx.frontier_path(0)) == 18
    assert ctx.solve((1, 1), (10, 10))[0] == ref.FOUND and len(ctx.path()) == 10
    for call in (ctx.frontiers, lambda: ctx.frontier_path(0), ctx.frontier_labels, ctx.explore_info):
        with pytest.raises(kh.KompassHipError, match=STATE):
            call()                                               # the explore-only getters after a solve
    ctx.set_clearance_cost(9, np.arange(10)[::-1])
    with pytest.raises(kh.KompassHipError, match=STATE):
        ctx.explore((1, 1))
    ctx.set_clearance_cost(0)
    ctx.set_oriented(9, 1, 10)
    with pytest.raises(kh.KompassHipError, match=STATE):
        ctx.explore((1, 1))
    ctx.set_oriented(0)
    assert ctx.explore((1, 1))[0] == ref.FOUND


# ---- the front ends ---------------------------------------------------------------------------------------------
def test_front_ends_on_a_world_map():
    """The robot sees a disc of a room through WorldMap.update; find_frontiers(map=world_map) is the statement on
    world_map.occupancy, explore() the first path of that list, through kompass_cpp and kompass_core."""
    import kompass_cpp
    from kompass_core.datatypes.laserscan import LaserScanData
    from kompass_core.mapping import LocalMapper, MapConfig, WorldMap
    from kompass_core.models import RobotState
    from kompass_core.planning import Frontier, GridPlanner
    from test_planner_gpu import _robot
    from test_worldmap_gpu import _room_scan

    res, origin = 0.05, (-1.0, -1.0)
    wm = WorldMap(160, 120, res, origin)
    lm = LocalMapper(MapConfig(width=4.0, height=4.0, resolution=res))
    for x, y, yaw in [(1.5, 2.0, 0.0), (2.0, 1.8, 0.5)]:
        state = RobotState(x=x, y=y, yaw=yaw)
        ang, rng = _room_scan(x, y, yaw, (2.6, 0.6, 3.0, 1.4))
        lm.update_from_scan(state, LaserScanData(angles=ang, ranges=rng, angle_increment=2 * math.pi / 360, range_max=8.0))
        assert wm.update(state, lm) > 0
    occ = np.asarray(wm.occupancy)
    assert (occ == U).sum() > 1000 and (occ == 0).sum() > 1000
    robot = _robot()
    radius = 0.1
    r2 = ref.radius_to_r2(radius, res)
    rx, ry = 2.0, 1.8
    cell = (ref.world_to_cell(rx, origin[0], res), ref.world_to_cell(ry, origin[1], res))
    for min_size, min_distance in [(8, 0.0), (3, 0.5)]:
        min_cost = int(math.floor(min_distance / float(np.float32(res)) * 10.0 + 0.5))
        want = fref.explore(occ, cell, r2, min_cost, min_size)
        assert want["status"] == ref.FOUND and len(want["frontiers"]) >= 1
        fe = GridPlanner(robot, allow_unknown=False)              # rule 21: the setting plays no part
        found = fe.find_frontiers(rx, ry, map=wm, min_size=min_size, min_distance=min_distance)
        assert fe.components == want["components"] and fe.status == ref.FOUND and len(found) == len(want["frontiers"])
        np.testing.assert_array_equal(np.asarray(fe.frontier_labels()), want["labels"])
        for k, (f, r) in enumerate(zip(found, want["frontiers"])):
            assert isinstance(f, Frontier) and f.entry_cell == r["entry"] and (f.size, f.root) == (r["size"], r["root"])
            assert f.entry == (float(ref.cell_to_world(r["entry"][0], origin[0], res)), float(ref.cell_to_world(r["entry"][1], origin[1], res)))
            assert f.cost == float(ref.cost_in_metres(r["cost"], res))
            cen = tuple(float(np.float32(float(np.float32(o)) + s / r["size"] * float(np.float32(res))))
                        for o, s in zip(origin, (r["sum_i"], r["sum_j"])))
            assert f.centroid == cen
            np.testing.assert_array_equal(fe.frontier_path_cells(k), want["paths"][k])
        with pytest.raises(IndexError):
            fe.frontier_path(len(found))
        # explore: the first path, as world points
        path = GridPlanner(robot).explore(rx, ry, map=wm, min_size=min_size, min_distance=min_distance)
        first = want["paths"][0]
        np.testing.assert_array_equal(np.asarray(path.x()), ref.cell_to_world(first[:, 0], origin[0], res).astype(np.float32))
        np.testing.assert_array_equal(np.asarray(path.y()), ref.cell_to_world(first[:, 1], origin[1], res).astype(np.float32))
        assert fe.solution is None and fe._planner.get_solution() is None
    # the host array and its metadata are the same query; a fully known map has no frontier and no path
    fe = GridPlanner(robot)
    again = fe.find_frontiers(rx, ry, map=occ, map_meta_data=wm.map_meta_data, min_size=3, min_distance=0.5)
    assert again == found
    known = np.where(occ == U, 0, occ)
    assert fe.explore(rx, ry, map=known, map_meta_data=wm.map_meta_data) is None and fe.status == fref.NO_FRONTIER
    assert fe.find_frontiers(-50.0, 0.0) == [] and fe.status == ref.START_OUTSIDE
    # what is not combined, and why
    box = _robot_box()
    with pytest.raises(ValueError, match="oriented"):
        GridPlanner(box, footprint="oriented").find_frontiers(rx, ry, map=wm)
    with pytest.raises(ValueError, match="clearance"):
        GridPlanner(robot, clearance_reach=0.3, clearance_weight=2.0).explore(rx, ry, map=wm)
    with pytest.raises(ValueError):
        fe.find_frontiers(rx, ry, min_size=0)
    # kompass_cpp directly
    p = kompass_cpp.planning.GridPlanner(kompass_cpp.types.RobotGeometry.CYLINDER, [radius, 0.4])
    p.set_space_bounds_from_map(origin[0], origin[1], 160, 120, res)
    p.set_grid(occ)
    assert p.explore(rx, ry, 0.5, 3) and p.get_components() == want["components"]
    assert [d["entry_cell"] for d in p.get_frontiers()] == [r["entry"] for r in want["frontiers"]]
    np.testing.assert_array_equal(p.get_frontier_path_cells(0), want["paths"][0])
    assert p.get_solution() is None and len(p.get_path_cells()) == 0
    with pytest.raises(IndexError):
        p.explore(rx, ry, 0.0, 0)


def test_an_explore_leaves_the_set_up_problem_alone():
    """setup_problem, find_frontiers from another cell (and from outside the map), then solve() and replan(): the path,
    status, cost and cells of a fresh planner's solve of the problem that was set up, not a plan from the robot's
    position.  With new metadata given to find_frontiers the problem's cells are those of the new bounds."""
    import kompass_cpp
    from kompass_core.planning import GridPlanner
    from test_planner_gpu import _robot

    grid = ragged((129, 67), 0.03, 4)
    res = 0.05
    meta = dict(origin_x=-1.0, origin_y=2.0, width=129, height=67, resolution=res)
    r2 = ref.radius_to_r2(0.1, res)
    valid = ref.validity(grid, r2, True) & fref.explore_validity(grid, r2)
    seed = tuple(int(v) for v in np.argwhere(valid)[0])
    reach = ref.cost_field(fref.explore_validity(grid, r2), seed)
    far = tuple(int(v) for v in np.unravel_index(np.argmax(np.where(reach == INF, 0, reach)), reach.shape))
    mid = tuple(int(v) for v in np.argwhere((reach > reach[far] // 2) & (reach != INF))[0])
    xy = lambda c, m=meta: (float(ref.cell_to_world(c[0], m["origin_x"], res)) + 0.01,       # noqa: E731
                            float(ref.cell_to_world(c[1], m["origin_y"], res)) + 0.01)
    (sx, sy), (gx, gy), (rx, ry) = xy(far), xy(seed), xy(mid)

    def fresh(m=meta):
        p = GridPlanner(_robot())
        p.setup_problem(m, sx, sy, 0.0, gx, gy, 0.0, grid=grid)
        path = p.solve()
        return p, path

    want, wpath = fresh()
    assert wpath is not None and want._planner.get_cells() == (far, seed)
    fe = GridPlanner(_robot())
    fe.setup_problem(meta, sx, sy, 0.0, gx, gy, 0.0, grid=grid)
    for robot_xy, solve in [((rx, ry), fe.solve), ((rx, ry), fe.replan), ((-99.0, -99.0), fe.solve)]:
        fe.find_frontiers(robot_xy[0], robot_xy[1], min_size=1)
        assert fe._planner.get_cells() == (far, seed)
        path = solve()
        assert path is not None and fe.status == want.status == ref.FOUND and fe.get_cost() == want.get_cost()
        np.testing.assert_array_equal(fe.path_cells, want.path_cells)
        np.testing.assert_array_equal(np.asarray(path.x()), np.asarray(wpath.x()))
        assert not fe.replanned
    # the same through kompass_cpp
    p = kompass_cpp.planning.GridPlanner(kompass_cpp.types.RobotGeometry.CYLINDER, [0.1, 0.4])
    p.set_space_bounds_from_map(meta["origin_x"], meta["origin_y"], 129, 67, res)
    p.set_grid(grid)
    p.setup_problem(sx, sy, 0.0, gx, gy, 0.0)
    p.explore(rx, ry, 0.0, 1)
    assert p.get_cells() == (far, seed) and p.solve()
    np.testing.assert_array_equal(p.get_path_cells(), want.path_cells)
    # metadata given to find_frontiers: the bounds move by ten cells, and so do the problem's cells
    moved = dict(meta, origin_x=meta["origin_x"] - 10 * res, origin_y=meta["origin_y"] - 10 * res)
    fe.find_frontiers(rx, ry, map=grid, map_meta_data=moved, min_size=1)
    other, _ = fresh(moved)
    assert fe._planner.get_cells() == other._planner.get_cells() != (far, seed)
    fe.solve()
    assert fe.status == other.status and fe.get_cost() == other.get_cost()
    np.testing.assert_array_equal(fe.path_cells, other.path_cells)


def _robot_box():
    from kompass_core.models import Robot, RobotGeometry, RobotType
    return Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.BOX, geometry_params=np.array([0.6, 0.2, 0.3]))


def test_torch_device_array_in_a_fresh_process():
    """A torch tensor on the device as the map, torch imported first: _torch_frontier_worker.py."""
    worker = Path(__file__).resolve().parent / "_torch_frontier_worker.py"
    p = subprocess.run([sys.executable, str(worker)], capture_output=True, text=True, timeout=TIME_LIMIT_S - 30)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]
