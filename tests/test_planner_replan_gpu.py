"""The grid planner's replan on the MI355X (kc_planner_replan / kc_planner_replan_info, kompass_cpp.planning,
kompass_core.planning; DESIGN.md 4.10 rules 19 and 20): after a solve, a changed grid and a replan, the field, the
validity map, the clearance maps, status, cost and path equal a fresh solve on a second context bit for bit, and the
CPU statement; the threshold and the touched cells equal tests/planner_replan_ref.py; the passes never exceed the
fresh solve's; nothing touched means no pass; whatever cannot be kept falls back to a full solve and says so.

Every test runs under the time limit of test_planner_gpu.py, for its reason: a solve that went wrong would run to
its pass cap, and only the thread method ends a native call."""
import ctypes

import numpy as np
import pytest

TIME_LIMIT_S = 120

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(TIME_LIMIT_S, method="thread")]

import kompass_cpp  # noqa: E402
import kompass_hip as kh  # noqa: E402
import planner_clearance_ref as cref  # noqa: E402
import planner_ref as ref  # noqa: E402
import planner_replan_ref as rref  # noqa: E402
from helpers import DeviceArray  # noqa: E402
from test_planner_replan_cpu import clutter, flip  # noqa: E402

INF = ref.INF
SHAPES = [(64, 64), (130, 97), (65, 300), (257, 63), (1, 90)]
C2, WEIGHT10 = 36, 25


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


def outputs(c, with_clearance):
    f, v = c.field()
    return (f, v, c.path()) + (c.clearance() if with_clearance else ())


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def statement(grid, goal, r2, unknown, table):
    """(valid, pen, field) of the CPU statement; pen is None without a clearance cost."""
    valid = ref.validity(grid, r2, unknown)
    if table is None:
        return valid, None, ref.cost_field(valid, goal)
    pen = cref.penalty(cref.clearance2(grid, C2, unknown), table)
    return valid, pen, cref.cost_field(valid, pen, goal)


def replan_and_check(ctx, other, old, grid_new, start, goal, r2, unknown, table, cpu=True):
    """`ctx` holds a finished solve for `goal` whose statement is old = (valid, pen, field).  Sets grid_new, replans,
    and compares with a fresh solve on `other`, with the statement and with rules 19 and 20.  -> (the new grid's
    statement or None, status, replan_info)."""
    ctx.set_grid(grid_new)
    st, cost, passes = ctx.replan(start, goal, r2, unknown)
    kept, T, touched, tiles = ctx.replan_info()
    other.set_grid(grid_new)
    fst, fcost, fpasses = other.solve(start, goal, r2, unknown)
    assert (st, cost) == (fst, fcost)
    got = outputs(ctx, table is not None)
    same(got, outputs(other, table is not None))
    assert 0 <= passes <= fpasses, (passes, fpasses)          # the pass bound: a condition, not a measurement
    assert kept
    w, h = grid_new.shape
    assert tiles <= -(-w // 64) * -(-h // 64)
    assert (passes == 0) == (tiles == 0) and (T != INF or tiles == 0)
    if st == ref.FOUND and table is not None:
        assert ctx.path_clearance() == other.path_clearance()
    if not cpu:
        return None, st, (kept, T, touched, tiles)
    new = statement(grid_new, goal, r2, unknown, table)
    np.testing.assert_array_equal(got[1], new[0])
    np.testing.assert_array_equal(got[0], new[2])
    assert st == ref.status(new[0], new[2], start, goal)
    if st == ref.FOUND:
        assert cost == new[2][start]
        want = ref.walk(new[0], new[2], start) if table is None else cref.walk(new[0], new[2], new[1], start)
        np.testing.assert_array_equal(got[2], want)
    else:
        assert cost == INF and len(got[2]) == 0
    t = rref.touched(old[0], new[0], old[1], new[1])
    assert touched == int(t.sum())
    assert T == rref.threshold(old[2], t)
    if T != INF:
        assert tiles == int(rref.active_tiles(rref.rollback(old[2], new[0], T, goal), new[0], goal).sum())
    return new, st, (kept, T, touched, tiles)


def solve_old(ctx, grid, start, goal, r2, unknown, table):
    """A finished solve of `grid` on ctx -> its statement, checked."""
    ctx.set_grid(grid)
    ctx.solve(start, goal, r2, unknown)
    old = statement(grid, goal, r2, unknown, table)
    f, v = ctx.field()
    np.testing.assert_array_equal(f, old[2])
    np.testing.assert_array_equal(v, old[0])
    return old


def pick_pair(ctx, grid, r2, unknown, rng):
    """(start, goal) from the device's own field: of three valid cells the goal that reaches farthest, the start the
    cell farthest from it.  None without a valid cell."""
    ctx.set_grid(grid)
    ctx.solve((0, 0), (0, 0), r2, unknown)
    valid = ctx.field()[1]
    idx = np.argwhere(valid)
    best = None
    for k in rng.integers(0, max(len(idx), 1), 3) if len(idx) else ():
        goal = tuple(int(v) for v in idx[k])
        ctx.solve(goal, goal, r2, unknown)
        f = ctx.field()[0]
        reach = np.where(f == INF, 0, f)
        far = tuple(int(v) for v in np.unravel_index(np.argmax(reach), reach.shape))
        if best is None or reach[far] > best[0]:
            best = (int(reach[far]), far, goal)
    return None if best is None else (best[1], best[2])


def ring(grid, centre, d):
    """The cells at Chebyshev distance d around `centre` occupied."""
    g = grid.copy()
    w, h = g.shape
    for i in range(centre[0] - d, centre[0] + d + 1):
        for j in range(centre[1] - d, centre[1] + d + 1):
            if 0 <= i < w and 0 <= j < h and max(abs(i - centre[0]), abs(j - centre[1])) == d:
                g[i, j] = 100
    return g


def toggle(g, i, j):
    g[i, j] = 0 if g[i, j] == 100 else 100


# ---- 1 and 2: bit-equality and the pass bound --------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("r2", [0, 5])
@pytest.mark.parametrize("clearance", [False, True])
@pytest.mark.parametrize("unknown", [True, False])
def test_bit_equality(ctx, other, shape, r2, clearance, unknown):
    rng = np.random.default_rng(hash((shape, r2, clearance, unknown)) % 2 ** 32)
    grid = clutter(shape, 0.03, rng.integers(2 ** 31))
    table = cref.clearance_table(WEIGHT10, r2, C2) if clearance else None
    for c in (ctx, other):
        c.set_clearance_cost(C2 if clearance else 0, table)
    pair = pick_pair(ctx, grid, r2, unknown, rng)
    assert pair is not None
    start, goal = pair
    old = solve_old(ctx, grid, start, goal, r2, unknown, table)
    path = ctx.path()
    w, h = shape
    flips = {}
    assert len(path) > 2, (start, goal)                         # a cell between start and goal: both cases below exist
    g = grid.copy()
    g[tuple(path[min(3, len(path) - 2)])] = 100                # on the old path near the start
    flips["on the path near the start"] = g
    g = grid.copy()
    g[tuple(path[-2])] = 100                                    # adjacent to the goal
    flips["beside the goal"] = g
    g = grid.copy()
    g[goal] = 100
    flips["the goal blocked"] = g
    g = grid.copy()
    if w > 64:
        for y in rng.integers(0, h, 2):
            toggle(g, 63, y), toggle(g, 64, h - 1 - y)
    if h > 64:
        for x in rng.integers(0, w, 2):
            toggle(g, x, 63), toggle(g, w - 1 - x, 64)
    if w > 64 or h > 64:
        flips["both sides of a tile edge"] = g
    flips["the start walled in"] = ring(grid, start, 4)        # farther than any footprint here: the start stays valid
    flips["1 to 40 each way"] = flip(grid, rng, int(rng.integers(1, 41)), int(rng.integers(1, 41)))
    seen = {}
    for name, g in flips.items():
        ctx.set_grid(grid)                                      # every flip set starts from the old grid's solve
        ctx.solve(start, goal, r2, unknown)
        _, st, info = replan_and_check(ctx, other, old, g, start, goal, r2, unknown, table)
        seen[name] = (st, info)
    st, (_, T, touched, tiles) = seen["the goal blocked"]
    assert st == ref.GOAL_INVALID and T == 0 and touched >= 1
    assert seen["beside the goal"][1][1] <= 10                 # the blocked cell's candidate is the goal's 0 + 10 at most


def test_goal_blocked_leaves_no_value(ctx, other):
    grid = clutter((130, 97), 0.03, 5)
    start, goal = pick_pair(ctx, grid, 0, True, np.random.default_rng(5))
    old = solve_old(ctx, grid, start, goal, 0, True, None)
    g = grid.copy()
    g[goal] = 100
    _, st, (kept, T, touched, tiles) = replan_and_check(ctx, other, old, g, start, goal, 0, True, None)
    assert st == ref.GOAL_INVALID and (ctx.field()[0] == INF).all() and T == 0 and touched == 1 and kept
    # the all-INF field of an invalid goal is not kept: the next replan is a full solve, and a right one
    ctx.set_grid(grid)
    assert ctx.replan(start, goal, 0, True)[0] == ref.FOUND and not ctx.replan_info()[0]
    other.set_grid(grid)
    other.solve(start, goal, 0, True)
    same(outputs(ctx, False), outputs(other, False))


def test_start_made_unreachable(ctx, other):
    grid = np.zeros((130, 97), np.int32)
    start, goal = (100, 50), (5, 5)
    old = solve_old(ctx, grid, start, goal, 5, True, None)
    _, st, (kept, T, touched, tiles) = replan_and_check(ctx, other, old, ring(grid, start, 6), start, goal, 5, True, None)
    assert st == ref.UNREACHABLE and kept and T < old[2][start] and tiles >= 1


def test_doorway_opened(ctx, other):
    """The doorway scene with its door first closed, then open: freed wall cells open a way where there was none."""
    grid, start, goal = cref.doorway_scene()
    closed = grid.copy()
    closed[48, 30:50] = 100
    for clearance in (False, True):
        table = cref.clearance_table(WEIGHT10, 4, C2) if clearance else None
        for c in (ctx, other):
            c.set_clearance_cost(C2 if clearance else 0, table)
        old = solve_old(ctx, closed, start, goal, 4, True, table)
        assert ctx.solve(start, goal, 4)[0] == ref.UNREACHABLE
        _, st, (kept, T, touched, tiles) = replan_and_check(ctx, other, old, grid, start, goal, 4, True, table)
        assert st == ref.FOUND and kept and T != INF and touched >= 20
        # and closed again
        new = statement(grid, goal, 4, True, table)
        _, st, _ = replan_and_check(ctx, other, new, closed, start, goal, 4, True, table)
        assert st == ref.UNREACHABLE


def test_freed_neighbour_allows_a_diagonal(ctx, other):
    """(41, 41) -> (40, 40) is a diagonal the blocked (41, 40) forbids; freeing it lowers old(41, 41) = 20 to 14 and
    T = old(40, 40) + 10 = 10 lies below both."""
    grid = np.zeros((70, 70), np.int32)
    grid[41, 40] = 100
    goal, start = (40, 40), (69, 69)
    old = solve_old(ctx, grid, start, goal, 0, True, None)
    assert old[2][41, 41] == 20
    _, st, (kept, T, touched, tiles) = replan_and_check(ctx, other, old, np.zeros((70, 70), np.int32), start, goal, 0, True, None)
    assert st == ref.FOUND and (T, touched) == (10, 1) and ctx.field()[0][41, 41] == 14


# ---- 3: nothing touched --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clearance", [False, True])
def test_nothing_touched(ctx, other, clearance):
    rng = np.random.default_rng(23)
    grid = clutter((130, 97), 0.03, 23)
    grid[20:25, 20:25] = 100                                    # a solid block: its centre may go without a trace
    r2 = 5
    table = cref.clearance_table(WEIGHT10, r2, C2) if clearance else None
    for c in (ctx, other):
        c.set_clearance_cost(C2 if clearance else 0, table)
    start, goal = pick_pair(ctx, grid, r2, True, rng)
    old = solve_old(ctx, grid, start, goal, r2, True, table)
    field = old[2]
    starts = [tuple(int(v) for v in c) for c in np.argwhere((field != INF) & (field > 0))[::97][:3]]
    # cells that stay valid (0 -> 50 wherever the cell is valid) and a cell that stays invalid (100 -> 90 in the middle of
    # the block: every cell of its disc is a blocking cell itself, and none outside the block has it as its nearest)
    twin = np.where(old[0] & (grid == 0), 50, grid).astype(np.int32)
    twin[22, 22] = 90
    assert (twin != grid).sum() > 1000
    for k, s in enumerate(starts):
        if k == 1:
            ctx.set_grid(grid)                                  # the same grid set again
        if k == 2:
            ctx.set_grid(twin)
        st, cost, passes = ctx.replan(s, goal, r2, True)
        kept, T, touched, tiles = ctx.replan_info()
        assert (st, cost, passes) == (ref.FOUND, field[s], 0) and kept and T == INF and (touched, tiles) == (0, 0)
        other.set_grid(twin if k == 2 else grid)
        assert other.solve(s, goal, r2, True)[:2] == (st, cost)
        same(outputs(ctx, clearance), outputs(other, clearance))
    np.testing.assert_array_equal(ref.validity(twin, r2), old[0])


# ---- 4: fall-backs -------------------------------------------------------------------------------------------------
def test_fall_backs(ctx, other):
    rng = np.random.default_rng(29)
    grid = clutter((130, 97), 0.03, 29)
    start, goal = pick_pair(ctx, grid, 1, True, rng)
    c = kh.PlannerContext()
    c.set_grid(grid)
    first = c.replan(start, goal, 1, True)                      # the first call of a context
    assert not c.replan_info()[0] and c.replan_info()[1:] == (INF, 0, 0)
    other.set_grid(grid)
    assert first == other.solve(start, goal, 1, True)
    same(outputs(c, False), outputs(other, False))
    c.close()
    table = cref.clearance_table(WEIGHT10, 1, C2)
    g2 = flip(grid, rng, 5, 5)
    cases = [dict(goal=start, start=goal), dict(r2=2), dict(unknown=False), dict(table=table), dict(table=table * 2, before=table),
             dict(shape=(97, 130))]
    for case in cases:
        ctx.set_clearance_cost(C2 if "before" in case else 0, case.get("before"))
        ctx.set_grid(grid)
        ctx.solve(start, goal, 1, True)
        if "table" in case:
            ctx.set_clearance_cost(C2, case["table"])
        other.set_clearance_cost(C2 if "table" in case else 0, case.get("table"))
        g = clutter(case["shape"], 0.03, 31) if "shape" in case else g2
        s, t = case.get("start", start), case.get("goal", goal)
        if "shape" in case:
            s, t = (s[1], s[0]), (t[1], t[0])
        args = (s, t, case.get("r2", 1), case.get("unknown", True))
        ctx.set_grid(g)
        got = ctx.replan(*args)
        assert not ctx.replan_info()[0], case
        other.set_grid(g)
        assert got == other.solve(*args), case
        same(outputs(ctx, "table" in case), outputs(other, "table" in case))
        # and the replan behind the fall-back keeps its field
        ctx.set_grid(g)
        assert ctx.replan(*args)[:2] == got[:2]
        assert ctx.replan_info()[0] == (got[0] not in (ref.GOAL_INVALID, ref.GOAL_OUTSIDE)), case
    # the context-level call has no start class: with the oriented footprint on it answers as kc_planner_solve does
    ctx.set_clearance_cost(0)
    ctx.set_oriented(9, 1, 10)
    with pytest.raises(kh.KompassHipError):
        ctx.replan(start, goal, 1, True)
    ctx.set_oriented(0)
    ctx.replan(start, goal, 1, True)
    assert not ctx.replan_info()[0]                             # switching the mode forgot the field


def test_oriented_mode_replans_in_full():
    G = kompass_cpp.types.RobotGeometry
    grid = np.zeros((72, 70), np.int32)
    grid[:, :30] = grid[:, 37:] = 100
    outs = []
    for call in ("solve", "replan"):
        p = kompass_cpp.planning.GridPlanner(G.BOX, [0.3, 0.1, 0.4])
        p.set_oriented_footprint(True, 1.0)
        p.set_space_bounds_from_map(0.0, 0.0, 72, 70, 0.05)
        p.set_grid(grid)
        p.setup_problem(0.26, 1.66, 0.0, 3.26, 1.66, 0.0)
        assert p.solve()
        g2 = grid.copy()
        g2[30, 36] = 100
        p.set_grid(g2)
        assert getattr(p, call)() and not p.replanned()
        outs.append((p.get_status(), p.get_cost(), p.get_passes(), p.get_path_states(), p.get_path_cells()) + p.get_oriented_field())
    assert outs[0][:3] == outs[1][:3]
    same(outs[0][3:], outs[1][3:])


# ---- 5: tile skipping ----------------------------------------------------------------------------------------------
def test_tiles_left_out(ctx, other):
    grid = clutter((257, 63), 0.03, 37)
    grid[:8, :8] = grid[-8:, -8:] = 0
    start, goal = (250, 58), (3, 3)
    old = solve_old(ctx, grid, start, goal, 0, True, None)
    assert old[2][start] != INF
    g = grid.copy()
    g[252, 57] = 100
    _, st, (kept, T, touched, tiles) = replan_and_check(ctx, other, old, g, start, goal, 0, True, None)
    assert st == ref.FOUND and kept and touched == 1 and 1 <= tiles < 5


# ---- 6: device-resident grids ----------------------------------------------------------------------------------------
def test_device_resident_grid(ctx, other):
    rng = np.random.default_rng(41)
    grid = clutter((130, 97), 0.03, 41)
    start, goal = pick_pair(ctx, grid, 1, True, rng)
    g2 = flip(grid, rng, 20, 20)
    old = solve_old(ctx, grid, start, goal, 1, True, None)
    _, st, info = replan_and_check(ctx, other, old, g2, start, goal, 1, True, None)
    host = (st, info) + outputs(ctx, False)
    for dtype in (np.int32, np.int8):
        a = np.asfortranarray(grid.astype(dtype))
        with DeviceArray(a) as buf:
            ctx.set_grid_device(buf.ptr, 130, 97, elem_bytes=a.itemsize)
            ctx.solve(start, goal, 1, True)
            b = np.asfortranarray(g2.astype(dtype))
            assert buf.hip.hipMemcpy(buf.p, b.ctypes.data_as(ctypes.c_void_p), b.nbytes, 1) == 0   # updated in place
            ctx.set_grid_device(buf.ptr, 130, 97, elem_bytes=a.itemsize)
            dst = ctx.replan(start, goal, 1, True)[0]
            dev = (dst, ctx.replan_info()) + outputs(ctx, False)
        assert dev[:2] == host[:2]
        same(dev[2:], host[2:])


# ---- 7: sequences ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clearance", [False, True])
def test_ten_replans_in_a_row(ctx, other, clearance):
    rng = np.random.default_rng(43)
    grid = clutter((130, 97), 0.03, 43)
    table = cref.clearance_table(WEIGHT10, 1, C2) if clearance else None
    for c in (ctx, other):
        c.set_clearance_cost(C2 if clearance else 0, table)
    start, goal = pick_pair(ctx, grid, 1, True, rng)
    ctx.set_grid(grid)
    ctx.solve(start, goal, 1, True)
    kept_count = 0
    for k in range(10):
        grid = flip(grid, rng, int(rng.integers(1, 15)), int(rng.integers(1, 15)))
        if k == 6 and len(ctx.path()):                          # and the robot moves on
            start = tuple(int(v) for v in ctx.path()[min(5, len(ctx.path()) - 1)])
        ctx.set_grid(grid)
        got = ctx.replan(start, goal, 1, True)
        kept_count += ctx.replan_info()[0]
        other.set_grid(grid)
        want = other.solve(start, goal, 1, True)
        assert got[:2] == want[:2] and got[2] <= want[2]
        same(outputs(ctx, clearance), outputs(other, clearance))
    assert kept_count >= 8                                      # a blocked goal is the one thing that drops the field
    # a solve after a replan is a solve
    assert ctx.solve(start, goal, 1, True) == want
    same(outputs(ctx, clearance), outputs(other, clearance))


# ---- 8: the class and the front end --------------------------------------------------------------------------------
RES, ORIGIN, DIMS = 0.05, (-1.0, 0.5), [0.1, 0.4]


def _doorway():
    grid, start, goal = cref.doorway_scene()
    closed = grid.copy()
    closed[48, 30:50] = 100
    xy = lambda c: (float(ref.cell_to_world(c[0], ORIGIN[0], RES)) + 0.01, float(ref.cell_to_world(c[1], ORIGIN[1], RES)) + 0.01)  # noqa: E731
    return closed, grid, xy(start), xy(goal), xy((8, 30))


def test_class_on_the_doorway_scene():
    closed, grid, s, t, s2 = _doorway()
    G = kompass_cpp.types.RobotGeometry

    def planner(g, start):
        p = kompass_cpp.planning.GridPlanner(G.CYLINDER, DIMS)
        p.set_clearance_cost(0.4, 4.0)
        p.set_space_bounds_from_map(ORIGIN[0], ORIGIN[1], 96, 80, RES)
        p.set_grid(g)
        p.setup_problem(start[0], start[1], 0.0, t[0], t[1], 0.0)
        return p

    p = planner(closed, s)
    assert not p.replan() and not p.replanned() and p.get_status() == ref.UNREACHABLE   # the first call: a full solve
    p.set_grid(grid)
    assert p.replan() and p.replanned() and p.get_replan_threshold() != INF and p.get_passes() >= 1
    q = planner(grid, s)
    assert q.solve() and not q.replanned() and q.get_replan_threshold() == INF

    def everything(x):
        cells, idx = x.get_any_angle_cells(64, True)
        path, anyp = x.get_solution(), x.get_any_angle_solution(64)
        return (x.get_path_cells(), np.asarray(path.x()), np.asarray(path.y()), cells, idx, np.asarray(anyp.x()),
                np.asarray(anyp.y()), np.float32(x.get_cost()), np.float32(x.get_path_length()),
                np.float32(x.get_path_min_clearance()), np.float32(x.get_any_angle_length(64)),
                np.float32(x.get_any_angle_min_clearance(64))) + x.get_field() + x.get_clearance()

    same(everything(p), everything(q))
    assert np.float32(p.get_cost()) == ref.cost_in_metres(1524, RES)
    assert p.get_passes() <= q.get_passes()
    # the robot has moved: a new start alone, no pass
    p.setup_problem(s2[0], s2[1], 0.0, t[0], t[1], 0.0)
    assert p.replan() and p.replanned() and p.get_passes() == 0 and p.get_replan_threshold() == INF
    q.setup_problem(s2[0], s2[1], 0.0, t[0], t[1], 0.0)
    assert q.solve()
    same(everything(p), everything(q))
    # another goal: a full solve
    p.setup_problem(s2[0], s2[1], 0.0, s[0], s[1], 0.0)
    assert p.replan() and not p.replanned()


def test_front_end_on_the_doorway_scene():
    from kompass_core.planning import GridPlanner
    from test_planner_gpu import _robot

    closed, grid, s, t, s2 = _doorway()
    meta = dict(origin_x=ORIGIN[0], origin_y=ORIGIN[1], width=96, height=80, resolution=RES)
    for any_angle in (False, True):
        fe = GridPlanner(_robot(tuple(DIMS)), any_angle=any_angle, max_span=64)
        with pytest.raises(RuntimeError):
            fe.replan()
        fe.setup_problem(meta, s[0], s[1], 0.0, t[0], t[1], 0.0, grid=closed)
        assert fe.solve() is None and not fe.replanned
        path = fe.replan(map=grid, start=s2)
        assert path is not None and fe.replanned and fe.status == ref.FOUND
        want = GridPlanner(_robot(tuple(DIMS)), any_angle=any_angle, max_span=64)
        want.setup_problem(meta, s2[0], s2[1], 0.0, t[0], t[1], 0.0, grid=grid)
        wpath = want.solve()
        np.testing.assert_array_equal(fe.path_cells, want.path_cells)
        np.testing.assert_array_equal(np.asarray(path.x()), np.asarray(wpath.x()))
        np.testing.assert_array_equal(np.asarray(path.y()), np.asarray(wpath.y()))
        assert fe.get_cost() == want.get_cost() and fe.passes <= want.passes
        # only the start, then only the map
        assert fe.replan(start=s) is not None and fe.replanned and fe.passes == 0
        assert fe.replan(map=closed) is None and fe.replanned and fe.status == ref.UNREACHABLE
