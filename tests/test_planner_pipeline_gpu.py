"""The grid planner's host pipeline on the MI355X ("Host flow of a solve"): the one pass loop through
more than one batch of kPlanBatch = 8 passes, in the oriented mode and in the disc mode with the clearance cost on,
and the invalidation ladder: one context through every call that forgets something, against a fresh context a step.

Every grid is at most 130 cells a side.  Every test runs under the time limit of test_planner_gpu.py, for its reason:
a solve that went wrong would run to its pass cap, and only the thread method ends a native call."""

import numpy as np
import pytest

TIME_LIMIT_S = 120

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(TIME_LIMIT_S, method="thread")]

import kompass_hip as kh  # noqa: E402
import planner_clearance_ref as cref  # noqa: E402
import planner_oriented_ref as oref  # noqa: E402
import planner_ref as ref  # noqa: E402
from test_planner_clearance_gpu import compare as compare_clearance  # noqa: E402
from test_planner_oriented_gpu import SMALL, compare as compare_oriented  # noqa: E402

TILE, BATCH = 64, 8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert kh.device_count() >= 1, "no HIP device visible"


@pytest.fixture()
def ctx():
    c = kh.PlannerContext()
    yield c
    c.close()


def fresh(*steps):
    """What the last of `steps` (functions of a context) returns on a context of its own, which is closed."""
    with kh.PlannerContext() as c:
        for step in steps:
            out = step(c)
    return out


# ---- more than one batch -------------------------------------------------------------------------------------------
def serpentine_scene():
    """130 x 130: walls one cell thick over the full height every 12 cells, a 12-cell gap at the top of the even ones
    and at the bottom of the odd ones; 11 lanes of 11 (the last of 10) free cells: (grid, start, goal)."""
    g = np.zeros((130, 130), np.int32)
    for k, i in enumerate(range(11, 130, 12)):
        g[i, :] = ref.OCCUPIED
        if k % 2 == 0:
            g[i, 118:] = 0
        else:
            g[i, :12] = 0
    return g, (5, 5), (125, 124)


def tile_crossings(cells):
    """How often a path steps from one 64-cell tile into another."""
    t = np.asarray(cells) // TILE
    return int(np.any(t[1:] != t[:-1], axis=1).sum())


def test_oriented_solve_through_more_than_one_batch(ctx):
    grid, start, goal = serpentine_scene()
    ctx.set_grid(grid)
    ctx.set_oriented(*SMALL, 10)
    want = compare_oriented(ctx, grid, start, 0, goal, *SMALL, 10)
    # a pass carries a value across one tile border at the most: the field at the start is final after more passes
    # than the path has crossings
    assert want["status"] == ref.FOUND and tile_crossings(want["cells"]) >= BATCH + 1
    passes = ctx.solve_oriented(start, 0, goal)[2]
    assert passes > BATCH
    assert fresh(lambda c: c.set_grid(grid), lambda c: c.set_oriented(*SMALL, 10), lambda c: c.solve_oriented(start, 0, goal))[2] == passes


def test_clearance_solve_through_more_than_one_batch(ctx):
    grid, start, goal = serpentine_scene()
    r2, c2, wt = 4, 25, 40
    table = cref.clearance_table(wt, r2, c2)
    want = cref.plan(grid, start, goal, r2, c2, wt)
    assert want["status"] == ref.FOUND and tile_crossings(want["cells"]) >= BATCH + 1
    ctx.set_grid(grid)
    ctx.set_clearance_cost(c2, table)
    assert compare_clearance(ctx, grid, [(start, goal)], r2, c2, table, maps=(want["valid"], want["clear2"])) == [ref.FOUND]
    np.testing.assert_array_equal(ctx.path(), want["cells"])
    passes = ctx.solve(start, goal, r2)[2]
    assert passes > BATCH
    assert fresh(lambda c: c.set_grid(grid), lambda c: c.set_clearance_cost(c2, table), lambda c: c.solve(start, goal, r2))[2] == passes


# ---- the ladder ----------------------------------------------------------------------------------------------------
R2, SPAN = 1, 32
START, MOVED, GOAL = (3, 3), (6, 9), (36, 30)
C2 = 16
TABLE = cref.clearance_table(40, R2, C2)


def ladder_grids():
    """A: 70 x 66 with two walls to go round; B: A with a 3 x 3 patch at the first wall's end, where every path of A
    turns; C: 40 x 40 with a block."""
    a = np.zeros((70, 66), np.int32)
    a[20, :41] = ref.OCCUPIED
    a[30, 20:] = ref.OCCUPIED
    b = a.copy()
    b[19:22, 42:45] = ref.OCCUPIED
    c = np.zeros((40, 40), np.int32)
    c[10:20, 10:30] = ref.OCCUPIED
    return a, b, c


def read(c, res, walk=True):
    """Everything the ABI hands out behind a step that returned `res`; a refused call gives its error code and text.
    walk = False leaves out the calls that would run the walk."""
    calls = dict(field=c.field, clearance=c.clearance, oriented_field=c.oriented_field, replan_info=c.replan_info,
                 shortcut=lambda: kh._fill(kh.lib().kc_planner_get_shortcut, c.h, [(np.int32, (2,)), (np.int32, ())]))
    if walk:
        calls.update(path=c.path, path_clearance=c.path_clearance, states=c.oriented_path)
    out = dict(res=res)
    for name, call in calls.items():
        try:
            out[name] = call()
        except (kh.KompassHipError, ValueError, IndexError) as e:
            out[name] = f"{type(e).__name__}: {e}"
    return out


def same(got, want):
    assert got.keys() == want.keys()
    for key in got:
        a, b = got[key], want[key]
        if isinstance(a, str) or isinstance(b, str) or key in ("res", "replan_info"):
            assert a == b, (key, a, b)
        elif isinstance(a, (tuple, list)):
            assert len(a) == len(b), key
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y, err_msg=key)
        else:
            np.testing.assert_array_equal(a, b, err_msg=key)


def test_ladder_every_step_as_on_a_fresh_context(ctx):
    A, B, Cg = ladder_grids()
    grid = lambda g: (lambda c: c.set_grid(g))                       # noqa: E731
    solve = lambda c: c.solve(START, GOAL, R2)                       # noqa: E731
    cost_on = lambda c: c.set_clearance_cost(C2, TABLE)              # noqa: E731
    box_on = lambda c: c.set_oriented(*SMALL, 10)                    # noqa: E731
    solve_box = lambda c: c.solve_oriented(START, 0, GOAL)           # noqa: E731
    refused = "KompassHipError: [kc "

    # 1. solve A, walk, shortcut
    ctx.set_grid(A)
    res = ctx.solve(START, GOAL, R2)
    assert res[0] == kh.PLAN_FOUND
    ctx.path()
    assert len(ctx.shortcut(SPAN)[1]) >= 3
    got = read(ctx, res)
    same(got, fresh(grid(A), lambda c: read(c, (solve(c), c.path(), c.shortcut(SPAN))[0])))
    assert got["replan_info"] == (False, kh.PLAN_INF, 0, 0) and not isinstance(got["shortcut"], str)

    # 2. a new grid of the same shape keeps the field and nothing else: the replan rolls back, no walk, no shortcut
    ctx.set_grid(B)
    res = ctx.replan(START, GOAL, R2)
    got = read(ctx, res, walk=False)
    same(got, fresh(grid(A), solve, grid(B), lambda c: read(c, c.replan(START, GOAL, R2), walk=False)))
    kept, T, touched, tiles = got["replan_info"]
    assert kept and T != kh.PLAN_INF and touched > 0 and tiles > 0 and got["shortcut"].startswith(refused)
    plain = fresh(grid(B), lambda c: read(c, solve(c)))
    assert res[:2] == plain["res"][:2] and res[0] == kh.PLAN_FOUND
    same(dict(f=got["field"]), dict(f=plain["field"]))

    # 3. the shortcut without a walk call runs the walk of the new field
    short = ctx.shortcut(SPAN)
    got = read(ctx, res[:2])
    want = fresh(grid(B), lambda c: (solve(c), c.shortcut(SPAN))[1])
    same(dict(s=short), dict(s=want))
    for key in ("field", "path", "shortcut", "path_clearance", "states"):
        same({key: got[key]}, {key: plain[key] if key != "shortcut" else want[:2]})

    # 4. a clearance cost drops the kept field: the replan falls back to the solve; walk
    ctx.set_clearance_cost(C2, TABLE)
    res = ctx.replan(START, GOAL, R2)
    got = read(ctx, res)
    same(got, fresh(grid(B), cost_on, lambda c: read(c, solve(c))))
    assert res[0] == kh.PLAN_FOUND and got["replan_info"] == (False, kh.PLAN_INF, 0, 0) and got["shortcut"].startswith(refused)
    assert not isinstance(got["clearance"], str) and isinstance(got["path_clearance"], int)

    # 5. cost off, the oriented footprint on, an oriented solve and its states
    ctx.set_clearance_cost(0)
    ctx.set_oriented(*SMALL, 10)
    res = ctx.solve_oriented(START, 0, GOAL)
    boxed = read(ctx, res)
    same(boxed, fresh(grid(B), box_on, lambda c: read(c, solve_box(c))))
    assert res[0] == kh.PLAN_FOUND and len(boxed["states"]) >= len(boxed["path"]) > 0
    # 6. no shortcut of a state walk, kept or new
    assert boxed["shortcut"].startswith(refused) and boxed["field"].startswith(refused) and boxed["clearance"].startswith(refused)
    with pytest.raises(kh.KompassHipError, match="any-angle"):
        ctx.shortcut(SPAN)

    # 7. the same box again keeps the masks: the same result
    ctx.set_oriented(*SMALL, 10)
    assert read(ctx, None, walk=False)["oriented_field"].startswith(refused)     # the solve is forgotten all the same
    same(read(ctx, ctx.solve_oriented(START, 0, GOAL)), boxed)

    # 8. the footprint off: the kept field went with it, the replan falls back; then only the start moves
    ctx.set_oriented(0)
    res = ctx.replan(START, GOAL, R2)
    got = read(ctx, res)
    same(got, plain)
    assert got["replan_info"] == (False, kh.PLAN_INF, 0, 0) and got["oriented_field"].startswith(refused)
    res = ctx.replan(MOVED, GOAL, R2)
    got = read(ctx, res)
    same(got, fresh(grid(B), solve, lambda c: read(c, c.replan(MOVED, GOAL, R2))))
    assert res[0] == kh.PLAN_FOUND and res[2] == 0 and got["replan_info"] == (True, kh.PLAN_INF, 0, 0)
    same(dict(f=got["field"]), dict(f=plain["field"]))

    # 9. a grid of another shape drops the kept field
    ctx.set_grid(Cg)
    res = ctx.replan(MOVED, GOAL, R2)
    got = read(ctx, res, walk=False)
    small = fresh(grid(Cg), lambda c: read(c, c.solve(MOVED, GOAL, R2), walk=False))
    same(got, small)
    assert res[0] == kh.PLAN_FOUND and got["replan_info"] == (False, kh.PLAN_INF, 0, 0)

    # 10. the path twice: the second from the kept walk
    first, second = ctx.path(), ctx.path()
    np.testing.assert_array_equal(first, second)
    np.testing.assert_array_equal(first, fresh(grid(Cg), lambda c: (c.solve(MOVED, GOAL, R2), c.path())[1]))
    ref.check_path(ref.validity(Cg, R2), first, MOVED, GOAL)
