"""The clearance rules of the grid planner (rules 6 to 8) as tests/planner_clearance_ref.py states
them, against planner_ref.py where the two must agree, on the doorway scene, and the host class's integer penalty
table against the statement's.  No GPU needed."""
import numpy as np
import pytest

import planner_clearance_ref as cref
import planner_ref as ref


def clutter(shape, density, seed):
    rng = np.random.default_rng(seed)
    grid = np.where(rng.random(shape) < density, 100, 0).astype(np.int32)
    grid[rng.random(shape) < 0.05] = -1
    return grid


@pytest.mark.parametrize("r2", [0, 1, 5, 9])
def test_clearance_within_the_footprint_is_invalidity(r2):
    for unknown in (True, False):
        grid = clutter((60, 45), 0.06, 17 + r2)
        for c2 in (r2, r2 + 7, 40):
            c = cref.clearance2(grid, c2, unknown)
            np.testing.assert_array_equal(c <= r2, ~ref.validity(grid, r2, unknown))
            assert ((c == 0) == ref.blocking(grid, unknown)).all()
            assert ((c <= c2) | (c == cref.CLEAR_FAR)).all()


def test_clearance_by_hand():
    g = np.zeros((9, 7), np.int32)
    g[0, 0] = 100
    c = cref.clearance2(g, 25)
    assert c[0, 0] == 0 and c[3, 4] == 25 and c[5, 0] == 25 and c[4, 4] == cref.CLEAR_FAR and c[8, 6] == cref.CLEAR_FAR
    g[8, 6] = -1
    assert cref.clearance2(g, 25)[8, 6] == cref.CLEAR_FAR and cref.clearance2(g, 25, False)[8, 6] == 0
    assert cref.clearance2(g, 25, False)[7, 4] == 5
    # the table: zero inside the footprint, the weight at its edge falling to zero at the reach, truncated
    t = cref.clearance_table(40, 4, 100)
    assert len(t) == 101 and (t[:5] == 0).all() and t[5] == 40 * 95 // 96 and t[52] == 20 and t[99] == 0 and t[100] == 0
    pen = cref.penalty(np.array([[0, 5], [cref.CLEAR_FAR, 100]], np.uint16), t)
    assert pen.tolist() == [[0, 39], [0, 0]] and pen.dtype == np.uint32


def test_a_zero_table_gives_the_plain_field():
    grid = clutter((60, 45), 0.1, 5)
    for r2, goal in [(0, (3, 4)), (2, (50, 40))]:
        valid = ref.validity(grid, r2)
        goal = tuple(int(v) for v in np.argwhere(valid)[np.argmin(np.abs(np.argwhere(valid) - goal).sum(1))])
        pen = np.zeros(grid.shape, np.uint32)
        f = cref.cost_field(valid, pen, goal)
        np.testing.assert_array_equal(f, ref.cost_field(valid, goal))
        far = np.unravel_index(np.argmax(np.where(f == ref.INF, 0, f)), f.shape)
        cells = cref.walk(valid, f, pen, far)
        ref.check_path(valid, cells, far, goal)
        assert cref.path_length(cells) == cref.path_cost(cells, pen) == f[far]   # rule 8 realises the field


def test_path_cost_sum_is_the_field_at_the_start():
    grid = clutter((60, 45), 0.04, 9)
    for r2, c2, wt in [(0, 9, 10), (1, 36, 25), (4, 100, 3000), (5, 5, 40)]:
        valid = ref.validity(grid, r2)
        pen = cref.penalty(cref.clearance2(grid, c2), cref.clearance_table(wt, r2, c2))
        goal = tuple(int(v) for v in np.argwhere(valid)[0])
        f = cref.cost_field(valid, pen, goal)
        assert f[goal] == 0
        reached = np.argwhere((f != ref.INF) & valid)
        for k in (len(reached) // 3, len(reached) - 1):
            start = tuple(int(v) for v in reached[k])
            cells = cref.walk(valid, f, pen, start)
            ref.check_path(valid, cells, start, goal)
            assert cref.path_cost(cells, pen) == f[start]
            assert cref.path_length(cells) <= f[start]
            assert len(cells) <= f[start] // 10 + 2


def test_class_table_is_the_statements():
    import kompass_cpp

    table = kompass_cpp.planning.GridPlanner.clearance_table
    cases = [(40, 4, 100), (25, 1, 36), (10, 0, 9), (40, 5, 5), (3000, 4, 100), (7, 9, 4), (1, 0, 1), (40, 0, 0),
             (123, 16, 64516), (0xFFFFFFFF, 3, 64516),     # the cap of the reach; a product that needs 64 bits
             (4_000_000_000, 64515, 64516)]
    for wt, r2, c2 in cases:
        got = np.asarray(table(wt, r2, c2))
        want = cref.clearance_table(wt, r2, c2)
        np.testing.assert_array_equal(got.astype(np.uint64), want.astype(np.uint64))
    assert (np.asarray(table(40, 5, 5)) == 0).all() and len(table(40, 5, 5)) == 6
    with pytest.raises(IndexError):
        table(1, 0, 64517)
    cls = kompass_cpp.planning.GridPlanner
    for name in ("set_clearance_cost", "get_clearance", "get_path_min_clearance", "get_path_length"):
        assert hasattr(cls, name), name


def test_clearance_is_present_in_the_abi_and_the_front_end():
    import inspect

    import kompass_hip as kh
    from kompass_core.planning import GridPlanner

    L = kh.lib()
    for name in ("kc_planner_set_clearance_cost", "kc_planner_get_clearance", "kc_planner_path_clearance"):
        assert hasattr(L, name) and name in kh.SIGNATURES, name
    for name in ("set_clearance_cost", "clearance", "path_clearance"):
        assert hasattr(kh.PlannerContext, name), name
    assert kh.PLAN_CLEAR_FAR == cref.CLEAR_FAR
    par = inspect.signature(GridPlanner.__init__).parameters
    assert par["clearance_reach"].default == 0.0 and par["clearance_weight"].default == 0.0   # off by default
    for name in ("set_clearance_cost", "min_clearance", "path_length", "clearance_field"):
        assert hasattr(GridPlanner, name), name


def test_doorway_scene():
    """96 x 80, a wall with a doorway and a block in front of it: the plain path comes within squared distance 8 of a
    blocking cell (footprint 4), the penalised one keeps 81."""
    grid, start, goal = cref.doorway_scene()
    r2, c2, wt = 4, 100, 40
    valid = ref.validity(grid, r2)
    clear2 = cref.clearance2(grid, c2)
    plain_field = ref.cost_field(valid, goal)
    plain = ref.walk(valid, plain_field, start)
    p = cref.plan(grid, start, goal, r2, c2, wt)
    assert p["status"] == ref.FOUND
    ref.check_path(valid, p["cells"], start, goal)
    assert p["min_clear2"] > cref.path_clearance(plain, clear2)
    assert (cref.path_clearance(plain, clear2), p["min_clear2"]) == (8, 81)
    assert (int(plain_field[start]), p["cost"], p["length"]) == (1138, 1524, 1418)
    assert cref.path_cost(p["cells"], p["pen"]) == p["cost"]
    assert p["length"] >= plain_field[start]   # no path is shorter than the shortest
