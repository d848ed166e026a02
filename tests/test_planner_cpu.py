"""The grid planner's CPU statement (tests/planner_ref.py) on cases worked out by hand, and the
presence of the planner in every layer.  No GPU needed."""
import numpy as np
import pytest

import planner_ref as ref

INF = ref.INF


def test_empty_grid_is_the_octile_distance():
    for (w, h), goal in [((7, 5), (0, 0)), ((9, 13), (4, 6)), ((1, 6), (0, 5)), ((70, 3), (69, 1))]:
        valid = np.ones((w, h), bool)
        f = ref.cost_field(valid, goal)
        np.testing.assert_array_equal(f, ref.octile(w, h, goal))
    f = ref.cost_field(np.ones((4, 4), bool), (0, 0))
    assert f[3, 3] == 42 and f[3, 0] == 30 and f[3, 1] == 34 and f[0, 0] == 0


def test_wall_with_one_gap():
    # a wall along i = 3 of a 7 x 7 grid, open only at j = 5; goal (0, 0), start (6, 0)
    g = np.zeros((7, 7), np.int32)
    g[3, :] = 100
    g[3, 5] = 0
    valid = ref.validity(g, 0)
    assert not valid[3, 0] and valid[3, 5] and valid.sum() == 49 - 6
    f = ref.cost_field(valid, (0, 0))
    # to the gap: (0,0) -> (2,2) two diagonals, (2,3), (2,4) wait for the wall: the gap (3,5) may only be entered
    # straight from (2,5), its diagonal neighbours sit beside wall cells
    assert f[2, 5] == 14 * 2 + 10 * 3
    assert f[3, 5] == f[2, 5] + 10 and f[4, 5] == f[3, 5] + 10
    assert f[6, 0] == f[4, 5] + 14 * 2 + 10 * 3
    assert (f[3, [0, 1, 2, 3, 4, 6]] == INF).all()
    cells = ref.walk(valid, f, (6, 0))
    ref.check_path(valid, cells, (6, 0), (0, 0))
    assert [3, 5] in cells.tolist() and [2, 5] in cells.tolist() and [4, 5] in cells.tolist()
    # close the gap: the far side is out of reach
    g[3, 5] = 100
    valid = ref.validity(g, 0)
    f = ref.cost_field(valid, (0, 0))
    assert (f[4:, :] == INF).all() and (f[:3, :] != INF).all()
    assert ref.status(valid, f, (6, 0), (0, 0)) == ref.UNREACHABLE


def test_corner_cutting_rule():
    # one occupied cell at (1, 1): (0, 1) -> (1, 2) and (1, 0) -> (2, 1) ... may not pass its corner
    g = np.zeros((3, 3), np.int32)
    g[1, 1] = 100
    valid = ref.validity(g, 0)
    f = ref.cost_field(valid, (0, 0))
    assert f[1, 0] == 10 and f[2, 0] == 20 and f[2, 1] == 30 and f[2, 2] == 40 and f[1, 2] == 30 and f[0, 2] == 20
    m = ref.move_masks(valid)
    assert m[1, 0] == 0b00000101  # E and W only: N is the obstacle, NE / NW pass its corners
    assert m[1, 1] == 0
    # two obstacles touching by a corner close the diagonal between them altogether
    g = np.zeros((2, 2), np.int32)
    g[0, 1] = g[1, 0] = 100
    valid = ref.validity(g, 0)
    assert (ref.cost_field(valid, (0, 0)) == np.array([[0, INF], [INF, INF]], np.uint32)).all()
    # and a free diagonal costs 14
    assert ref.cost_field(np.ones((2, 2), bool), (0, 0))[1, 1] == 14


def test_blocked_goal_and_unreachable_start():
    g = np.zeros((5, 5), np.int32)
    g[4, 4] = 100
    valid = ref.validity(g, 0)
    f = ref.cost_field(valid, (4, 4))
    assert (f == INF).all()
    assert ref.status(valid, f, (0, 0), (4, 4)) == ref.GOAL_INVALID
    assert ref.status(valid, f, (4, 4), (0, 0)) == ref.START_INVALID
    assert ref.status(valid, f, (5, 0), (0, 0)) == ref.START_OUTSIDE
    assert ref.status(valid, f, (0, 0), (0, -1)) == ref.GOAL_OUTSIDE
    out = ref.plan(g, (0.0, 0.0), 1.0, (0.2, 0.2), (4.1, 4.3), 0.0)
    assert out["status"] == ref.GOAL_INVALID and out["cells"] is None and out["cost"] is None
    # a ring around the start
    g = np.zeros((7, 7), np.int32)
    g[2:5, 2] = g[2:5, 4] = g[2, 2:5] = g[4, 2:5] = 100
    valid = ref.validity(g, 0)
    f = ref.cost_field(valid, (0, 0))
    assert valid[3, 3] and f[3, 3] == INF
    assert ref.status(valid, f, (3, 3), (0, 0)) == ref.UNREACHABLE


def test_allow_unknown_both_ways():
    g = np.zeros((5, 3), np.int32)
    g[2, :] = -1
    open_ = ref.validity(g, 0, allow_unknown=True)
    shut = ref.validity(g, 0, allow_unknown=False)
    assert open_.all() and not shut[2].any() and shut[[0, 1, 3, 4]].all()
    assert ref.cost_field(open_, (0, 1))[4, 1] == 40
    assert ref.cost_field(shut, (0, 1))[4, 1] == INF
    # other values are free cells
    g[:] = 37
    assert ref.validity(g, 4, allow_unknown=False).all()


def test_footprint_radius_zero_and_one_cell():
    g = np.zeros((7, 7), np.int32)
    g[3, 3] = 100
    v0 = ref.validity(g, ref.radius_to_r2(0.0, 0.05))
    assert (~v0).sum() == 1 and not v0[3, 3]
    v1 = ref.validity(g, ref.radius_to_r2(0.05, 0.05))
    assert ref.radius_to_r2(0.05, 0.05) == 1
    assert sorted(map(tuple, np.argwhere(~v1))) == [(2, 3), (3, 2), (3, 3), (3, 4), (4, 3)]
    v2 = ref.validity(g, 2)  # the diagonal neighbours come in at R2 = 2
    assert (~v2).sum() == 9
    # a blocker at the rim: cells outside the grid do not block, and nothing wraps around
    g = np.zeros((4, 4), np.int32)
    g[0, 0] = 100
    v = ref.validity(g, 4)
    assert sorted(map(tuple, np.argwhere(~v))) == [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0)]


def test_radius_rule():
    assert ref.radius_to_r2(0.3, 0.05) == 36  # 0.3f / 0.05f is 5.99999998: still six cells
    assert ref.radius_to_r2(0.0, 0.1) == 0
    assert ref.radius_to_r2(0.26, 0.1) == 6
    assert ref.radius_to_r2(1.0, 0.25) == 16
    assert ref.footprint_radius(ref.CYLINDER, [0.2, 0.4]) == float(np.float32(0.2))
    assert ref.footprint_radius(ref.SPHERE, [0.25]) == 0.25
    assert abs(ref.footprint_radius(ref.BOX, [0.4, 0.3, 0.5]) - 0.25) < 1e-7


def test_walk_order_simplify_and_frames():
    valid = np.ones((5, 5), bool)
    f = ref.cost_field(valid, (4, 2))
    cells = ref.walk(valid, f, (0, 0))
    # (1, 1) holds 34 and is the one smallest neighbour of the start; from (2, 2) on the row is the only descent
    assert cells.tolist() == [[0, 0], [1, 1], [2, 2], [3, 2], [4, 2]]
    assert ref.simplify(cells).tolist() == [[0, 0], [2, 2], [4, 2]]
    # a tie: from (1, 0) towards the goal (0, 1), E (2, 0) is worse, N (1, 1) = 10 and W (0, 0) = 10 tie, NW (0, 1)
    # = 0 is the minimum
    f = ref.cost_field(valid, (0, 1))
    assert ref.walk(valid, f, (1, 0)).tolist() == [[1, 0], [0, 1]]
    # equal values: the first in E, N, W, S, NE, NW, SW, SE wins
    f = ref.cost_field(valid, (2, 2))
    assert f[1, 0] == f[0, 1] == 24
    assert ref.walk(valid, f, (0, 0)).tolist()[1] == [1, 1]
    f2 = np.where(valid, np.uint32(20), np.uint32(0)).astype(np.uint32)
    f2[2, 2] = 30
    f2[3, 2] = f2[2, 3] = f2[1, 1] = 0
    assert ref.walk(valid, f2, (2, 2)).tolist() == [[2, 2], [3, 2]]
    # frames: truncation towards zero as localToGrid, the inverse without a half-cell shift
    assert ref.world_to_cell(1.26, 1.0, 0.05) == 5 and ref.world_to_cell(0.99, 1.0, 0.05) == 0
    assert ref.world_to_cell(0.94, 1.0, 0.05) == -1 and ref.world_to_cell(float("nan"), 0.0, 0.05) is None
    assert ref.cell_to_world(5, 1.0, 0.05) == np.float32(1.0) + np.float32(5) * np.float32(0.05)
    assert ref.cost_in_metres(42, 0.5) == np.float32(2.1)
    out = ref.plan(np.zeros((5, 5), np.int32), (1.0, -1.0), 0.5, (1.1, -0.9), (3.2, 0.1), 0.0, do_simplify=True)
    assert out["status"] == ref.FOUND and out["start"] == (0, 0) and out["goal"] == (4, 2)
    np.testing.assert_array_equal(out["points"], np.float32([[1.0, -1.0], [2.0, 0.0], [3.0, 0.0]]))
    assert out["cost"] == np.float32(48 * 0.5 / 10)


def test_planner_is_present_in_every_layer():
    import kompass_cpp
    import kompass_hip as kh

    L = kh.lib()
    for name in ("kc_planner_create", "kc_planner_destroy", "kc_planner_set_grid_host", "kc_planner_set_grid_device",
                 "kc_planner_solve", "kc_planner_get_field", "kc_planner_get_path"):
        assert hasattr(L, name) and name in kh.SIGNATURES, name
    cls = kompass_cpp.planning.GridPlanner
    for name in ("set_space_bounds_from_map", "setup_problem", "solve", "get_solution", "get_cost", "set_grid"):
        assert hasattr(cls, name), name
    from kompass_core.planning import GridPlanner  # noqa: F401

    if kh.device_count() == 0:  # no CPU fallback
        with pytest.raises(kh.KompassHipError):
            kh.PlannerContext()
        with pytest.raises(RuntimeError):
            cls(kompass_cpp.types.RobotGeometry.CYLINDER, [0.1, 0.4])
    with pytest.raises(ValueError):
        cls(kompass_cpp.types.RobotGeometry.BOX, [0.1])
