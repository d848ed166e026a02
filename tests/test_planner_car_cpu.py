"""The grid planner's car motion (rules 27 to 36) as tests/planner_car_ref.py states it: the heading
table and the turn cells against the host class's device-free statics, the statement's own properties on the issue's
scenes and on planner_oriented_ref's, and the three scenes whose figures the issue gives.  No GPU needed."""
import math

import numpy as np
import pytest

import planner_car_ref as cref
import planner_oriented_ref as oref
import planner_ref as ref

# the sixteen multiples of pi / 8 (a half rounds away from zero) and the three values around the first boundary
HEADING_TABLE = [(k * math.pi / 8, h) for k, h in zip(range(-8, 8), (4, 4, 5, 5, 6, 6, 7, 7, 0, 1, 1, 2, 2, 3, 3, 4))]
HEADING_TABLE += [(0.39, 0), (0.40, 1), (-0.40, 7)]


def test_heading_table():
    import kompass_cpp

    cls = kompass_cpp.planning.GridPlanner.heading_class
    for yaw, h in HEADING_TABLE:
        # a multiple of pi / 8 in double is not the exact half: nudge it off the boundary towards where lround sends a half
        y = yaw + math.copysign(1e-12, yaw) if yaw else yaw
        assert cref.heading_class(y) == h, yaw
        assert cls(y) == h, yaw
        assert cls(yaw) == cref.heading_class(yaw), yaw
    for yaw in np.linspace(-20.0, 20.0, 801):
        assert cls(float(yaw)) == cref.heading_class(float(yaw)), yaw
        assert cls(float(yaw)) & 3 == oref.orientation_class(float(yaw)), yaw      # rule 28's h & 3 is rule 13's class
    for h in range(8):                                                              # D[h] points along h * 45 degrees
        assert cref.heading_class(math.atan2(cref.D[h][1], cref.D[h][0])) == h
        assert cref.D[h] == tuple(-v for v in cref.D[(h + 4) & 7])
        assert cref.step(h) == (14 if cref.D[h][0] and cref.D[h][1] else 10)
        assert cref.D[h] in (oref.CLASS_DIR[h & 3], tuple(-v for v in oref.CLASS_DIR[h & 3]))


def test_turn_cells():
    import kompass_cpp

    tc = kompass_cpp.planning.GridPlanner.turn_cells
    for radius, res, n in [(0.5, 0.05, 5), (1.0, 0.1, 5), (0.01, 0.05, 1)]:
        assert cref.turn_cells(radius, res) == n
        assert tc(radius, res) == n
        assert tc(float(np.float32(radius)), float(np.float32(res))) == n
    assert math.tan(math.pi / 8) == pytest.approx(cref.TAN_PI_8, abs=1e-16)
    for n in range(1, 9):   # rule 31: the fillet inside n cells of tangent, n / tan(pi / 8) cells, has at least the asked radius
        r_cells = (n - 0.5) / cref.TAN_PI_8
        assert cref.turn_cells(r_cells * 0.5, 0.5) == n == tc(r_cells * 0.5, 0.5) and n / cref.TAN_PI_8 >= r_cells
    with pytest.raises(ValueError):
        tc(float("nan"), 0.05)
    with pytest.raises(ValueError):
        tc(0.5, 0.0)


def _check_plan(grid, p, start, h0, goal, hg, n, rw):
    """The properties the issue asks of the statement, on one solved plan."""
    valid, moves, field = p["valid"], p["moves"], p["field"]
    cells, heads, states, prims = p["cells"], p["heads"], p["states"], p["prims"]
    assert tuple(states[0]) == (start[0], start[1], h0) and tuple(states[-1][:2]) == tuple(goal)
    assert hg == cref.ANY or states[-1][2] == hg
    assert tuple(cells[0]) == tuple(start) and tuple(cells[-1]) == tuple(goal)
    d = np.diff(cells, axis=0)
    assert len(d) == 0 or (np.abs(d).max(axis=1) == 1).all()                      # 8-neighbours, so no duplicates
    assert valid[heads, cells[:, 0], cells[:, 1]].all()                            # valid in the heading held there
    turn = np.nonzero(np.diff(heads))[0]                                           # index of the last step before a change
    assert all((int(heads[k + 1]) - int(heads[k])) % 8 in (1, 7) for k in turn)
    assert (np.diff(turn) >= 2 * n).all() if len(turn) > 1 else True              # 2 n unit steps between two corners
    arcs = [int(x) for x in prims if int(x) not in (cref.S, cref.B)]
    assert len(turn) == len(arcs)                                                  # the heading changes only across an arc
    for a, b, prim in zip(states[:-1], states[1:], prims):
        assert tuple(b) == cref.target(int(a[0]), int(a[1]), int(a[2]), int(prim), n)
        assert moves[a[2], a[0], a[1]] >> int(prim) & 1
        assert rw or int(prim) < cref.B
    assert sum(p["step_costs"]) == p["cost"] == int(field[h0, start[0], start[1]])
    assert cref.forward_cost(valid, moves, start, h0, goal, hg, n, rw) == p["cost"]
    assert len(cells) == 1 + sum(1 if int(x) in (cref.S, cref.B) else 2 * n for x in prims)
    assert len({tuple(s) for s in states.tolist()}) == len(states)                 # no state comes twice


def test_dead_end_corridor_figures():
    grid, start, goal = cref.dead_end_scene()
    for n in (1, 2):                                   # no reverse: a car cannot turn round in five cells of width
        p = cref.plan(grid, start, 0, goal, cref.ANY, n, 0, r2=1)
        assert p["status"] == ref.UNREACHABLE and p["cost"] == ref.INF
        assert cref.forward_cost(p["valid"], p["moves"], start, 0, goal, cref.ANY, n, 0) == ref.INF
    p = cref.plan(grid, start, 0, goal, cref.ANY, 1, 2, r2=1)
    assert (p["status"], p["cost"]) == (ref.FOUND, 274)
    assert [cref.MOVE_NAMES[m] for m in p["prims"]] == ["BL", "R", "BL", "R"] + ["S"] * 13   # a three-point turn
    _check_plan(grid, p, start, 0, goal, cref.ANY, 1, 2)
    p = cref.plan(grid, start, 0, goal, cref.ANY, 2, 2, r2=1)
    assert (p["status"], p["cost"]) == (ref.FOUND, 300)
    assert [cref.MOVE_NAMES[m] for m in p["prims"]] == ["B"] * 15
    _check_plan(grid, p, start, 0, goal, cref.ANY, 2, 2)


def test_free_grid_goal_heading_figures():
    grid, start, goal = cref.free_scene()
    p = cref.plan(grid, start, 0, goal, 4, 2, 0)
    assert (p["status"], p["cost"]) == (ref.FOUND, 410)
    assert [cref.MOVE_NAMES[m] for m in p["prims"]] == ["S"] + ["L"] * 5 + ["S"] * 8 + ["R"]
    _check_plan(grid, p, start, 0, goal, 4, 2, 0)
    # the moves byte refuses what would leave the grid and allows an arc that ends in the last column or row
    m = p["moves"]
    assert m[0, 39 - 4, 10] >> cref.L & 1 and cref.target(35, 10, 0, cref.L, 2)[0] == 39
    assert not m[0, 39 - 3, 10] >> cref.L & 1 and not m[0, 39, 10] & 1
    assert m[2, 10, 29 - 4] >> cref.R & 1 and cref.target(10, 25, 2, cref.R, 2)[1] == 29
    assert not m[2, 10, 29 - 3] >> cref.R & 1
    assert not (m >> cref.B).any()                     # rw = 0: B, BL and BR do not exist
    # the same cell in another heading: leave and come back
    q = cref.plan(grid, start, 0, start, 4, 2, 0)
    assert q["status"] == ref.FOUND and q["cost"] > 0 and len(q["states"]) > 1
    _check_plan(grid, q, start, 0, start, 4, 2, 0)


@pytest.mark.parametrize("scene", ["corridor", "l", "clutter"])
def test_properties_on_the_oriented_scenes(scene):
    grid, start, goal = {"corridor": oref.corridor_scene, "l": oref.l_scene, "clutter": oref.clutter_scene}[scene]()
    found = 0
    for n, rw, r2, box, hg in [(1, 0, 0, None, cref.ANY), (2, 2, 4, None, 0), (3, 1, 0, (9, 1), cref.ANY), (2, 3, 0, (9, 1), 4)]:
        p = cref.plan(grid, start, 0, goal, hg, n, rw, r2=r2, box=box)
        assert p["status"] in (ref.FOUND, ref.UNREACHABLE, ref.GOAL_INVALID, ref.START_INVALID)
        if p["status"] == ref.FOUND:
            found += 1
            _check_plan(grid, p, start, 0, goal, hg, n, rw)
        else:
            assert cref.forward_cost(p["valid"], p["moves"], start, 0, goal, hg, n, rw) == ref.INF
        # rule 28: the box's headings h and h + 4 share a mask, and turn validity plays no part
        if box:
            np.testing.assert_array_equal(p["valid"][:4], p["valid"][4:])
            np.testing.assert_array_equal(p["valid"][:4], oref.oriented_validity(grid, *box))
        # an invalid state has no move; a reachable state's value is the best of its primitives (rule 32)
        assert not p["moves"][~p["valid"]].any()
    assert found >= 2


def test_field_is_the_fixed_point_of_rule_32():
    grid, start, goal = oref.clutter_scene()
    n, rw = 2, 3
    p = cref.plan(grid, start, 0, goal, cref.ANY, n, rw, r2=1)
    f, m = p["field"].astype(np.int64), p["moves"]
    rng = np.random.default_rng(3)
    for _ in range(400):
        h, i, j = int(rng.integers(8)), int(rng.integers(72)), int(rng.integers(70))
        cands = []
        for prim in range(6):
            if m[h, i, j] >> prim & 1:
                ti, tj, th = cref.target(i, j, h, prim, n)
                if f[th, ti, tj] != ref.INF:
                    cands.append(int(f[th, ti, tj]) + cref.cost_of(h, prim, n, rw))
        if (i, j) == tuple(goal) and p["valid"][h, i, j]:
            assert f[h, i, j] == 0
        else:
            assert f[h, i, j] == (min(cands) if cands else ref.INF)


def test_range_rule():
    assert cref.check_range(8, 16, 72 * 70)
    assert not cref.check_range(9, 1, 100) and not cref.check_range(1, 17, 100) and not cref.check_range(0, 0, 100)
    assert cref.check_range(1, 0, 22369621) and not cref.check_range(1, 0, 22369622)   # 24 * 8 * cells <= 0xFFFFFFFE


def test_argument_errors_that_need_no_device():
    from kompass_core.planning import GridPlanner
    from test_planner_oriented_cpu import _box_robot

    robot = _box_robot()
    with pytest.raises(ValueError, match="motion"):
        GridPlanner(robot, motion="bicycle")
    with pytest.raises(ValueError, match="goal_heading"):
        GridPlanner(robot, motion="car", min_turning_radius=0.5, goal_heading="north")
    with pytest.raises(ValueError, match="min_turning_radius"):
        GridPlanner(robot, motion="car")
    with pytest.raises(ValueError, match="clearance"):
        GridPlanner(robot, motion="car", min_turning_radius=0.5, clearance_reach=0.3, clearance_weight=2.0)
    with pytest.raises(ValueError, match="any-angle"):
        GridPlanner(robot, motion="car", min_turning_radius=0.5, any_angle=True)
    with pytest.raises(ValueError, match="reverse_weight"):
        GridPlanner(robot, motion="car", min_turning_radius=0.5, allow_reverse=True, reverse_weight=17)
