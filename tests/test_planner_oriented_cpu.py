"""The oriented box footprint of the grid planner (rules 13 to 18) as tests/planner_oriented_ref.py
states it: the class table and the masks against the host class's device-free statics, the turning disc against the
masks, the disc footprint against the oriented one, the field's own consistency, and the argument errors that need no
device.  No GPU needed."""
import math

import numpy as np
import pytest

import planner_oriented_ref as oref
import planner_ref as ref

CLASS_TABLE = [(0.0, 0), (math.pi / 4, 1), (math.pi / 2, 2), (3 * math.pi / 4, 3), (math.pi, 0), (-math.pi / 4, 3),
               (-math.pi / 2, 2), (0.39, 0), (0.40, 1), (-0.40, 3)]


def test_class_table():
    import kompass_cpp

    cls = kompass_cpp.planning.GridPlanner.orientation_class
    for yaw, k in CLASS_TABLE:
        assert oref.orientation_class(yaw) == k, yaw
        assert cls(yaw) == k, yaw
    # halves away from zero, and whole turns
    for yaw in np.linspace(-20.0, 20.0, 801):
        assert cls(float(yaw)) == oref.orientation_class(float(yaw)), yaw
    assert [oref.DIRECTION_CLASS[q] for q in range(8)] == [0, 2, 0, 2, 1, 3, 1, 3]
    for q, (di, dj) in enumerate(ref.NEIGHBOURS):   # a direction or its opposite is its class's axis
        assert oref.CLASS_DIR[oref.DIRECTION_CLASS[q]] in ((di, dj), (-di, -dj))
    for k in range(4):                              # ... and the axis is the first of the two in rule 4's order
        first = min(q for q in range(8) if oref.DIRECTION_CLASS[q] == k)
        assert ref.NEIGHBOURS[first] == oref.CLASS_DIR[k]


def test_mask_sizes_and_the_class_masks():
    import kompass_cpp

    mask = kompass_cpp.planning.GridPlanner.oriented_mask
    assert oref.box_a2_b2(oref.BIG_BOX, 0.0, oref.RES) == (225, 4)
    assert oref.box_a2_b2(oref.SMALL_BOX, 0.0, oref.RES) == (9, 1)
    assert [len(oref.oriented_mask(k, 225, 4)) for k in range(4)] == [155, 107, 155, 107]
    assert [len(oref.oriented_mask(k, 9, 1)) for k in range(4)] == [21, 13, 21, 13]
    for a2, b2 in [(225, 4), (9, 1), (1, 0), (4, 4), (2, 7), (400, 399), (64516, 0), (30000, 2)]:
        for k in range(4):
            got = np.asarray(mask(k, a2, b2))
            want = oref.oriented_mask(k, a2, b2)
            assert got.shape == (len(want), 2) and got.dtype == np.int32
            assert set(map(tuple, got.tolist())) == set(want), (k, a2, b2)
            assert len(set(map(tuple, got.tolist()))) == len(want)
            assert (0, 0) in want
            # a box is symmetric under a half turn
            assert {(-di, -dj) for di, dj in want} == set(want)


def test_the_turning_disc_contains_every_mask():
    """T2 = A2 + B2: k = 0, 2 give di^2 + dj^2 <= A2 + B2 at once; k = 1, 3 give (di + dj)^2 + (dj - di)^2 = 2 (di^2 +
    dj^2) <= 2 A2 + 2 B2.  Over all A2 <= 400, B2 <= A2, offset by offset, and with equality somewhere."""
    r = math.isqrt(800) + 1
    d = np.arange(-r, r + 1, dtype=np.int32)
    di, dj = d[:, None], d[None, :]
    ii, jj, ss, dd = di * di, dj * dj, (di + dj) ** 2, (dj - di) ** 2
    b = np.arange(401, dtype=np.int32)[None, None, :]
    # the B2 halves of the four masks do not depend on A2: once, for every B2
    jb, ib, db, sb = jj[..., None] <= b, ii[..., None] <= b, dd[..., None] <= 2 * b, ss[..., None] <= 2 * b
    d2 = (ii + jj)[..., None]
    tight = 0
    for a2 in range(401):
        n = a2 + 1   # B2 = 0 .. A2
        masks = ((ii <= a2)[..., None] & jb[..., :n], (ss <= 2 * a2)[..., None] & db[..., :n],
                 (jj <= a2)[..., None] & ib[..., :n], (dd <= 2 * a2)[..., None] & sb[..., :n])
        outside = d2 > a2 + b[..., :n]
        edge = d2 == a2 + b[..., :n]
        for m in masks:
            assert not (m & outside).any(), a2
            tight += int((m & edge).any())
    assert tight > 0
    # the statement's masks are these sets
    for a2, b2 in [(225, 4), (9, 1), (400, 400)]:
        for k in range(4):
            assert all(i * i + j * j <= a2 + b2 for i, j in oref.oriented_mask(k, a2, b2))


@pytest.fixture(scope="module")
def bernoulli():
    """Seeded 72 x 70 Bernoulli(0.01) grid, the small box at margin 0: validity, turn validity and the field, once."""
    grid, start, goal = oref.clutter_scene()
    a2, b2 = oref.box_a2_b2(oref.SMALL_BOX, 0.0, oref.RES)
    turn10 = 7
    p = oref.plan(grid, start, 0, goal, a2, b2, turn10)
    for a in (p["valid"], p["turn"], p["field"]):
        a.setflags(write=False)
    return dict(grid=grid, start=start, goal=goal, a2=a2, b2=b2, turn10=turn10, **p)


def test_a_cell_valid_for_the_disc_is_valid_in_every_class(bernoulli):
    r2 = ref.radius_to_r2(ref.footprint_radius(ref.BOX, oref.SMALL_BOX), oref.RES)
    disc = ref.validity(bernoulli["grid"], r2)
    assert disc.any() and not disc.all()
    assert (bernoulli["valid"] | ~disc[None]).all()
    # and the turning disc, which is rule 2's test as well, is inside every class
    assert (bernoulli["valid"] | ~bernoulli["turn"][None]).all()
    # the point of the mode: states the disc refuses
    assert (bernoulli["valid"] & ~disc[None]).any()


def test_bellman_consistency_and_the_walk_sum(bernoulli):
    valid, turn, field, turn10 = bernoulli["valid"], bernoulli["turn"], bernoulli["field"], bernoulli["turn10"]
    goal = bernoulli["goal"]
    big = 1 << 40
    f = np.where(field == oref.INF, big, field.astype(np.int64))
    want = np.full(f.shape, big, np.int64)
    for k in range(4):
        di, dj = oref.CLASS_DIR[k]
        for sgn in (1, -1):
            nv = ref._shift(valid[k], sgn * di, sgn * dj)
            nf = ref._shift(f[k], sgn * di, sgn * dj, fill=big)
            want[k] = np.minimum(want[k], np.where(valid[k] & nv, nf + oref.STEP_COST[k], big))
        for nk in ((k + 1) % 4, (k + 3) % 4):
            want[k] = np.minimum(want[k], np.where(turn & valid[k], f[nk] + turn10, big))
    want = np.minimum(want, big)
    want[:, goal[0], goal[1]] = np.where(valid[:, goal[0], goal[1]], 0, big)
    want[~valid] = big
    np.testing.assert_array_equal(f, want)
    assert (f[valid] < big).any() and (field[~valid] == oref.INF).all()
    # the issue's prototype values at the start, by class
    s = bernoulli["start"]
    assert field[:, s[0], s[1]].tolist() == [922, 929, 928, 929]
    for k0 in range(4):
        states, costs = oref.walk(valid, turn, field, s, k0, turn10)
        assert sum(costs) == int(field[k0, s[0], s[1]])
        assert tuple(states[0]) == (s[0], s[1], k0) and tuple(states[-1][:2]) == goal
        assert all(valid[k, i, j] for i, j, k in states.tolist())
        cells = oref.collapse(states)
        assert (np.abs(np.diff(cells, axis=0)).max(axis=1) == 1).all()
        assert len(cells) == len(states) - sum(c == turn10 for c in costs)


def test_the_issues_scenes_in_the_statement():
    grid, s, t = oref.corridor_scene()
    p = oref.plan(grid, s, 0, t, 225, 4, 10)
    assert (p["status"], p["cost"]) == (ref.FOUND, 670)
    assert p["valid"].sum(axis=(1, 2)).tolist() == [216, 0, 0, 0] and not p["turn"].any()
    r2 = ref.radius_to_r2(ref.footprint_radius(ref.BOX, oref.BIG_BOX), oref.RES)
    assert not ref.validity(grid, r2)[s]          # the disc never enters the corridor
    grid, s, t = oref.l_scene()
    p = oref.plan(grid, s, 0, t, 225, 4, 10)
    assert (p["status"], p["cost"], int(p["turn"].sum())) == (ref.FOUND, 782, 31)
    ks = p["states"][:, 2]
    assert ks[np.r_[True, ks[1:] != ks[:-1]]].tolist() == [0, 1, 2] and sum(p["step_costs"]) == 782
    grid, s, t = oref.l_scene(bay=False)
    p = oref.plan(grid, s, 0, t, 225, 4, 10)
    assert p["status"] == ref.UNREACHABLE and not p["turn"].any()


def _box_robot(dims=oref.BIG_BOX):
    from kompass_core.models import Robot, RobotGeometry, RobotType
    return Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.BOX,
                 geometry_params=np.array(dims))


def test_argument_errors_that_need_no_device():
    import kompass_cpp
    from kompass_core.models import Robot, RobotGeometry, RobotType
    from kompass_core.planning import GridPlanner

    mask = kompass_cpp.planning.GridPlanner.oriented_mask
    for k in (-1, 4):
        with pytest.raises(ValueError):
            mask(k, 9, 1)
    with pytest.raises(IndexError):          # T2 beyond 254 cells
        mask(0, 64516, 1)
    assert len(mask(0, 64516, 0)) == 2 * 254 + 1
    cylinder = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER,
                     geometry_params=np.array((0.1, 0.4)))
    with pytest.raises(ValueError, match="footprint"):
        GridPlanner(_box_robot(), footprint="ellipse")
    with pytest.raises(ValueError, match="BOX"):
        GridPlanner(cylinder, footprint="oriented")
    with pytest.raises(ValueError, match="clearance"):
        GridPlanner(_box_robot(), footprint="oriented", clearance_reach=0.4, clearance_weight=4.0)
    with pytest.raises(ValueError, match="any-angle"):
        GridPlanner(_box_robot(), footprint="oriented", any_angle=True)
    for bad in (0.0, 0.04, -1.0, 1000.06, float("nan")):
        with pytest.raises(ValueError, match="turn_cost"):
            GridPlanner(_box_robot(), footprint="oriented", turn_cost=bad)


def test_oriented_is_present_in_every_layer():
    import inspect

    import kompass_cpp
    import kompass_hip as kh
    from kompass_core.planning import GridPlanner

    L = kh.lib()
    for name in ("kc_planner_set_oriented", "kc_planner_solve_oriented", "kc_planner_get_oriented_field",
                 "kc_planner_get_oriented_path"):
        assert hasattr(L, name) and name in kh.SIGNATURES, name
    assert L.kc_abi_version() == 1
    for name in ("set_oriented", "solve_oriented", "oriented_field", "oriented_path"):
        assert hasattr(kh.PlannerContext, name), name
    cls = kompass_cpp.planning.GridPlanner
    for name in ("set_oriented_footprint", "oriented_on", "get_path_states", "orientation_class", "oriented_mask",
                 "get_oriented_field"):
        assert hasattr(cls, name), name
    par = inspect.signature(GridPlanner.__init__).parameters
    assert par["footprint"].default == "disc" and par["turn_cost"].default == 1.0   # off by default
    assert hasattr(GridPlanner, "get_path_states")
