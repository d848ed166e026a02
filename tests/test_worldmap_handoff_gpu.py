"""World map -> controller hand-off on the device (kc_dwa_set_worldmap, DESIGN.md 4.11 rules 16 to 19).

The occupied cells of a device-resident world map within sensor range of the robot become the controller's sensor data
without a host round trip.  Expected result: the oracle's point-list cycle on the list of the numpy statement
(tests/worldmap_points_ref.py) of the same map."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import synthetic as syn  # noqa: E402
import worldmap_points_ref as pref  # noqa: E402
import worldmap_ref as ref  # noqa: E402

from helpers import assert_cycle_equal, hip_context, oracle_cycle  # noqa: E402

RES = 0.05


def _cycle_from_ctx(ctx, inp):
    """One cycle on whatever sensor state the context holds (as test_grid_handoff does it)."""
    ctx.set_weights(kh.make_weights(*inp["weights"]))
    ctx.set_tracked_segment(inp["seg_xyz"], inp["acc_at_seg"], inp["ref_len"])
    ctx.set_samples(inp["vx"], inp["vy"], inp["omega"])
    res = ctx.cycle(inp["state"], inp["P"])
    px, py, raw, costs = ctx.get_samples(with_costs=True)
    out = dict(px=px.copy(), py=py.copy(), raw=raw.copy(), costs=costs.copy(), res=res.as_dict())
    if res.found:
        out["best"] = ctx.get_best()
    return out


def cluttered_world(W, H, density, robot_cell, seed=8):
    """cls[I, J] of a W x H world: clutter that thins out near the robot, a free disc around it (the scene of
    test_grid_handoff.test_foreign_grid_on_device, in the world's layout)."""
    r = np.random.default_rng(seed)
    cls = r.choice(np.int8([ref.UNEXPLORED, ref.EMPTY, ref.OCCUPIED]), size=(W, H), p=[0.3, 0.7 - density, density]).astype(np.int8)
    ii, jj = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    d2 = (ii - robot_cell[0]) ** 2 + (jj - robot_cell[1]) ** 2
    sparse = r.random((W, H)) < 0.004
    cls[(d2 < (3.0 / RES) ** 2) & (cls == ref.OCCUPIED) & ~sparse] = ref.EMPTY
    cls[d2 < (0.6 / RES) ** 2] = ref.EMPTY
    return cls


def origin_for(state, robot_cell, res=RES):
    """The origin that puts the robot a third of a cell off the centre of robot_cell."""
    r = float(np.float32(res))
    return state[0] - (robot_cell[0] + 0.33) * r, state[1] - (robot_cell[1] - 0.21) * r


def same_cycle(a, b):
    for k in ("raw", "px", "py", "costs"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["res"] == b["res"]


@pytest.mark.parametrize("shape,dims,density", [
    (kh.CYLINDER, [0.1, 0.4], 0.004),
    (kh.BOX, [0.3, 0.2, 0.4], 0.004),
    (kh.CYLINDER, [0.1, 0.4], 0.2),       # > 16 k points in the window: host lists from the device list
    (kh.SPHERE, [0.15], 0.004),
])
def test_world_map_to_controller_on_device(shape, dims, density):
    inp = syn.make_controller_inputs("cfg2", seed=4, scale=0.25)
    inp["robot"] = dict(shape=shape, dims=dims)
    st = inp["state"]
    W, H, cell = 420, 380, (205, 183)
    origin = origin_for(st, cell)
    cls = cluttered_world(W, H, density, cell)
    pts, n, _ = pref.worldmap_points_ref(cls, RES, origin, st[0], st[1], inp["max_range"])
    inp["points"] = pts
    assert (n > 16384) == (density > 0.1)
    assert 0 < n < int((cls == ref.OCCUPIED).sum()), "the window must leave some of the map's obstacles out"
    o = oracle_cycle(inp)
    assert 0 < len(o["raw"]) < len(inp["vx"]), "scene must drop some samples and keep some"
    with kh.WorldMapContext(W, H, RES, origin) as wm:
        wm.set_prior(cls)
        ctx = hip_context(kh, inp)
        for _ in range(2):                               # twice: counters re-armed, buffers reused
            ctx.set_worldmap(st, wm, inp["max_range"])
            assert_cycle_equal(o, _cycle_from_ctx(ctx, inp))
        # same state as the point-list entry with the statement's list
        ctx2 = hip_context(kh, inp)
        ctx2.set_points(st, pts, inp["max_range"])
        assert_cycle_equal(o, _cycle_from_ctx(ctx2, inp))
        # pose batch on the same sensor state walks the host lists (fetched lazily from the device list)
        r = np.random.default_rng(8)
        x, y, yaw = r.random(300) * 8 - 4, r.random(300) * 8 - 4, r.random(300) * 6.28 - 3.14
        got = ctx.check_poses(x, y, yaw)
        want = np.array([o["coll"].check_at(a, b, c) for a, b, c in zip(x, y, yaw)], bool)
        np.testing.assert_array_equal(np.asarray(got, bool), want)


def test_empty_window_and_errors():
    inp = syn.make_controller_inputs("cfg1", seed=1, scale=1.0)
    st = inp["state"]
    inp["points"] = np.zeros((0, 3), np.float32)
    o = oracle_cycle(inp)
    assert len(o["raw"]) == len(inp["vx"])          # nothing to collide with
    occupied = np.full((64, 48), ref.OCCUPIED, np.int8)
    unknown = np.full((64, 48), ref.UNEXPLORED, np.int8)
    ctx = hip_context(kh, inp)
    # a map the window misses altogether (no launch), and one it covers that holds no obstacle (a launch without a hit)
    for origin, prior in [((500.0, -300.0), occupied), ((-1.0, -1.0), unknown)]:
        with kh.WorldMapContext(64, 48, RES, origin) as wm:
            wm.set_prior(prior)
            ctx.set_worldmap(st, wm, inp["max_range"])
            assert_cycle_equal(o, _cycle_from_ctx(ctx, inp))
    with kh.WorldMapContext(64, 48, RES, (-1.0, -1.0)) as wm:
        with pytest.raises(ValueError):
            ctx.set_worldmap(st, None, inp["max_range"])
        for bad in (0.0, -2.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                ctx.set_worldmap(st, wm, bad)
        with pytest.raises(IndexError):
            ctx.set_worldmap(st, wm, 200.0)                                  # 4000 cells
        with pytest.raises(IndexError):
            ctx.set_worldmap((1e6, 0.0, 0.0, 0.0), wm, inp["max_range"])     # 2 10^7 cells from the origin
        # a refusal leaves the sensor state alone
        assert_cycle_equal(o, _cycle_from_ctx(ctx, inp))


@pytest.mark.skipif(kh.device_count() < 2, reason="needs a second device")
def test_map_on_another_device_is_refused():
    inp = syn.make_controller_inputs("cfg1", seed=1, scale=1.0)
    ctx = hip_context(kh, inp)
    with kh.WorldMapContext(64, 48, RES, (-1.0, -1.0), device=1) as wm:
        with pytest.raises(ValueError, match="device"):
            ctx.set_worldmap(inp["state"], wm, inp["max_range"])


def test_mapper_and_world_map_take_turns_on_one_context():
    """The two hand-offs share their tail and the counter block: each must leave them as a fresh context has them."""
    inp = syn.make_controller_inputs("cfg1", seed=3, scale=1.0)
    st = inp["state"]
    ang, rng = syn.dense_scan(360, 0.3)
    m = kh.MapperContext(200, 200, RES, (0, 0, 0), 0.0, 360)
    W, H, cell = 150, 130, (70, 66)
    origin = origin_for(st, cell)
    cls = cluttered_world(W, H, 0.01, cell, seed=5)
    cls[cell[0] + 14:cell[0] + 17, cell[1] - 3:cell[1] + 9] = ref.OCCUPIED   # a wall the straight samples run into
    with kh.WorldMapContext(W, H, RES, origin) as wm:
        wm.set_prior(cls)

        def from_mapper(ctx):
            m.scan_to_grid_device(ang, rng)
            ctx.set_grid_from_mapper(st, m, inp["max_range"])
            return _cycle_from_ctx(ctx, inp)

        def from_world(ctx):
            ctx.set_worldmap(st, wm, 3.0)
            return _cycle_from_ctx(ctx, inp)

        want_mapper, want_world = from_mapper(hip_context(kh, inp)), from_world(hip_context(kh, inp))
        assert want_mapper["res"] != want_world["res"], "the two sources must be told apart"
        ctx = hip_context(kh, inp)
        same_cycle(from_world(ctx), want_world)
        same_cycle(from_mapper(ctx), want_mapper)
        same_cycle(from_world(ctx), want_world)
        same_cycle(from_mapper(ctx), want_mapper)
        # and the world map's result is the oracle's on the statement's list
        pts, n, _ = pref.worldmap_points_ref(cls, RES, origin, st[0], st[1], 3.0)
        assert n > 30
        assert_cycle_equal(oracle_cycle(dict(inp, points=pts, max_range=3.0)), want_world)


def test_an_obstacle_only_the_map_remembers():
    """A short wall across the path, seen by an earlier scan and fused into the map; the current scan has those beams out
    of range, so the mapper's grid does not hold it.  Fed from the mapper the controller's best trajectory runs through the
    wall's cells; fed from the map it goes round them."""
    import math

    inp = syn.make_controller_inputs("cfg1", seed=3, scale=1.0)
    st = inp["state"]
    assert tuple(st[:3]) == (0.0, 0.0, 0.0)
    n = 360
    ang = -math.pi + np.arange(n) * (2 * math.pi / n)
    wall = (ang >= -1e-9) & (ang <= math.atan(0.2 / 0.6) + 1e-9)             # the beams that meet x = 0.6, 0 <= y <= 0.2
    earlier, now = np.full(n, 3.0), np.full(n, 3.0)
    earlier[wall] = 0.6 / np.cos(ang[wall])
    now[wall] = 30.0                                                          # beyond the grid: no return
    r = float(np.float32(RES))
    c0, c1 = ref.central(200, 200)
    origin = (-c0 * r, -c1 * r)                                               # world cell (I, J) is local cell (i, j)
    m = kh.MapperContext(200, 200, RES, (0, 0, 0), 0.0, n)
    with kh.WorldMapContext(200, 200, RES, origin) as wm:
        want = ref.WorldMapRef(200, 200, RES, origin)
        g1 = m.scan_to_grid(ang, earlier).copy()
        m.scan_to_grid_device(ang, earlier)
        assert wm.update_from_mapper(m, (0.0, 0.0, 0.0)) == want.update(g1, (0.0, 0.0, 0.0))
        g2 = m.scan_to_grid(ang, now).copy()
        m.scan_to_grid_device(ang, now)                                       # the mapper's current grid
        block = np.argwhere((g1 == ref.OCCUPIED) & (g2 != ref.OCCUPIED))
        assert len(block) >= 4 and (want.cls[block[:, 0], block[:, 1]] == ref.OCCUPIED).all()
        centres = (block - [c0, c1]) * r

        def crosses(best):
            bx, by, _ = best
            I = np.rint((bx.astype(np.float64) - origin[0]) / r).astype(int)
            J = np.rint((by.astype(np.float64) - origin[1]) / r).astype(int)
            return bool((want.cls[I, J] == ref.OCCUPIED).any())

        def clearance(best):
            bx, by, _ = best
            return float(np.hypot(bx[:, None] - centres[None, :, 0], by[:, None] - centres[None, :, 1]).min())

        a = hip_context(kh, inp)
        a.set_grid_from_mapper(st, m, inp["max_range"])
        from_mapper = _cycle_from_ctx(a, inp)
        assert from_mapper["res"]["found"] and crosses(from_mapper["best"])
        assert clearance(from_mapper["best"]) < inp["robot"]["dims"][0]
        b = hip_context(kh, inp)
        b.set_worldmap(st, wm, inp["max_range"])
        from_world = _cycle_from_ctx(b, inp)
        assert from_world["res"]["found"] and not crosses(from_world["best"])
        assert clearance(from_world["best"]) >= inp["robot"]["dims"][0]
        assert 0 < from_world["res"]["n_admissible"] < from_mapper["res"]["n_admissible"]
        pts, _, _ = pref.worldmap_points_ref(want.cls, RES, origin, st[0], st[1], inp["max_range"])
        assert_cycle_equal(oracle_cycle(dict(inp, points=pts)), from_world)


# ---- class level: kompass_core's controllers take the map as local_map= -------------------------------------------
ROOM_RES, ROOM_ORIGIN = 0.1, (-1.05, -2.95)


def room_cls():
    """70 x 60 cells of 0.1 m: walls all round, a block beside the straight path, unknown space behind the far wall."""
    cls = np.full((70, 60), ref.EMPTY, np.int8)
    cls[0, :] = cls[62, :] = cls[:, 0] = cls[:, 59] = ref.OCCUPIED
    cls[63:, :] = ref.UNEXPLORED
    cls[28:32, 31:36] = ref.OCCUPIED          # x 1.75 .. 2.05, y 0.15 .. 0.55
    cls[40:43, 22:28] = ref.OCCUPIED          # x 2.95 .. 3.15, y -0.75 .. -0.25
    return cls


def _front_end_world(cls):
    from kompass_core.mapping import WorldMap

    wm = WorldMap(cls.shape[0], cls.shape[1], ROOM_RES, ROOM_ORIGIN)
    wm.set_prior(cls)
    return wm


def _robot():
    from kompass_core.models import Robot, RobotGeometry, RobotType
    return Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER,
                 geometry_params=np.array([0.1, 0.4]))


def _limits():
    from kompass_core.models import AngularCtrlLimits, LinearCtrlLimits, RobotCtrlLimits
    return RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=2.0, max_decel=2.0),
                           omega_limits=AngularCtrlLimits(max_vel=2.0, max_acc=3.0, max_decel=3.0, max_steer=2.0))


PATH = np.stack([np.linspace(0.0, 4.5, 46), np.zeros(46)], 1)


@pytest.mark.parametrize("max_range", [10.0, 2.0])
def test_dwa_front_end_takes_the_world_map(max_range):
    from kompass_core.control import DWA, DWAConfig
    from kompass_core.models import RobotState

    cls = room_cls()
    wm = _front_end_world(cls)
    cfg = dict(max_linear_samples=6, max_angular_samples=9, prediction_horizon=10, control_horizon=2, octree_resolution=0.1)
    a, b = (DWA(robot=_robot(), ctrl_limits=_limits(), config=DWAConfig(**cfg)) for _ in range(2))
    for c in (a, b):
        c.set_path(PATH)
        c.planner.set_sensor_max_range(max_range)
    state = RobotState(x=0.0, y=0.05, yaw=0.1, speed=0.0)
    moved = 0.0
    for step in range(5):
        pts, n, _ = pref.worldmap_points_ref(cls, ROOM_RES, ROOM_ORIGIN, state.x, state.y, max_range)
        assert (n < int((cls == ref.OCCUPIED).sum())) == (max_range < 5.0)     # the short range cuts the room
        np.testing.assert_array_equal(pref.sort_points(wm.points(state, max_range), ROOM_RES, ROOM_ORIGIN), pts)
        assert a.loop_step(current_state=state, local_map=wm, debug=(step == 2))  # debug: excluded as for the mapper
        assert b.loop_step(current_state=state, point_cloud=pts)
        assert a.has_result() and b.has_result()
        for name in ("linear_x_control", "linear_y_control", "angular_control"):
            assert list(getattr(a, name)) == list(getattr(b, name)), (step, name)
        state.simulate(v_x=a.linear_x_control[0], v_y=a.linear_y_control[0], omega=a.angular_control[0], dt=0.1)
        moved += abs(a.linear_x_control[0])
    assert moved > 0.0
    # the class of kompass_cpp goes in as it is
    assert a.loop_step(current_state=state, local_map=wm._map)


def test_pure_pursuit_front_end_takes_the_world_map():
    from kompass_core.control import PurePursuit, PurePursuitConfig
    from kompass_core.models import RobotState

    cls = room_cls()
    cls[14:17, 28:32] = ref.OCCUPIED          # x 0.35 .. 0.55, y -0.15 .. 0.15: across the path, the search must act
    wm = _front_end_world(cls)
    robot = _robot()
    a, b, free = (PurePursuit(robot, _limits(), config=PurePursuitConfig(wheel_base=robot.wheelbase, lookahead_distance=0.4),
                              control_time_step=0.1) for _ in range(3))
    for c in (a, b, free):
        c.set_path(PATH)
    state = RobotState(x=0.0, y=0.0, yaw=0.0, speed=0.0)
    differs = False
    for step in range(5):
        pts, n, _ = pref.worldmap_points_ref(cls, ROOM_RES, ROOM_ORIGIN, state.x, state.y, 10.0)
        assert n == int((cls == ref.OCCUPIED).sum())
        ok_a = a.loop_step(current_state=state, local_map=wm)
        ok_b = b.loop_step(current_state=state, point_cloud=pts)
        free.loop_step(current_state=state)
        assert ok_a == ok_b, step
        cmd = lambda c: (c.linear_x_control[0], c.linear_y_control[0], c.angular_control[0])   # noqa: E731
        assert cmd(a) == cmd(b), step
        differs = differs or cmd(a) != cmd(free)
        state.simulate(v_x=a.linear_x_control[0], v_y=a.linear_y_control[0], omega=a.angular_control[0], dt=0.1)
    assert differs, "the obstacles must change at least one command, or the map was not looked at"
