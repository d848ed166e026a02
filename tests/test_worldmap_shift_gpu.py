"""The rolling window on the device (kc_worldmap_shift and its kin, DESIGN.md 4.11 rules 46 to 51) against the numpy
statement tests/worldmap_shift_ref.py, bit for bit: the planes, the origin and the offset after every shift, the device
pointers, every consumer of the map at the new origin through the C ABI, the C++ class and the Python front end, the
distance plane, the localiser's particles, the planner's bounds, and a window that follows a robot off its first
rectangle.

The map is 70 x 45: wider than the 64 lanes of a workgroup row, neither side a multiple of 4, a last partial row group."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_cpp  # noqa: E402
import kompass_hip as kh  # noqa: E402
import worldmap_dist_ref as dref  # noqa: E402
import worldmap_match_ref as mtref  # noqa: E402
import worldmap_mcl_field_ref as fref  # noqa: E402
import worldmap_mcl_ref as mref  # noqa: E402
import worldmap_points_ref as pref  # noqa: E402
import worldmap_ref as ref  # noqa: E402
import worldmap_scan_ref as scref  # noqa: E402
import worldmap_shift_ref as sref  # noqa: E402

RES, ORIGIN = 0.05, (-0.33, 1.7)
R = float(np.float32(RES))
W, H = 70, 45
SHIFTS = [(1, 0), (-1, 0), (0, 1), (0, -1), (3, -2), (63, 7), (64, 0), (69, 0), (70, 0), (-75, 46), (0, 0)]
NO_BOX = (-1, -1, -1, -1)
ANGLES = np.arange(24) * (2 * math.pi / 24) + 0.02


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def local_grids(origin=ORIGIN, n=3):
    """Three seeded local grids and the world poses they are fused at."""
    rng = np.random.default_rng(3)
    out = []
    for k in range(n):
        g = rng.choice(np.int32([-1, 0, 100, 50]), size=(31, 27), p=[0.2, 0.45, 0.3, 0.05]).astype(np.int32)
        out.append((g, (origin[0] + (20 + 12 * k) * R, origin[1] + (18 + 4 * k) * R, 0.4 * k)))
    return out


GRIDS = local_grids()


def statement():
    """The 70 x 45 statement in the mixed state: evidence strictly between e_min and e_max."""
    want = sref.RollingWorldMapRef(W, H, RES, ORIGIN)
    for g, pose in GRIDS:
        want.update(g, pose)
    e = want.evidence
    assert ((e > -8) & (e < 14) & (e != ref.NEVER)).sum() > 200 and (want.cls == ref.OCCUPIED).sum() > 100
    return want


def ct_pair():
    """A C ABI context in the mixed state and its statement."""
    ctx, want = kh.WorldMapContext(W, H, RES, ORIGIN), statement()
    for g, pose in GRIDS:
        ctx.update(g, pose)
    return ctx, want


def ct_same(ctx, want):
    cls, ev = ctx.planes()
    np.testing.assert_array_equal(ev, want.evidence)
    np.testing.assert_array_equal(cls, want.cls)
    assert ctx.info() == (want.W, want.H, np.float32(RES), want.origin)       # the very doubles of rule 46
    assert ctx.offset() == want.offset and ctx.origin == want.origin


# ---- planes ----
@pytest.mark.parametrize("d", SHIFTS)
def test_each_shift_on_a_fresh_copy(d):
    ctx, want = ct_pair()
    with ctx:
        ct_same(ctx, want)
        ctx.shift(*d)
        want.shift(*d)
        ct_same(ctx, want)
        if abs(d[0]) >= W or abs(d[1]) >= H:
            assert (want.evidence == ref.NEVER).all()                          # a clear at the new offset
        g, pose = GRIDS[1]                                                     # the map goes on at the new origin
        assert ctx.update(g, pose) == want.update(g, pose)
        ct_same(ctx, want)


def test_six_shifts_in_a_row_and_the_offset_cap():
    ctx, want = ct_pair()
    with ctx:
        for k, d in enumerate(SHIFTS[:6]):
            ctx.shift(*d)
            want.shift(*d)
            ct_same(ctx, want)
            if k == 2:
                g, pose = GRIDS[0]
                assert ctx.update(g, pose) == want.update(g, pose)
        assert want.offset == (66, 5)
        for d in [(sref.MAX_SHIFT - 65, 0), (0, -sref.MAX_SHIFT - 6), (2 ** 31 - 1, 0)]:
            with pytest.raises(IndexError):
                ctx.shift(*d)
            ct_same(ctx, want)                                                 # a refusal leaves the state untouched
        ctx.shift(-66, -5)                                                     # back: the origin given, not a sum
        want.shift(-66, -5)
        assert ctx.origin == ORIGIN
        ct_same(ctx, want)


def class_pairs():
    """The C++ class and the Python front end in the mixed state, as (name, map, getters) with one statement each."""
    from kompass_core.mapping import WorldMap
    from kompass_core.models import RobotState

    cpp = kompass_cpp.mapping.WorldMap(width=W, height=H, resolution=RES, origin_x=ORIGIN[0], origin_y=ORIGIN[1])
    fe = WorldMap(W, H, RES, ORIGIN)
    for g, (x, y, yaw) in GRIDS:
        assert cpp.update(g, x, y, yaw) == fe.update(RobotState(x=x, y=y, yaw=yaw), g) > 0
    return cpp, fe


def test_classes_report_origin_offset_and_no_changed_cells():
    cpp, fe = class_pairs()
    want = statement()
    assert cpp.get_changed() > 0 and fe.changed > 0
    for d in SHIFTS[:6] + [(0, 0), (70, 0)]:
        cpp.shift(*d)
        fe.shift(*d)
        want.shift(*d)
        for cls, ev, origin, offset, changed, box in [
                (cpp.get_cls(), cpp.get_evidence(), cpp.origin, cpp.offset(), cpp.get_changed(), cpp.get_changed_box()),
                (fe.occupancy, fe.evidence, (fe.map_meta_data["origin_x"], fe.map_meta_data["origin_y"]), fe.offset, fe.changed,
                 fe.changed_box)]:
            np.testing.assert_array_equal(ev, want.evidence)
            np.testing.assert_array_equal(cls, want.cls)
            assert tuple(origin) == want.origin and tuple(offset) == want.offset
            assert (changed, tuple(box)) == (0, NO_BOX) == want.last
        if d == (3, -2):                                                       # an update in between: changed() counts again
            g, (x, y, yaw) = GRIDS[2]
            n, box = want.update(g, (x, y, yaw))
            assert cpp.update(g, x, y, yaw) == n > 0 and tuple(cpp.get_changed_box()) == box
            fe._map.update(g, x, y, yaw)
    with pytest.raises(IndexError):
        cpp.shift(2 ** 30, 0)
    assert tuple(cpp.offset()) == want.offset


def test_a_map_of_more_cells_than_one_grid_of_workgroups_strides_over():
    """2100 x 300 = 630 000 cells: more than kWmMaxBlocks (2048) workgroups of 256 lanes hold at a lane a cell."""
    rng = np.random.default_rng(9)
    prior = rng.choice(np.int8([-1, 0, 100]), size=(2100, 300), p=[0.3, 0.5, 0.2]).astype(np.int8)
    g = rng.choice(np.int32([-1, 0, 100]), size=(200, 180)).astype(np.int32)
    with kh.WorldMapContext(2100, 300, RES, ORIGIN) as ctx:
        want = sref.RollingWorldMapRef(2100, 300, RES, ORIGIN)
        ctx.set_prior(prior)
        want.map.set_prior(prior)
        pose = (ORIGIN[0] + 1000 * R, ORIGIN[1] + 150 * R, 0.3)
        assert ctx.update(g, pose) == want.update(g, pose)
        ctx.shift(-17, 5)
        want.shift(-17, 5)
        ct_same(ctx, want)
        assert (want.cls[:17] == ref.UNEXPLORED).all() and (want.cls[:, 295:] == ref.UNEXPLORED).all()


# ---- pointers ----
def test_pointers_survive_a_shift():
    """kc_worldmap_grid_device and kc_worldmap_distance_device give the addresses they gave before the shift, and the
    shifted content lies there: a planner that holds the address from before the shift (it classifies the plane when it is
    handed the address) plans on the shifted map, and the distance plane read through the old address is the new one."""
    from helpers import hip_runtime

    ctx, want = ct_pair()
    with ctx, kh.PlannerContext() as held, kh.PlannerContext() as fresh:
        ctx.set_distance(6)
        p_cls, p_dist = ctx.grid_device_ptr(), ctx.distance_device_ptr()
        ctx.shift(5, -3)
        want.shift(5, -3)
        assert (ctx.grid_device_ptr(), ctx.distance_device_ptr()) == (p_cls, p_dist)
        held.set_grid_device(p_cls, W, H, elem_bytes=1)
        fresh.set_grid(want.cls)
        free = np.argwhere(want.cls == ref.EMPTY)
        start, goal = tuple(int(v) for v in free[0]), tuple(int(v) for v in free[-1])
        assert held.solve(start, goal) == fresh.solve(start, goal)
        np.testing.assert_array_equal(held.path(), fresh.path())
        np.testing.assert_array_equal(held.field()[0], fresh.field()[0])
        rt = hip_runtime()
        got = np.empty((W, H), np.uint16, order="F")
        assert rt.hipMemcpy(got.ctypes.data, p_dist, got.nbytes, 2) == 0      # hipMemcpyDeviceToHost
        np.testing.assert_array_equal(got, want.distance(6))


# ---- consumers after a shift of (5, -3) ----
POSE = (ORIGIN[0] + 33.3 * R, ORIGIN[1] + 20.6 * R, 0.35)                   # a world pose, the same before and after
MATCH = dict(n_yaw=2, yaw_step=math.radians(1.5), reach=3)


def expected_after_shift():
    want = statement()
    want.shift(5, -3)
    pts, n, bounds = want.points(POSE[0], POSE[1], 1.0)
    assert 10 < n < (want.cls == ref.OCCUPIED).sum()
    ranges, cells = want.scan([POSE], ANGLES, 1.5)
    assert (cells[0] >= 0).sum() >= 6
    local = mtref.gather(want.map, (POSE[0] + 2 * R, POSE[1] - R, POSE[2] + math.radians(1.5)), 41, 37)
    m, _, corrected = mtref.match_pose(want.map, local, POSE, **MATCH)
    assert m.points > 20 and (m.k, m.u, m.v) != (0, 0, 0)
    return want, (pts, n, bounds), (ranges[0], cells[0]), local, m, corrected


def test_consumers_through_the_c_abi():
    want, (pts, n, bounds), (ranges, cells), local, m, _ = expected_after_shift()
    ctx, _ = ct_pair()
    with ctx:
        ctx.shift(5, -3)
        got, b = ctx.points(POSE[0], POSE[1], 1.0)
        np.testing.assert_array_equal(pref.sort_points(got, RES, want.origin), pts)
        assert b == bounds and ctx.points(POSE[0], POSE[1], 1.0, count_only=True) == (n, bounds)
        r, c = ctx.scan(POSE, ANGLES, 1.5, return_cells=True)
        np.testing.assert_array_equal(r, ranges)
        np.testing.assert_array_equal(c, cells)
        assert ctx.match(local, POSE, **MATCH) == m._asdict()
        g, pose = GRIDS[2]
        assert ctx.update(g, pose) == want.update(g, pose)
        ct_same(ctx, want)


def test_consumers_through_the_classes_and_the_controller():
    from kompass_core.models import RobotState

    want, (pts, n, bounds), (ranges, cells), local, m, corrected = expected_after_shift()
    cpp, fe = class_pairs()
    cpp.shift(5, -3)
    fe.shift(5, -3)
    state = RobotState(x=POSE[0], y=POSE[1], yaw=POSE[2])
    for got in (cpp.points(POSE[0], POSE[1], 1.0), fe.points(state, 1.0)):
        np.testing.assert_array_equal(pref.sort_points(got, RES, want.origin), pts)
    for r, c in (cpp.scan(*POSE, ANGLES, 1.5, False, True), fe.scan(state, ANGLES, 1.5, return_cells=True)):
        np.testing.assert_array_equal(r, ranges)
        np.testing.assert_array_equal(c, cells)
    for got in (cpp.match(local, *POSE, MATCH["n_yaw"], MATCH["yaw_step"], MATCH["reach"]), fe.match(state, local, **MATCH)):
        assert (got.k, got.u, got.v, got.score, got.score_guess, got.points, tuple(got.pose)) == tuple(m)
        assert (got.x, got.y, got.yaw) == corrected
    g, (x, y, yaw) = GRIDS[2]
    exp = want.update(g, (x, y, yaw))
    assert cpp.update(g, x, y, yaw) == exp[0] == fe.update(RobotState(x=x, y=y, yaw=yaw), g)
    assert tuple(cpp.get_changed_box()) == exp[1] == tuple(fe.changed_box)
    for cls, ev in ((cpp.get_cls(), cpp.get_evidence()), (fe.occupancy, fe.evidence)):
        np.testing.assert_array_equal(ev, want.evidence)
        np.testing.assert_array_equal(cls, want.cls)


def test_dwa_takes_its_obstacles_from_the_shifted_map():
    """DWA.loop_step(local_map=world_map) after a shift: its obstacle list is that of kc_worldmap_points, so its commands
    are those of a controller given the statement's list of the shifted planes at the new origin."""
    from kompass_core.control import DWA, DWAConfig
    from kompass_core.models import RobotState
    from test_worldmap_handoff_gpu import PATH, ROOM_ORIGIN, ROOM_RES, _front_end_world, _limits, _robot, room_cls

    cls = room_cls()
    wm = _front_end_world(cls)
    want = sref.RollingWorldMapRef(cls.shape[0], cls.shape[1], ROOM_RES, ROOM_ORIGIN)
    want.map.set_prior(cls)
    wm.shift(5, -3)
    want.shift(5, -3)
    np.testing.assert_array_equal(wm.occupancy, want.cls)
    cfg = dict(max_linear_samples=6, max_angular_samples=9, prediction_horizon=10, control_horizon=2, octree_resolution=0.1)
    a, b = (DWA(robot=_robot(), ctrl_limits=_limits(), config=DWAConfig(**cfg)) for _ in range(2))
    for c in (a, b):
        c.set_path(PATH)
        c.planner.set_sensor_max_range(2.0)
    state = RobotState(x=0.0, y=0.05, yaw=0.1, speed=0.0)
    for step in range(3):
        pts, n, _ = want.points(state.x, state.y, 2.0)
        assert 0 < n < int((want.cls == ref.OCCUPIED).sum())
        stale, _, _ = pref.worldmap_points_ref(want.cls, ROOM_RES, ROOM_ORIGIN, state.x, state.y, 2.0)
        assert not np.array_equal(stale, pts)                                  # a cached origin would show
        np.testing.assert_array_equal(pref.sort_points(wm.points(state, 2.0), ROOM_RES, want.origin), pts)
        assert a.loop_step(current_state=state, local_map=wm)
        assert b.loop_step(current_state=state, point_cloud=pts)
        for name in ("linear_x_control", "linear_y_control", "angular_control"):
            assert list(getattr(a, name)) == list(getattr(b, name)), (step, name)
        state.simulate(v_x=a.linear_x_control[0], v_y=a.linear_y_control[0], omega=a.angular_control[0], dt=0.1)


# ---- distance plane ----
@pytest.mark.parametrize("unknown_blocks", [False, True])
@pytest.mark.parametrize("reach", [6, 70])                                   # 70: above the tiled kernel's 63, the two-pass path
def test_distance_plane_after_shifts(reach, unknown_blocks):
    flags = dref.UNKNOWN_BLOCKS if unknown_blocks else 0
    ctx, want = ct_pair()
    with ctx:
        ctx.set_distance(reach, unknown_blocks=unknown_blocks)
        np.testing.assert_array_equal(ctx.distance(), want.distance(reach, flags))
        ctx.shift(5, -3)
        want.shift(5, -3)
        np.testing.assert_array_equal(ctx.distance(), want.distance(reach, flags))
        assert ctx.distance_info()[2:] == ((0, 0, W - 1, H - 1), True)        # rule 48: wholly dirty
        for k, d in enumerate([(-2, 4), (1, 1)]):                             # update -> shift -> update -> read
            g, pose = GRIDS[k]
            assert ctx.update(g, pose) == want.update(g, pose)
            ctx.shift(*d)
            want.shift(*d)
        g, pose = GRIDS[2]
        assert ctx.update(g, pose) == want.update(g, pose)
        np.testing.assert_array_equal(ctx.distance(), want.distance(reach, flags))
        ct_same(ctx, want)


# ---- localiser ----
ROOM_ORIGIN0 = (-1.0, 0.5)
N_PART, ROOM_REACH = 128, 4


@pytest.fixture(scope="module")
def room_scene():
    """The 120 x 90 room of the localiser's statement tests, its drive, and the true scans along it."""
    import test_worldmap_mcl_cpu as t

    cls = t.room()
    path = [(x + ROOM_ORIGIN0[0], y + ROOM_ORIGIN0[1], yaw) for x, y, yaw in t.drive(6)]
    table = scref.scan_table(ANGLES)
    scans = [scref.scan_pose(cls, t.ROOM_RES, ref.quantise_pose(t.ROOM_RES, ROOM_ORIGIN0, *p), table, t.ROOM_RANGE)[0] for p in path]
    return cls, path, scans, t.ROOM_RES, t.ROOM_RANGE


def mcl_scales(res, noise=(0.01, 0.005, 0.005)):
    cells = 65536.0 / float(np.float32(res))
    return (mref.noise_scale(noise[0] * cells), mref.noise_scale(noise[1] * cells), mref.noise_scale(noise[2] / (2 * math.pi) * 65536.0))


@pytest.mark.parametrize("model", ["beam", "field"])
def test_localiser_follows_the_window(room_scene, model):
    """6 steps, a shift of (4, -2) after step 3, a resample after step 4: states, acc, the record and the resampled states
    equal the statement with shift_particles applied at the same point.  Beam: the step is the first entry after the
    shift; field: kc_mcl_particles is."""
    cls, path, scans, res, range_max = room_scene
    rolling = sref.RollingWorldMapRef(cls.shape[0], cls.shape[1], res, ROOM_ORIGIN0)
    rolling.map.set_prior(cls)
    with kh.WorldMapContext(cls.shape[0], cls.shape[1], res, ROOM_ORIGIN0) as wm:
        wm.set_prior(cls)
        with kh.MclContext(wm, N_PART, ANGLES, range_max, 5) as dev:
            if model == "beam":
                want = mref.MclRef(rolling.cls, res, N_PART, ANGLES, range_max, 5)
                tables = mref.sensor_tables(res, 0.1)
                dev.set_model(*tables)
                want.set_model(*tables)
            else:
                wm.set_distance(ROOM_REACH)
                want = fref.MclFieldRef(rolling.cls, res, N_PART, ANGLES, range_max, 5,
                                        dist=dref.DistRef(rolling.cls, ROOM_REACH, 0))
                pen_d2, pen_far, _, wtab, w_shift = fref.field_tables(res, 0.1, reach=ROOM_REACH)
                dev.set_field_model(pen_d2, pen_far, wtab, w_shift)
                want.set_field_model(pen_d2, pen_far, wtab, w_shift)
            _, _, tx0, ty0 = ref.quantise_pose(res, ROOM_ORIGIN0, path[0][0] + 0.1, path[0][1] - 0.05, 0.0)
            cells = 65536.0 / float(np.float32(res))
            init = (tx0, ty0, mref.quantise_heading(path[0][2] + 0.03), mref.noise_scale(0.1 * cells),
                    mref.noise_scale(0.05 / (2 * math.pi) * 65536.0))
            dev.init_pose(*init)
            want.init_pose(*init)

            def same(what):
                for name, g, w in zip(("tx", "ty", "h", "acc"), dev.particles(), want.particles()):
                    assert g.dtype == w.dtype and np.array_equal(g, w), (model, what, name)

            for k in range(1, 7):
                args = (*mref.odometry_increment(res, path[k - 1], path[k]), *mcl_scales(res),
                        mref.quantise_ranges(scans[k], res, range_max))
                got, exp = dev.step(*args), want.step(*args)
                assert got.as_tuple() == exp.as_tuple(), (model, k)
                same(f"step {k}")
                if k == 3:
                    wm.shift(4, -2)
                    rolling.shift(4, -2)
                    want.cls = rolling.cls
                    if model == "field":
                        want.dist = dref.DistRef(rolling.cls, ROOM_REACH, 0)  # rule 48: wholly dirty
                        acc_before = want.particles()[3]
                    want.tx, want.ty = sref.shift_particles(want.tx, want.ty, 4, -2)
                    if model == "field":
                        same("right after the shift")
                        assert np.array_equal(dev.particles()[3], acc_before)
                if k == 4:
                    dev.resample()
                    want.resample()
                    same("resample")


def test_resample_and_device_pointers_apply_the_shift_first(room_scene):
    """The other two entries of rule 50 as the first after a shift: kc_mcl_resample, kc_mcl_particles_device."""
    from helpers import hip_runtime

    cls, path, scans, res, range_max = room_scene
    short = float(np.float32(float(np.float32(res)) * 6.5))
    n = 65
    with kh.WorldMapContext(cls.shape[0], cls.shape[1], res, ROOM_ORIGIN0) as wm:
        wm.set_prior(cls)
        with kh.MclContext(wm, n, ANGLES, short, 9) as dev:
            want = mref.MclRef(cls, res, n, ANGLES, short, 9)
            tables = mref.sensor_tables(res, 0.1)
            dev.set_model(*tables)
            want.set_model(*tables)
            init = (55 << 16, 22 << 16, 3000, mref.noise_scale(3 * 65536), mref.noise_scale(2000))
            dev.init_pose(*init)
            want.init_pose(*init)
            zq = mref.quantise_ranges(np.full(24, 0.2), res, short)
            assert dev.step(30000, 0, 100, 0, 0, 0, zq).as_tuple() == want.step(30000, 0, 100, 0, 0, 0, zq).as_tuple()
            wm.shift(-7, 3)
            want.tx, want.ty = sref.shift_particles(want.tx, want.ty, -7, 3)
            dev.resample()
            want.resample()
            wm.shift(2, 2)
            want.tx, want.ty = sref.shift_particles(want.tx, want.ty, 2, 2)
            rt = hip_runtime()
            ptx, pty, _, _ = dev.particles_device()
            gx, gy = np.empty(n, np.int64), np.empty(n, np.int64)
            assert rt.hipMemcpy(gx.ctypes.data, ptx, gx.nbytes, 2) == 0 and rt.hipMemcpy(gy.ctypes.data, pty, gy.nbytes, 2) == 0
            assert gx.tolist() == want.tx and gy.tolist() == want.ty
            for g, w in zip(dev.particles(), want.particles()):
                assert np.array_equal(g, w)


def test_front_end_estimate_across_a_shift(room_scene):
    """mapping.MCL reports world-frame poses from the current origin.  The bound is rule 46's rounding, not a chosen
    tolerance: with u = 2^-53, x = fl(fl(ox0 + fl(OI r)) + fl(t r)) carries at most u (|OI r| + |o| + |t r| + |x|), and the
    same cell count in the frame before the shift, fl(ox0 + fl((t + di) r)), at most u (|(t + di) r| + |x|): together below
    6 u M with M = |ox0| + (|OI| + |t| + |t + di|) r (t: the position in cells, exact in double)."""
    from kompass_core.mapping import MCL, WorldMap

    cls, path, scans, res, range_max = room_scene
    r = float(np.float32(res))
    fe_map = WorldMap(cls.shape[0], cls.shape[1], res, ROOM_ORIGIN0)
    fe_map.set_prior(cls)
    fe = MCL(fe_map, N_PART, ANGLES, range_max, sigma_hit=0.1, seed=5, motion_noise=(0.01, 0.005, 0.005), spread=False)
    fe.init(path[0], 0.1, 0.05)
    want = mref.MclRef(cls, res, N_PART, ANGLES, range_max, 5)
    want.set_model(*mref.sensor_tables(res, 0.1))
    _, _, tx0, ty0 = ref.quantise_pose(res, ROOM_ORIGIN0, path[0][0], path[0][1], 0.0)
    cells = 65536.0 / r
    want.init_pose(tx0, ty0, mref.quantise_heading(path[0][2]), mref.noise_scale(0.1 * cells), mref.noise_scale(0.05 / (2 * math.pi) * 65536.0))
    u = 2.0 ** -53

    def bound(o0, OI, t, d):
        return 6 * u * (abs(o0) + (abs(OI) + abs(t) + abs(t + d)) * r)

    x0, y0, yaw0, acc0 = fe.particles()
    fe_map.shift(4, -2)
    x1, y1, yaw1, acc1 = fe.particles()
    assert fe_map.offset == (4, -2) and np.array_equal(yaw0, yaw1) and np.array_equal(acc0, acc1)
    tx, ty = np.array(want.tx, np.float64) / 65536.0, np.array(want.ty, np.float64) / 65536.0
    assert (np.abs(x1 - x0) <= [bound(ROOM_ORIGIN0[0], 4, t - 4, 4) for t in tx]).all() and (x0 == ROOM_ORIGIN0[0] + tx * r).all()
    assert (np.abs(y1 - y0) <= [bound(ROOM_ORIGIN0[1], -2, t + 2, -2) for t in ty]).all()
    # a step on the shifted map: the statement on the shifted plane with shift_particles applied, its estimate's cell
    # counts taken back into the frame before the shift
    _, want.cls = sref.shift_planes(cls, cls, 4, -2)
    want.tx, want.ty = sref.shift_particles(want.tx, want.ty, 4, -2)
    rec = want.step(*mref.odometry_increment(res, path[0], path[1]), *mcl_scales(res), mref.quantise_ranges(scans[1], res, range_max))
    est = mref.estimate(rec, res, ROOM_ORIGIN0)
    e = fe.step(path[0], path[1], scans[1])
    assert tuple(e.record) == rec.as_tuple() and (e.txe, e.tye) == (est["txe"], est["tye"]) and e.yaw == est["yaw"]
    x_before = ROOM_ORIGIN0[0] + (e.txe + (4 << 16)) / 65536.0 * r
    y_before = ROOM_ORIGIN0[1] + (e.tye - (2 << 16)) / 65536.0 * r
    assert abs(e.x - x_before) <= bound(ROOM_ORIGIN0[0], 4, e.txe / 65536.0, 4)
    assert abs(e.y - y_before) <= bound(ROOM_ORIGIN0[1], -2, e.tye / 65536.0, -2)
    assert e.x == sref.origin_after(ROOM_ORIGIN0[0], res, 4) + e.txe / 65536.0 * r
    assert math.hypot(e.x - path[1][0], e.y - path[1][1]) < 0.3               # and it is where the robot is


# ---- planner ----
def planner_world():
    """70 x 45 at 0.1 m: free inside, a wall with a gap across the way, never-observed cells on the right."""
    cls = np.full((W, H), ref.EMPTY, np.int8)
    cls[0, :] = cls[:, 0] = cls[:, H - 1] = ref.OCCUPIED
    cls[35, 0:30] = ref.OCCUPIED
    cls[35, 12:16] = ref.EMPTY
    cls[60:, :] = ref.UNEXPLORED
    return cls


def test_planner_does_not_carry_its_field_across_a_shift():
    from kompass_core.mapping import WorldMap
    from kompass_core.planning import GridPlanner
    from test_planner_gpu import _robot

    res, origin = 0.1, (-1.0, 2.0)
    wm = WorldMap(W, H, res, origin)
    wm.set_prior(planner_world())
    start, goal = (origin[0] + 15.5 * 0.1, origin[1] + 30.5 * 0.1), (origin[0] + 50.5 * 0.1, origin[1] + 8.5 * 0.1)
    fe = GridPlanner(_robot())
    fe.setup_problem(None, start[0], start[1], 0.0, goal[0], goal[1], 0.0, grid=wm)
    first = fe.solve()
    assert first is not None and fe.replan(map=wm) is not None and fe.replanned   # no shift: the field is kept
    cells_before = np.asarray(fe.path_cells).copy()
    wm.shift(8, 0)
    path = fe.replan(map=wm)
    assert path is not None and not fe.replanned
    fresh = GridPlanner(_robot())
    fresh.setup_problem(wm.map_meta_data, start[0], start[1], 0.0, goal[0], goal[1], 0.0, grid=wm.occupancy)
    wpath = fresh.solve()
    assert wpath is not None and fe.status == fresh.status and fe.get_cost() == fresh.get_cost()
    np.testing.assert_array_equal(fe.path_cells, fresh.path_cells)
    np.testing.assert_array_equal(np.asarray(path.x()), np.asarray(wpath.x()))
    np.testing.assert_array_equal(np.asarray(path.y()), np.asarray(wpath.y()))
    assert np.asarray(fe.path_cells).reshape(-1, 2)[0, 0] == cells_before.reshape(-1, 2)[0, 0] - 8   # the same world start
    assert fe.replan(map=wm) is not None and fe.replanned                          # and from here on it is kept again
    # frontiers: the map's metadata is read again as well
    wm.shift(0, 3)
    rx, ry = start
    found = fe.find_frontiers(rx, ry, map=wm, min_size=3)
    again = GridPlanner(_robot()).find_frontiers(rx, ry, map=wm.occupancy, map_meta_data=wm.map_meta_data, min_size=3)
    assert found and found == again
    # the C++ class, a kompass_cpp.planning.GridPlanner: replan(world_map)
    inner = wm._map
    a = fe._planner
    a.setup_problem(start_x=start[0], start_y=start[1], start_yaw=0.0, goal_x=goal[0], goal_y=goal[1], goal_yaw=0.0)
    assert a.solve()
    inner.shift(-4, -3)
    assert a.replan(inner) and not a.replanned()
    fresh = GridPlanner(_robot())
    fresh.setup_problem(wm.map_meta_data, start[0], start[1], 0.0, goal[0], goal[1], 0.0, grid=wm.occupancy)
    assert fresh.solve() is not None
    np.testing.assert_array_equal(a.get_path_cells(False), fresh.path_cells)
    assert a.replan(inner) and a.replanned()


# ---- follow ----
def test_follow_rolls_the_window_off_its_first_rectangle():
    from kompass_core.mapping import WorldMap
    from kompass_core.models import RobotState

    wm = WorldMap(W, H, RES, ORIGIN)
    want = sref.RollingWorldMapRef(W, H, RES, ORIGIN)
    rng = np.random.default_rng(21)
    shifts = 0
    for k in range(60):
        g = rng.choice(np.int32([-1, 0, 100]), size=(21, 19), p=[0.2, 0.6, 0.2]).astype(np.int32)
        x, y, yaw = ORIGIN[0] + 0.5 + 0.15 * k, ORIGIN[1] + 1.0 + 0.01 * k, 0.05 * k
        before = want.offset
        n = wm.update(RobotState(x=x, y=y, yaw=yaw), g, follow=(10, 16))
        assert (n, wm.changed_box) == want.update(g, (x, y, yaw), follow=(10, 16)), k
        assert wm.offset == want.offset
        assert (wm.map_meta_data["origin_x"], wm.map_meta_data["origin_y"]) == want.origin
        shifts += want.offset != before
        np.testing.assert_array_equal(wm.evidence, want.evidence)
        np.testing.assert_array_equal(wm.occupancy, want.cls)
    assert shifts >= 8 and want.offset[0] >= W and want.offset[1] == 0       # off the original rectangle entirely
    with pytest.raises(ValueError):
        wm.update(RobotState(x=x, y=y, yaw=yaw), g, follow=(23, 16))         # 2 * margin >= min(W, H)
    assert wm.offset == want.offset
