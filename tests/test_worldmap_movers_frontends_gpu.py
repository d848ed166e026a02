"""The closed loop on raw scans through the front ends: kompass_core.mapping.WorldMap.detect_movers -> MoverTracker ->
WorldMap.integrate_scan(skip=...) -> kompass_core.control.MPPI.loop_step(moving_obstacles=...), forty steps of the crossing
scene of DESIGN.md 4.12, against the statements tests/worldmap_movers_ref.py, tests/worldmap_integrate_ref.py and
tests/mppi_movers_ref.py driven with the same measured ranges and the same quantised inputs.

The scan is simulated: the static scene's ranges by the virtual scan's statement, shortened by the walker's disc of 2
cells; 360 beams, 60 cells of range."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import mppi_movers_ref as mm  # noqa: E402
import mppi_ref as mp  # noqa: E402
import worldmap_dist_ref as dref  # noqa: E402
import worldmap_integrate_ref as iref  # noqa: E402
import worldmap_movers_ref as wmr  # noqa: E402
import worldmap_ref as ref  # noqa: E402
import worldmap_scan_ref as sref  # noqa: E402

RES, ORIGIN, DT = 0.05, (-0.33, 1.7), 0.1
R32 = float(np.float32(RES))
BEAMS, RANGE_CELLS, WALKER_R = 360, 60, 2.0
ONE = 1 << 16


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def front_end(cfg):
    from kompass_core.control import MPPI
    from kompass_core.models import AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry, RobotType
    robot = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER, geometry_params=np.array([0.1, 0.4]))
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=1000.0, max_decel=1000.0),
                          omega_limits=AngularCtrlLimits(max_vel=1.5, max_steer=0.7, max_acc=1000.0, max_decel=1000.0))
    return MPPI(robot, lim, cfg, control_time_step=DT), robot, lim


def test_a_mover_at_a_known_cell_comes_back_there():
    """Three returns in the middle of cell (12, 8) of an open map: the front end's centre is that cell's centre in world
    metres, origin + 12 res, which MPPI's moversOf quantises to OX = 12 << 16 (4.12 rule 1); after a shift of the window
    the same world point is found again, from rule 46's origin."""
    from kompass_core.mapping import WorldMap
    wm = WorldMap(64, 16, RES, origin=ORIGIN)
    wm.set_prior(np.full((64, 16), ref.EMPTY, np.int8))
    wm.enable_distance(reach_cells=3)
    at = lambda i, j: (ORIGIN[0] + i * R32, ORIGIN[1] + j * R32)           # noqa: E731
    x, y = at(2, 8)
    for shift in ((0, 0), (3, -2)):
        if shift != (0, 0):
            wm.shift(*shift)
        det = wm.detect_movers((x, y, 0.0), [10 * R32] * 3, angles=[0.0, 0.0, 0.0], range_max=60 * R32)
        assert det.record == (3, 1, 1, 1) and det.labels.tolist() == [0, 0, 0]
        cx, cy, rad = det.clusters[0]
        wx, wy = at(12, 8)
        assert abs(cx - wx) <= 1e-9 and abs(cy - wy) <= 1e-9 and rad == 0.0
        ox, oy = wm.map_meta_data["origin_x"], wm.map_meta_data["origin_y"]
        assert round((cx - ox) / R32 * 65536.0) == (12 - shift[0]) << 16 and round((cy - oy) / R32 * 65536.0) == (8 - shift[1]) << 16


def test_integrate_scan_with_a_skip_mask():
    """A masked beam says nothing; no mask, an empty one and an all-false one are the call as it was."""
    from kompass_core.mapping import WorldMap
    cls = np.full((40, 30), ref.EMPTY, np.int8)
    angles = np.linspace(-1.0, 1.0, 21)
    ranges = np.full(21, 12 * R32)
    pose = (ORIGIN[0] + 10 * R32, ORIGIN[1] + 15 * R32, 0.2)
    planes = []
    for skip in (None, np.zeros(21, bool), np.arange(21) % 3 == 0):
        wm = WorldMap(40, 30, RES, origin=ORIGIN, hit=12)
        wm.set_prior(cls)
        want = iref.IntegrateRef(40, 30, RES, ORIGIN)
        want.set_model(hit=12)
        want.set_prior(cls)
        changed = wm.integrate_scan(pose, ranges, angles=angles, range_max=20 * R32, skip=skip)
        zq = wmr.quantise_ranges(ranges, RES, 20 * R32)
        if skip is not None:
            zq = wmr.apply_skip(zq, skip)
        _, w_changed, _ = want.integrate(pose, angles, zq, 20 * R32)
        assert changed == w_changed
        assert np.array_equal(wm.occupancy, want.cls) and np.array_equal(wm.evidence, want.evidence)
        planes.append(wm.occupancy)
    assert np.array_equal(planes[0], planes[1]) and not np.array_equal(planes[0], planes[2])
    with pytest.raises(ValueError):
        wm.integrate_scan(pose, ranges, angles=angles, range_max=20 * R32, skip=np.zeros(20, bool))


def test_forty_steps_of_the_crossing_scene_on_raw_scans():
    import kompass_cpp
    from kompass_core.control import MPPIConfig
    from kompass_core.mapping import MoverTracker, WorldMap
    from kompass_core.models import RobotState, RobotType
    static = mp.scene_cls()
    rmax = RANGE_CELLS * R32
    angles = -math.pi + np.arange(BEAMS) * (2 * math.pi / BEAMS)
    table = sref.scan_table(angles)
    # the front ends
    wm = WorldMap(mp.SCENE_W, mp.SCENE_H, RES, origin=ORIGIN)
    wm.set_prior(static)
    wm.enable_distance(reach_cells=mp.SCENE_REACH)
    tracker = MoverTracker()
    cfg = MPPIConfig(seed=3)
    fe, robot, lim = front_end(cfg)
    pts = [(ORIGIN[0] + x * R32, ORIGIN[1] + y * R32) for x, y in mp.SCENE_VERTICES]
    fe.set_path(np.array(pts))
    # the statements
    world = iref.IntegrateRef(mp.SCENE_W, mp.SCENE_H, RES, ORIGIN)
    world.set_prior(static)
    dist = dref.DistRef(world.cls, mp.SCENE_REACH)
    det_ref = wmr.MoversRef(world, dist)
    track_ref = wmr.MoverTracker(gate=wmr.GATE * R32)
    q = kompass_cpp.control.MPPI.quantise(RobotType.to_kompass_cpp_lib(robot.robot_type), lim.to_kompass_cpp_lib(), DT, RES,
                                          cfg.to_kompass_cpp())
    model, costs = mp.Model(*q[:5], tuple(q[5])), mp.scene_costs()
    state = RobotState(x=pts[0][0], y=pts[0][1], yaw=0.0, speed=0.0)
    prev, seen, tracked = None, 0, 0
    for n in range(40):
        pose = ref.quantise_pose(RES, ORIGIN, state.x, state.y, state.yaw)
        walker = (mm.CROSS_START[0] + n * mm.CROSS_V[0], mm.CROSS_START[1] + n * mm.CROSS_V[1], WALKER_R)
        ranges, _ = sref.scan_pose(static, RES, pose, table, rmax)
        ranges = wmr.shorten_by_discs(ranges, RES, pose, angles, [walker])
        zq = wmr.quantise_ranges(ranges, RES, rmax)
        # detect
        det = wm.detect_movers(state, ranges, angles=angles, range_max=rmax)
        w_labels, w_rec, w_clusters = det_ref.detect(pose, angles, zq, rmax)
        assert det.record == tuple(w_rec), n
        assert det.labels.tobytes() == w_labels.tobytes(), n
        assert det.raw == [tuple(c) for c in w_clusters], n
        w_world = [wmr.cluster_world(c, RES, ORIGIN) for c in w_clusters]
        assert np.allclose(det.clusters, np.array(w_world).reshape(-1, 3), rtol=0.0, atol=1e-12), n
        seen += int(w_rec.n_kept > 0)
        # track
        tracker.update(det, DT)
        track_ref.update(w_world, DT)
        movers = tracker.moving_obstacles()
        assert movers.shape == (len(track_ref.tracks), 5)
        assert np.allclose(movers, np.array(track_ref.moving_obstacles()).reshape(-1, 5), rtol=0.0, atol=1e-9), n
        assert [t.id for t in tracker.tracks] == [t.id for t in track_ref.tracks]
        tracked += len(movers)
        # integrate, the walker's beams kept out
        mask = tracker.skip_mask(det)
        assert np.array_equal(mask, wmr.skip_mask(w_labels))
        changed = wm.integrate_scan(state, ranges, angles=angles, range_max=rmax, skip=mask)
        _, w_changed, w_box = world.integrate(pose, angles, wmr.apply_skip(zq, mask), rmax)
        dist.mark(w_changed, w_box)
        assert changed == w_changed, n
        assert np.array_equal(wm.occupancy, world.cls) and np.array_equal(wm.evidence, world.evidence), n
        assert not ((np.asarray(world.cls) == ref.OCCUPIED) & (static != ref.OCCUPIED)).any(), n   # no phantom cell
        # control
        assert fe.loop_step(current_state=state, local_map=wm, moving_obstacles=movers)
        i = fe.planner.last_inputs
        mv = mm.Movers(*[tuple(int(a) for a in col) for col in i["movers"][:7]], int(i["movers"][7]))
        assert len(mv.ox) == len(movers)
        U = [tuple(i["u"][3 * k:3 * k + 3]) for k in range(cfg.horizon)]
        assert U == ([(0, 0, 0)] * cfg.horizon if prev is None else mp.shift(prev))
        wU, wrec, _ = mm.step(dist.field(), cfg.samples, cfg.seed, model, costs, i["px"], i["py"], i["tx"], i["ty"], i["h"], U, n, mv)
        got = list(fe.planner.last_sequence)
        prev = [tuple(got[3 * k:3 * k + 3]) for k in range(cfg.horizon)]
        assert prev == wU, n
        assert fe.record + (fe.n_hit_moving,) == tuple(wrec), (n, fe.record, fe.n_hit_moving, tuple(wrec))
        vx, om = fe.linear_x_control[0], fe.angular_control[0]
        state = RobotState(x=state.x + vx * math.cos(state.yaw) * DT, y=state.y + vx * math.sin(state.yaw) * DT,
                           yaw=state.yaw + om * DT, speed=vx)
    print("steps with a kept cluster:", seen, "mover rows handed to MPPI:", tracked)
    assert seen > 0 and tracked > 0                                        # the walker does come into view on the way
