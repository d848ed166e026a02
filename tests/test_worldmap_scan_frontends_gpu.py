"""The world map's virtual scan through the class level (DESIGN.md 4.11 rules 20 to 27): `mapping.WorldMap.scan` / `scans` /
`laser_scan` against the Python statement, `control.DVZ.loop_step(local_map=world_map)` and
`kompass_cpp.utils.CriticalZoneChecker.check(world_map, x, y, yaw, forward[, ranges])` on a wall that only the map
remembers, and the merge with the present scan."""
import json
import math
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import worldmap_ref as ref  # noqa: E402
import worldmap_scan_ref as sref  # noqa: E402

GOLD = Path(__file__).resolve().parent / "golden"
DT = 0.1
RES, ORIGIN = 0.05, (-2.5, -1.5)
W = H = 80
START = (-0.51731912, 0.0, math.pi / 2)      # the golden path's start, heading +y
RANGE_MAX = 3.0


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def wall_cls():
    """A wall across the path 12 cells (0.6 m) ahead of START, 21 cells wide; everything else observed empty"""
    cls = np.full((W, H), ref.EMPTY, np.int8)
    cls[30:51, 42] = ref.OCCUPIED
    return cls


def front_end_world(cls):
    from kompass_core.mapping import WorldMap

    wm = WorldMap(W, H, RES, ORIGIN)
    wm.set_prior(cls)
    return wm


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def test_front_end_scans_against_the_statement():
    from kompass_core.datatypes.laserscan import LaserScanData
    from kompass_core.models import RobotState

    cls = wall_cls()
    cls[60:, :] = ref.UNEXPLORED
    wm = front_end_world(cls)
    ang = np.arange(90) * (2 * math.pi / 90) + 0.01
    poses = [START, (0.3, 0.4, -1.0), (-1.2, 1.1, 2.5)]
    for unknown in (False, True):
        flags = sref.UNKNOWN_BLOCKS if unknown else 0
        want_r, want_c = sref.scan(cls, RES, ORIGIN, poses, ang, RANGE_MAX, flags)
        assert same(wm.scans(poses, ang, RANGE_MAX, unknown_blocks=unknown), want_r)
        for p, pose in enumerate(poses):
            state = RobotState(x=pose[0], y=pose[1], yaw=pose[2])
            assert same(wm.scan(state, ang, RANGE_MAX, unknown_blocks=unknown), want_r[p])
            r, c = wm.scan(pose, ang, RANGE_MAX, unknown_blocks=unknown, return_cells=True)
            assert same(r, want_r[p]) and same(c, want_c[p])
    assert (want_c >= 0).any() and (want_c < 0).any()
    scan = wm.laser_scan(RobotState(x=START[0], y=START[1], yaw=START[2]), range_max=RANGE_MAX)
    full = np.arange(360) * (2 * math.pi / 360)
    assert isinstance(scan, LaserScanData) and same(scan.angles, full) and scan.range_max == RANGE_MAX
    assert same(scan.ranges, sref.scan(cls, RES, ORIGIN, [START], full, RANGE_MAX)[0][0])
    for exc, call in [(ValueError, lambda: wm.scan(START, ang, 0.0)), (IndexError, lambda: wm.scan(START, ang, 500.0)),
                      (ValueError, lambda: wm.scan(START, [], 1.0)), (ValueError, lambda: wm.scan(START, [math.nan], 1.0)),
                      (IndexError, lambda: wm.scan((1e6, 0.0, 0.0), ang, 1.0)),
                      (IndexError, lambda: wm.scans([START] * 65, np.zeros(65536), 1.0))]:
        with pytest.raises(exc):
            call()
        assert same(wm.scan(START, ang, RANGE_MAX), sref.scan(cls, RES, ORIGIN, [START], ang, RANGE_MAX)[0][0])


# ---- DVZ --------------------------------------------------------------------------------------------------------------
def dvz_setup():
    from kompass_core.control import DVZ
    from kompass_core.models import (AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry,
                                     RobotType)
    robot = Robot(robot_type=RobotType.ACKERMANN, geometry_type=RobotGeometry.Type.CYLINDER,
                  geometry_params=np.array([0.1, 0.4]))
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=5.0, max_decel=10.0),
                          omega_limits=AngularCtrlLimits(max_vel=4.0, max_acc=3.0, max_decel=3.0, max_steer=np.pi))
    d = json.loads((GOLD / "global_path.json").read_text())
    path = np.array([[p["pose"]["position"]["x"], p["pose"]["position"]["y"]] for p in d["poses"]])
    robot.state.x, robot.state.y, robot.state.yaw = START
    dvz = DVZ(robot=robot, ctrl_limits=lim, control_time_step=DT)
    dvz.set_path(path)
    return dvz, robot


REFERENCE_CMD = np.array([[0.5, 0.0, 0.0]])   # the reference command of the step: 0.5 m/s straight on


def step_outputs(dvz):
    return dvz.zone.total_deformation, list(dvz.linear_x_control), list(dvz.angular_control)


def one_step(**kwargs):
    """A fresh controller's first step under REFERENCE_CMD -> (total deformation, linear x list, angular list)"""
    dvz, robot = dvz_setup()
    assert dvz.loop_step(current_state=robot.state, initial_control_seq=REFERENCE_CMD, **kwargs)
    return step_outputs(dvz)


def scan_data(obstacle_ahead=None):
    """A present scan in the robot's frame: clear, or with something `obstacle_ahead` metres in front"""
    from kompass_core.datatypes.laserscan import LaserScanData

    ang = np.arange(360) * (2 * math.pi / 360)
    r = np.full(360, RANGE_MAX)
    if obstacle_ahead is not None:
        r[(ang < 0.3) | (ang > 2 * math.pi - 0.3)] = obstacle_ahead
    return LaserScanData(ranges=r, angles=ang, range_max=RANGE_MAX)


def test_dvz_sees_a_wall_only_the_map_remembers():
    wm = front_end_world(wall_cls())
    clear = scan_data()
    without = one_step(laser_scan=clear)
    assert without == one_step(laser_scan=clear, local_map=None), "no map: the step is what it was"
    assert without[0] == 0.0
    with_map = one_step(laser_scan=clear, local_map=wm)
    assert with_map[0] > 0.0 and max(with_map[1]) < max(without[1])
    # the same through the class the front end holds, and without a present scan: 360 beams over [0, 2 pi)
    assert one_step(laser_scan=clear, local_map=wm._map) == with_map
    from_map_alone = one_step(local_map=wm)
    assert from_map_alone[0] > 0.0
    # the deformation is the zone's on the statement's ranges
    dvz, robot = dvz_setup()
    want = sref.scan(wall_cls(), RES, ORIGIN, [START], clear.angles, RANGE_MAX)[0][0]
    dvz.loop_step(current_state=robot.state, initial_control_seq=REFERENCE_CMD,
                  laser_scan=type(clear)(ranges=want, angles=clear.angles, range_max=RANGE_MAX))
    assert step_outputs(dvz) == with_map
    with pytest.raises(TypeError, match="laser_scan"):
        dvz.loop_step(current_state=robot.state)


def test_dvz_merges_the_present_scan_with_the_map():
    wall, empty = front_end_world(wall_cls()), front_end_world(np.full((W, H), ref.EMPTY, np.int8))
    present_only = one_step(laser_scan=scan_data(0.4), local_map=empty)
    assert present_only == one_step(laser_scan=scan_data(0.4)) and present_only[0] > 0.0
    map_only = one_step(laser_scan=scan_data(), local_map=wall)
    both = one_step(laser_scan=scan_data(0.4), local_map=wall)
    assert map_only[0] > 0.0 and both[0] >= present_only[0] and both[0] >= map_only[0] and both[0] > map_only[0]
    # the nearer of the two decides a beam: a present obstacle behind the wall changes nothing
    assert one_step(laser_scan=scan_data(2.0), local_map=wall)[0] >= map_only[0]
    ang = scan_data().angles
    v = sref.scan(wall_cls(), RES, ORIGIN, [START], ang, RANGE_MAX)[0][0]
    from kompass_core.mapping import WorldMap
    q = scan_data(0.4).ranges.copy()
    q[5], q[6] = math.nan, math.inf
    want = np.array([sref.merge(float(a), float(b)) for a, b in zip(q, v)])
    assert same(WorldMap.merge_scan(q, v), want)


# ---- CriticalZoneChecker ---------------------------------------------------------------------------------------------
def checker(cls_name="CriticalZoneChecker", pos=(0.0, 0.0, 0.0), rot=(0.0, 0.0, 0.0, 1.0), angles=None):
    import kompass_cpp.utils as ut
    from kompass_cpp.types import RobotGeometry

    angles = np.arange(360) * (2 * math.pi / 360) if angles is None else angles
    return getattr(ut, cls_name)(input_type=ut.CriticalZoneChecker.InputType.LASERSCAN, robot_shape=RobotGeometry.CYLINDER,
                                 robot_dimensions=[0.2, 0.4], sensor_position_body=np.array(pos, np.float32),
                                 sensor_rotation_body=np.array(rot, np.float32), critical_angle=160.0, critical_distance=0.4,
                                 slowdown_distance=1.0, scan_angles=list(angles), min_height=0.0, max_height=2.0,
                                 range_max=RANGE_MAX)


@pytest.mark.parametrize("cls_name", ["CriticalZoneChecker", "CriticalZoneCheckerGPU"])
def test_checker_stops_for_a_wall_only_the_map_remembers(cls_name):
    wall, empty = front_end_world(wall_cls()), front_end_world(np.full((W, H), ref.EMPTY, np.int8))
    c = checker(cls_name)
    clear = list(scan_data().ranges)
    assert c.check(ranges=clear, forward=True) == 1.0
    assert c.check(wall, *START, True) == 0.0                              # the face is 0.575 - 0.2 m from the hull
    assert c.check(wall._map, *START, True) == 0.0                         # the class itself
    assert c.check(wall, *START, False) == 1.0 and c.check(empty, *START, True) == 1.0
    # the merged form: an obstacle only in the present scan, only in the map, in both
    near, slow = list(scan_data(0.3).ranges), list(scan_data(0.9).ranges)
    assert c.check(empty, *START, True, near) == c.check(ranges=near, forward=True) == 0.0
    between = c.check(ranges=slow, forward=True)
    assert 0.0 < between < 1.0 and c.check(empty, *START, True, slow) == between
    assert c.check(wall, *START, True, clear) == 0.0
    assert c.check(wall, *START, True, near) == 0.0 and c.check(wall, *START, True, slow) == 0.0
    with pytest.raises(IndexError):
        c.check(wall, *START, True, clear[:100])
    with pytest.raises(IndexError):
        c.check(wall, 1e6, 0.0, 0.0, True)
    with pytest.raises(TypeError):
        c.check(object(), *START, True)
    assert c.check(wall, *START, True) == 0.0


def test_checker_composes_the_pose_with_the_planar_mount():
    cls = wall_cls()
    wall = front_end_world(cls)
    ang = np.arange(180) * (2 * math.pi / 180)
    pos, rot = (0.22, -0.1, 0.4), (0.0, 0.0, math.sin(0.35), math.cos(0.35))   # yawed by 0.7 rad
    c = checker(pos=pos, rot=rot, angles=ang)
    rot32 = np.float32(rot).astype(np.float64)
    pos32 = np.float32(pos).astype(np.float64)
    mount_yaw = 2.0 * math.atan2(rot32[2], rot32[3])
    with kh.ZoneContext(kh.CYLINDER, [0.2, 0.4], pos, rot, 160.0, 0.4, 1.0, ang, 0.0, 2.0, RANGE_MAX) as zone, \
            kh.WorldMapContext(W, H, RES, ORIGIN) as ctx:
        ctx.set_prior(cls)
        seen = set()
        for x, y, yaw in [START, (START[0], 0.1, math.pi / 2), (START[0], -0.3, 1.2), (START[0], 1.2, -math.pi / 2)]:
            cy, sy = math.cos(yaw), math.sin(yaw)
            frame = (x + cy * pos32[0] - sy * pos32[1], y + sy * pos32[0] + cy * pos32[1], yaw + mount_yaw)
            for forward in (True, False):
                got = c.check(wall, x, y, yaw, forward)
                assert got == zone.check_worldmap(ctx, frame, forward)
                assert got == zone.check(sref.scan(cls, RES, ORIGIN, [frame], ang, RANGE_MAX)[0][0], forward)
                seen.add(got)
        assert 0.0 in seen and 1.0 in seen
    tilted = checker(rot=(0.1, 0.0, 0.0, 0.99))
    with pytest.raises(ValueError, match="about z"):
        tilted.check(wall, *START, True)
    assert tilted.check(ranges=list(scan_data().ranges), forward=True) == 1.0
