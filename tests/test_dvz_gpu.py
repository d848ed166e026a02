"""DVZ on the MI355X: kc_dvz_deform (one launch) against the restatement of tests/dvz_ref.py -- per-beam deformed
radii bit for bit, the sums within the bound of a reordered double sum and bit-identical from call to call --; the
DVZ and Stanley controllers on the reference test's path (tests/test_controllers.py::test_dvz / test_stanley), and
DVZ's commands beside an obstacle against a CPU run of the restatement with the Stanley class."""
import json
import math
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dvz_ref as ref  # noqa: E402
import kompass_hip as kh  # noqa: E402

GOLD = Path(__file__).resolve().parent / "golden"
DT = 0.1


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same_float(got, want):
    return (got == want) or (math.isnan(got) and math.isnan(want))


def scene(kind, n, rng):
    """(angles, ranges) of a scan of n beams over a full turn."""
    ang = np.linspace(-math.pi, math.pi, n, endpoint=False) if n else np.empty(0)
    if kind == "room":  # a 4 x 3 room, the robot off its centre
        c, s = np.cos(ang), np.sin(ang)
        with np.errstate(divide="ignore"):
            tx = np.where(c > 0, (2.0 - 0.4) / c, np.where(c < 0, (-2.0 - 0.4) / c, np.inf))
            ty = np.where(s > 0, (1.5 + 0.2) / s, np.where(s < 0, (-1.5 + 0.2) / s, np.inf))
        r = np.minimum(tx, ty)
    elif kind == "corridor":  # walls 0.45 m to either side
        s = np.abs(np.sin(ang))
        with np.errstate(divide="ignore"):
            r = np.where(s > 1e-9, 0.45 / np.maximum(s, 1e-300), 30.0)
        r = np.minimum(r, 30.0)
    else:  # random clutter, angles not sorted
        ang = rng.uniform(-2 * math.pi, 4 * math.pi, n)
        r = rng.uniform(0.02, 3.0, n)
    return ang, r


ZONES = [ref.zone(0.2), ref.zone(0.25, 0.5, 1.2, 1.0, 0.6), ref.zone(0.1, 2.0, 0.8, 2.0, -0.5),
         ref.zone(0.3, 1.0, 0.3, 1.0, 0.0)]


def _check(ctx, z, ang, rng_):
    total, orient, count, radii = ctx.deform(z, ang, rng_, radii=True)
    want_r, wt, wo, wc, abs_t, abs_o = ref.deform(z, ang, rng_)
    assert np.array_equal(_bits(radii), _bits(want_r)), np.nonzero(_bits(radii) != _bits(want_r))[0][:10]
    assert count == wc
    n = len(ang)
    for got, want, bound in ((total, wt, abs_t), (orient, wo, abs_o)):
        if math.isfinite(want) and math.isfinite(bound):
            assert abs(got - want) <= n * 2.0**-52 * bound, (got, want, n)
        else:
            assert _same_float(got, want) or (math.isinf(bound) and not math.isfinite(got)), (got, want)
    # the same bits on every call, with and without the radii
    again = ctx.deform(z, ang, rng_)
    assert _bits([again[0], again[1]]).tolist() == _bits([total, orient]).tolist() and again[2] == count
    return total, count


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 360, 1440, 4096, 65536])
def test_deform_matches_the_restatement(n):
    rng = np.random.default_rng(n + 7)
    ctx = kh.DvzContext(max(n, 1))
    deformed = 0
    for kind in ("room", "corridor", "clutter"):
        ang, r = scene(kind, n, rng)
        for z in ZONES:
            _, c = _check(ctx, z, ang, r)
            deformed += c
    if n:
        assert deformed > 0
    else:
        assert ctx.deform(ZONES[0], [], []) == (0.0, 0.0, 0)
    ctx.close()


def test_non_finite_and_zero_ranges():
    rng = np.random.default_rng(3)
    ctx = kh.DvzContext(4096)
    for n in (64, 360, 4096):
        ang, r = scene("clutter", n, rng)
        r = r.copy()
        k = rng.permutation(n)
        r[k[: n // 8]] = np.nan
        r[k[n // 8: n // 4]] = np.inf
        r[k[n // 4: n // 4 + 3]] = -np.inf
        for z in ZONES:
            total, _ = _check(ctx, z, ang, r)
        # NaN / +inf: no deformation; the finite beams alone give the same record
        fin = np.isfinite(r)
        a2, r2 = ang.copy(), r.copy()
        r2[k[n // 4: n // 4 + 3]] = 50.0
        t_nan = ctx.deform(ZONES[0], a2, r2)
        t_fin = ctx.deform(ZONES[0], a2[fin], r2[fin])
        assert t_nan[2] == t_fin[2]
        # a zero range: the beam's term is +inf
        r3 = r2.copy()
        r3[k[0]] = 0.0
        t_zero, _, c_zero = ctx.deform(ZONES[0], a2, r3)
        assert t_zero == math.inf and c_zero == t_nan[2] + 1
        _check(ctx, ZONES[1], a2, r3)
    ctx.close()


def test_host_trig_beyond_the_device_range():
    # angles kc_trig_exact.h does not cover: the host's libm fills the cos / sin table; still bit-equal
    rng = np.random.default_rng(11)
    ctx = kh.DvzContext(1024)
    ang = rng.uniform(-1e9, 1e9, 1000)
    ang[::7] = rng.uniform(-3.0, 3.0, len(ang[::7]))
    r = rng.uniform(0.05, 2.0, 1000)
    for z in ZONES:
        _check(ctx, z, ang, r)
    ctx.close()


def test_argument_errors():
    ctx = kh.DvzContext(100)
    with pytest.raises(IndexError):
        ctx.deform(ZONES[0], np.zeros(101), np.ones(101))
    for bad in ((0.0, 0.4, -0.6, 0.0, 0.0), (1.0, -0.4, -0.6, 0.0, 0.0), (math.nan, 0.4, 0.0, 0.0, 0.0)):
        with pytest.raises(ValueError):
            ctx.deform(bad, np.zeros(10), np.ones(10))
    with pytest.raises(ValueError):
        ctx.deform(ZONES[0], np.zeros(10), np.ones(9))
    ctx.close()


# ------------------------------------------------------------------ controllers
def _setup():
    from kompass_core.models import (AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry,
                                     RobotType)
    robot = Robot(robot_type=RobotType.ACKERMANN, geometry_type=RobotGeometry.Type.CYLINDER,
                  geometry_params=np.array([0.1, 0.4]))
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=5.0, max_decel=10.0),
                          omega_limits=AngularCtrlLimits(max_vel=4.0, max_acc=3.0, max_decel=3.0, max_steer=np.pi))
    d = json.loads((GOLD / "global_path.json").read_text())
    path = np.array([[p["pose"]["position"]["x"], p["pose"]["position"]["y"]] for p in d["poses"]])
    robot.state.x, robot.state.y, robot.state.yaw = -0.51731912, 0.0, np.pi / 2
    return robot, lim, path


def run_control(controller, path, robot, scan, steps=100):
    """The reference test's loop: every command of the lists is applied for one time step."""
    controller.set_path(path)
    i, end_reached = 0, False
    while not end_reached and i < steps:
        ok = controller.loop_step(current_state=robot.state, laser_scan=scan)
        if not ok or not controller.path:
            end_reached = controller.reached_end()
            break
        for vx, vy, om in zip(controller.linear_x_control, controller.linear_y_control, controller.angular_control):
            robot.set_control(velocity_x=vx, velocity_y=vy, omega=om)
            robot.get_state(dt=DT)
            i += 1
            end_reached = controller.reached_end()
    return end_reached, i


def test_dvz_and_stanley_reach_the_end():
    from kompass_core.control import DVZ, Stanley, StanleyConfig
    from kompass_core.datatypes.laserscan import LaserScanData

    robot, lim, path = _setup()
    st = Stanley(robot=robot, ctrl_limits=lim, config=StanleyConfig(cross_track_gain=1.5, heading_gain=2.0))
    reached, steps = run_control(st, path, robot, LaserScanData())
    assert reached and steps <= 100, steps
    robot, lim, path = _setup()
    dvz = DVZ(robot=robot, ctrl_limits=lim, control_time_step=DT)
    reached, steps = run_control(dvz, path, robot, LaserScanData())
    assert reached and steps <= 100, steps
    assert dvz.zone.total_deformation == 0.0


def test_dvz_commands_beside_an_obstacle_match_the_restatement():
    from kompass_core.control import DVZ, Stanley, StanleyConfig
    from kompass_core.datatypes.laserscan import LaserScanData

    robot, lim, path = _setup()
    dvz = DVZ(robot=robot, ctrl_limits=lim, control_time_step=DT)
    dvz.set_path(path)
    # an obstacle ahead to the right of the robot, 0.5 - 0.7 m out, in the scan's frame every step
    ang = np.linspace(0.0, 2 * math.pi, 360, endpoint=False)
    r = np.full(360, 20.0)
    side = (ang > 5.6) & (ang < 6.2)
    r[side] = 0.5 + 0.2 * np.abs(np.sin(3 * ang[side]))
    scan = LaserScanData(ranges=r, angles=ang)
    # the CPU run: the Stanley class as DVZ's generator, the restated zone and laws
    gen = Stanley(robot=robot, ctrl_limits=lim, config=StanleyConfig(heading_gain=1.0, cross_track_gain=2.0),
                  generate_reference=True)
    gen.set_path(path)
    laws = ref.DvzLaws(1.0, 5.0, 4.0, 3.0)
    lin = 0.0
    seen = 0
    for step in range(100):
        state = robot.state
        ok = dvz.loop_step(current_state=state, laser_scan=scan, debug=(step % 10 == 0))
        assert ok
        if gen.loop_step(current_state=state):
            rl, ra = gen.linear_x_control[0], gen.angular_control[0]
        else:
            rl, ra = 0.0, 0.0
        z = ref.zone(robot.radius, 1.0, 1.0, 1.0, lin)
        radii, total, orient, count, _, _ = ref.deform(z, ang, r)
        laws.set_sums(total, orient, len(ang))
        lin = laws.linear(rl, lin, DT)
        w = laws.angular(ra)
        assert count > 0 and dvz.zone.total_deformation > 0.0
        seen += 1
        np.testing.assert_allclose([dvz.zone.total_deformation, dvz.zone.deformation_orientation],
                                   [laws.total, laws.orient], rtol=1e-12, atol=0)
        np.testing.assert_allclose(dvz._dvz_linear, lin, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(dvz._dvz_angular, w, rtol=1e-12, atol=1e-300)
        if step % 10 == 0:
            got = np.array([p[1] for p in dvz.zone.deformation_plot])
            assert np.array_equal(_bits(got), _bits(radii))
        # the output lists (rotate, then move), and the robot moves by them
        cmds = list(zip(dvz.linear_x_control, dvz.linear_y_control, dvz.angular_control))
        if abs(w) > 0.01:
            assert len(cmds) in (1, 2)
        for vx, vy, om in cmds:
            robot.set_control(velocity_x=vx, velocity_y=vy, omega=om)
            robot.get_state(dt=DT)
        if dvz.reached_end():
            break
    assert seen >= 10


def test_dvz_angles_from_the_scan_limits():
    from kompass_core.control import DVZ
    from kompass_core.datatypes.laserscan import LaserScanData

    robot, lim, path = _setup()
    dvz = DVZ(robot=robot, ctrl_limits=lim, control_time_step=DT)
    dvz.set_path(path)
    # no explicit angles: np.arange(angle_min, angle_max, angle_increment) into [0, 2 pi)
    scan = LaserScanData(angle_min=-math.pi, angle_max=math.pi, angle_increment=2 * math.pi / 720,
                         angles=np.zeros(720), ranges=np.linspace(0.2, 3.0, 720))
    scan.angles = np.zeros(720)
    dvz.loop_step(current_state=robot.state, laser_scan=scan, debug=True)
    ang = np.arange(-math.pi, math.pi, 2 * math.pi / 720) % (2 * math.pi)
    z = ref.zone(robot.radius, 1.0, 1.0, 1.0, 0.0)
    radii, total, orient, count, abs_t, _ = ref.deform(z, ang, scan.ranges)
    plot = dvz.zone.deformation_plot
    assert len(plot) == len(ang) and count > 0
    assert np.array_equal(_bits([p[0] for p in plot]), _bits(ang))
    assert np.array_equal(_bits([p[1] for p in plot]), _bits(radii[:len(plot)]))
    assert abs(dvz.zone.total_deformation * len(ang) - total) <= 2 * len(ang) * 2.0**-52 * abs_t
