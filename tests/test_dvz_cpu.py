"""Stanley and DVZ without a GPU: the restatement of tests/dvz_ref.py against the reference's literal expressions
(`** 2`, np.cos, sequential sums) -- the bound of the squares-as-products deviation --, closed forms of the zone,
the Stanley class (parameters and ranges of stanley.h, lock-step with the restated law on the reference test's
path, bit for bit), the front-end validators, and DvzContext's argument errors before any device use."""
import ctypes as C
import json
import math
from pathlib import Path

import numpy as np
import pytest

import dvz_ref as ref
import kompass_cpp
import kompass_hip as kh
from kompass_core.algorithms import DeformableVirtualZoneParams
from kompass_core.control import DVZConfig, Stanley, StanleyConfig
from kompass_core.models import AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry, RobotType

GOLD = Path(__file__).resolve().parent / "golden"
DT = 0.1


def _ulps(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


@pytest.mark.parametrize("n", [1, 2, 63, 360, 1440, 4096])
def test_restatement_against_the_literal_reference(n):
    rng = np.random.default_rng(n)
    for z in (ref.zone(0.2), ref.zone(0.25, 0.5, 1.2, 1.0, 0.6), ref.zone(0.1, 2.0, 0.8, 2.0, -0.5)):
        ang = rng.uniform(-math.pi, 2 * math.pi, n)
        r = rng.uniform(0.02, 2.5, n)
        got = ref.deform(z, ang, r)
        lit = ref.deform(z, ang, r, literal=True)
        assert _ulps(got[0], lit[0]).max() <= 2
        assert got[3] == lit[3]
        for k in (1, 2):
            assert got[k] == pytest.approx(lit[k], rel=1e-13, abs=0)


def test_closed_forms_of_the_zone():
    # at rest, side ratio 1: an ellipse of semi-axes (margin, 2 radius) centred 2/3 margin ahead of the robot
    for radius, margin in ((0.1, 1.0), (0.3, 0.7), (0.05, 2.5)):
        z = ref.zone(radius, 1.0, margin, 1.0, 0.0)
        major, minor, sx, _, _ = z
        assert (major, minor) == (margin, 2 * radius)
        assert ref.beam(z, 0.0, 99.0)[0] == pytest.approx(margin + 2 / 3 * margin, rel=1e-15)
        assert ref.beam(z, math.pi, 99.0)[0] == pytest.approx(margin - 2 / 3 * margin, rel=1e-12)
        # a scan outside the zone everywhere: no deformation
        ang = np.linspace(0, 2 * math.pi, 720, endpoint=False)
        radii, total, orient, count, _, _ = ref.deform(z, ang, np.full(720, 2 * margin + 1.0))
        assert (total, orient, count) == (0.0, 0.0, 0)
        und = np.array([ref.beam(z, a, 99.0)[0] for a in ang])
        assert np.array_equal(radii, und)


# ---------------------------------------------------------------- Stanley
RANGES = {  # stanley.h: name -> (default, lo, hi)
    "wheel_base": (0.3, 0.0001, 100.0),
    "heading_gain": (1.0, 0.0, 10.0),
    "cross_track_min_linear_vel": (0.05, 0.0, 10.0),
    "cross_track_gain": (10.0, 0.0, 50.0),
}


def test_stanley_parameters_and_ranges():
    cfg = kompass_cpp.control.StanleyParameters()
    assert isinstance(cfg, kompass_cpp.control.FollowerParameters)
    assert issubclass(kompass_cpp.control.Stanley, kompass_cpp.control.Follower)
    for name, (default, lo, hi) in RANGES.items():
        cfg.from_dict({name: float(lo)})
        cfg.from_dict({name: float(hi)})
        cfg.from_dict({name: float(default)})
        with pytest.raises(Exception):
            cfg.from_dict({name: lo - abs(lo) * 0.5 - 1e-3})
        with pytest.raises(Exception):
            cfg.from_dict({name: hi * 2})
    for m in ("compute_velocity_commands", "execute", "set_robot_wheelbase"):
        assert hasattr(kompass_cpp.control.Stanley, m)


def _limits():
    return RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=5.0, max_decel=10.0),
                           omega_limits=AngularCtrlLimits(max_vel=4.0, max_acc=3.0, max_decel=3.0, max_steer=np.pi))


def _path():
    d = json.loads((GOLD / "global_path.json").read_text())
    return np.array([[p["pose"]["position"]["x"], p["pose"]["position"]["y"], 0.0] for p in d["poses"]], np.float32)


def _planner(params, lim, wheel_base=None):
    st = kompass_cpp.control.Stanley(params)
    k = lim.to_kompass_cpp_lib()
    st.set_linear_ctr_limits(k.linear_x_limits, k.linear_y_limits)
    st.set_angular_ctr_limits(k.angular_limits)
    if wheel_base is not None:
        st.set_robot_wheelbase(wheel_base)
    st.set_current_path(kompass_cpp.types.Path(points=_path()))
    return st


@pytest.mark.parametrize("variant", ["default", "config", "wheelbase", "steer_limit"])
def test_stanley_lock_step_with_the_restatement(variant):
    lim = _limits()
    params = kompass_cpp.control.StanleyParameters()
    if variant == "config":
        # the reference's parameterised constructor hands its config to the Follower only: the gains stay
        params.from_dict({"cross_track_gain": 3.0, "heading_gain": 0.2, "wheel_base": 0.5})
    if variant == "steer_limit":
        lim.omega_limits.max_steer = 0.3
    wb = 0.34 if variant == "wheelbase" else None
    st = _planner(params, lim, wb)
    law = ref.StanleyLaw((1.0, 5.0, 10.0), (4.0, lim.omega_limits.max_steer, 3.0, 3.0),
                         wheel_base=wb if wb is not None else 1.0)
    x, y, yaw = -0.51731912, 0.0, math.pi / 2
    steps = 0
    for steps in range(150):
        st.set_current_state(x, y, yaw, 0.0)
        if st.is_goal_reached():
            break
        res = st.compute_velocity_commands(DT)
        assert res.status == kompass_cpp.control.FollowingStatus.COMMAND_FOUND
        t = st.get_tracked_target()
        want = law.step(t.crosstrack_error, t.heading_error, t.reverse, DT)
        v = res.velocity_command
        assert (v.vx, v.vy, v.omega, v.steer_ang) == want, (steps, (v.vx, v.vy, v.omega, v.steer_ang), want)
        got = (st.get_vx_cmd(), st.get_vy_cmd(), st.get_omega_cmd())
        assert got == ref.clamp_cmds(want, 1.0, 0.0, 4.0)
        x += got[0] * math.cos(yaw) * DT
        y += got[0] * math.sin(yaw) * DT
        yaw += got[2] * DT
    assert st.is_goal_reached(), steps


def test_stanley_front_end_matches_the_class():
    robot = Robot(robot_type=RobotType.ACKERMANN, geometry_type=RobotGeometry.Type.CYLINDER,
                  geometry_params=np.array([0.1, 0.4]))
    lim = _limits()
    fe = Stanley(robot=robot, ctrl_limits=lim, generate_reference=True)
    fe.set_path(_path()[:, :2])
    direct = _planner(StanleyConfig(wheel_base=robot.wheelbase).to_kompass_cpp(), lim)
    from kompass_core.models import RobotState
    state = RobotState(x=-0.51731912, y=0.0, yaw=math.pi / 2)
    for _ in range(100):
        ok = fe.loop_step(current_state=state)
        direct.set_current_state(state.x, state.y, state.yaw, state.speed)
        if direct.is_goal_reached():
            assert fe.reached_end() and (fe.linear_x_control, fe.angular_control) == ([0.0], [0.0])
            break
        assert ok
        direct.compute_velocity_commands(DT)
        assert (fe.linear_x_control, fe.linear_y_control, fe.angular_control) == (
            [direct.get_vx_cmd()], [direct.get_vy_cmd()], [direct.get_omega_cmd()])
        state.simulate(v_x=fe.linear_x_control[0], omega=fe.angular_control[0], dt=DT)
    assert fe.reached_end()


# ------------------------------------------------------------- front end
def test_front_end_defaults_and_validators():
    s = StanleyConfig()
    assert (s.control_time_step, s.wheel_base, s.heading_gain, s.cross_track_min_linear_vel, s.cross_track_gain,
            s.max_angle_error, s.max_distance_error, s.min_angular_vel) == (0.1, 0.266, 0.7, 0.05, 1.5, np.pi / 16,
                                                                           0.1, 0.01)
    d = DVZConfig()
    assert (d.min_front_margin, d.K_linear, d.K_angular, d.K_I, d.side_margin_width_ratio, d.heading_gain,
            d.cross_track_gain) == (1.0, 1.0, 1.0, 5.0, 1.0, 1.0, 2.0)
    assert isinstance(d, DeformableVirtualZoneParams)
    for cls, bad in ((StanleyConfig, dict(control_time_step=0.0)), (StanleyConfig, dict(wheel_base=2e3)),
                     (StanleyConfig, dict(heading_gain=-0.1)), (StanleyConfig, dict(cross_track_min_linear_vel=0.0)),
                     (StanleyConfig, dict(cross_track_gain=101.0)), (StanleyConfig, dict(max_angle_error=4.0)),
                     (StanleyConfig, dict(max_distance_error=0.0)), (StanleyConfig, dict(min_angular_vel=-1.0)),
                     (DVZConfig, dict(min_front_margin=-0.1)), (DVZConfig, dict(K_linear=0.05)),
                     (DVZConfig, dict(K_angular=11.0)), (DVZConfig, dict(K_I=0.0)),
                     (DVZConfig, dict(side_margin_width_ratio=0.001)), (DVZConfig, dict(heading_gain=101.0)),
                     (DVZConfig, dict(cross_track_gain=-1.0))):
        with pytest.raises(ValueError):
            cls(**bad)
    assert isinstance(s.to_kompass_cpp(), kompass_cpp.control.StanleyParameters)


def test_dvz_context_argument_errors_before_device_use():
    with pytest.raises(ValueError):
        kh.DvzContext(0)
    with pytest.raises(ValueError):
        kh.DvzContext(-5)
    with pytest.raises(IndexError):
        kh.DvzContext(2**25)
    out = (C.c_double * 3)()
    a = np.zeros(4)
    zone = kh.DvzZone(1.0, 0.2, -0.6, 0.0, 0.0)
    assert kh.lib().kc_dvz_deform(None, C.byref(zone), a.ctypes.data_as(C.POINTER(C.c_double)),
                                  a.ctypes.data_as(C.POINTER(C.c_double)), 4, out, None) == kh.KC_OK - 1
    if kh.device_count() == 0:  # no device: an error, never a CPU fallback
        with pytest.raises(kh.KompassHipError):
            kh.DvzContext(360)
