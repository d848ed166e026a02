"""PurePursuit surface without a GPU: the classes exist with the reference's parameters and ranges
(pure_pursuit.h:20-38, src/kompass_core/control/pure_pursuit.py), the front-end validators, geometry errors
before any device use, and the restatement's candidate order (pure_pursuit.cpp:163-212)."""
import numpy as np
import pytest

import kompass_cpp
from kompass_core.control import PurePursuit, PurePursuitConfig
from kompass_core.models import Robot, RobotCtrlLimits, LinearCtrlLimits, AngularCtrlLimits, RobotGeometry, RobotType
from pure_pursuit_ref import candidates, f32, search_offsets

RANGES = {  # name: (default, lo, hi, int)
    "wheel_base": (0.34, 0.0, 100.0, False),
    "prediction_horizon": (10, 0, 100, True),
    "lookahead_gain_forward": (0.8, 0.001, 10.0, False),
    "path_search_step": (0.2, 0.001, 1000.0, False),
    "max_search_candidates": (10, 2, 1000, True),
}


def test_cpp_classes_exist_and_take_the_reference_parameters():
    cfg = kompass_cpp.control.PurePursuitConfig()
    assert isinstance(cfg, kompass_cpp.control.FollowerParameters)
    assert issubclass(kompass_cpp.control.PurePursuit, kompass_cpp.control.Follower)
    for name, (default, lo, hi, is_int) in RANGES.items():
        cast = int if is_int else float
        cfg.from_dict({name: cast(lo)})
        cfg.from_dict({name: cast(hi)})
        cfg.from_dict({name: cast(default)})
        below = cast(lo - 1) if is_int else lo - abs(lo) * 0.5 - 1e-3
        with pytest.raises(Exception):
            cfg.from_dict({name: below})
        with pytest.raises(Exception):
            cfg.from_dict({name: cast(hi + 1) if is_int else hi * 2})
    doc = kompass_cpp.control.PurePursuit.__init__.__doc__
    for arg in ("control_type", "control_limits", "robot_shape_type", "robot_dimensions", "sensor_position_robot",
                "sensor_rotation_robot", "octree_res", "config"):
        assert arg in doc
    assert doc[doc.find("octree_res"):].split(",")[0].endswith("= 0.1")
    ex = kompass_cpp.control.PurePursuit.execute.__doc__
    for arg in ("current_position", "laser_scan", "point_cloud"):
        assert arg in ex


def test_front_end_config_defaults_and_validators():
    c = PurePursuitConfig()
    assert (c.wheel_base, c.lookahead_gain_forward, c.prediction_horizon, c.path_search_step,
            c.max_search_candidates) == (0.34, 0.8, 10, 0.2, 10)
    for bad in (dict(wheel_base=-0.1), dict(wheel_base=100.5), dict(lookahead_gain_forward=0.05),
                dict(lookahead_gain_forward=5.5), dict(prediction_horizon=-1), dict(prediction_horizon=101),
                dict(path_search_step=0.0005), dict(path_search_step=1001.0), dict(max_search_candidates=1),
                dict(max_search_candidates=1001)):
        with pytest.raises(ValueError):
            PurePursuitConfig(**bad)
    assert isinstance(c.to_kompass_cpp(), kompass_cpp.control.PurePursuitConfig)


def test_invalid_robot_shape_raises_before_device_use():
    # (a missing dimension is std::out_of_range in the reference's collision checker too: IndexError)
    with pytest.raises((ValueError, IndexError)):
        kompass_cpp.control.PurePursuit(
            control_type=kompass_cpp.control.ControlType.DIFFERENTIAL_DRIVE,
            control_limits=kompass_cpp.control.ControlLimitsParams(),
            robot_shape_type=kompass_cpp.types.RobotGeometry.BOX, robot_dimensions=[0.4],
            sensor_position_robot=[0, 0, 0], sensor_rotation_robot=[0, 0, 0, 1])
    robot = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER,
                  geometry_params=np.array([0.1, 0.4]))
    robot.geometry_params = np.array([0.1])  # (Robot validates at construction only)
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=2.0, max_decel=2.0),
                          omega_limits=AngularCtrlLimits(max_vel=1.0, max_steer=0.7, max_acc=2.0, max_decel=2.0))
    with pytest.raises(ValueError):
        PurePursuit(robot, lim)


def test_wheelbase_follows_the_reference_definition():
    r = Robot(robot_type=RobotType.OMNI, geometry_type=RobotGeometry.Type.BOX, geometry_params=np.array([0.6, 0.4, 0.3]))
    assert r.wheelbase == pytest.approx(0.4)
    r = Robot(robot_type=RobotType.OMNI, geometry_type=RobotGeometry.Type.CYLINDER, geometry_params=np.array([0.2, 0.4]))
    assert r.wheelbase == pytest.approx(0.2)


def test_candidate_enumeration_by_hand():
    offs = search_offsets(0.2, 3)  # rounded up to 4: +-0.2, +-0.6 (float values)
    assert offs == [f32(0.2), f32(-0.2), f32(0.6), f32(-0.6)]
    nom = (0.5, 0.1, 0.3)
    w = [0.3 + o for o in offs]
    diff = candidates(nom, offs, omni=False)
    assert diff == [nom] + [(0.5, 0.1, x) for x in w] + [(-0.5, 0.1, x) for x in w]
    omni = candidates(nom, offs, omni=True)
    vy = [0.1 + o for o in offs]
    want = [nom]
    for vx in (0.5, -0.5):
        prev_vy = 0.1  # the vy shift of the previous offset stays in the candidate
        for k in range(4):
            want += [(vx, prev_vy, w[k]), (vx, vy[k], 0.3)]
            prev_vy = vy[k]
    assert omni == want
    assert len(omni) == 1 + 4 * 4 and len(diff) == 1 + 2 * 4
