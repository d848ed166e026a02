"""PurePursuit front-end (reference: src/kompass_core/control/pure_pursuit.py).
Same config fields, defaults and validators, constructor and loop_step
dispatch; the planner is `kompass_cpp.control.PurePursuit`, whose avoidance
search runs on the MI355X in one launch per step."""
from __future__ import annotations

import logging
from typing import List, Optional

import numpy as np
from attrs import asdict, define, field, validators

import kompass_cpp
from ..mapping.world_map import cpp_world_map
from ..models import Robot, RobotCtrlLimits, RobotGeometry, RobotState, RobotType
from ._base_ import FollowerConfig, FollowerTemplate


def _rng(lo, hi):
    return [validators.ge(lo), validators.le(hi)]


@define
class PurePursuitConfig(FollowerConfig):
    wheel_base: float = field(default=0.34, validator=_rng(0.0, 100.0))
    lookahead_gain_forward: float = field(default=0.8, validator=_rng(0.1, 5.0))
    # collision avoidance
    prediction_horizon: int = field(default=10, validator=_rng(0, 100))
    path_search_step: float = field(default=0.2, validator=_rng(0.001, 1000.0))
    max_search_candidates: int = field(default=10, validator=_rng(2, 1000))
    proximity_sensor_position_to_robot: np.ndarray = field(default=np.array([0.0, 0.0, 0.0], dtype=np.float32))
    proximity_sensor_rotation_to_robot: np.ndarray = field(default=np.array([0.0, 0.0, 0.0, 1.0], dtype=np.float32))

    def to_kompass_cpp(self) -> "kompass_cpp.control.PurePursuitConfig":
        """Every scalar field, the follower's included, goes to the C++ parameter set (its from_dict)."""
        cfg = kompass_cpp.control.PurePursuitConfig()
        ints = {"prediction_horizon", "max_search_candidates"}
        d = {}
        for k, v in asdict(self).items():
            if isinstance(v, (bool, np.bool_)):
                d[k] = bool(v)
            elif isinstance(v, (int, float, np.integer, np.floating)):
                d[k] = int(v) if k in ints else float(v)
        cfg.from_dict(d)
        return cfg


class PurePursuit(FollowerTemplate):
    def __init__(self, robot: Robot, ctrl_limits: RobotCtrlLimits, config: Optional[PurePursuitConfig] = None,
                 config_file: Optional[str] = None, config_root_name: Optional[str] = None,
                 control_time_step: float = 0.1, sensor_position: Optional[List[float]] = None,
                 sensor_rotation: Optional[List[float]] = None, octree_res: float = 0.1, **_):
        if not RobotGeometry.is_valid_parameters(robot.geometry_type, robot.geometry_params):
            raise ValueError(f"invalid geometry parameters {robot.geometry_params} for {robot.geometry_type}")
        self._robot = robot
        if config is None:
            config = PurePursuitConfig(wheel_base=robot.wheelbase)
        if config_file:
            raise NotImplementedError("config files are not read by this build; pass a PurePursuitConfig")
        # (the reference takes sensor_position / sensor_rotation and then uses the config's fields)
        self._config = config
        self._control_time_step = control_time_step
        self._got_path = False
        self._planner = kompass_cpp.control.PurePursuit(
            control_type=RobotType.to_kompass_cpp_lib(robot.robot_type),
            control_limits=ctrl_limits.to_kompass_cpp_lib(),
            robot_shape_type=RobotGeometry.Type.to_kompass_cpp_lib(robot.geometry_type),
            robot_dimensions=[float(v) for v in robot.geometry_params],
            sensor_position_robot=config.proximity_sensor_position_to_robot,
            sensor_rotation_robot=config.proximity_sensor_rotation_to_robot,
            octree_res=octree_res,
            config=config.to_kompass_cpp(),
        )
        self._result = None
        logging.info("PURE PURSUIT CONTROLLER IS READY")

    @property
    def planner(self) -> "kompass_cpp.control.Follower":
        return self._planner

    def loop_step(self, *, current_state: RobotState, **kwargs) -> bool:
        """One control step; sensor data (first given of local_map, laser_scan, point_cloud) turns the
        avoidance search on."""
        self._planner.set_current_state(current_state.x, current_state.y, current_state.yaw, current_state.speed)
        self._planner.set_current_velocity(
            kompass_cpp.types.Velocity2D(vx=current_state.vx, vy=current_state.vy, omega=current_state.omega))
        dt = self._control_time_step
        world_map = cpp_world_map(kwargs.get("local_map"))
        if world_map is not None:
            # not in the reference: the world map's occupied cells within sensor range, extracted on the device
            self._result = self._planner.execute(dt, world_map)
        elif kwargs.get("local_map") is not None:
            self._result = self._planner.execute(dt, np.asarray(kwargs["local_map"], dtype=np.float32))
        elif kwargs.get("laser_scan") is not None:
            scan = kwargs["laser_scan"]
            sensor = kompass_cpp.types.LaserScan(ranges=np.ascontiguousarray(scan.ranges, dtype=np.float64),
                                                 angles=np.ascontiguousarray(scan.angles, dtype=np.float64))
            self._result = self._planner.execute(dt, sensor)
        elif kwargs.get("point_cloud") is not None:
            cloud = kwargs["point_cloud"]
            self._result = self._planner.execute(dt, np.asarray(getattr(cloud, "data", cloud), dtype=np.float32))
        else:
            self._result = self._planner.execute(dt)
        return self._result.status in (kompass_cpp.control.FollowingStatus.COMMAND_FOUND,
                                       kompass_cpp.control.FollowingStatus.GOAL_REACHED)

    def logging_info(self) -> str:
        if self._result:
            v = self._result.velocity_command
            return f"Follower status: {self._result.status}, Cmd: vx={v.vx:.2f}, vy={v.vy:.2f}, w={v.omega:.2f}"
        return "Follower not started"

    @property
    def linear_x_control(self) -> List[float]:
        return [self._result.velocity_command.vx] if self._result else [0.0]

    @property
    def linear_y_control(self) -> List[float]:
        return [self._result.velocity_command.vy] if self._result else [0.0]

    @property
    def angular_control(self) -> List[float]:
        return [self._result.velocity_command.omega] if self._result else [0.0]
