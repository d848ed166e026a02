"""Stanley front-end (reference: src/kompass_core/control/stanley.py).
Same config fields, defaults and validators, constructor, loop_step and control getters; the planner is
`kompass_cpp.control.Stanley` (host logic only).  `generate_reference=True` is the mode the DVZ controller uses:
one command per step, zero once the end is reached."""
from __future__ import annotations

import logging
from typing import List, Optional

import numpy as np
from attrs import asdict, define, field, validators

import kompass_cpp
from ..models import Robot, RobotCtrlLimits, RobotState, RobotType
from ._base_ import FollowerConfig, FollowerTemplate


def _rng(lo, hi):
    return [validators.ge(lo), validators.le(hi)]


@define
class StanleyConfig(FollowerConfig):
    control_time_step: float = field(default=0.1, validator=_rng(1e-6, 1e3))
    wheel_base: float = field(default=0.266, validator=_rng(1e-3, 1e3))
    heading_gain: float = field(default=0.7, validator=_rng(0.0, 1e2))
    cross_track_min_linear_vel: float = field(default=0.05, validator=_rng(1e-4, 1e2))
    cross_track_gain: float = field(default=1.5, validator=_rng(0.0, 1e2))
    max_angle_error: float = field(default=np.pi / 16, validator=_rng(1e-9, np.pi))
    max_distance_error: float = field(default=0.1, validator=_rng(1e-9, 1e9))
    min_angular_vel: float = field(default=0.01, validator=_rng(0.0, 1e9))

    def to_kompass_cpp(self) -> "kompass_cpp.control.StanleyParameters":
        """Every scalar field goes to the C++ parameter set (its from_dict keeps the names it knows)."""
        cfg = kompass_cpp.control.StanleyParameters()
        d = {}
        for k, v in asdict(self).items():
            if isinstance(v, (bool, np.bool_)):
                d[k] = bool(v)
            elif isinstance(v, (int, float, np.integer, np.floating)):
                d[k] = float(v)
        cfg.from_dict(d)
        return cfg


class Stanley(FollowerTemplate):
    def __init__(self, robot: Robot, ctrl_limits: RobotCtrlLimits, config: Optional[StanleyConfig] = None,
                 config_file: Optional[str] = None, config_root_name: Optional[str] = None,
                 generate_reference: bool = False, **_):
        self.__generate_reference = generate_reference
        self._robot = robot
        if not config:
            config = StanleyConfig(wheel_base=robot.wheelbase)
        if config_file:
            raise NotImplementedError("config files are not read by this build; pass a StanleyConfig")
        self._config = config
        self._control_time_step = config.control_time_step
        self._got_path = False
        self._planner = kompass_cpp.control.Stanley(config.to_kompass_cpp())
        lim = ctrl_limits.to_kompass_cpp_lib()
        self._planner.set_linear_ctr_limits(lim.linear_x_limits, lim.linear_y_limits)
        self._planner.set_angular_ctr_limits(lim.angular_limits)
        self.__max_angular = ctrl_limits.omega_limits.max_vel
        self._result = kompass_cpp.control.FollowingResult()
        logging.info("STANLEY PATH CONTROLLER IS READY")

    @property
    def planner(self) -> "kompass_cpp.control.Follower":
        return self._planner

    def loop_step(self, *, current_state: RobotState, **_) -> bool:
        self._planner.set_current_state(current_state.x, current_state.y, current_state.yaw, current_state.speed)
        # the end is reached: no new command
        if self.reached_end():
            return True
        self._result = self._planner.compute_velocity_commands(self._control_time_step)
        return self._result.status == kompass_cpp.control.FollowingStatus.COMMAND_FOUND

    def logging_info(self) -> str:
        return f"Follower current status: {self._result.status}, Velocity command: {self._result.velocity_command}"

    def _rotate_first(self) -> bool:
        return self._robot.robot_type != RobotType.ACKERMANN and \
            abs(self._planner.get_omega_cmd()) > self._config.min_angular_vel

    def _in_place(self) -> bool:
        return abs(self.orientation_error) > self._config.max_angle_error and \
            abs(self.distance_error) < self._config.max_distance_error

    @property
    def linear_x_control(self) -> List[float]:
        if self.__generate_reference:
            return [self._planner.get_vx_cmd()] if not self.reached_end() else [0.0]
        if self._rotate_first():
            if self._in_place():
                return [0.0]
            return [0.0, self._planner.get_vx_cmd()]  # rotate, then move
        return [self._planner.get_vx_cmd()]

    @property
    def linear_y_control(self) -> List[float]:
        if self.__generate_reference:
            return [self._planner.get_vy_cmd()] if not self.reached_end() else [0.0]
        if self._rotate_first():
            if self._in_place():
                return [0.0]
            return [0.0, self._planner.get_vy_cmd()]
        return [self._planner.get_vy_cmd()]

    @property
    def angular_control(self) -> List[float]:
        if self.__generate_reference:
            return [self._planner.get_omega_cmd()] if not self.reached_end() else [0.0]
        if self._rotate_first():
            if self._in_place():
                return [self.in_place_rotation()]
            return [self._planner.get_omega_cmd(), 0.0]
        return [self._planner.get_omega_cmd()]

    def in_place_rotation(self) -> float:
        rotation_val = self.__max_angular * self.orientation_error / (self._control_time_step * 2 * np.pi)
        return min(max(rotation_val, -self.__max_angular), self.__max_angular)
