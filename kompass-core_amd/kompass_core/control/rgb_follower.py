"""VisionRGBFollower front-end (reference: src/kompass_core/control/rgb_follower.py).
Same config fields, defaults and validators, constructor, loop_step and control getters; the planner is
`kompass_cpp.control.RGBFollower` (host logic only: a proportional law on one 2-D box)."""
from __future__ import annotations

import logging
from typing import List, Optional

import numpy as np
from attrs import asdict, define, field, validators

import kompass_cpp
from kompass_cpp.types import Bbox2D
from ..models import Robot, RobotCtrlLimits, RobotType


def _rng(lo, hi):
    return [validators.ge(lo), validators.le(hi)]


def _cpp_params(config, params) -> "kompass_cpp.configure.ConfigParameters":
    """Every scalar field goes to the C++ parameter set with its own type; None (target_distance) is -1."""
    d = {}
    for k, v in asdict(config).items():
        k = k.lstrip("_")
        if v is None:
            d[k] = -1.0
        elif isinstance(v, (bool, np.bool_)):
            d[k] = bool(v)
        elif isinstance(v, (int, np.integer)):
            d[k] = int(v)
        elif isinstance(v, (float, np.floating)):
            d[k] = float(v)
    params.from_dict(d)
    return params


@define
class VisionRGBFollowerConfig:
    control_time_step: float = field(default=0.1, validator=_rng(1e-4, 1e6))
    control_horizon: int = field(default=2, validator=_rng(1, 1000))
    buffer_size: int = field(default=1, validator=_rng(1, 10))
    tolerance: float = field(default=0.1, validator=_rng(1e-6, 1.0))
    target_distance: Optional[float] = field(default=None)
    target_wait_timeout: float = field(default=30.0, validator=_rng(0.0, 1e3))
    target_search_timeout: float = field(default=30.0, validator=_rng(0.0, 1e3))
    target_search_pause: float = field(default=2.0, validator=_rng(0.0, 1e3))
    target_search_radius: float = field(default=0.5, validator=_rng(1e-4, 1e4))
    rotation_gain: float = field(default=1.0, validator=_rng(1e-9, 1.0))
    speed_gain: float = field(default=0.7, validator=_rng(1e-9, 10.0))
    min_vel: float = field(default=0.1, validator=_rng(1e-9, 1e9))
    enable_search: bool = field(default=True)
    camera_position_to_robot: np.ndarray = field(default=np.array([0.0, 0.0, 0.0], dtype=np.float32))
    camera_rotation_to_robot: np.ndarray = field(default=np.array([0.0, 0.0, 0.0, 1.0], dtype=np.float32))

    def to_kompass_cpp(self) -> "kompass_cpp.control.RGBFollowerParameters":
        return _cpp_params(self, kompass_cpp.control.RGBFollowerParameters())


class VisionRGBFollower:
    """Follows one 2-D box: its size against the reference size, its centre against the image centre."""

    def __init__(self, robot: Robot, ctrl_limits: RobotCtrlLimits, config: Optional[VisionRGBFollowerConfig] = None,
                 config_file: Optional[str] = None, config_root_name: Optional[str] = None, **_):
        self._config = config or VisionRGBFollowerConfig()
        if config_file:
            raise NotImplementedError("config files are not read by this build; pass a VisionRGBFollowerConfig")
        self.__controller = kompass_cpp.control.RGBFollower(
            control_type=RobotType.to_kompass_cpp_lib(robot.robot_type),
            control_limits=ctrl_limits.to_kompass_cpp_lib(),
            config=self._config.to_kompass_cpp(),
        )
        self._found_ctrl = False
        self._ctrl = None
        logging.info("VISION TARGET FOLLOWING CONTROLLER IS READY")

    def set_initial_tracking_2d_target(self, target_box: Bbox2D, **_) -> bool:
        self.__controller.reset_target(target_box)
        return True

    @property
    def dist_error(self) -> float:
        return float(self.__controller.get_errors()[0])

    @property
    def orientation_error(self) -> float:
        return float(self.__controller.get_errors()[1])

    def loop_step(self, *, detections_2d: Optional[List[Bbox2D]], **_) -> bool:
        self._found_ctrl = self.__controller.run(detections_2d[0] if detections_2d else None)
        if self._found_ctrl:
            self._ctrl = self.__controller.get_ctrl()
        return self._found_ctrl

    def logging_info(self) -> str:
        return f"Vision Object Follower found control: {self.linear_x_control}, {self.angular_control}"

    @property
    def linear_x_control(self):
        return self._ctrl.vx if self._found_ctrl else None

    @property
    def linear_y_control(self):
        return self._ctrl.vy if self._found_ctrl else None

    @property
    def angular_control(self):
        return self._ctrl.omega if self._found_ctrl else None
