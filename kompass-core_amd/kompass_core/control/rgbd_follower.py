"""VisionRGBDFollower front-end (reference: src/kompass_core/control/rgbd_follower.py).
Same config fields, defaults and validators, constructor, loop_step semantics and output properties; the planner
is `kompass_cpp.control.RGBDFollower`.  The depth frame may be a uint16 numpy array or a frame already on the
device (an object with `__cuda_array_interface__`, such as a torch ROCm tensor): it is read in place, after the
work queued on torch's current stream."""
from __future__ import annotations

import logging
from typing import List, Optional, Union

import numpy as np
from attrs import define, field

import kompass_cpp
from kompass_cpp.types import Bbox2D, TrajectoryPath, TrajectoryVelocities2D, Velocity2D
from ..models import Robot, RobotCtrlLimits, RobotGeometry, RobotState, RobotType
from ._base_ import FollowerConfig
from .rgb_follower import _cpp_params, _rng


@define
class VisionRGBDFollowerConfig(FollowerConfig):
    control_time_step: float = field(default=0.1, validator=_rng(1e-4, 1e6))
    control_horizon: int = field(default=2, validator=_rng(1, 1000))
    prediction_horizon: int = field(default=10, validator=_rng(1, 1000))
    buffer_size: int = field(default=1, validator=_rng(1, 10))
    target_distance: Optional[float] = field(default=None)
    target_wait_timeout: float = field(default=30.0, validator=_rng(0.0, 1e3))
    target_search_timeout: float = field(default=30.0, validator=_rng(0.0, 1e3))
    target_search_pause: float = field(default=2.0, validator=_rng(0.0, 1e3))
    target_search_radius: float = field(default=0.5, validator=_rng(1e-4, 1e4))
    enable_search: bool = field(default=True)
    distance_tolerance: float = field(default=0.05, validator=_rng(1e-6, 1e3))
    angle_tolerance: float = field(default=0.1, validator=_rng(1e-6, 1e3))
    target_orientation: float = field(default=0.0, validator=_rng(-np.pi, np.pi))
    rotation_gain: float = field(default=0.5, validator=_rng(1e-2, 10.0))
    speed_gain: float = field(default=1.0, validator=_rng(1e-2, 10.0))
    # track in the robot's frame (default) or in the world frame (False: loop_step needs current_state)
    _use_local_coordinates: bool = field(default=True, alias="_use_local_coordinates")
    error_pose: float = field(default=0.05, validator=_rng(1e-9, 1e9))
    error_vel: float = field(default=0.05, validator=_rng(1e-9, 1e9))
    error_acc: float = field(default=0.05, validator=_rng(1e-9, 1e9))
    depth_conversion_factor: float = field(default=1e-3, validator=_rng(1e-9, 1e9))
    min_depth: float = field(default=0.0, validator=_rng(0.0, 1e3))
    max_depth: float = field(default=1e3, validator=_rng(1e-3, 1e9))
    camera_position_to_robot: np.ndarray = field(default=np.array([0.0, 0.0, 0.0], dtype=np.float32))
    camera_rotation_to_robot: np.ndarray = field(default=np.array([0.0, 0.0, 0.0, 1.0], dtype=np.float32))

    def to_kompass_cpp(self) -> "kompass_cpp.control.RGBDFollowerParameters":
        """None (target_distance) becomes -1; `_use_local_coordinates` goes as `use_local_coordinates`."""
        return _cpp_params(self, kompass_cpp.control.RGBDFollowerParameters())


class _TorchFrame:
    """A torch device tensor's interface with the stream its producer queued on (torch writes none)."""

    def __init__(self, t):
        import torch

        if t.device.index not in (None, 0):
            raise ValueError(f"the depth frame is on {t.device}; the detector reads device 0 (cuda:0)")
        self._t = t
        s = torch.cuda.current_stream(t.device).cuda_stream
        self.__cuda_array_interface__ = dict(t.__cuda_array_interface__, stream=int(s) if s else 1)


def _frame(img):
    if img is not None and type(img).__module__.split(".")[0] == "torch" and \
            hasattr(img, "__cuda_array_interface__"):
        return _TorchFrame(img)
    return img


class VisionRGBDFollower:
    """Follows a target seen by an RGB-D camera: 2-D detections + an aligned depth frame -> 3-D boxes (one
    device launch per frame) -> tracker -> pursuit law over the prediction horizon; wait / search / give up when
    the target is lost."""

    def __init__(self, robot: Robot, ctrl_limits: RobotCtrlLimits, config: Optional[VisionRGBDFollowerConfig] = None,
                 config_file: Optional[str] = None, config_root_name: Optional[str] = None,
                 control_time_step: Optional[float] = None, camera_focal_length: Optional[List[float]] = None,
                 camera_principal_point: Optional[List[float]] = None, **_):
        self._config = config or VisionRGBDFollowerConfig()
        if config_file:
            raise NotImplementedError("config files are not read by this build; pass a VisionRGBDFollowerConfig")
        if control_time_step:
            self._config.control_time_step = control_time_step
        self._planner = kompass_cpp.control.RGBDFollower(
            control_type=RobotType.to_kompass_cpp_lib(robot.robot_type),
            control_limits=ctrl_limits.to_kompass_cpp_lib(),
            robot_shape_type=RobotGeometry.Type.to_kompass_cpp_lib(robot.geometry_type),
            robot_dimensions=[float(v) for v in np.asarray(robot.geometry_params).ravel()],
            vision_sensor_position_wrt_body=self._config.camera_position_to_robot,
            vision_sensor_rotation_wrt_body=self._config.camera_rotation_to_robot,
            config=self._config.to_kompass_cpp(),
        )
        if camera_focal_length is not None and camera_principal_point is not None:
            self._planner.set_camera_intrinsics(camera_focal_length[0], camera_focal_length[1],
                                                camera_principal_point[0], camera_principal_point[1])
        self._result = kompass_cpp.control.SamplingControlResult()
        self._end_of_ctrl_horizon: int = max(self._config.control_horizon, 1)
        logging.info("RGBDFollower CONTROLLER IS READY")

    @property
    def planner(self) -> "kompass_cpp.control.RGBDFollower":
        return self._planner

    def set_camera_intrinsics(self, fx: float, fy: float, cx: float, cy: float) -> None:
        self._planner.set_camera_intrinsics(fx, fy, cx, cy)

    def _global_state(self, current_state: Optional[RobotState]) -> None:
        if not self._config._use_local_coordinates:
            # global mode: the detector places the boxes with the robot's pose
            self._planner.set_current_state(current_state.x, current_state.y, current_state.yaw,
                                            current_state.speed)

    def set_initial_tracking_2d_target(self, current_state: RobotState, target_box: Bbox2D,
                                       aligned_depth_image) -> bool:
        try:
            self._global_state(current_state)
            return self._planner.set_initial_tracking(_frame(aligned_depth_image), target_box,
                                                      current_state.yaw if current_state else 0.0)
        except Exception as e:
            logging.error(f"Could not set initial tracking state: {e}")
            return False

    def set_initial_tracking_image(self, current_state: RobotState, pose_x_img: int, pose_y_img: int,
                                   detected_boxes: List[Bbox2D], aligned_depth_image) -> bool:
        try:
            self._global_state(current_state)
            if any(detected_boxes):
                return self._planner.set_initial_tracking(pose_x_img, pose_y_img, _frame(aligned_depth_image),
                                                          detected_boxes,
                                                          current_state.yaw if current_state else 0.0)
            logging.error("Could not set initial tracking state: No detections are provided")
            return False
        except Exception as e:
            logging.error(f"Could not set initial tracking state: {e}")
            return False

    @property
    def dist_error(self) -> float:
        return float(self._planner.get_errors()[0])

    @property
    def orientation_error(self) -> float:
        return float(self._planner.get_errors()[1])

    def loop_step(self, *, current_state: Optional[RobotState] = None, detections_2d: Optional[List[Bbox2D]] = None,
                  depth_image=None, **_) -> bool:
        """One step.  Global mode (`_use_local_coordinates=False`) needs `current_state`; errors are logged and
        False returned."""
        robot_cmd = None
        if not self._config._use_local_coordinates:
            if current_state is None:
                logging.error("Global mode (use_local_coordinates=False) requires current_state in loop_step")
                return False
            self._planner.set_current_state(current_state.x, current_state.y, current_state.yaw,
                                            current_state.speed)
            robot_cmd = Velocity2D(vx=current_state.vx, vy=current_state.vy, omega=current_state.omega)
        elif current_state is not None:
            robot_cmd = Velocity2D(vx=current_state.vx, vy=current_state.vy, omega=current_state.omega)
        try:
            self._result = self._planner.get_tracking_ctrl(_frame(depth_image), detections_2d,
                                                           robot_cmd or self._last_cmd)
        except Exception as e:
            logging.error(f"Could not find velocity command: {e}")
            return False
        return self._result.is_found

    def has_result(self) -> bool:
        return self._result.is_found

    def logging_info(self) -> str:
        if self._result.is_found:
            return f"RGBDFollower Controller found trajectory with cost: {self._result.cost}"
        return "RGBDFollower Controller Failed to find a valid trajectory"

    @property
    def control_till_horizon(self) -> Optional[TrajectoryVelocities2D]:
        if self._result.is_found:
            return self._result.trajectory.velocities
        return None

    def optimal_path(self) -> Optional[TrajectoryPath]:
        if not self._result.is_found:
            return None
        return self._result.trajectory.path

    @property
    def result_cost(self) -> Optional[float]:
        if self._result.is_found:
            return self._result.cost
        return None

    @property
    def linear_x_control(self) -> Union[List[float], np.ndarray]:
        if self._result.is_found:
            return self.control_till_horizon.vx[: self._end_of_ctrl_horizon]
        return [0.0]

    @property
    def linear_y_control(self) -> Union[List[float], np.ndarray]:
        if self._result.is_found:
            return self.control_till_horizon.vy[: self._end_of_ctrl_horizon]
        return [0.0]

    @property
    def angular_control(self) -> Union[List[float], np.ndarray]:
        if self._result.is_found:
            return self.control_till_horizon.omega[: self._end_of_ctrl_horizon]
        return [0.0]

    @property
    def _last_cmd(self) -> Velocity2D:
        vx, vy, om = self.linear_x_control, self.linear_y_control, self.angular_control
        # (a one-step control horizon holds no command: zeros)
        return Velocity2D(vx=float(vx[-1]) if len(vx) else 0.0, vy=float(vy[-1]) if len(vy) else 0.0,
                          omega=float(om[-1]) if len(om) else 0.0)
