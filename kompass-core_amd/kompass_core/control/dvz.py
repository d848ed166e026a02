"""DVZ front-end (reference: src/kompass_core/control/dvz.py): the Deformable Virtual Zone reactive controller.
A Stanley follower in `generate_reference` mode gives the path-tracking command; the zone's deformation by the
laser scan (one launch on the MI355X per step, kompass_core.algorithms.dvz) bends it away from obstacles."""
from __future__ import annotations

import logging
from typing import List, Optional

import numpy as np
from attrs import define, field, validators

import kompass_cpp
from ..algorithms import DeformableVirtualZone, DeformableVirtualZoneParams
from ..algorithms.dvz import _to_0_2pi
from ..datatypes.laserscan import LaserScanData
from ..mapping.world_map import WorldMap, cpp_world_map
from ..models import Robot, RobotCtrlLimits, RobotState
from ._base_ import FollowerTemplate
from .stanley import Stanley, StanleyConfig


@define
class DVZConfig(DeformableVirtualZoneParams):
    # gains of the internal Stanley generator
    heading_gain: float = field(default=1.0, validator=[validators.ge(0.0), validators.le(1e2)])
    cross_track_gain: float = field(default=2.0, validator=[validators.ge(0.0), validators.le(1e2)])


class DVZ(FollowerTemplate):
    """Deviation from the reference: `initial_control_seq` counts as given when it is not None (the reference
    tests its truth value, which raises for a numpy array).  As in the reference, the rotate-then-move output lists
    apply to every robot type: its type test compares the robot's type string with the enum member."""

    def __init__(self, robot: Robot, ctrl_limits: RobotCtrlLimits, control_time_step: float,
                 config_file: Optional[str] = None, config: Optional[DVZConfig] = None,
                 config_yaml_root_name: Optional[str] = None, **_):
        self._robot = robot
        self._control_time_step = control_time_step
        if not config:
            config = DVZConfig()
        if config_file:
            raise NotImplementedError("config files are not read by this build; pass a DVZConfig")
        self._config = config
        self._path_controller = DeformableVirtualZone(robot=robot, ctrl_limits=ctrl_limits, config=config)
        self._dvz_linear: float = 0.0
        self._dvz_angular: float = 0.0
        generator_config = StanleyConfig(heading_gain=config.heading_gain, cross_track_gain=config.cross_track_gain)
        self.__reference_cmd_generator = Stanley(robot=robot, ctrl_limits=ctrl_limits, config=generator_config,
                                                 generate_reference=True)
        logging.info("DVZ PATH CONTROLLER IS READY")
        self.rotating_in_place: bool = False

    @property
    def planner(self) -> "kompass_cpp.control.Follower":
        return self.__reference_cmd_generator.planner

    @property
    def zone(self) -> DeformableVirtualZone:
        """The zone and its last deformation (total_deformation, deformation_orientation, deformation_plot ...)."""
        return self._path_controller

    def reached_end(self) -> bool:
        return self.__reference_cmd_generator.reached_end()

    def interpolated_path(self) -> "kompass_cpp.types.Path":
        return self.__reference_cmd_generator.interpolated_path()

    @property
    def tracked_state(self) -> Optional[RobotState]:
        return self.__reference_cmd_generator.tracked_state

    def set_path(self, global_path, **_) -> None:
        self.__reference_cmd_generator.set_path(global_path=global_path)

    def loop_step(self, *, laser_scan: Optional[LaserScanData] = None, current_state: RobotState, local_map=None,
                  initial_control_seq: Optional[np.ndarray] = None, debug: bool = False, **_) -> bool:
        """local_map (not in the reference): a `WorldMap`; the zone is then deformed by the map's virtual scan at
        current_state (DESIGN.md 4.11 rules 20 to 27) over laser_scan's angles, or 360 beams over [0, 2 pi) without
        one, merged with laser_scan's ranges by a per-beam minimum when it has them.  Without local_map the step is
        the reference's and laser_scan is required."""
        world_map = cpp_world_map(local_map)
        if world_map is not None:
            laser_scan = self._scan_from_map(local_map, laser_scan, current_state)
        elif laser_scan is None:
            raise TypeError("DVZ.loop_step() missing 1 required keyword-only argument: 'laser_scan'")
        if initial_control_seq is not None:
            seq = np.asarray(initial_control_seq)
            ref_linear_x = seq[0, 0]
            ref_angular = seq[0, 2]  # (omni motion: not in DVZ, as in the reference)
        elif self.__reference_cmd_generator.loop_step(current_state=current_state):
            ref_linear_x = self.__reference_cmd_generator.linear_x_control[0]
            ref_angular = self.__reference_cmd_generator.angular_control[0]
        else:
            # no reference command: zero, and the zone still reacts
            ref_linear_x, ref_angular = 0.0, 0.0
        self._get_dvz_deformation(laser_scan, debug)
        self._dvz_linear = self._path_controller.compute_linear_control(ref_linear_x, self._dvz_linear,
                                                                        self._control_time_step)
        self._dvz_angular = self._path_controller.compute_angular_control(ref_angular)
        return True

    @staticmethod
    def _scan_from_map(local_map, laser_scan: Optional[LaserScanData], current_state: RobotState) -> LaserScanData:
        """The scan the zone sees with a world map: the map's ranges at current_state, under the present ones where
        those are nearer.  The ranges come to the host (`WorldMap.scan`) and go the usual way from there; the route
        that keeps them on the device is `kompass_hip.DvzContext.deform_worldmap`."""
        front = local_map if isinstance(local_map, WorldMap) else None
        if laser_scan is None:
            angles = np.arange(360) * (2 * np.pi / 360)
            range_max = LaserScanData().range_max
        else:
            if laser_scan.angles.any():
                angles = laser_scan.angles
            else:
                angles = _to_0_2pi(np.arange(laser_scan.angle_min, laser_scan.angle_max, laser_scan.angle_increment))
            range_max = laser_scan.range_max
        pose = (float(current_state.x), float(current_state.y), float(current_state.yaw))
        a = np.ascontiguousarray(angles, dtype=np.float64)
        ranges = front.scan(pose, a, range_max) if front is not None else cpp_world_map(local_map).scan(*pose, a, float(range_max))
        if laser_scan is not None and laser_scan.ranges.size == a.size:
            ranges = WorldMap.merge_scan(laser_scan.ranges, ranges)
        return LaserScanData(range_max=range_max, ranges=ranges, angles=a)

    def _get_dvz_deformation(self, laser_scan_data: LaserScanData, debug: bool = False) -> None:
        if laser_scan_data.angles.any():
            angles = laser_scan_data.angles
        else:
            angles = _to_0_2pi(np.arange(laser_scan_data.angle_min, laser_scan_data.angle_max,
                                         laser_scan_data.angle_increment))
        self._path_controller.update_zone_size(self._dvz_linear)
        self._path_controller.set_scan_values(scan_values=laser_scan_data.ranges, scan_angles=angles)
        self._path_controller.get_total_deformation(compute_deformation_plot=debug)

    def logging_info(self) -> str:
        return f"Total DVZ deformation : {self._path_controller.total_deformation}"

    def _rotate_first(self) -> bool:
        return abs(self._dvz_angular) > self.__reference_cmd_generator._config.min_angular_vel

    def _in_place(self) -> bool:
        cfg = self.__reference_cmd_generator._config
        return abs(self.orientation_error) > cfg.max_angle_error and abs(self.distance_error) < cfg.max_distance_error

    @property
    def linear_x_control(self) -> List[float]:
        if self._rotate_first():
            if self._in_place():
                return [0.0]
            return [0.0, self._dvz_linear]  # rotate, then move
        return [self._dvz_linear]

    @property
    def linear_y_control(self) -> List[float]:
        if self._rotate_first():
            if self._in_place():
                return [0.0]
            return [0.0, 0.0]
        return [0.0]

    @property
    def angular_control(self) -> List[float]:
        if self._rotate_first():
            if self._in_place():
                self.rotating_in_place = True
                return [self.__reference_cmd_generator.in_place_rotation()]
            self.rotating_in_place = False
            return [self._dvz_angular, 0.0]
        return [self._dvz_angular]
