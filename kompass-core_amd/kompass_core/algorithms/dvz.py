"""Deformable Virtual Zone (reference: src/kompass_core/algorithms/dvz.py; Lapierre, Zapata and Lepinay,
"Simultaneous Path Following and Obstacle Avoidance Control of a Unicycle-type Robot", ICRA 2007).

The zone is an ellipse around the robot that grows with its speed; a laser scan that reaches into it deforms it.
The per-beam part -- the zone's radius at every beam angle, the radius the scan leaves of it, the deformation and
its angle-weighted sum -- is one launch on the MI355X (`kompass_hip.DvzContext`, csrc/kc_dvz.hip).  The zone
constants, the normalisation of the sums and the two control laws are scalar host work, as in the reference.
Deliberate deviation: the reference's squares (`x ** 2`, libm pow) are products here."""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
from attrs import define, field, validators

import kompass_hip as kh
from ..models import Robot, RobotCtrlLimits

EPSILON_ANG = 0.01  # keeps the linear law's division away from zero


def _rng(lo, hi):
    return [validators.ge(lo), validators.le(hi)]


def _to_0_2pi(value):
    """Angle(s) into [0, 2 pi) with Python's / numpy's remainder (the sign of the divisor)."""
    return value % (2 * math.pi)


def _to_plus_minus_pi(ang: float) -> float:
    return (ang + math.pi) % (2 * math.pi) - math.pi


@define
class DeformableVirtualZoneParams:
    min_front_margin: float = field(default=1.0, validator=_rng(0.0, 1e2))
    K_linear: float = field(default=1.0, validator=_rng(0.1, 10.0))
    K_angular: float = field(default=1.0, validator=_rng(0.1, 10.0))
    K_I: float = field(default=5.0, validator=_rng(0.1, 10.0))
    side_margin_width_ratio: float = field(default=1.0, validator=_rng(1e-2, 1e2))


class DeformableVirtualZone:
    """The zone of one robot and its deformation by the last scan (plotting is not part of this build)."""

    def __init__(self, robot: Robot, ctrl_limits: RobotCtrlLimits, config: DeformableVirtualZoneParams,
                 device: int = 0) -> None:
        self.robot = robot
        self.config = config
        self.ctrl_limits = ctrl_limits
        self._device = device
        self._ctx: Optional[kh.DvzContext] = kh.DvzContext(4096, device)
        self._set_control_regularization()
        self.update_zone_size(robot_speed=robot.state.speed if robot.state else 0.0)
        self._init_constant_zone_parameters()
        self.scan_values = np.empty(0)
        self.scan_angles = np.empty(0)
        self._init_deformation()

    def _init_constant_zone_parameters(self) -> None:
        side_margin = self.robot.radius / self.config.side_margin_width_ratio
        self.zone_minor_radius: float = self.robot.radius + side_margin
        self.zone_minor_radius_diff = 0.0
        self.zone_center_shift_y: float = 0.0  # a_y of the paper
        self.zone_ori_shift: float = 0.0  # gamma of the paper
        self.zone_shift_y_diff: float = 0.0

    def set_from_yaml(self, path_to_file: str) -> None:
        raise NotImplementedError("config files are not read by this build; pass a DeformableVirtualZoneParams")

    def _set_control_regularization(self) -> None:
        """Gains that keep the controls within the limits: a deformation of 1/4 at pi/4 gives the largest action."""
        deformation_max_at_angle = 0.25
        angle_max_angular = np.pi / 4
        self.angular_regulation = self.ctrl_limits.omega_limits.max_acc / (angle_max_angular * deformation_max_at_angle)
        self.linear_regulation = self.ctrl_limits.vx_limits.max_acc / deformation_max_at_angle

    def update_zone_size(self, robot_speed: float) -> None:
        """The zone's length grows with |speed|; two thirds of it lie ahead of the robot."""
        max_vel = self.ctrl_limits.vx_limits.max_vel
        self.zone_major_radius = (1 + (abs(robot_speed) / max_vel)) * self.config.min_front_margin
        self.zone_major_radius_diff = self.config.min_front_margin / max_vel
        zone_shift_const = 2 / 3
        sign_speed = 1 if robot_speed == 0 else np.sign(robot_speed)
        self.zone_center_shift_x: float = -zone_shift_const * sign_speed * self.zone_major_radius
        self.zone_shift_x_diff: float = -zone_shift_const * self.zone_major_radius_diff

    def set_scan_values(self, scan_values: np.ndarray, scan_angles: np.ndarray) -> None:
        self.scan_values = scan_values
        self.scan_angles = scan_angles

    # ---- gradients of the deformation terms (J_A, J_B, J_C of the paper): scalar host helpers
    def _get_grad_A_linear(self, angle: float) -> float:
        t1 = self.zone_minor_radius * self.zone_minor_radius_diff * np.cos(angle) ** 2
        t2 = self.zone_major_radius * self.zone_major_radius_diff * np.sin(angle) ** 2
        return 2 * (t1 + t2)

    def _get_grad_A_angular(self, angle: float) -> float:
        return 2 * np.cos(angle) * np.sin(angle) * (self.zone_minor_radius**2 - self.zone_major_radius**2)

    def _get_grad_B_linear(self, angle: float) -> float:
        t1 = np.cos(angle) * (self.zone_minor_radius**2 * self.zone_shift_x_diff
                              + 2 * self.zone_center_shift_x * self.zone_minor_radius * self.zone_minor_radius_diff)
        t2 = np.sin(angle) * (self.zone_major_radius**2 * self.zone_shift_y_diff
                              + 2 * self.zone_center_shift_y * self.zone_major_radius * self.zone_major_radius_diff)
        return 2 * (t1 + t2)

    def _get_grad_B_angular(self, angle: float) -> float:
        return 2 * (self.zone_center_shift_x * self.zone_minor_radius**2 * np.sin(angle)
                    - self.zone_center_shift_y * self.zone_major_radius**2 * np.cos(angle))

    def _get_grad_C_linear(self) -> float:
        t1 = self.zone_center_shift_x * self.zone_minor_radius * (
            self.zone_minor_radius * self.zone_shift_x_diff + self.zone_center_shift_x * self.zone_minor_radius_diff)
        t2 = self.zone_center_shift_y * self.zone_major_radius * (
            self.zone_major_radius * self.zone_shift_y_diff + self.zone_center_shift_y * self.zone_major_radius_diff)
        t3 = self.zone_major_radius * self.zone_minor_radius * (
            self.zone_major_radius * self.zone_minor_radius_diff + self.zone_minor_radius * self.zone_major_radius_diff)
        return 2 * (t1 + t2 - t3)

    def get_gradients(self, angle: float) -> None:
        self.grad_A_ang: float = self._get_grad_A_angular(angle)
        self.grad_A_u: float = self._get_grad_A_linear(angle)
        self.grad_B_ang: float = self._get_grad_B_angular(angle)
        self.grad_B_u: float = self._get_grad_B_linear(angle)
        self.grad_C_u: float = self._get_grad_C_linear()

    # ---- the deformation
    def _init_deformation(self) -> None:
        self.total_deformation: float = 0.0
        self.deformation_orientation: float = 0.0
        self.deformation_plot = []

    def _regulate_deformation(self) -> None:
        """Mean deformation angle, deformation per beam, and the regulation term 1 / (1 + K_I * deformation)."""
        self.deformation_orientation = self.deformation_orientation / self.total_deformation
        self.total_deformation = self.total_deformation / self.regularization_coeff
        self.deformation_regulation: float = 1 / (1 + self.config.K_I * self.total_deformation)

    def zone(self) -> "kh.DvzZone":
        return kh.DvzZone(self.zone_major_radius, self.zone_minor_radius, self.zone_center_shift_x,
                          self.zone_center_shift_y, self.zone_ori_shift)

    def get_total_deformation(self, compute_deformation_plot: bool = False) -> None:
        """Deformation of the zone by the scan of set_scan_values: one device launch, then the host's
        normalisation.  A scan with fewer ranges than angles is an IndexError, as in the reference."""
        self._init_deformation()
        angles = np.ascontiguousarray(self.scan_angles, dtype=np.float64).reshape(-1)
        ranges = np.ascontiguousarray(self.scan_values, dtype=np.float64).reshape(-1)
        n = len(angles)
        self.regularization_coeff = n
        if len(ranges) < n:
            raise IndexError(f"{len(ranges)} scan values for {n} scan angles")
        if n > self._ctx.max_beams:
            self._ctx.close()
            self._ctx = kh.DvzContext(max(n, 2 * self._ctx.max_beams), self._device)
        res = self._ctx.deform(self.zone(), angles, ranges[:n], radii=compute_deformation_plot)
        self.total_deformation, self.deformation_orientation = res[0], res[1]
        if compute_deformation_plot:
            self.deformation_plot = list(zip(angles.tolist(), res[3].tolist()))
        if self.total_deformation > 0.0:
            self._regulate_deformation()

    def set_control_params(self, linear_gain: float, angular_gain: float, deformation_gain: float) -> None:
        self.config.K_linear = linear_gain
        self.config.K_angular = angular_gain
        self.config.K_I = deformation_gain
        self._set_control_regularization()

    def compute_linear_control(self, ref_control_linear: float, old_control: float, time_step: float) -> float:
        """The reference command blended with a deceleration that grows with the deformation; not above max_vel."""
        if self.total_deformation > 0.0:
            orientation_regulated = _to_plus_minus_pi(self.deformation_orientation) + EPSILON_ANG
            dvz_acc = -self.config.K_linear * self.total_deformation * self.linear_regulation / orientation_regulated
            dvz_control = dvz_acc * time_step + old_control
            linear_ctr = (1 - self.deformation_regulation) * dvz_control + \
                self.deformation_regulation * ref_control_linear
        else:
            linear_ctr = ref_control_linear
        return min(linear_ctr, self.ctrl_limits.vx_limits.max_vel)

    def compute_angular_control(self, ref_control_angular: float) -> float:
        """The reference command blended with a turn away from the deformation; not above max_vel."""
        if self.total_deformation > 0.0:
            inv_angle = _to_plus_minus_pi(np.pi - self.deformation_orientation)
            dvz_control = -self.config.K_angular * inv_angle * self.total_deformation * self.angular_regulation
            angular_ctr = (1 - self.deformation_regulation) * dvz_control + \
                self.deformation_regulation * ref_control_angular
        else:
            angular_ctr = ref_control_angular
        return min(angular_ctr, self.ctrl_limits.omega_limits.max_vel)
