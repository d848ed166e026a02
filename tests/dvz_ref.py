"""Independent Python restatement of the reference's Deformable Virtual Zone (src/kompass_core/algorithms/dvz.py,
control/dvz.py) and of the Stanley law (src/controllers/stanley.cpp), for the tests.  Not collected by pytest.

Per beam: cos / sin are math.cos / math.sin (the host libm: np.cos / np.sin of the reference give the same bits),
squares are products (the device's deliberate deviation from `x ** 2`), and the two sums run
sequentially in beam order.  `beam_literal` keeps the reference's own expressions (`** 2` on numpy float64) so
the deviation can be bounded.  The Stanley restatement takes the tracked target (cross-track and heading error)
from the class's Follower -- closest-point tracking is shared with the other followers -- and restates the law and
the command limits on top of it."""
from __future__ import annotations

import math

import numpy as np

TWO_PI = 2 * math.pi
EPSILON_ANG = 0.01


def f32(v) -> float:
    return float(np.float32(v))


def to_0_2pi(a: float) -> float:
    # Python's float %: the sign of the divisor
    return a % TWO_PI


def to_plus_minus_pi(a: float) -> float:
    return (a + math.pi) % TWO_PI - math.pi


# ------------------------------------------------------------------ the zone
def zone(robot_radius, side_ratio=1.0, min_front_margin=1.0, max_vel=1.0, speed=0.0):
    """(major, minor, shift_x, shift_y, ori) as update_zone_size / the constant zone parameters leave them."""
    major = (1 + abs(speed) / max_vel) * min_front_margin
    sign = 1.0 if speed == 0 else math.copysign(1.0, speed)
    shift_x = -(2 / 3) * sign * major
    minor = robot_radius + robot_radius / side_ratio
    return (major, minor, shift_x, 0.0, 0.0)


def beam(z, angle: float, rng: float):
    """(undeformed, deformed, deformation term, orientation term) of one beam; the terms are None undeformed."""
    major, minor, sx, sy, ori = z
    c, s = math.cos(angle - ori), math.sin(angle - ori)
    p, q = minor * c, major * s
    a = p * p + q * q
    b = 2 * (sx * c * (minor * minor) + sy * s * (major * major))
    u, v, w = sx * minor, sy * major, minor * major
    cc = u * u + v * v - w * w
    disc = b * b - 4 * a * cc
    root = math.sqrt(disc) if disc >= 0 else math.nan
    und = (-b + root) / (2 * a)
    dfm = rng if und > rng else und
    if dfm < und:
        t = (und - dfm) / dfm if dfm != 0 else math.copysign(math.inf, und - dfm) * math.copysign(1.0, dfm)
        m = to_0_2pi(angle)
        return und, dfm, t, t * m
    return und, dfm, None, None


def beam_literal(z, angle, rng):
    """The reference's expressions as written: `** 2`, np.cos / np.sin / np.sqrt on numpy float64."""
    major, minor, sx, sy, ori = z
    angle = np.float64(angle)
    with np.errstate(all="ignore"):
        ac, as_ = np.cos(angle - ori), np.sin(angle - ori)
        a = (minor * ac) ** 2 + (major * as_) ** 2
        b = 2 * (sx * ac * minor**2 + sy * as_ * major**2)
        cc = (sx * minor) ** 2 + (sy * major) ** 2 - (minor * major) ** 2
        und = (-b + np.sqrt(b**2 - 4 * a * cc)) / (2 * a)
        dfm = np.float64(rng) if und > rng else und
        if dfm < und:
            t = (und - dfm) / dfm
            return float(und), float(dfm), float(t), float(t * (angle % TWO_PI))
    return float(und), float(dfm), None, None


def deform(z, angles, ranges, literal=False):
    """(radii, total, orientation sum, count, |terms| sum, |orientation terms| sum), sequential in beam order."""
    f = beam_literal if literal else beam
    radii = np.empty(len(angles))
    total = orient = 0.0
    abs_t = abs_o = 0.0
    count = 0
    for i, (a, r) in enumerate(zip(angles, ranges)):
        _, dfm, t, o = f(z, float(a), float(r))
        radii[i] = dfm
        if t is not None:
            total += t
            orient += o
            abs_t += abs(t)
            abs_o += abs(o)
            count += 1
    return radii, total, orient, count, abs_t, abs_o


# ---------------------------------------------------------- the DVZ control laws
class DvzLaws:
    """Normalisation and the two control laws of DeformableVirtualZone, on given sums."""

    def __init__(self, vx_max, vx_acc, omega_max, omega_acc, k_linear=1.0, k_angular=1.0, k_i=5.0):
        self.vx_max, self.omega_max = vx_max, omega_max
        self.linear_regulation = vx_acc / 0.25
        self.angular_regulation = omega_acc / (math.pi / 4 * 0.25)
        self.k_linear, self.k_angular, self.k_i = k_linear, k_angular, k_i
        self.total = self.orient = 0.0
        self.regulation = None

    def set_sums(self, total, orient, n):
        self.total, self.orient = total, orient
        if total > 0.0:
            self.orient = orient / total
            self.total = total / n
            self.regulation = 1 / (1 + self.k_i * self.total)

    def linear(self, ref, old, dt):
        if self.total > 0.0:
            acc = -self.k_linear * self.total * self.linear_regulation / (to_plus_minus_pi(self.orient) + EPSILON_ANG)
            v = (1 - self.regulation) * (acc * dt + old) + self.regulation * ref
        else:
            v = ref
        return min(v, self.vx_max)

    def angular(self, ref):
        if self.total > 0.0:
            inv = to_plus_minus_pi(math.pi - self.orient)
            w = (1 - self.regulation) * (-self.k_angular * inv * self.total * self.angular_regulation) + \
                self.regulation * ref
        else:
            w = ref
        return min(w, self.omega_max)


# ---------------------------------------------------------------- Stanley
def normalize_pi(a: float) -> float:
    a = math.fmod(a + math.pi, TWO_PI)
    if a < 0:
        a += TWO_PI
    return a - math.pi


def restrict(cur, target, acc, dec, vmax, dt):
    cmd = cur
    if cur < target:
        cmd = min(cur + acc * dt, target)
    elif cur > target:
        cmd = max(cur - dec * dt, target)
    return -vmax if cmd < -vmax else (vmax if vmax < cmd else cmd)


class StanleyLaw:
    """stanley.cpp:27-105 on a tracked target.  The gains are the default StanleyParameters (the reference's
    parameterised constructor passes its config to the Follower only) and the wheel base is 1.0 until set."""

    def __init__(self, vx_limits, omega_limits, cross_track_gain=10.0, heading_gain=1.0, min_velocity=0.05,
                 wheel_base=1.0):
        self.vx_max, self.vx_acc, self.vx_dec = vx_limits
        self.w_max, self.max_angle, self.w_acc, self.w_dec = omega_limits
        self.k_ct, self.k_h, self.v_min, self.wheel_base = cross_track_gain, heading_gain, min_velocity, wheel_base
        self.cmd = (0.0, 0.0, 0.0, 0.0)  # vx, vy, omega, steer

    def step(self, crosstrack, heading, reverse, dt):
        target_speed = -self.vx_max if reverse else self.vx_max
        steer = -self.k_ct * math.atan2(crosstrack, max(abs(target_speed), self.v_min)) + \
            self.k_h * normalize_pi(heading)
        v = f32(restrict(self.cmd[0], target_speed, self.vx_acc, self.vx_dec, self.vx_max, dt))
        steer = min(max(steer, -self.max_angle), self.max_angle)
        omega = math.tan(steer) * abs(v) / self.wheel_base
        omega = restrict(self.cmd[2], omega, self.w_acc, self.w_dec, self.w_max, dt)
        self.cmd = (v, 0.0, omega, steer)
        return self.cmd


def clamp_cmds(cmd, vx_max, vy_max, w_max):
    """Follower::get*Cmd: each command clamped to +-its limit."""
    vx, vy, w = cmd[0], cmd[1], cmd[2]
    return (max(min(vx, vx_max), -vx_max), max(min(vy, vy_max), -vy_max), max(min(w, w_max), -w_max))
