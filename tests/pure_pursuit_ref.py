"""Independent Python restatement of the reference PurePursuit follower (src/controllers/pure_pursuit.cpp) and of
Follower::calculateExponentialSpeedFactor (src/controllers/follower.cpp:319-352), for the tests.  Not collected by
pytest.  The collision gate is the oracle's CollisionChecker (ko.Collision.check_at); Path::State::update takes a
float time step and the host libm's cos / sin (math.cos / math.sin); std::hypot is libm's hypot (Python's
math.hypot is its own algorithm)."""
from __future__ import annotations

import ctypes
import ctypes.util
import math

import numpy as np

from oracle import ko

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.hypot.restype = ctypes.c_double
_libm.hypot.argtypes = [ctypes.c_double, ctypes.c_double]
hypot = _libm.hypot

ACKERMANN, DIFFERENTIAL_DRIVE, OMNI = "ACKERMANN", "DIFFERENTIAL_DRIVE", "OMNI"
GOAL_REACHED, COMMAND_FOUND, NO_COMMAND_POSSIBLE = "GOAL_REACHED", "COMMAND_FOUND", "NO_COMMAND_POSSIBLE"

F32 = np.float32


def f32(v) -> float:
    return float(F32(v))


def normalize_pi(a: float) -> float:
    # utils/angles.h normalizeToMinusPiPlusPi
    a = math.fmod(a + math.pi, 2 * math.pi)
    if a < 0:
        a += 2 * math.pi
    return a - math.pi


def state_update(x, y, yaw, vx, vy, om, dt):
    # datatypes/path.h:24-30: the step is a float
    dtf = f32(dt)
    c, s = math.cos(yaw), math.sin(yaw)
    return x + (vx * c - vy * s) * dtf, y + (vx * s + vy * c) * dtf, yaw + om * dtf


def restrict(cur, target, acc, dec, vmax, dt):
    # controller.cpp restrictVelocityTolimits
    cmd = cur
    if cur < target:
        cmd = min(cur + acc * dt, target)
    elif cur > target:
        cmd = max(cur - dec * dt, target)
    return -vmax if cmd < -vmax else (vmax if vmax < cmd else cmd)


def search_offsets(step: float, m: int):
    # pure_pursuit.cpp:31-39: m rounded up to even; +-step * (i + 1) for even i, stored as float
    if m % 2:
        m += 1
    out = []
    for i in range(0, m, 2):
        out += [f32(step * (i + 1)), f32(-step * (i + 1))]
    return out


def candidates(nominal, offsets, omni: bool):
    """The nominal command, then findSafeCommand's order (:163-212): the forward pass, then the reverse pass from
    the nominal command with vx negated; an omni robot's candidate keeps the previous vy shift when the next omega
    offset is tried."""
    vx0, vy0, om0 = nominal
    out = [(vx0, vy0, om0)]
    for start_vx in (vx0, -vx0):
        cand = [start_vx, vy0, om0]
        for off in offsets:
            cand[2] = om0 + off
            out.append(tuple(cand))
            if omni:
                cand[2] = om0
                cand[1] = vy0 + off
                out.append(tuple(cand))
    return out


def first_clear(coll: ko.Collision, start, cands, horizon: int, dt: float) -> int:
    """checkCommandCollisions over the list: the first candidate none of whose `horizon` poses collides, or -1."""
    for i, (vx, vy, om) in enumerate(cands):
        x, y, yaw = start
        clear = True
        for _ in range(horizon):
            x, y, yaw = state_update(x, y, yaw, vx, vy, om, dt)
            if coll.check_at(x, y, yaw):
                clear = False
                break
        if clear:
            return i
    return -1


def poses(start, cands, horizon: int, dt: float):
    """Every pose of every candidate, candidate-major (for kc_dwa_check_poses)."""
    xs, ys, ts = [], [], []
    for vx, vy, om in cands:
        x, y, yaw = start
        for _ in range(horizon):
            x, y, yaw = state_update(x, y, yaw, vx, vy, om, dt)
            xs.append(x)
            ys.append(y)
            ts.append(yaw)
    return np.array(xs), np.array(ys), np.array(ts)


class PurePursuitRef:
    def __init__(self, ctrl_type, limits, shape, dims, sensor_pos=(0, 0, 0), sensor_rot=(0, 0, 0, 1), res=0.1,
                 **cfg):
        c = dict(lookahead_distance=1.0, speed_regulation_curvature=0.5, speed_regulation_angular=0.5,
                 min_speed_regulation_factor=0.5, goal_dist_tolerance=0.1, max_point_interpolation_distance=0.01,
                 path_segment_length=1.0, lookahead_gain_forward=0.8, prediction_horizon=10, path_search_step=0.2,
                 max_search_candidates=10)
        c.update(cfg)
        self.cfg = c
        self.type = ctrl_type
        self.vx_max, self.vx_acc, self.vx_dec = limits
        self.offsets = search_offsets(c["path_search_step"], c["max_search_candidates"])
        self.coll = ko.Collision(shape, dims, sensor_pos, sensor_rot, res)
        self.ready = False
        self.at_goal = False
        self.last_found = 0
        self.state = (0.0, 0.0, 0.0)
        self.vel = (0.0, 0.0, 0.0)

    def set_path(self, points):
        p = ko.Path(np.asarray(points, np.float32)).interpolate(self.cfg["max_point_interpolation_distance"])
        self.px = np.asarray(p.x, np.float32).copy()
        self.py = np.asarray(p.y, np.float32).copy()
        k = np.asarray(p.curvature, np.float32)
        # follower.cpp:319-352 from the nearest-point index -- which PurePursuit never moves from 0: the curvature
        # sum is the same every step
        cs, dist = 0.0, 0.0
        for i in range(len(self.px) - 1):
            cs += abs(float(k[i]))
            dx = F32(self.px[i] - self.px[i + 1])
            dy = F32(self.py[i] - self.py[i + 1])
            dist += float(np.sqrt(F32(F32(dx * dx + dy * dy) + F32(0.0))))
            if dist >= self.cfg["lookahead_distance"]:
                break
        self.curv_sum = cs
        self.ready = True
        self.at_goal = False

    def speed_factor(self, omega):
        if not self.ready:
            return 1.0
        e = self.cfg["speed_regulation_curvature"] * self.curv_sum + self.cfg["speed_regulation_angular"] * abs(omega)
        return max(math.exp(-e), self.cfg["min_speed_regulation_factor"])

    def lookahead_point(self, radius):
        # pure_pursuit.cpp:214-272: the last segment cut by the circle, t2 before t1; else the end inside the circle;
        # else the same with 1.1 x the radius
        x, y = self.state[0], self.state[1]
        i0 = self.last_found
        p1x, p1y = self.px[i0:-1], self.py[i0:-1]
        d_x = (self.px[i0 + 1:] - p1x).astype(np.float64)  # float differences, widened
        d_y = (self.py[i0 + 1:] - p1y).astype(np.float64)
        f_x = p1x.astype(np.float64) - x
        f_y = p1y.astype(np.float64) - y
        a = d_x * d_x + d_y * d_y
        b = 2.0 * (f_x * d_x + f_y * d_y)
        c = (f_x * f_x + f_y * f_y) - (radius * radius)
        disc = b * b - 4.0 * a * c
        with np.errstate(invalid="ignore", divide="ignore"):
            sq = np.sqrt(disc)
            t1 = (-b - sq) / (2.0 * a)
            t2 = (-b + sq) / (2.0 * a)
        ok = disc >= 0.0
        use2 = ok & (t2 >= 0.0) & (t2 <= 1.0)
        use1 = ok & ~use2 & (t1 >= 0.0) & (t1 <= 1.0)
        hit = np.nonzero(use2 | use1)[0]
        if len(hit) == 0:
            ex, ey = float(self.px[-1]), float(self.py[-1])
            if hypot(ex - x, ey - y) < radius:
                self.last_found = len(self.px) - 1
                return ex, ey
            return self.lookahead_point(1.1 * radius)
        k = int(hit[-1])
        t = t2[k] if use2[k] else t1[k]
        self.last_found = i0 + k
        return f32(float(p1x[k]) + t * d_x[k]), f32(float(p1y[k]) + t * d_y[k])

    def execute(self, dt):
        if not self.ready:
            return (GOAL_REACHED if self.at_goal else NO_COMMAND_POSSIBLE), (0.0, 0.0, 0.0)
        x, y, yaw = self.state
        cvx, cvy, com = self.vel
        L = max(hypot(cvx, cvy) * self.cfg["lookahead_gain_forward"], self.cfg["lookahead_distance"])
        tx, ty = self.lookahead_point(L)
        dx, dy = tx - x, ty - y
        alpha = normalize_pi(math.atan2(dy, dx) - yaw)
        dist = hypot(dx, dy)
        v = self.vx_max
        v *= self.speed_factor(com)
        if self.type == OMNI and not abs(alpha) > math.pi * 0.9:
            cmd = [v * math.cos(alpha), v * math.sin(alpha), 2.0 * alpha]
        else:
            safe = 0.001 if dist < 0.001 else dist
            cmd = [v, 0.0, v * (2.0 * math.sin(alpha) / safe)]
        v_safe = restrict(cvx, cmd[0], self.vx_acc, self.vx_dec, self.vx_max, dt)
        if abs(cmd[0]) > 1e-4:
            cmd[2] = cmd[2] * (v_safe / cmd[0])
        cmd[0] = v_safe
        # :130-139
        if hypot(float(self.px[-1]) - x, float(self.py[-1]) - y) < self.cfg["goal_dist_tolerance"]:
            self.at_goal = True
            return GOAL_REACHED, (0.0, 0.0, 0.0)
        return COMMAND_FOUND, tuple(cmd)

    def execute_with_points(self, dt, cloud):
        self.coll.update_state(*self.state)
        self.coll.update_points(cloud, True)
        return self._avoid(dt)

    def execute_with_scan(self, dt, ranges, angles):
        self.coll.update_state(*self.state)
        self.coll.update_scan(ranges, angles)
        return self._avoid(dt)

    def _avoid(self, dt):
        status, cmd = self.execute(dt)
        if status != COMMAND_FOUND:
            return status, cmd
        cands = candidates(cmd, self.offsets, self.type == OMNI)
        i = first_clear(self.coll, self.state, cands, self.cfg["prediction_horizon"], dt)
        return COMMAND_FOUND, (cands[i] if i >= 0 else (0.0, 0.0, 0.0))


def apply_control(state, cmd, dt):
    """controller_test_helpers.h:9-27: the simulated robot (double step, yaw wrapped into [-pi, pi])."""
    x, y, yaw = state
    vx, vy, om = cmd
    dx = (vx * math.cos(yaw) - vy * math.sin(yaw)) * dt
    dy = (vx * math.sin(yaw) + vy * math.cos(yaw)) * dt
    x += dx
    y += dy
    yaw += om * dt
    while yaw > math.pi:
        yaw -= 2.0 * math.pi
    while yaw < -math.pi:
        yaw += 2.0 * math.pi
    return x, y, yaw
