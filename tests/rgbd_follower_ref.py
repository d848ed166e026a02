"""Independent numpy restatement of the reference RGB-D follower, for the tests (not collected by pytest):
LinearSSKalmanFilter (utils/kalman_filter.cpp), FeatureBasedBboxTracker (vision/tracker.cpp), TrackedBbox3D
(datatypes/tracking.h), RGBFollower's search commands (controllers/rgb_follower.cpp) and RGBDFollower's pursuit
law, reference segment and wait -> search -> give-up pipeline (controllers/rgbd_follower.{h,cpp}).

float32 where the reference stores floats, float64 where it uses doubles; the 9x9 inverse is numpy's, so the
Kalman state agrees with the C++ to a relative tolerance, not bit for bit.  The pixel part (2-D -> 3-D boxes)
is depth_detector_ref.Detector."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

F = np.float32
D = np.float64


@dataclass
class Box:
    center: np.ndarray
    size: np.ndarray
    label: str = ""
    timestamp: float = 0.0
    center_img: tuple = (0, 0)
    size_img: tuple = (0, 0)
    pc_points: list = field(default_factory=list)

    def __post_init__(self):
        self.center = np.asarray(self.center, F).copy()
        self.size = np.asarray(self.size, F).copy()
        self.timestamp = F(self.timestamp)


def normalize_pi(a):
    a = math.fmod(float(a) + math.pi, 2 * math.pi)
    if a < 0:
        a += 2 * math.pi
    return a - math.pi


# ------------------------------------------------------------------------------------------------ Kalman filter
class Kalman:
    def __init__(self, dt, e_pos, e_vel, e_acc):
        dt = F(dt)
        h = F(0.5 * D(dt) ** 2)
        A = np.zeros((9, 9), F)
        for i in range(8):
            A[i, i] = 1
        for i in range(6):
            A[i, i + 3] = dt
        for i in range(3):
            A[i, i + 6] = h
        self.A = A  # A[8, 8] = 0, as in the reference's comma initialiser
        self.Q = np.diag(np.array([e_pos] * 3 + [e_vel] * 3 + [e_acc] * 3, F)).astype(F)
        self.R = self.Q.copy()
        self.P = np.eye(9, dtype=F)
        self.x = np.zeros(9, F)

    def estimate(self, z):
        """One prediction step whatever the gap (the reference drops numberSteps), then the update."""
        pred = (self.A @ self.x).astype(F)
        self.P = (self.A @ self.P @ self.A.T + self.Q).astype(F)
        S = (self.R + self.P).astype(F)
        K = (self.P @ np.linalg.inv(S.astype(D)).astype(F)).astype(F)
        self.x = (pred + K @ (np.asarray(z, F) - pred)).astype(F)
        self.P = ((np.eye(9, dtype=F) - K) @ self.P).astype(F)


# ------------------------------------------------------------------------------------------------ tracker
class Tracked:
    def __init__(self, box: Box):
        self.box = Box(box.center, box.size, box.label, box.timestamp, box.center_img, box.size_img,
                       list(box.pc_points))
        self.vel = np.zeros(3, F)
        self.acc = np.zeros(3, F)

    def yaw(self):
        return F(math.atan2(float(self.vel[1]), float(self.vel[0])))

    def update_from(self, b: Box):
        ts = F(b.timestamp - self.box.timestamp)
        if ts <= 0:
            self.vel = np.zeros(3, F)
            self.acc = np.zeros(3, F)
        else:
            nv = ((b.center - self.box.center) / ts).astype(F)
            self.acc = ((nv - self.vel) / ts).astype(F)
            self.vel = nv
        self.box = Box(b.center, b.size, b.label, b.timestamp, b.center_img, b.size_img, list(b.pc_points))

    def predict_const_acc(self, dt):
        p = Tracked(self.box)
        p.vel = (self.vel + self.acc * F(dt)).astype(F)
        p.acc = self.acc.copy()
        p.box.center = (p.box.center + p.vel * F(dt)).astype(F)
        return p


def std_dev(points):
    pts = np.asarray(points, F).reshape(-1, 3)
    n = F(max(len(pts) - 1, 1))  # mean AND variance over max(n - 1, 1)
    mean = (pts.sum(0, dtype=F) / n).astype(F)
    var = (((pts - mean) ** 2).sum(0, dtype=F) / n).astype(F)
    return np.sqrt(var).astype(F)


def features(b: Box):
    f = np.zeros(9, F)
    f[0:2] = b.center[:2]
    f[2:5] = b.size
    f[5] = len(b.pc_points)
    if f[5] > 0:
        f[6:9] = std_dev(b.pc_points)
    return f


class Tracker:
    def __init__(self, dt, e_pos, e_vel, e_acc):
        self.dt = F(dt)
        self.kf = Kalman(dt, e_pos, e_vel, e_acc)
        self.tracked: Optional[Tracked] = None
        self.label = ""
        self.chosen = None  # index into the label-filtered list of the last accepted box

    def set_initial(self, box: Box, yaw=0.0):
        self.tracked = Tracked(box)
        self.label = box.label
        self.kf.x = np.zeros(9, F)
        self.kf.x[0], self.kf.x[1], self.kf.x[2] = box.center[0], box.center[1], F(yaw)
        return True

    def set_initial_pixel(self, px, py, boxes: List[Box], yaw=0.0):
        for b in boxes:
            cx, cy = b.center_img
            sx, sy = b.size_img
            if cx - int(sx / 2) <= px <= cx + int(sx / 2) and cy - int(sy / 2) <= py <= cy + int(sy / 2):
                return self.set_initial(b, yaw)
        return False

    def update(self, boxes: List[Box]) -> bool:
        cands = [b for b in boxes if b.label == self.label]
        if not cands:
            return False
        dt = F(cands[0].timestamp - self.tracked.box.timestamp)  # from the first box of the label
        if len(cands) == 1:
            best, k = F(1.0), 0
        else:
            ref = features(self.tracked.predict_const_acc(dt).box)
            best, k = F(0.0), 0
            for i, b in enumerate(cands):
                e = (features(b) - ref).astype(F)
                nz = np.abs(ref) > 0
                e[nz] = e[nz] / np.abs(ref[nz])
                sq = F(0.0)
                for v in e:  # the float norm, then exp(-norm^2) in double narrowed to float
                    sq = F(sq + v * v)
                s = F(np.exp(-D(F(np.sqrt(sq))) ** 2))
                if s > best:
                    best, k = s, i
        if not best > 0.0:  # minAcceptedSimilarityScore_ = 0, strict
            return False
        self.chosen = k
        self.tracked.update_from(cands[k])
        t = self.tracked
        z = np.array([t.box.center[0], t.box.center[1], t.yaw(), t.vel[0], t.vel[1], 0, t.acc[0], t.acc[1], 0], F)
        self.kf.estimate(z)
        return True


# ------------------------------------------------------------------------------------------------ search commands
def search_commands(last_direction, timeout, radius, dt, max_omega, min_vel, max_vel, rotate_in_place,
                    pause=1.0, enable_pause=False):
    """getFindTargetCmds: pi, -2 pi, pi with the float clock t += dt."""
    out = []
    part = F(D(timeout) / 4)

    def gen(total, tmax):
        total, tmax, r = F(total), F(tmax), F(radius)
        sign = -1.0 if total < 0 else 1.0
        rot_time = tmax
        pause_steps = int(D(pause) / D(dt))
        if enable_pause:
            rot_time = F(D(tmax) * (1 - pause_steps / D(dt)))
        om = D(F(total / rot_time))
        om = max(min(om, max_omega), min_vel)
        t = F(0.0)
        while t <= tmax:
            if rotate_in_place:
                out.append((0.0, 0.0, sign * om))
            else:
                out.append((max_vel, 0.0, sign * max_vel / D(r)))
            if enable_pause:
                out.extend([(0.0, 0.0, 0.0)] * (pause_steps + 1))
            t = F(D(t) + D(dt))

    gen(last_direction * math.pi, part)
    gen(-2.0 * last_direction * math.pi, F(2.0 * D(part)))
    gen(last_direction * math.pi, part)
    return out


# ------------------------------------------------------------------------------------------------ follower
@dataclass
class Config:
    control_time_step: float = 0.1
    control_horizon: int = 2
    prediction_horizon: int = 10
    distance_tolerance: float = 0.1
    angle_tolerance: float = 0.1
    target_orientation: float = 0.0
    target_distance: float = 0.1
    use_local_coordinates: bool = True
    error_pose: float = 0.05
    error_vel: float = 0.05
    error_acc: float = 0.05
    rotation_gain: float = 1.0
    speed_gain: float = 1.0
    min_vel: float = 0.1
    enable_search: bool = False
    target_wait_timeout: float = 30.0
    target_search_timeout: float = 30.0
    target_search_radius: float = 0.5
    target_search_pause: float = 1.0


class Follower:
    def __init__(self, cfg: Config, robot_radius, max_vel, max_omega, rotate_in_place=True):
        self.c = cfg
        self.robot_radius = D(robot_radius)
        self.max_vel, self.max_omega = D(max_vel), D(max_omega)
        self.rotate_in_place = rotate_in_place
        self.tracker = Tracker(cfg.control_time_step, cfg.error_pose, cfg.error_vel, cfg.error_acc)
        self.track_velocity = not cfg.use_local_coordinates
        self.state = (0.0, 0.0, 0.0)
        self.target_radius = F(0.0)
        self.wait = 0.0
        self.search = 0.0
        self.queue: list = []
        self.latest_omega = 0.0
        self.errors = (F(0.0), F(0.0))

    def refresh(self):
        s = self.tracker.tracked.box.size
        self.target_radius = F(F(0.5) * max(s[0], s[1]))

    def set_initial(self, box, yaw=0.0):
        self.tracker.set_initial(box, yaw)
        self.refresh()

    # the pursuit law (getPureTrackingCtrl)
    def law(self, tx, ty, tyaw, tv, state, update):
        c = self.c
        if self.track_velocity:
            d = math.sqrt((D(tx) - D(F(state[0]))) ** 2 + (D(ty) - D(F(state[1]))) ** 2)
            dist = F(D(F(d)) - self.robot_radius - D(self.target_radius))
            psi = F(normalize_pi(math.atan2(D(ty) - state[1], D(tx) - state[0]) - state[2]))
            gamma = F(normalize_pi(D(tyaw) - state[2]))
        else:
            d = math.sqrt(D(tx) ** 2 + D(ty) ** 2)
            dist = F(D(F(d)) - self.robot_radius - D(self.target_radius))
            psi = F(normalize_pi(D(F(math.atan2(float(ty), float(tx))))))
            gamma = F(0.0)
        dist = max(dist, F(0.001))
        derr = F(D(c.target_distance) - D(dist))
        aerr = F(normalize_pi(D(c.target_orientation) - D(psi)))
        if update:
            self.errors = (derr, aerr)
        diff = F(gamma - psi)
        sd, cd = F(math.sin(diff)), F(math.cos(diff))
        tvf = F(1.0 if self.track_velocity else 0.0)
        vx, om = 0.0, 0.0
        if abs(derr) > c.distance_tolerance or abs(aerr) > c.angle_tolerance:
            v = D(tvf * (F(tv) * cd)) - c.speed_gain * self.max_vel * D(F(math.tanh(derr)))
            v = min(max(v, -self.max_vel), self.max_vel)
            if abs(v) < c.min_vel:
                v = 0.0
            om = D(F(tvf * F(tv) * sd / dist)) + v * D(F(math.sin(psi))) / D(dist) - \
                c.rotation_gain * self.max_omega * D(F(math.tanh(aerr)))
            om = min(max(om, -self.max_omega), self.max_omega)
            if abs(om) < c.min_vel:
                om = 0.0
            vx = v
        return vx, om

    def segment(self, pose):
        """(vx [ph-1], omega [ph-1], path x [ph], path y [ph]) of the reference segment from the filtered pose."""
        c = self.c
        dt = F(c.control_time_step)
        st = list(self.state) if self.track_velocity else [0.0, 0.0, 0.0]
        tx, ty, tyaw, tvx, tvy, tom = (F(v) for v in pose)
        vxs, oms, px, py = [], [], [], []
        for step in range(c.prediction_horizon):
            px.append(F(st[0]))
            py.append(F(st[1]))
            tv = F(math.sqrt(D(tvx) ** 2 + D(tvy) ** 2))
            v, om = self.law(tx, ty, tyaw, tv, st, step == 0)
            cy, sy = math.cos(st[2]), math.sin(st[2])
            st = [st[0] + v * cy * D(dt), st[1] + v * sy * D(dt), st[2] + om * D(dt)]
            if self.track_velocity:
                # constant velocity in the target's own frame
                cyw, syw = math.cos(D(tyaw)), math.sin(D(tyaw))
                tx = F(D(tx) + (D(tvx) * cyw - D(tvy) * syw) * D(dt))
                ty = F(D(ty) + (D(tvx) * syw + D(tvy) * cyw) * D(dt))
                tyaw = F(D(tyaw) + D(tom) * D(dt))
            else:
                mx, myaw = F(v * D(dt)), F(om * D(dt))
                cc, ss = math.cos(myaw), math.sin(myaw)
                dx, dy = D(tx) - D(mx), D(ty)
                tx, ty = F(cc * dx + ss * dy), F(-ss * dx + cc * dy)
                tyaw, tvx, tvy, tom = F(0), F(0), F(0), F(0)
            if step < c.prediction_horizon - 1:
                vxs.append(F(v))
                oms.append(F(om))
        return vxs, oms, px, py

    def step(self, boxes: List[Box]):
        """One getTrackingCtrl(Bbox3D list): ("found" | "hold" | "search" | "give_up", vx, omega)."""
        c = self.c
        pose = None
        if boxes:
            if self.tracker.update(boxes):
                self.refresh()
                k = self.tracker.kf.x
                pose = (k[0], k[1], k[2], k[3], k[4], k[5])
        if pose is not None:
            self.wait = self.search = 0.0
            vx, om, px, py = self.segment(pose)
            if vx:
                self.latest_omega = float(om[0])
            return "found", vx, om
        h = c.control_horizon
        # wait
        if c.enable_search:
            if not self.wait >= c.control_time_step:
                self.queue = []
                self.wait += (h - 1) * c.control_time_step
                return "hold", [F(0)] * (h - 1), [F(0)] * (h - 1)
        elif not self.wait >= c.target_wait_timeout:
            self.wait += (h - 1) * c.control_time_step
            return "hold", [F(0)] * (h - 1), [F(0)] * (h - 1)
        # search
        if c.enable_search:
            self.wait = 0.0
            if not self.queue:
                # NOTE (reference): the commands come from the RGBFollower base, constructed with ITS default
                # config (30 s, 0.5 m, 0.1 s steps, min_vel 0.1), not from this follower's parameters
                self.queue = search_commands(-1 if self.latest_omega < 0 else 1, 30.0, 0.5, 0.1, self.max_omega,
                                             0.1, self.max_vel, self.rotate_in_place)
            if not self.search >= c.target_search_timeout:
                vx, om = [], []
                for _ in range(h - 1):
                    if not self.queue:
                        return "give_up", [], []  # an empty result, the timers keep running
                    cmd = self.queue.pop(0)
                    self.search += c.control_time_step
                    vx.append(F(cmd[0]))
                    om.append(F(cmd[2]))
                return "search", vx, om
        self.wait = self.search = 0.0
        self.queue = []
        return "give_up", [], []
