"""The vision followers without a GPU: RGBDFollower through its Bbox3D path (no device) step by step against the
independent restatement of tests/rgbd_follower_ref.py, the reference behaviours the restatement pins (abs in the
tolerance test, one Kalman prediction per update, the tracker's and the follower's details), the reference's
tracker and following scenarios restated, RGBFollower on 2-D boxes, and the Python front ends."""
import logging
import math

import numpy as np
import pytest

import kompass_cpp
import rgbd_follower_ref as ref
from kompass_core.control import (VisionRGBDFollower, VisionRGBDFollowerConfig, VisionRGBFollower,
                                  VisionRGBFollowerConfig)
from kompass_core.models import AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry, RobotType

C = kompass_cpp.control
T = kompass_cpp.types
RTOL, ATOL = 1e-5, 1e-6
MAX_VEL, MAX_OMEGA = 1.0, 2.0


def limits(max_vel=MAX_VEL, max_omega=MAX_OMEGA):
    return C.ControlLimitsParams(C.LinearVelocityControlParams(max_vel, 5.0, 5.0),
                                 C.LinearVelocityControlParams(max_vel, 5.0, 5.0),
                                 C.AngularVelocityControlParams(math.pi, max_omega, 5.0, 5.0))


def params(cfg: ref.Config):
    p = C.RGBDFollowerParameters()
    d = dict(cfg.__dict__)
    p.from_dict({k: (v if isinstance(v, (bool, int)) else float(v)) for k, v in d.items()})
    return p


def follower(cfg: ref.Config, shape=T.RobotGeometry.CYLINDER, dims=(0.3, 0.6), ctrl=C.ControlType.DIFFERENTIAL_DRIVE):
    return C.RGBDFollower(ctrl, limits(), shape, list(dims), [0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], params(cfg))


def cpp_box(b: ref.Box):
    return T.Bbox3D(b.center.tolist(), b.size.tolist(), list(b.center_img), list(b.size_img), float(b.timestamp),
                    b.label, [list(p) for p in b.pc_points])


def pair(cfg: ref.Config, first: ref.Box, yaw=0.0, dims=(0.3, 0.6)):
    f = follower(cfg, dims=dims)
    assert f.set_initial_tracking(first.center_img[0], first.center_img[1], [cpp_box(first)], yaw)
    r = ref.Follower(cfg, dims[0], MAX_VEL, MAX_OMEGA)
    r.set_initial(first, yaw)
    return f, r


def step_both(f, r, boxes, state=None):
    """One step on both sides; asserts every output agrees and returns the restatement's outcome."""
    if state is not None:
        f.set_current_state(*state, 0.0)
        r.state = tuple(state)
    res = f.get_tracking_ctrl([cpp_box(b) for b in boxes], T.Velocity2D())
    kind, vx, om = r.step(boxes)
    if kind == "give_up":
        assert not res.is_found
        return kind
    assert res.is_found and res.cost == 0.0
    v = res.trajectory.velocities
    assert len(v.vx) == len(vx), kind
    np.testing.assert_allclose(v.vx, vx, rtol=RTOL, atol=ATOL, err_msg=kind)
    np.testing.assert_allclose(v.omega, om, rtol=RTOL, atol=ATOL, err_msg=kind)
    np.testing.assert_array_equal(v.vy, np.zeros(len(vx), np.float32))
    np.testing.assert_allclose(f.get_tracked_state(), r.tracker.kf.x, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(f.get_errors(), r.errors, rtol=RTOL, atol=ATOL)
    q = f.pending_search_commands()
    assert len(q) == len(r.queue)
    if q:
        np.testing.assert_allclose(np.array(q), np.array(r.queue), rtol=1e-12)
    if kind == "found":
        raw = f.get_raw_tracking()
        chosen = [b for b in boxes if b.label == r.tracker.label][r.tracker.chosen]
        np.testing.assert_array_equal(raw.center, chosen.center)
        assert f.target_radius() == r.target_radius
    return kind


def box(x, y, sx=0.4, sy=0.4, sz=1.0, label="person", ts=0.0, cimg=(320, 240), simg=(60, 120), pc=()):
    return ref.Box([x, y, 0.0], [sx, sy, sz], label, ts, cimg, simg, list(pc))


# ---------------------------------------------------------------------------------------------- pinned behaviours
def test_abs_in_the_tolerance_test_is_the_float_one():
    """0.1 < |distance_error| < 1: ::abs(int) would truncate it to 0 and send no command."""
    cfg = ref.Config(target_distance=1.0, distance_tolerance=0.05, prediction_horizon=4)
    f, r = pair(cfg, box(2.0, 0.0))
    assert step_both(f, r, [box(2.0, 0.0)]) == "found"
    dist_err = f.get_errors()[0]
    assert 0.1 < abs(dist_err) < 1.0
    vx = f.get_tracking_ctrl([cpp_box(box(2.0, 0.0))], T.Velocity2D()).trajectory.velocities.vx
    assert vx[0] > 0.4


def test_follower_command_getters_read_the_last_found_command():
    """The reference's latest_velocity_command_ is the Follower's: get_vx_cmd / get_omega_cmd return the front
    command of the last found segment (clamped by the Follower's own limits, 1.0 by default)."""
    cfg = ref.Config(target_distance=1.0, distance_tolerance=0.05, prediction_horizon=4)
    f, r = pair(cfg, box(2.0, 0.3))
    assert f.get_vx_cmd() == 0.0 and f.get_omega_cmd() == 0.0
    res = f.get_tracking_ctrl([cpp_box(box(2.0, 0.3))], T.Velocity2D())
    v = res.trajectory.velocities
    assert abs(v.vx[0]) < 1.0 and abs(v.omega[0]) < 1.0 and v.vx[0] != 0.0 and v.omega[0] != 0.0
    assert f.get_vx_cmd() == v.vx[0] and f.get_omega_cmd() == v.omega[0] and f.get_vy_cmd() == 0.0


def test_depth_frame_must_be_uint16_2d_before_anything_else():
    """Host frames are converted (and kept alive) before the follower is called: the dtype and shape rules apply
    to array-likes too, ahead of the missing-intrinsics error."""
    f = follower(ref.Config())

    class Frame:  # an __array_interface__ object, as PIL images are
        def __init__(self, a):
            self.a = a

        @property
        def __array_interface__(self):
            return dict(shape=self.a.shape, typestr=self.a.dtype.str, data=self.a.tobytes(), version=3)

    boxes = [T.Bbox2D([1, 1], [5, 5])]
    with pytest.raises(TypeError, match="uint16"):
        f.get_tracking_ctrl(Frame(np.zeros((8, 8), np.float32)), boxes, T.Velocity2D())
    with pytest.raises(ValueError, match="2-D"):
        f.get_tracking_ctrl(Frame(np.zeros(8, np.uint16)), boxes, T.Velocity2D())
    with pytest.raises(RuntimeError, match="setCameraIntrinsics"):
        f.get_tracking_ctrl(Frame(np.zeros((8, 8), np.uint16)), boxes, T.Velocity2D())


def test_kalman_predicts_one_step_whatever_the_gap():
    cfg = ref.Config(prediction_horizon=3)
    f, r = pair(cfg, box(2.0, 0.0, ts=0.0))
    for k, ts in enumerate([0.5, 1.5, 1.6, 3.0]):  # gaps of 5, 10, 1 and 14 time steps
        step_both(f, r, [box(2.0 + 0.3 * (k + 1), 0.2 * k, ts=ts)])
    # the same measurements with the gap's number of predictions end elsewhere
    kf = ref.Kalman(0.1, 0.05, 0.05, 0.05)
    tr = ref.Tracked(box(2.0, 0.0))
    kf.x[:2] = [2.0, 0.0]
    last = 0.0
    for k, ts in enumerate([0.5, 1.5, 1.6, 3.0]):
        tr.update_from(box(2.0 + 0.3 * (k + 1), 0.2 * k, ts=ts))
        z = np.array([tr.box.center[0], tr.box.center[1], tr.yaw(), tr.vel[0], tr.vel[1], 0, tr.acc[0],
                      tr.acc[1], 0], np.float32)
        for _ in range(max(int(np.float32(ts - last) / np.float32(0.1)), 1) - 1):
            kf.x = (kf.A @ kf.x).astype(np.float32)
            kf.P = (kf.A @ kf.P @ kf.A.T + kf.Q).astype(np.float32)
        kf.estimate(z)
        last = ts
    assert not np.allclose(f.get_tracked_state(), kf.x, rtol=1e-3)


def test_single_label_box_is_taken_without_features():
    cfg = ref.Config(prediction_horizon=3)
    f, r = pair(cfg, box(2.0, 0.0))
    far = box(40.0, -30.0, sx=5.0, sy=7.0)
    assert step_both(f, r, [far, box(2.0, 0.0, label="chair")]) == "found"
    np.testing.assert_array_equal(f.get_raw_tracking().center, far.center)


def test_zero_similarity_is_rejected_strictly():
    cfg = ref.Config(prediction_horizon=3)
    f, r = pair(cfg, box(1.0, 1.0, sx=1.0, sy=1.0))
    far = [box(1e4, 1e4, sx=1e3, sy=1e3), box(-1e4, 2e4, sx=2e3, sy=1e3)]
    assert step_both(f, r, far) == "hold"
    np.testing.assert_array_equal(f.get_raw_tracking().center, [1.0, 1.0, 0.0])


def test_tracker_features_zero_reference_and_point_spread():
    """A reference feature of 0 is not normalised (x = 0 here), and the point-spread features divide the mean and
    the variance by max(n - 1, 1): the candidate with the matching spread wins."""
    rng = np.random.default_rng(3)
    pts = rng.normal(0.0, 0.2, (5, 3)).astype(np.float32)
    cfg = ref.Config(prediction_horizon=3)
    f, r = pair(cfg, box(0.0, 1.0, pc=pts))
    for k in range(6):
        a = box(0.0, 1.0 + 0.01 * k, pc=pts * 3.0)
        b = box(0.0, 1.0 - 0.01 * k, pc=pts)
        c = box(0.05 * k, 1.0, pc=rng.normal(0.0, 0.2, (1, 3)))
        step_both(f, r, [a, b, c] if k % 2 else [c, b, a])


def test_velocity_reset_when_time_does_not_advance():
    cfg = ref.Config(prediction_horizon=3, use_local_coordinates=False)
    f, r = pair(cfg, box(2.0, 0.0))
    for k in range(4):  # timestamps stay 0: vel and acc measurements are 0
        step_both(f, r, [box(2.0 + 0.5 * k, 0.0)], state=(0.0, 0.0, 0.0))
    assert np.all(np.abs(f.get_tracked_state()[3:]) < 0.05)


@pytest.mark.parametrize("shape,dims,radius", [(T.RobotGeometry.CYLINDER, [0.3, 0.6], 0.3),
                                               (T.RobotGeometry.SPHERE, [0.25], 0.25),
                                               (T.RobotGeometry.BOX, [0.6, 0.8, 0.4], 0.5)])
def test_robot_radius_and_goal_tolerance(shape, dims, radius):
    cfg = ref.Config(error_pose=0.07)
    f = follower(cfg, shape=shape, dims=dims)
    assert f.robot_radius() == pytest.approx(radius, rel=1e-6)
    assert f.goal_dist_tolerance() == pytest.approx(0.07)


def test_target_radius_refreshes_only_on_success():
    cfg = ref.Config(prediction_horizon=3)
    f, r = pair(cfg, box(2.0, 0.0, sx=0.4, sy=0.9))
    assert f.target_radius() == np.float32(0.45)
    step_both(f, r, [box(2.0, 0.0, sx=0.8, sy=0.2)])
    assert f.target_radius() == np.float32(0.4)
    step_both(f, r, [box(2.0, 0.0, sx=3.0, sy=3.0, label="chair")])  # not the tracked label
    assert f.target_radius() == np.float32(0.4)


def test_state_restored_after_the_reference_segment():
    cfg = ref.Config(prediction_horizon=8, use_local_coordinates=False, target_distance=0.5)
    f, r = pair(cfg, box(3.0, 1.0))
    step_both(f, r, [box(3.0, 1.0)], state=(0.5, -0.2, 0.3))
    for _ in range(3):  # no new state: the segment must have put the robot back
        step_both(f, r, [box(3.0, 1.0)])


def test_wait_clock_and_give_up():
    cfg = ref.Config(control_horizon=3, prediction_horizon=5, target_wait_timeout=1.0)
    f, r = pair(cfg, box(2.0, 0.5))
    step_both(f, r, [box(2.0, 0.5)])
    kinds = [step_both(f, r, []) for _ in range(8)]
    assert kinds == ["hold"] * 5 + ["give_up"] + ["hold"] * 2  # (h - 1) * dt = 0.2 s per hold


@pytest.mark.parametrize("timeout,dt,radius,ctrl", [(30.0, 0.1, 0.5, C.ControlType.DIFFERENTIAL_DRIVE),
                                                    (3.0, 0.07, 0.5, C.ControlType.OMNI),
                                                    (2.2, 0.1, 0.8, C.ControlType.ACKERMANN),
                                                    (10.0, 0.3, 0.5, C.ControlType.DIFFERENTIAL_DRIVE)])
def test_search_commands(timeout, dt, radius, ctrl):
    cfg = ref.Config(control_horizon=3, prediction_horizon=5, enable_search=True, target_search_timeout=timeout,
                     control_time_step=dt, target_search_radius=radius)
    f = C.RGBDFollower(ctrl, limits(), T.RobotGeometry.CYLINDER, [0.3, 0.6], [0, 0, 0], [0, 0, 0, 1], params(cfg))
    r = ref.Follower(cfg, 0.3, MAX_VEL, MAX_OMEGA, rotate_in_place=ctrl != C.ControlType.ACKERMANN)
    first = box(2.0, -0.8)  # to the right: the last command turns clockwise, the search starts that way
    assert f.set_initial_tracking(320, 240, [cpp_box(first)])
    r.set_initial(first)
    step_both(f, r, [first])
    kinds = [step_both(f, r, []) for _ in range(int(timeout / dt) + 6)]
    assert kinds[0] == "hold" and kinds[1] == "search" and "give_up" in kinds


def test_errors_before_initialisation():
    f = follower(ref.Config())
    with pytest.raises(RuntimeError, match="setInitialTracking"):
        f.get_tracking_ctrl([cpp_box(box(1.0, 0.0))], T.Velocity2D())
    img = np.zeros((48, 64), np.uint16)
    with pytest.raises(RuntimeError, match="setCameraIntrinsics"):
        f.get_tracking_ctrl(img, [T.Bbox2D([1, 1], [5, 5])], T.Velocity2D())
    with pytest.raises(RuntimeError, match="setCameraIntrinsics"):
        f.set_initial_tracking(img, T.Bbox2D([1, 1], [5, 5]))
    assert not f.set_initial_tracking(0, 0, [cpp_box(box(1.0, 0.0, cimg=(300, 300), simg=(10, 10)))])
    assert f.depth_calls() == 0
    # an empty detection list needs no tracker
    assert f.get_tracking_ctrl([], T.Velocity2D()).is_found


def test_initial_tracking_by_pixel_takes_the_first_box_holding_it():
    cfg = ref.Config(prediction_horizon=3)
    boxes = [box(5.0, 0.0, cimg=(100, 100), simg=(20, 20)), box(2.0, 0.0, cimg=(300, 200), simg=(61, 41)),
             box(3.0, 0.0, cimg=(310, 200), simg=(40, 40))]
    f = follower(cfg)
    r = ref.Tracker(0.1, 0.05, 0.05, 0.05)
    for px, py in [(330, 220), (270, 180), (269, 200), (110, 110), (0, 0), (300, 221)]:
        ok = f.set_initial_tracking(px, py, [cpp_box(b) for b in boxes])
        assert ok == r.set_initial_pixel(px, py, boxes)
        if ok:
            np.testing.assert_array_equal(f.get_raw_tracking().center, r.tracked.box.center)


# ---------------------------------------------------------------------------------------------- per-step comparison
SCENARIOS = [
    ("local", ref.Config(prediction_horizon=10, target_distance=0.6, distance_tolerance=0.05)),
    ("local-search", ref.Config(prediction_horizon=6, control_horizon=3, enable_search=True, target_distance=0.3,
                                target_search_timeout=2.0, rotation_gain=0.5)),
    ("global", ref.Config(prediction_horizon=10, use_local_coordinates=False, target_distance=0.4,
                          target_orientation=0.3)),
    ("global-wait", ref.Config(prediction_horizon=4, control_horizon=4, use_local_coordinates=False,
                               target_wait_timeout=0.9, speed_gain=0.6)),
]


@pytest.mark.parametrize("name,cfg", SCENARIOS, ids=[s[0] for s in SCENARIOS])
def test_steps_match_the_restatement(name, cfg):
    rng = np.random.default_rng(len(name))
    f, r = pair(cfg, box(2.5, 0.4, ts=0.0))
    state = np.array([0.0, 0.0, 0.0])
    kinds = set()
    tx, ty = 2.5, 0.4
    for k in range(80):
        t = 0.1 * (k + 1)
        tx += 0.03 * math.cos(0.1 * k)
        ty += 0.02 * math.sin(0.07 * k)
        boxes = []
        if not (20 <= k < 20 + 12 or 55 <= k < 58):  # lost for a while, twice
            boxes.append(box(tx + rng.normal(0, 0.01), ty + rng.normal(0, 0.01), ts=t if k % 3 else 0.0))
            if k % 4 == 0:
                boxes.insert(0, box(tx + 1.5, ty - 1.0, sx=0.7, sy=0.3, ts=t))  # a second person
            if k % 5 == 1:
                boxes.append(box(tx, ty, sx=2.0, sy=2.0, label="car", ts=t))
        st = tuple(state) if not cfg.use_local_coordinates else None
        kinds.add(step_both(f, r, boxes, state=st))
        state += [0.02, 0.01, 0.005]
    assert "found" in kinds and ("hold" in kinds)


# ---------------------------------------------------------------------------------------------- reference scenarios
def test_tracker_follows_moving_boxes():
    """tests/test_tracker (reference) restated: boxes moving at constant velocity with measurement noise among
    distractors; the filtered position stays within 0.1 m on average."""
    rng = np.random.default_rng(7)
    cfg = ref.Config(prediction_horizon=3)
    start = box(1.0, 1.0, ts=0.0)
    f, _ = pair(cfg, start)
    errs = []
    for k in range(1, 60):
        t = 0.1 * k
        cx, cy = 1.0 + 0.5 * t, 1.0 + 0.2 * t
        boxes = [box(cx + rng.normal(0, 0.02), cy + rng.normal(0, 0.02), ts=t),
                 box(cx + 3.0, cy - 2.0, sx=0.9, sy=0.9, ts=t), box(cx, cy, label="dog", ts=t)]
        rng.shuffle(boxes)
        f.get_tracking_ctrl([cpp_box(b) for b in boxes], T.Velocity2D())
        s = f.get_tracked_state()
        errs.append(math.hypot(s[0] - cx, s[1] - cy))
    assert np.mean(errs) <= 0.1


def _simulate(local, target_path, steps=150):
    cfg = ref.Config(prediction_horizon=10, use_local_coordinates=local, target_distance=0.5,
                     distance_tolerance=0.05, angle_tolerance=0.05)
    p = params(cfg)
    f = C.RGBDFollower(C.ControlType.DIFFERENTIAL_DRIVE, limits(), T.RobotGeometry.CYLINDER, [0.3, 0.6],
                       [0, 0, 0], [0, 0, 0, 1], p)
    x = y = yaw = 0.0
    dt = cfg.control_time_step

    def seen(t):
        gx, gy = target_path(t)
        if local:
            dx, dy = gx - x, gy - y
            return box(math.cos(yaw) * dx + math.sin(yaw) * dy, -math.sin(yaw) * dx + math.cos(yaw) * dy, ts=t)
        return box(gx, gy, ts=t)

    assert f.set_initial_tracking(320, 240, [cpp_box(seen(0.0))])
    for k in range(steps):
        t = dt * (k + 1)
        if not local:
            f.set_current_state(x, y, yaw, 0.0)
        res = f.get_tracking_ctrl([cpp_box(seen(t))], T.Velocity2D())
        assert res.is_found
        v, w = float(res.trajectory.velocities.vx[0]), float(res.trajectory.velocities.omega[0])
        x += v * math.cos(yaw) * dt
        y += v * math.sin(yaw) * dt
        yaw += w * dt
    return abs(f.get_errors()[0]), cfg.distance_tolerance


@pytest.mark.parametrize("local", [True, False], ids=["local", "global"])
@pytest.mark.parametrize("moving", [False, True], ids=["static", "moving"])
def test_following_reaches_the_target(local, moving):
    path = (lambda t: (3.0 + 0.05 * t, 1.5 + 0.03 * t)) if moving else (lambda t: (3.0, 1.5))
    err, tol = _simulate(local, path)
    assert err < 2 * tol


# ---------------------------------------------------------------------------------------------- RGBFollower
def rgb_ref_track(box2d, target, tol, kv, kw, min_vel, max_vel=MAX_VEL, max_om=MAX_OMEGA):
    F = np.float32
    (tx, ty), (sx, sy), (iw, ih) = box2d
    cur = F(F(sx * sy) / F(iw * ih))
    derr = F(np.float64(target) - cur)
    dtol = F(tol * target)
    cx, cy = tx + sx // 2, ty + sy // 2
    ey = F(F(2.0) * (F(cy) / F(ih) - F(0.5)))
    ex = F(F(2.0) * (F(cx) / F(iw) - F(0.5)))
    if abs(derr) < dtol and abs(ey) < tol and abs(ex) < tol:
        return 0.0, 0.0, derr, ex
    ds = F((derr / np.float64(target)) * max_vel) if abs(derr) > dtol else F(0.0)
    om = F(-kw * ex * max_om)
    v = F(kv * ds)
    om = om if abs(om) >= min_vel else F(0.0)
    om = min(max(om, F(-max_om)), F(max_om))
    v = v if abs(v) >= min_vel else F(0.0)
    v = min(max(v, F(-max_vel)), F(max_vel))
    return float(v), float(om), derr, ex


def test_rgb_follower_on_2d_boxes():
    p = C.RGBFollowerParameters()
    p.from_dict({"tolerance": 0.1, "rotation_gain": 0.8, "speed_gain": 0.7, "min_vel": 0.05,
                 "enable_search": True, "target_search_timeout": 3.0, "control_time_step": 0.1})
    f = C.RGBFollower(C.ControlType.DIFFERENTIAL_DRIVE, limits(), p)
    assert C.RGBFollowerConfig is C.RGBFollowerParameters
    first = T.Bbox2D([300, 200], [60, 120])
    f.reset_target(first)
    target = np.float32(60 * 120) / np.float32(640 * 480)
    rng = np.random.default_rng(2)
    for _ in range(30):
        tl = [int(rng.integers(0, 500)), int(rng.integers(0, 300))]
        sz = [int(rng.integers(10, 140)), int(rng.integers(10, 180))]
        assert f.run(T.Bbox2D(tl, sz))
        v, om, derr, ex = rgb_ref_track((tl, sz, (640, 480)), float(target), 0.1, 0.7, 0.8, 0.05)
        out = f.get_ctrl()
        np.testing.assert_allclose([out.vx[0], out.omega[0]], [v, om], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(f.get_errors(), [derr, ex], rtol=1e-6, atol=1e-7)
    # lost: search commands, the direction from the last centre (x - y / 2 > 0 -> +1)
    assert f.run(None)
    q = [(0.0, 0.0, v[2]) for v in ref.search_commands(1, 3.0, 0.5, 0.1, MAX_OMEGA, 0.05, MAX_VEL, True)]
    assert len(f.pending_search_commands()) == len(q) - 1
    np.testing.assert_allclose(f.get_ctrl().omega, [q[0][2]], rtol=1e-6)
    steps = 1
    while f.run(None):
        steps += 1
    assert steps == 30  # 3 s of search at 0.1 s


def test_rgb_follower_waits_without_search():
    p = C.RGBFollowerParameters()
    p.from_dict({"target_wait_timeout": 0.5, "enable_search": False})
    f = C.RGBFollower(C.ControlType.ACKERMANN, limits(), p)
    f.reset_target(T.Bbox2D([300, 200], [60, 120]))
    assert f.run(T.Bbox2D([100, 200], [60, 120]))
    held = [f.run(None) for _ in range(7)]
    assert held == [True] * 5 + [False, True]
    assert list(f.get_ctrl().vx) == [0.0]


# ---------------------------------------------------------------------------------------------- Python front ends
def robot():
    return Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER,
                 geometry_params=np.array([0.3, 0.6]))


def ctrl_limits():
    return RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=3.0, max_decel=3.0),
                           omega_limits=AngularCtrlLimits(max_vel=2.0, max_acc=3.0, max_decel=3.0, max_steer=np.pi))


@pytest.mark.parametrize("kw", [dict(control_horizon=0), dict(prediction_horizon=1001), dict(rotation_gain=0.0),
                                dict(target_orientation=4.0), dict(distance_tolerance=0.0), dict(max_depth=0.0),
                                dict(buffer_size=11), dict(target_search_timeout=-1.0)])
def test_rgbd_config_validators(kw):
    with pytest.raises(ValueError):
        VisionRGBDFollowerConfig(**kw)


@pytest.mark.parametrize("kw", [dict(tolerance=2.0), dict(rotation_gain=1.5), dict(control_horizon=0),
                                dict(min_vel=0.0)])
def test_rgb_config_validators(kw):
    with pytest.raises(ValueError):
        VisionRGBFollowerConfig(**kw)


def test_rgbd_config_defaults_and_transfer():
    c = VisionRGBDFollowerConfig()
    assert (c.control_horizon, c.prediction_horizon, c.target_distance, c.enable_search, c.rotation_gain,
            c.distance_tolerance, c._use_local_coordinates, c.target_search_pause) == (2, 10, None, True, 0.5,
                                                                                        0.05, True, 2.0)
    np.testing.assert_array_equal(c.camera_rotation_to_robot, [0, 0, 0, 1])
    c2 = VisionRGBDFollowerConfig(_use_local_coordinates=False, target_distance=0.7)
    assert c2._use_local_coordinates is False
    c2.to_kompass_cpp()


def test_rgbd_front_end_loop_step(caplog):
    from kompass_core.models import RobotState

    c = VisionRGBDFollower(robot(), ctrl_limits(), VisionRGBDFollowerConfig(_use_local_coordinates=False))
    with caplog.at_level(logging.ERROR):
        assert c.loop_step(current_state=None, detections_2d=[], depth_image=None) is False
    assert "requires current_state" in caplog.text
    # before the camera intrinsics: logged, False
    img = np.zeros((48, 64), np.uint16)
    st = RobotState(x=0.0, y=0.0, yaw=0.0)
    assert c.loop_step(current_state=st, detections_2d=[T.Bbox2D([1, 1], [5, 5])], depth_image=img) is False
    assert not c.has_result() and c.linear_x_control == [0.0] and c.control_till_horizon is None
    assert c.optimal_path() is None and c.result_cost is None
    assert "Failed" in c.logging_info()
    assert c.set_initial_tracking_2d_target(st, T.Bbox2D([1, 1], [5, 5]), img) is False
    assert c.set_initial_tracking_image(st, 3, 3, [], img) is False
    # through the planner's Bbox3D path
    p = c.planner
    assert p.set_initial_tracking(320, 240, [cpp_box(box(2.0, 0.5))])
    r = p.get_tracking_ctrl([cpp_box(box(2.0, 0.5))], T.Velocity2D())
    assert r.is_found and len(r.trajectory.velocities.vx) == 9
    assert c.dist_error == pytest.approx(p.get_errors()[0])


def test_rgb_front_end_loop_step():
    c = VisionRGBFollower(robot(), ctrl_limits(), VisionRGBFollowerConfig(enable_search=False))
    assert c.set_initial_tracking_2d_target(T.Bbox2D([300, 200], [60, 120]))
    assert c.loop_step(detections_2d=[T.Bbox2D([400, 200], [30, 60])])
    assert c.linear_x_control[0] > 0.0 and c.angular_control[0] < 0.0
    assert c.dist_error > 0.0 and c.orientation_error > 0.0
    assert "found control" in c.logging_info()
