"""PurePursuit on the MI355X: kc_dwa_first_clear_command (one launch) against the oracle's first clear candidate and
against the per-pose path (kc_dwa_check_poses on the host-enumerated poses); the class in the reference test's nine
scenarios (tests/pure_pursuit_test.cpp) lock-step with the restatement of tests/pure_pursuit_ref.py, bit for bit;
the kompass_core front end against the class."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_cpp  # noqa: E402
import kompass_hip as kh  # noqa: E402
import pure_pursuit_ref as ref  # noqa: E402
from oracle import ko  # noqa: E402

SHAPES = [(kh.CYLINDER, [0.2, 0.4]), (kh.BOX, [0.5, 0.3, 0.4]), (kh.SPHERE, [0.25])]
DT = 0.1


def _cands(rng, n):
    if n == 1:
        return np.array([0.6]), np.array([0.0]), np.array([0.2])
    nominal = (0.8, 0.1, 0.3)
    m = (n - 1) // 4
    offs = ref.search_offsets(0.05, m)
    c = np.array(ref.candidates(nominal, offs, omni=True))
    assert len(c) == n
    return c[:, 0], c[:, 1], c[:, 2]


def _check(ctx, coll, start, vx, vy, om, H):
    got = ctx.first_clear_command(start, vx, vy, om, H, DT)
    cands = list(zip(vx, vy, om))
    want = ref.first_clear(coll, start, cands, H, DT)
    assert got == want, (got, want, len(cands), H)
    if H > 0 and len(cands) * H <= 200_000:
        x, y, t = ref.poses(start, cands, H, DT)
        hit = ctx.check_poses(x, y, t).reshape(len(cands), H).any(axis=1)
        clear = np.nonzero(~hit)[0]
        assert got == (int(clear[0]) if len(clear) else -1)
    return got


@pytest.mark.parametrize("shape,dims", SHAPES)
def test_first_clear_command_kernel_level(shape, dims):
    rng = np.random.default_rng(17)
    start = (0.3, -0.2, 0.4)
    # a ring of obstacles 1.2 m out with a gap behind the robot: forward candidates are blocked, the reverse pass
    # finds the gap some way in
    ang = rng.uniform(0, 2 * math.pi, 1500)
    keep = np.abs(((ang - (start[2] + math.pi)) + math.pi) % (2 * math.pi) - math.pi) > 0.5
    r = rng.uniform(1.1, 1.5, keep.sum())
    cloud = np.stack([start[0] + r * np.cos(ang[keep]), start[1] + r * np.sin(ang[keep]),
                      rng.uniform(-0.1, 0.1, keep.sum())], 1).astype(np.float32)
    ctx = kh.DwaContext(shape, dims, octree_res=0.1, max_samples=4, max_points=4)
    coll = ko.Collision(shape, dims, res=0.1)
    # no sensor data yet: nothing is hit
    assert ctx.first_clear_command(start, [0.5], [0.0], [0.1], 10, DT) == 0
    ctx.set_points(start + (0.0,), cloud)
    coll.update_state(*start)
    coll.update_points(cloud, True)
    seen = set()
    for n in (1, 41, 4001):
        vx, vy, om = _cands(rng, n)
        for H in (0, 1, 10, 100):
            if n == 4001 and H == 100:
                continue  # (below: the deep reverse-pass case at H = 100)
            seen.add(_check(ctx, coll, start, vx, vy, om, H))
    # a clear index deep in the reverse pass (diff-drive order, 1000 offsets: the reverse pass starts at 1001): a
    # ring with a narrow gap behind the robot, off its axis
    rng2 = np.random.default_rng(17)
    ang = rng2.uniform(0, 2 * math.pi, 3000)
    keep = np.abs(((ang - (start[2] + math.pi + 0.3)) + math.pi) % (2 * math.pi) - math.pi) > 0.35
    r = rng2.uniform(1.1, 1.5, keep.sum())
    gap = np.stack([start[0] + r * np.cos(ang[keep]), start[1] + r * np.sin(ang[keep]),
                    rng2.uniform(-0.1, 0.1, keep.sum())], 1).astype(np.float32)
    ctx.set_points(start + (0.0,), gap)
    coll.update_points(gap, True)
    c = np.array(ref.candidates((0.8, 0.0, 0.0), ref.search_offsets(0.0005, 1000), omni=False))
    deep = _check(ctx, coll, start, c[:, 0], c[:, 1], c[:, 2], 100)
    assert deep > 1001 + 100, deep
    # none clear: every candidate drives into a closed ring
    ring = np.stack([start[0] + 1.0 * np.cos(np.linspace(0, 6.28, 800)),
                     start[1] + 1.0 * np.sin(np.linspace(0, 6.28, 800)), np.zeros(800)], 1).astype(np.float32)
    ctx.set_points(start + (0.0,), ring)
    coll.update_points(ring, True)
    assert _check(ctx, coll, start, *_cands(rng, 41), 100) == -1
    assert 0 in seen
    ctx.close()


def test_first_clear_command_scan_and_tilted_mount():
    rng = np.random.default_rng(5)
    ang = np.linspace(0, 2 * math.pi, 720, endpoint=False)
    ranges = 1.0 + 0.6 * rng.random(720)
    start = (0.1, 0.2, -0.3)
    s = math.sin(0.2)
    for srot in [(0, 0, 0, 1), (0.0, s, 0.0, math.cos(0.2))]:
        for shape, dims in SHAPES:
            ctx = kh.DwaContext(shape, dims, (0.05, 0.0, 0.1), srot, 0.05, max_samples=4, max_points=4)
            coll = ko.Collision(shape, dims, (0.05, 0.0, 0.1), srot, 0.05)
            ctx.set_scan(start + (0.0,), ranges, ang, 10.0)
            coll.update_state(*start)
            coll.update_scan(ranges, ang)
            for n in (1, 41):
                vx, vy, om = _cands(rng, n)
                for H in (0, 1, 10, 100):
                    _check(ctx, coll, start, vx * 0.5, vy, om, H)
            ctx.close()


def test_one_launch_refusals_match_the_pose_path():
    ctx = kh.DwaContext(kh.CYLINDER, [0.2, 0.4], octree_res=0.01, max_samples=4, max_points=4)
    ctx.set_points((0, 0, 0, 0), np.float32([[1.0, 0.0, 0.0]]))
    # a window of more than 8190 cells per side: KC_ERR_RANGE from both
    with pytest.raises(IndexError, match="collision window"):
        ctx.first_clear_command((0, 0, 0), [1000.0], [0.0], [0.0], 100, DT)
    with pytest.raises(IndexError, match="collision window"):
        ctx.check_poses([0.0, 10000.0], [0.0, 0.0], [0.0, 0.0])
    # ... and both accept the same scene within it
    assert ctx.first_clear_command((0, 0, 0), [1.0], [0.0], [0.0], 10, DT) == -1
    assert ctx.check_poses([0.1, 1.0], [0.0, 0.0], [0.0, 0.0]).any()
    ctx.close()


# ---------------------------------------------------------------- lane layouts of pp_search_kernel
# A candidate owns G lanes, G the power of two >= H + 1 capped at 64; poses past 64 go through chunks of 64 with the
# pose carried across by the segment's last lane.  The horizons: G = 4, 8, 16, 32, 64 with the segment exactly full
# (H + 1 == G) and one short of / one past it; one full chunk (63), a second chunk of one lane (64) and of two (65);
# two full chunks and a third of one and two lanes (127, 128, 129); four chunks (200).
HORIZONS = (2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 65, 127, 128, 129, 200)
START = (0.3, -0.2, 0.4)


def _target_poses(H):
    t = {1, H}
    if H > 64:
        t |= {64, 65}
    if H > 128:
        t |= {128, 129}
    return sorted(t)


def _which_pose_scene(H):
    """(targets, candidates, cloud): one candidate per target pose index j, driving 0.8 m a step along its own arc
    (its own heading in the body frame -- vy != 0 -- and its own omega != 0), and a small cluster of points exactly
    where its pose j is: the steps are longer than robot plus cluster, so pose j is the candidate's only pose that
    touches anything.  The candidate after them backs away slowly from all of it."""
    targets = _target_poses(H)
    cands, pts = [], []
    for k, j in enumerate(targets):
        phi = 1.9 if j == 1 else -1.0 + 2.0 * k / len(targets)
        om = (0.08 + 0.02 * k) * (1 if k % 2 else -1)
        c = (8.0 * math.cos(phi), 8.0 * math.sin(phi), om)
        x, y, _ = ref.poses(START, [c], H, DT)
        pts += [(x[j - 1] + dx, y[j - 1] + dy, 0.0) for dx, dy in ((0, 0), (0.03, 0), (-0.03, 0), (0, 0.03), (0, -0.03))]
        cands.append(c)
    cands.append((-0.5, -0.3, 0.1))
    return targets, cands, np.asarray(pts, np.float32)


def _hit_poses(coll, cand, H):
    x, y, t = ref.poses(START, [cand], H, DT)
    return [j + 1 for j in range(H) if coll.check_at(x[j], y[j], t[j])]


@pytest.mark.parametrize("shape,dims", SHAPES)
def test_first_clear_command_horizons_and_which_pose_hits(shape, dims):
    ctx = kh.DwaContext(shape, dims, octree_res=0.1, max_samples=4, max_points=4)
    coll = ko.Collision(shape, dims, res=0.1)
    coll.update_state(*START)
    for H in HORIZONS:
        targets, cands, cloud = _which_pose_scene(H)
        ctx.set_points(START + (0.0,), cloud)
        coll.update_points(cloud, True)
        # on the reference alone: candidate k is hit by its pose targets[k] and by no other, the last by none
        hit = [_hit_poses(coll, c, H) for c in cands]
        assert hit == [[j] for j in targets] + [[]], (H, hit)
        first_hits = {h[0] for h in hit if h}
        assert first_hits >= {1, H} | ({64, 65} if H > 64 else set()) | ({128, 129} if H > 128 else set())
        vx, vy, om = (np.array(v) for v in zip(*cands))
        assert _check(ctx, coll, START, vx, vy, om, H) == len(cands) - 1
        # ... and without the clear candidate: none
        assert _check(ctx, coll, START, vx[:-1], vy[:-1], om[:-1], H) == -1
        # each of them alone (a hit that only a neighbour segment of the wavefront saw would pass above)
        for k in range(len(cands) - 1):
            assert ctx.first_clear_command(START, vx[k:k + 1], vy[k:k + 1], om[k:k + 1], H, DT) == -1, (H, targets[k])
    ctx.close()


@pytest.mark.parametrize("shape,dims", [SHAPES[0], SHAPES[1]])
def test_first_clear_command_horizons_on_the_tilted_mount(shape, dims):
    rng = np.random.default_rng(5)
    ang = np.linspace(0, 2 * math.pi, 720, endpoint=False)
    ranges = 1.0 + 0.6 * rng.random(720)
    start = (0.1, 0.2, -0.3)
    srot = (0.0, math.sin(0.2), 0.0, math.cos(0.2))
    ctx = kh.DwaContext(shape, dims, (0.05, 0.0, 0.1), srot, 0.05, max_samples=4, max_points=4)
    coll = ko.Collision(shape, dims, (0.05, 0.0, 0.1), srot, 0.05)
    ctx.set_scan(start + (0.0,), ranges, ang, 10.0)
    coll.update_state(*start)
    coll.update_scan(ranges, ang)
    # Pitched by 0.4 rad, the beams ahead of and behind the sensor leave the robot's height; the ones to its sides stay
    # level.  So the candidates drive sideways, the fast ones first: they reach the ring 1 to 1.6 m away within the
    # horizon -- the fastest some steps before its end, the next ones nearer to it -- and the slow ones do not.
    n = 24
    answers = set()
    for H in HORIZONS:
        speed = np.linspace(1.9, 0.4, n) * (1.3 / (DT * H))
        vy = speed * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        vx = rng.uniform(-0.1, 0.1, n) * speed
        om = rng.uniform(-0.5, 0.5, n) / (DT * H)
        want = ref.first_clear(coll, start, list(zip(vx, vy, om)), H, DT)
        assert want > 0, (H, want)  # on the reference: some candidates collide, one further down is clear
        answers.add(want)
        assert _check(ctx, coll, start, vx, vy, om, H) == want
        assert _check(ctx, coll, start, vx[:want], vy[:want], om[:want], H) == -1
    assert len(answers) > 1
    ctx.close()


def _wall_scene(rng, n, clear_at):
    """n candidates that drive into a wall 0.55 m in front of the robot within their first three poses, but for the
    one at `clear_at`, which backs away."""
    th = START[2] + np.arange(-1.2, 1.2, 0.02)
    wall = np.stack([START[0] + 0.55 * np.cos(th), START[1] + 0.55 * np.sin(th), np.zeros(len(th))], 1).astype(np.float32)
    vx, vy, om = rng.uniform(1.5, 2.2, n), rng.uniform(-0.1, 0.1, n), rng.uniform(-0.3, 0.3, n)
    if clear_at is not None:
        vx[clear_at], vy[clear_at], om[clear_at] = -0.5, 0.02, 0.1
    return wall, vx, vy, om


# 4 wavefronts a workgroup, 64 / G candidates a wavefront, at most 4096 workgroups: 16384 candidates at G = 64 (H = 63)
# and 32768 at G = 32 (H = 31) before the grid-stride loop runs a second round
@pytest.mark.parametrize("H,n,clear_at", [(63, 3, 2), (63, 4, 3), (63, 5, 4), (63, 16401, 16400), (63, 16401, 7),
                                          (31, 1, 0), (31, 2, 1), (31, 3, 2), (31, 32771, 32770), (31, 32771, None)])
def test_first_clear_command_candidate_counts(H, n, clear_at):
    shape, dims = SHAPES[1]
    rng = np.random.default_rng(n + H)
    wall, vx, vy, om = _wall_scene(rng, n, clear_at)
    ctx = kh.DwaContext(shape, dims, octree_res=0.1, max_samples=4, max_points=4)
    coll = ko.Collision(shape, dims, res=0.1)
    ctx.set_points(START + (0.0,), wall)
    coll.update_state(*START)
    coll.update_points(wall, True)
    # on the reference: everyone but the clear one is stopped within three poses, the clear one by nothing
    for i in range(n):
        if i == clear_at:
            assert _hit_poses(coll, (vx[i], vy[i], om[i]), H) == []
        else:
            x, y, t = ref.poses(START, [(vx[i], vy[i], om[i])], 3, DT)
            assert any(coll.check_at(x[j], y[j], t[j]) for j in range(3)), i
    assert _check(ctx, coll, START, vx, vy, om, H) == (-1 if clear_at is None else clear_at)
    ctx.close()


def _gap_ring(rng, start):
    """the ring of test_first_clear_command_kernel_level around a start with any yaw: the gap lies behind the robot"""
    back = math.atan2(-math.sin(start[2]), -math.cos(start[2]))  # (the host libm's reduction of the yaw)
    ang = rng.uniform(0, 2 * math.pi, 1500)
    keep = np.abs(((ang - back) + math.pi) % (2 * math.pi) - math.pi) > 0.5
    r = rng.uniform(1.1, 1.5, keep.sum())
    return np.stack([start[0] + r * np.cos(ang[keep]), start[1] + r * np.sin(ang[keep]),
                     rng.uniform(-0.1, 0.1, keep.sum())], 1).astype(np.float32)


@pytest.mark.parametrize("shape,dims", SHAPES)
def test_first_clear_command_yaws_beyond_the_device_trig(shape, dims):
    """|yaw| + omega_max * dt * H >= 1e8: the kernel reads cos / sin from a table the host's libm filled, one row a
    candidate.  The reference's Path::State::update uses that libm too."""
    rng = np.random.default_rng(23)
    ctx = kh.DwaContext(shape, dims, octree_res=0.1, max_samples=4, max_points=4)
    coll = ko.Collision(shape, dims, res=0.1)
    vx, vy, om = _cands(rng, 41)
    seen = []
    for yaw in (1.5e8, -2.0e8):
        start = (0.3, -0.2, yaw)
        cloud = _gap_ring(rng, start)
        ctx.set_points(start + (0.0,), cloud)
        coll.update_state(*start)
        coll.update_points(cloud, True)
        for H in (10, 100):
            k = 3.0 if H == 10 else 1.0  # (fast enough to reach the ring in ten steps)
            seen.append(_check(ctx, coll, start, vx * k, vy * k, om, H))
    # a small start yaw, one candidate whose omega alone takes the yaw past 1e8: first in the list, and last
    start = (0.3, -0.2, 0.4)
    cloud = _gap_ring(rng, start)
    ctx.set_points(start + (0.0,), cloud)
    coll.update_state(*start)
    coll.update_points(cloud, True)
    for H in (10, 100):
        assert 1.2e8 * float(np.float32(DT)) * H >= 1e8 and abs(om).max() < 10.0
        wild = (np.array([0.9]), np.array([0.0]), np.array([1.2e8]))
        seen.append(_check(ctx, coll, start, *(np.concatenate([a, w]) for a, w in zip((vx, vy, om), wild)), H))
        seen.append(_check(ctx, coll, start, *(np.concatenate([w, a]) for a, w in zip((vx, vy, om), wild)), H))
        seen.append(_check(ctx, coll, start, vx, vy, om, H))  # (the same list on the device's own trig)
    assert any(i > 0 for i in seen), seen  # some answers lie behind candidates that collide
    ctx.close()


# ---------------------------------------------------------------- class level
TYPES = {"Ackermann": ref.ACKERMANN, "DiffDrive": ref.DIFFERENTIAL_DRIVE, "Omni": ref.OMNI}
CPP_TYPES = {ref.ACKERMANN: kompass_cpp.control.ControlType.ACKERMANN,
             ref.DIFFERENTIAL_DRIVE: kompass_cpp.control.ControlType.DIFFERENTIAL_DRIVE,
             ref.OMNI: kompass_cpp.control.ControlType.OMNI}
CFG = dict(wheel_base=0.34, speed_regulation_curvature=0.5, speed_regulation_angular=0.5,
           max_point_interpolation_distance=0.05, path_segment_length=1.0, goal_dist_tolerance=0.3)
OBSTACLES = {"Straight": (4.0, 0.0), "UTurn": (10.0, 0.0), "Circle": (5.0, 8.5)}


def _frange(a, b, step):
    out, v = [], a
    while v <= b:
        out.append(v)
        v += step
    return out


def path_points(name):
    # controller_test_helpers.h:29-73
    if name == "Straight":
        return [(x, 0.0, 0.0) for x in _frange(0.0, 10.0, 0.5)]
    if name == "UTurn":
        pts = [(x, 0.0, 0.0) for x in _frange(0.0, 5.0, 0.5)]
        pts += [(5.0 + 5.5 * math.cos(a), 2.5 + 5.5 * math.sin(a), 0.0) for a in _frange(-math.pi / 2, math.pi / 2, 0.2)]
        x = 5.0
        while x >= 0.0:
            pts.append((x, 5.0, 0.0))
            x -= 0.5
        return pts
    return [(10.0 * math.cos(a), 10.0 * math.sin(a), 0.0) for a in _frange(0.0, 3.0 * math.pi / 2.0, 0.1)]


def round_obstacle(x, y, radius, res=0.1):
    # controller_test_helpers.h:75-89
    cloud, r = [], 0.0
    while r <= radius:
        th = 0.0
        while th < 2 * math.pi:
            cloud.append((x + r * math.cos(th), y + r * math.sin(th), 0.0))
            th += res / r if r > 0 else float("inf")
        if r == 0:
            cloud.append((x, y, 0.0))
        r += res
    return np.asarray(cloud, np.float32)


def make_cpp(ctype):
    lim = kompass_cpp.control.ControlLimitsParams(
        vel_x_ctr_params=kompass_cpp.control.LinearVelocityControlParams(1.0, 2.0, 2.0),
        vel_y_ctr_params=kompass_cpp.control.LinearVelocityControlParams(1.0, 2.0, 2.0),
        omega_ctr_params=kompass_cpp.control.AngularVelocityControlParams(0.7, 1.0, 2.0, 2.0))
    cfg = kompass_cpp.control.PurePursuitConfig()
    cfg.from_dict(CFG)
    return kompass_cpp.control.PurePursuit(
        control_type=CPP_TYPES[ctype], control_limits=lim, robot_shape_type=kompass_cpp.types.RobotGeometry.CYLINDER,
        robot_dimensions=[0.1, 0.4], sensor_position_robot=[0.0, 0.0, 0.0], sensor_rotation_robot=[0, 0, 0, 1],
        octree_res=0.1, config=cfg)


STATUS = {kompass_cpp.control.FollowingStatus.GOAL_REACHED: ref.GOAL_REACHED,
          kompass_cpp.control.FollowingStatus.COMMAND_FOUND: ref.COMMAND_FOUND,
          kompass_cpp.control.FollowingStatus.NO_COMMAND_POSSIBLE: ref.NO_COMMAND_POSSIBLE}


@pytest.mark.parametrize("avoid", [False, True])
@pytest.mark.parametrize("pname", ["Straight", "UTurn", "Circle"])
@pytest.mark.parametrize("rname", ["Ackermann", "DiffDrive", "Omni"])
def test_reference_scenarios_lock_step(rname, pname, avoid):
    ctype = TYPES[rname]
    pp = make_cpp(ctype)
    rf = ref.PurePursuitRef(ctype, (1.0, 2.0, 2.0), kh.CYLINDER,
                            [0.1, 0.4], res=0.1, **CFG)
    pts = path_points(pname)
    path = kompass_cpp.types.Path(points=np.asarray(pts, np.float32))
    pp.set_current_path(path)
    rf.set_path(pts)
    p32 = np.asarray(pts, np.float32)
    start_yaw = float(np.arctan2(p32[1, 1] - p32[0, 1], p32[1, 0] - p32[0, 0]).astype(np.float32))
    state = (float(p32[0, 0]) + (0.2 if pname == "Circle" else 0.0), float(p32[0, 1]), start_yaw)
    cloud = round_obstacle(*OBSTACLES[pname], 0.3) if avoid else None
    checker = ko.Collision(kh.CYLINDER, [0.1, 0.4], res=0.1)
    if avoid:
        checker.update_state(0.0, 0.0, 0.0)
        checker.update_points(cloud, True)
    vel = (0.0, 0.0, 0.0)
    steps, reached = 0, False
    while not reached and steps < 1000:
        st = kompass_cpp.types.State(state[0], state[1], state[2], 0.0)
        if avoid:
            pp.set_current_state(st)
            r = pp.execute(DT, cloud)
        else:
            r = pp.execute(st, DT)
        rf.state, rf.vel = state, vel
        ws, wc = rf.execute_with_points(DT, cloud) if avoid else rf.execute(DT)
        v = r.velocity_command
        got = (v.vx, v.vy, v.omega)
        assert STATUS[r.status] == ws and got == wc, (steps, STATUS[r.status], ws, got, wc)
        if ws == ref.GOAL_REACHED:
            reached = True
            break
        assert ws != ref.NO_COMMAND_POSSIBLE
        pp.set_current_velocity(v)
        vel = got
        state = ref.apply_control(state, got, DT)
        if avoid:
            assert not checker.check_at(*state), (steps, state)
        steps += 1
    assert reached or steps == 1000


def test_front_end_loop_step_matches_the_class():
    from kompass_core.control import PurePursuit, PurePursuitConfig
    from kompass_core.datatypes.laserscan import LaserScanData
    from kompass_core.models import (AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry,
                                     RobotState, RobotType)

    robot = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER,
                  geometry_params=np.array([0.1, 0.4]))
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=2.0, max_decel=2.0),
                          omega_limits=AngularCtrlLimits(max_vel=1.0, max_steer=0.7, max_acc=2.0, max_decel=2.0))
    cfg = PurePursuitConfig(wheel_base=robot.wheelbase, lookahead_distance=1.0)
    pts = path_points("Straight")
    cloud = round_obstacle(2.0, 0.0, 0.3)
    ang = np.linspace(-math.pi, math.pi, 360, endpoint=False)
    ranges = np.full(360, 8.0)
    ranges[np.abs(ang) < 0.15] = 1.5
    scan = LaserScanData(ranges=ranges, angles=ang)
    for kind in ("laser_scan", "point_cloud"):
        fe = PurePursuit(robot, lim, config=cfg, control_time_step=DT)
        fe.set_path(np.asarray(pts))
        direct = kompass_cpp.control.PurePursuit(
            control_type=kompass_cpp.control.ControlType.DIFFERENTIAL_DRIVE, control_limits=lim.to_kompass_cpp_lib(),
            robot_shape_type=kompass_cpp.types.RobotGeometry.CYLINDER, robot_dimensions=[0.1, 0.4],
            sensor_position_robot=[0.0, 0.0, 0.0], sensor_rotation_robot=[0, 0, 0, 1], octree_res=0.1,
            config=cfg.to_kompass_cpp())
        direct.set_current_path(kompass_cpp.types.Path(points=np.asarray(pts, np.float32)))
        state = RobotState(x=0.0, y=0.0, yaw=0.0, speed=0.0)
        for _ in range(40):
            if kind == "laser_scan":
                ok = fe.loop_step(current_state=state, laser_scan=scan)
                sensor = kompass_cpp.types.LaserScan(ranges=scan.ranges, angles=scan.angles)
            else:
                ok = fe.loop_step(current_state=state, point_cloud=cloud)
                sensor = cloud
            assert ok
            direct.set_current_state(state.x, state.y, state.yaw, state.speed)
            direct.set_current_velocity(kompass_cpp.types.Velocity2D(vx=state.vx, vy=state.vy, omega=state.omega))
            r = direct.execute(DT, sensor)
            want = (r.velocity_command.vx, r.velocity_command.vy, r.velocity_command.omega)
            got = (fe.linear_x_control[0], fe.linear_y_control[0], fe.angular_control[0])
            assert got == want
            state.simulate(v_x=got[0], v_y=got[1], omega=got[2], dt=DT)
