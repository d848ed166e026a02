"""The MPPI controller on the device (kc_mppi_*) against the statement tests/mppi_ref.py: every S_k, the
record and U' bit for bit, with 1, 4 and 8 lanes a sample.  The statement's vectorised form is the reference;
tests/test_mppi_cpu.py shows it equal to the loop form.  One reference a case, shared by the three roll-out variants.

Two maps: 37 x 29 (the width is no multiple of 4) with scattered obstacles, and the closed-loop scene of 4.12."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import mppi_ref as mp  # noqa: E402
import worldmap_dist_ref as dref  # noqa: E402
import worldmap_mcl_ref as mref  # noqa: E402
import worldmap_ref as ref  # noqa: E402

RES, ORIGIN = 0.05, (-0.33, 1.7)
W, H, REACH = 37, 29, 5
OCC, EMP = ref.OCCUPIED, ref.EMPTY
ONE = 1 << 16
PEN_D2 = [min(65535, 7 * (25 - d) + (d % 3)) for d in range(26)]           # not monotonic: a wrong index shows
WTAB = [round(65536 * math.exp(-i / 8.0)) for i in range(128)]
MODEL = mp.Model(0, 2 * ONE, 0, 1500, 0, (mref.noise_scale(0.4 * ONE), 0, mref.noise_scale(400.0)))
COSTS = mp.Costs(2, PEN_D2, 11, 3000, 8, 300 << 16, 20, WTAB, 3)


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def small_cls():
    rng = np.random.default_rng(11)
    c = rng.choice(np.int8([OCC, EMP]), size=(W, H), p=[0.04, 0.96]).astype(np.int8)
    c[0, :] = c[-1, :] = OCC
    c[:, 0] = c[:, -1] = OCC
    c[14:23, 10:19] = EMP                                                  # room for the robot
    return c


@pytest.fixture(scope="module")
def small():
    c = small_cls()
    return c, dref.dist2_plane(c, REACH)


def boxed_cls():
    """The small map with a ring of occupied cells two cells around the robot's cell (18, 14)."""
    c = small_cls()
    c[16, 12:17] = c[20, 12:17] = OCC
    c[16:21, 12] = c[16:21, 16] = OCC
    return c


@pytest.fixture(scope="module")
def boxed():
    c = boxed_cls()
    return c, dref.dist2_plane(c, REACH)


@pytest.fixture(scope="module")
def scene():
    c = mp.scene_cls()
    return c, dref.dist2_plane(c, mp.SCENE_REACH)


def straight_path(n, x0=18.0, y0=14.0, dx=0.9, dy=0.35):
    return [round((x0 + dx * j) * ONE) for j in range(n)], [round((y0 + dy * j) * ONE) for j in range(n)]


def nominal(T, F=40000, L=0, Hh=120):
    return [(F + 500 * (t % 3), L, Hh - 40 * (t % 5)) for t in range(T)]


def open_map(cls, reach):
    w, h = cls.shape
    m = kh.WorldMapContext(w, h, RES, ORIGIN)
    m.set_prior(cls)
    m.set_distance(reach)
    return m


def configure(dev, model, costs, px, py):
    dev.set_model(model.f_lo, model.f_hi, model.l_hi, model.h_hi, model.kq, model.s)
    dev.set_costs(costs.r2, costs.pen_d2, costs.pen_far, costs.pen_hit, costs.w_path, costs.qcap, costs.w_goal, costs.wtab,
                  costs.w_shift)
    dev.set_path(px, py)


def same(dev, want, tx, ty, h, U, step, what=""):
    """One device step with each roll-out variant against the statement's (U', Record, S)."""
    wU, wrec, wS = want
    for team in (1, 4, 8):
        dev.set_team(team)
        gU, grec = dev.step(tx, ty, h, U, step)
        gS = dev.costs()
        bad = np.flatnonzero(gS.astype(np.int64) != np.asarray(wS, np.int64))
        assert bad.size == 0, (what, team, bad[:5].tolist(), gS[bad[:5]].tolist(), [int(wS[i]) for i in bad[:5]])
        assert grec.as_tuple() == tuple(wrec), (what, team, grec.as_tuple(), tuple(wrec))
        assert [tuple(int(v) for v in r) for r in gU] == list(wU), (what, team)


def case(cls, plane, reach, K, T, M, model=MODEL, costs=COSTS, pose=(18 * ONE + 700, 14 * ONE - 300, 3000), U=None, step=5,
         seed=9, path=None):
    px, py = path if path is not None else straight_path(M)
    U = nominal(T) if U is None else U
    want = mp.step(plane, K, seed, model, costs, px, py, *pose, U, step)
    with open_map(cls, reach) as m, kh.MppiContext(m, K, T, seed) as dev:
        configure(dev, model, costs, px, py)
        same(dev, want, *pose, U, step, (K, T, M))
    return want


@pytest.mark.parametrize("K,T,M", [(1, 1, 1), (63, 2, 2), (64, 33, 255), (65, 64, 256), (257, 33, 2), (1024, 2, 255)])
def test_shapes_on_the_small_map(small, K, T, M):
    _, rec, _ = case(*small, REACH, K, T, M)
    assert rec.den >= WTAB[0]


@pytest.mark.parametrize("K,T,M", [(1024, 32, 96), (257, 64, 256), (65, 1, 255)])
def test_shapes_on_the_scene(scene, K, T, M):
    px, py = mp.quantise_points(mp.polyline_points())
    pts = (px * 3)[:M], (py * 3)[:M]                                       # the path, repeated to the window's length
    _, rec, _ = case(*scene, mp.SCENE_REACH, K, T, M, mp.scene_model(), mp.scene_costs(), (px[40], py[40], 2900),
                     nominal(T, 90000 if T <= 32 else 30000, 0, 60), 17, 2, pts)
    assert rec.n_hit < K


def test_states_leave_the_map(small):
    """Two cells from the upper edge, heading out through a gap in the border: the samples' later states lie outside the
    map, where d2 is FAR and the index must not be formed.  A second robot stands outside the map altogether."""
    cls, plane = small
    costs = COSTS._replace(r2=0)                                           # only an occupied cell itself hits
    c = cls.copy()
    c[10:20, H - 1] = EMP                                                  # a gap in the border to drive out through
    plane2 = dref.dist2_plane(c, REACH)
    pose = (15 * ONE, (H - 3) * ONE, 16384)                                # heading +y
    U = nominal(12, 110000, 0, 0)
    want = case(c, plane2, REACH, 257, 12, 7, costs=costs, pose=pose, U=U, path=straight_path(7, 15.0, H - 3.0, 0.0, 1.0))
    assert want[1].n_hit < 257
    last = mp.rollout(want[0], *pose)[-1]
    assert mp.cell(last[0], last[1])[1] >= H                               # the blended sequence itself ends outside
    case(cls, plane, REACH, 65, 4, 3, pose=(-3 * ONE, 40 * ONE, 100))


def test_boxed_in_every_sample_hits_at_step_0(boxed):
    cls, plane = boxed
    costs = COSTS._replace(r2=25)                                          # within 5 cells of the ring, whatever the step
    K, T, M = 257, 5, 4
    want = case(cls, plane, REACH, K, T, M, costs=costs)
    U2, rec, S = want
    assert rec.n_hit == K and rec.k_best == 0 and rec.den == K * WTAB[0]
    assert set(int(s) for s in S) == {costs.pen_hit * T + costs.w_goal * (M - 1)}


def test_saturation(small, boxed):
    """pen_hit = 2^20, T = 64 and a path 5000 cells away: every step adds qcap w_path >> 16 = 2^24, every total is cut at
    2^30, and the ties at the cap go to sample 0 and path point 0."""
    cls, plane = small
    costs = COSTS._replace(pen_hit=1 << 20, w_path=1, qcap=1 << 40, w_goal=1 << 20)
    model = MODEL._replace(f_hi=2000)                                      # stays in its room: no hit
    far = ([5000 * ONE + 77 * j for j in range(9)], [4000 * ONE] * 9)
    _, rec, S = case(cls, plane, REACH, 65, 64, 9, model, costs, U=[(1000, 0, 10)] * 64, path=far)
    assert rec.s_min == rec.s_0 == 1 << 30 and rec.k_best == 0 and rec.n_hit == 0
    assert int(S.min()) == int(S.max()) == 1 << 30
    _, rec, _ = case(*boxed, REACH, 64, 64, 9, model, costs._replace(r2=25), U=[(1000, 0, 10)] * 64, path=far)
    assert rec.n_hit == 64 and rec.s_min == (1 << 26) + (8 << 20)          # all hit at step 0: no saturation there


def test_omni_with_lateral_noise(small):
    model = MODEL._replace(f_lo=-ONE, l_hi=ONE, s=(MODEL.s[0], mref.noise_scale(0.3 * ONE), MODEL.s[2]))
    case(*small, REACH, 257, 9, 33, model, U=nominal(9, 30000, -20000, 90))


def test_cone_and_reverse(small):
    """kq > 0 with F_lo < 0: the cone takes |F|, and a sample that backs up may still turn."""
    model = MODEL._replace(f_lo=-ONE, f_hi=ONE, kq=2000, h_hi=3000)
    want = case(*small, REACH, 257, 9, 33, model, U=nominal(9, -30000, 0, 2500))
    assert any(F < 0 for F, _, _ in want[0])
    assert all(abs(Hh) <= (abs(F) * 2000) >> 16 for F, _, Hh in want[0])


def test_heading_wrap(small):
    case(*small, REACH, 65, 6, 9, pose=(18 * ONE, 14 * ONE, 65535), U=nominal(6, 40000, 0, 900))
    case(*small, REACH, 65, 6, 9, pose=(18 * ONE, 14 * ONE, 3), U=nominal(6, 40000, 0, -900))


def test_step_sees_an_update_near_the_robot(small):
    """The plane is refreshed lazily: an update only marks its box, and the next step must find the refreshed cells."""
    cls, plane = small
    K, T, M = 257, 8, 17
    px, py = straight_path(M)
    pose, U = (18 * ONE, 14 * ONE, 3000), nominal(T)
    with open_map(cls, REACH) as m, kh.MppiContext(m, K, T, 4) as dev:
        configure(dev, MODEL, COSTS, px, py)
        same(dev, mp.step(plane, K, 4, MODEL, COSTS, px, py, *pose, U, 0), *pose, U, 0, "before")
        grid = np.full((3, 3), 100, np.int32)                              # a block of occupied cells in front of the robot
        where = (ORIGIN[0] + 21.0 * m.resolution, ORIGIN[1] + 15.0 * m.resolution, 0.0)
        changed = [m.update(grid, where)[0] for _ in range(4)]             # the prior's empty cells stand at e_min = -8, a hit adds 3
        assert changed[:2] == [0, 0] and changed[2] > 0
        now = np.ascontiguousarray(m.planes()[0])                          # the class plane alone: no refresh
        assert (now != cls).any() and (now[19:24, 13:18] == OCC).any()
        plane2 = dref.dist2_plane(now, REACH)
        assert (plane2 != plane).any()
        want = mp.step(plane2, K, 4, MODEL, COSTS, px, py, *pose, U, 1)
        assert list(want[2]) != list(mp.step(plane, K, 4, MODEL, COSTS, px, py, *pose, U, 1)[2])
        same(dev, want, *pose, U, 1, "after the update")


def test_step_after_a_shift(small):
    """The window moves by (3, -2) cells: the plane is wholly dirty, poses and path are given in the new offset."""
    cls, plane = small
    K, T, M = 65, 8, 17
    with open_map(cls, REACH) as m, kh.MppiContext(m, K, T, 4) as dev:
        m.shift(3, -2)
        now = np.ascontiguousarray(m.planes()[0])
        assert (now[:W - 3, 2:] == cls[3:, :H - 2]).all()
        plane2 = dref.dist2_plane(now, REACH, 0)
        px, py = straight_path(M, 15.0, 16.0)
        pose, U = (15 * ONE, 16 * ONE, 3000), nominal(T)
        configure(dev, MODEL, COSTS, px, py)
        same(dev, mp.step(plane2, K, 4, MODEL, COSTS, px, py, *pose, U, 3), *pose, U, 3, "after the shift")


def test_two_contexts_on_one_map(small):
    cls, plane = small
    px, py = straight_path(9)
    pose = (18 * ONE, 14 * ONE, 3000)
    with open_map(cls, REACH) as m, kh.MppiContext(m, 65, 4, 1) as a, kh.MppiContext(m, 257, 7, 2) as b:
        configure(a, MODEL, COSTS, px, py)
        configure(b, MODEL._replace(h_hi=700), COSTS._replace(w_goal=3), px[:5], py[:5])
        for n in range(2):
            same(a, mp.step(plane, 65, 1, MODEL, COSTS, px, py, *pose, nominal(4), n), *pose, nominal(4), n, "a")
            same(b, mp.step(plane, 257, 2, MODEL._replace(h_hi=700), COSTS._replace(w_goal=3), px[:5], py[:5], *pose, nominal(7), n),
                 *pose, nominal(7), n, "b")


def test_refusals_of_a_step(small):
    cls, _ = small
    px, py = straight_path(5)
    with kh.WorldMapContext(W, H, RES, ORIGIN) as m, kh.MppiContext(m, 8, 3, 0) as dev:
        m.set_prior(cls)
        U = nominal(3)
        with pytest.raises(kh.KompassHipError):                            # no model
            dev.step(0, 0, 0, U, 0)
        configure(dev, MODEL, COSTS, px, py)
        with pytest.raises(kh.KompassHipError):                            # the plane is off
            dev.step(0, 0, 0, U, 0)
        m.set_distance(4)                                                  # reach^2 = 16 < c2 = 25
        with pytest.raises(kh.KompassHipError):
            dev.step(0, 0, 0, U, 0)
        m.set_distance(REACH)
        with pytest.raises(IndexError):
            dev.step(0, 0, 65536, U, 0)
        with pytest.raises(IndexError):
            dev.step(0, 0, 0, [(0, 0, 40000)] * 3, 0)
        with pytest.raises(kh.KompassHipError):                            # no costs before a step
            dev.costs()
        dev.step(0, 0, 0, U, 0)


def test_create_destroy_loop(small):
    cls, plane = small
    px, py = straight_path(5)
    pose, U = (18 * ONE, 14 * ONE, 3000), nominal(3)
    want = mp.step(plane, 64, 6, MODEL, COSTS, px, py, *pose, U, 1)
    with open_map(cls, REACH) as m:
        for _ in range(20):
            with kh.MppiContext(m, 64, 3, 6) as dev:
                configure(dev, MODEL, COSTS, px, py)
                gU, grec = dev.step(*pose, U, 1)
                assert grec.as_tuple() == tuple(want[1])


def test_forty_closed_loop_steps_through_the_front_end(scene):
    """kompass_core.control.MPPI over the scene against the statement driven with the inputs the front end quantised:
    the window, the pose, the warm-started sequence and the step number of every call."""
    import kompass_cpp
    from kompass_core.control import MPPI, MPPIConfig
    from kompass_core.mapping import WorldMap
    from kompass_core.models import (AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry, RobotState,
                                     RobotType)
    cls, plane = scene
    res, dt = 0.05, 0.1
    wm = WorldMap(mp.SCENE_W, mp.SCENE_H, res, origin=ORIGIN)
    wm.set_prior(cls)
    robot = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER, geometry_params=np.array([0.1, 0.4]))
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=1000.0, max_decel=1000.0),
                          omega_limits=AngularCtrlLimits(max_vel=1.5, max_steer=0.7, max_acc=1000.0, max_decel=1000.0))
    cfg = MPPIConfig(seed=3, control_horizon=4)
    fe = MPPI(robot, lim, cfg, control_time_step=dt)
    with pytest.raises(TypeError):
        fe.loop_step(current_state=RobotState(x=0.0, y=0.0, yaw=0.0), local_map=np.zeros((4, 4)))
    r32 = float(np.float32(res))
    pts = [(ORIGIN[0] + x * r32, ORIGIN[1] + y * r32) for x, y in mp.SCENE_VERTICES]
    fe.set_path(np.array(pts))
    q = kompass_cpp.control.MPPI.quantise(RobotType.to_kompass_cpp_lib(robot.robot_type), lim.to_kompass_cpp_lib(), dt, res,
                                          cfg.to_kompass_cpp())
    model = mp.Model(*q[:5], tuple(q[5]))
    assert model[:5] == (0, 131072, 0, 1565, 0) and model.s[1] == 0
    t = kompass_cpp.control.MPPI.costs_of(cfg.to_kompass_cpp())
    costs = mp.Costs(t[0], list(t[1]), t[2], t[3], t[4], t[5], t[6], list(t[7]), t[8])
    assert costs == mp.scene_costs()
    state = RobotState(x=pts[0][0], y=pts[0][1], yaw=0.0, speed=0.0)
    prev, x0, short = None, state.x, False
    for n in range(40):
        assert fe.loop_step(current_state=state, local_map=wm)
        i = fe.planner.last_inputs
        U = [tuple(i["u"][3 * k:3 * k + 3]) for k in range(cfg.horizon)]
        assert i["step"] == n and 2 <= len(i["px"]) <= cfg.window
        if len(i["px"]) < cfg.window:                                      # the window has reached the path's end, which the
            # follower's interpolation (a point every 0.01 m = 0.2 cell) leaves within a step of the last vertex
            assert abs(i["px"][-1] - 110 * ONE) <= ONE // 4 and abs(i["py"][-1] - 45 * ONE) <= ONE // 4
        short = short or len(i["px"]) < cfg.window
        assert U == ([(0, 0, 0)] * cfg.horizon if prev is None else mp.shift(prev))
        assert (i["tx"] - i["px"][0]) ** 2 + (i["ty"] - i["py"][0]) ** 2 < (4 * ONE) ** 2   # the window starts beside the robot
        wU, wrec, wS = mp.step(plane, cfg.samples, cfg.seed, model, costs, i["px"], i["py"], i["tx"], i["ty"], i["h"], U, n)
        got = list(fe.planner.last_sequence)
        prev = [tuple(got[3 * k:3 * k + 3]) for k in range(cfg.horizon)]
        assert prev == wU, n
        assert fe.record == tuple(wrec), (n, fe.record, tuple(wrec))
        assert np.array_equal(np.array(fe.planner.sample_costs(), np.int64), np.asarray(wS, np.int64)), n
        vx, om = fe.linear_x_control, fe.angular_control
        assert len(vx) == len(om) == 4 and fe.linear_y_control == [0.0] * 4
        assert vx[0] == pytest.approx(prev[0][0] / 65536.0 * r32 / dt) and om[1] == pytest.approx(prev[1][2] / 65536.0 * 2 * math.pi / dt)
        path = fe.predicted_path()
        want = mp.rollout(prev, i["tx"], i["ty"], i["h"])
        assert len(path) == cfg.horizon
        assert path[-1][0] == pytest.approx(ORIGIN[0] + want[-1][0] / 65536.0 * r32) and path[-1][1] == pytest.approx(
            ORIGIN[1] + want[-1][1] / 65536.0 * r32)
        state = RobotState(x=state.x + vx[0] * math.cos(state.yaw) * dt, y=state.y + vx[0] * math.sin(state.yaw) * dt,
                           yaw=state.yaw + om[0] * dt, speed=vx[0])
    assert state.x > x0 + 20 * r32                                         # it has driven
    assert short                                                           # both kinds of window were seen
