"""Moving obstacles in the MPPI controller on the device (kc_mppi_set_movers; DESIGN.md 4.12 rules 13 to 18) against the
statement tests/mppi_movers_ref.py: every S_k, the record with n_hit_moving and U' bit for bit, with 1, 4 and 8 lanes a
sample.  The statement's vectorised form is the reference; tests/test_mppi_movers_cpu.py shows it equal to the loop form
and, with no mover, to tests/mppi_ref.py.  One reference a case, shared by the three roll-out variants.

The map is the 37 x 29 one of tests/test_mppi_gpu.py (the width is no multiple of 4), rebuilt here; the robot stands in
its free room, cells 14 .. 22 x 10 .. 18."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import mppi_movers_ref as mm  # noqa: E402
import mppi_ref as mp  # noqa: E402
import worldmap_dist_ref as dref  # noqa: E402
import worldmap_mcl_ref as mref  # noqa: E402
import worldmap_ref as ref  # noqa: E402

RES, ORIGIN = 0.05, (-0.33, 1.7)
W, H, REACH = 37, 29, 5
OCC, EMP = ref.OCCUPIED, ref.EMPTY
ONE = 1 << 16
PEN_D2 = [min(65535, 7 * (25 - d) + (d % 3)) for d in range(26)]
WTAB = [round(65536 * math.exp(-i / 8.0)) for i in range(128)]
MODEL = mp.Model(0, 2 * ONE, 0, 1500, 0, (mref.noise_scale(0.4 * ONE), 0, mref.noise_scale(400.0)))
COSTS = mp.Costs(2, PEN_D2, 11, 3000, 8, 300 << 16, 20, WTAB, 3)
POSE = (18 * ONE + 700, 14 * ONE - 300, 3000)
PEN_MV = 2500


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def small_cls():
    rng = np.random.default_rng(11)
    c = rng.choice(np.int8([OCC, EMP]), size=(W, H), p=[0.04, 0.96]).astype(np.int8)
    c[0, :] = c[-1, :] = OCC
    c[:, 0] = c[:, -1] = OCC
    c[14:23, 10:19] = EMP
    return c


@pytest.fixture(scope="module")
def small():
    c = small_cls()
    return c, dref.dist2_plane(c, REACH)


@pytest.fixture(scope="module")
def boxed():
    """The small map with a ring of occupied cells two cells around the robot's cell (18, 14)."""
    c = small_cls()
    c[16, 12:17] = c[20, 12:17] = OCC
    c[16:21, 12] = c[16:21, 16] = OCC
    return c, dref.dist2_plane(c, REACH)


def straight_path(n, x0=18.0, y0=14.0, dx=0.9, dy=0.35):
    return [round((x0 + dx * j) * ONE) for j in range(n)], [round((y0 + dy * j) * ONE) for j in range(n)]


def nominal(T, F=40000, L=0, Hh=120):
    return [(F + 500 * (t % 3), L, Hh - 40 * (t % 5)) for t in range(T)]


def movers_around(n, around=POSE, seed=0, spread=9):
    """n movers within `spread` cells of a place, walking up to half a cell a step; hit distances 0 to 3 cells, ramps up
    to 40 cells^2 wide with tops up to 40 * 30: some samples are ended, most pay a soft term from several movers.  The
    first stands five cells beside the place, so that a list of one is felt too."""
    rng = np.random.default_rng(100 + seed + n)
    rows = [(around[0] + 2 * ONE, around[1] - 5 * ONE, 1000, -2000, ONE, 40 << 16, 7 * ONE)]
    for _ in range(n - 1):
        hq = (int(rng.integers(0, 4)) ** 2 << 16) + int(rng.integers(0, ONE))
        sq = hq + int(rng.integers(1, 40 * ONE))
        rows.append((around[0] + int(rng.integers(-spread * ONE, spread * ONE)), around[1] + int(rng.integers(-spread * ONE, spread * ONE)),
                     int(rng.integers(-ONE // 2, ONE // 2)), int(rng.integers(-ONE // 2, ONE // 2)), hq, sq, int(rng.integers(0, 30 * ONE))))
    return mm.movers(rows, PEN_MV)


def open_map(cls, reach=REACH):
    w, h = cls.shape
    m = kh.WorldMapContext(w, h, RES, ORIGIN)
    m.set_prior(cls)
    m.set_distance(reach)
    return m


def configure(dev, model, costs, px, py, mv=None):
    dev.set_model(model.f_lo, model.f_hi, model.l_hi, model.h_hi, model.kq, model.s)
    dev.set_costs(costs.r2, costs.pen_d2, costs.pen_far, costs.pen_hit, costs.w_path, costs.qcap, costs.w_goal, costs.wtab,
                  costs.w_shift)
    dev.set_path(px, py)
    if mv is not None:
        dev.set_movers(*mv[:7], mv.pen_hit)


def same(dev, want, tx, ty, h, U, step, what=""):
    """One device step with each roll-out variant against the statement's (U', Record, S)."""
    wU, wrec, wS = want
    for team in (1, 4, 8):
        dev.set_team(team)
        gU, grec = dev.step(tx, ty, h, U, step)
        gS = dev.costs()
        bad = np.flatnonzero(gS.astype(np.int64) != np.asarray(wS, np.int64))
        assert bad.size == 0, (what, team, bad[:5].tolist(), gS[bad[:5]].tolist(), [int(wS[i]) for i in bad[:5]])
        assert grec.as_tuple() + (int(grec.n_hit_moving),) == tuple(wrec), (what, team, grec.as_tuple(), grec.n_hit_moving, tuple(wrec))
        assert [tuple(int(v) for v in r) for r in gU] == list(wU), (what, team)


def case(cls, plane, K, T, M, mv, model=MODEL, costs=COSTS, pose=POSE, U=None, step=5, seed=9, path=None):
    px, py = path if path is not None else straight_path(M)
    U = nominal(T) if U is None else U
    want = mm.step(plane, K, seed, model, costs, px, py, *pose, U, step, mv)
    with open_map(cls) as m, kh.MppiContext(m, K, T, seed) as dev:
        configure(dev, model, costs, px, py, mv)
        same(dev, want, *pose, U, step, (K, T, M, len(mv.ox)))
    return want


@pytest.mark.parametrize("N", [1, 3, 7, 8, 9, 63, 64])
def test_mover_counts_around_the_team_sizes_and_the_cap(small, N):
    U = nominal(33, 9000)                                                  # slowly: most samples stay in the room
    _, rec, S = case(*small, 65, 33, 255, movers_around(N), U=U)
    free = mp.step(small[1], 65, 9, MODEL, COSTS, *straight_path(255), *POSE, U, 5)[2]
    assert (np.asarray(S) != np.asarray(free)).any()                       # the list is felt
    print(f"N = {N}: n_hit {rec.n_hit}, n_hit_moving {rec.n_hit_moving}")
    assert rec.n_hit_moving <= rec.n_hit
    if N >= 9:
        assert rec.n_hit_moving > 0                                        # both branches of rule 16 are taken


@pytest.mark.parametrize("K,T", [(1, 1), (63, 2), (257, 64), (1024, 2)])
def test_shapes(small, K, T):
    case(*small, K, T, 17, movers_around(9, seed=K))


# ---- one sample (no noise), positions in integers: from cell (18, 14) one cell along +x to (19, 14) ----
ON_CELL = (18 * ONE, 14 * ONE, 0)
Q9 = 9 << 16                                                               # a mover at rest at (22, 14): dx = -3 * 256


def one(small, mv, U=((ONE, 0, 0),), path=None):
    return case(*small, 1, len(U), 1, mv, pose=ON_CELL, U=list(U), path=path or ([30 * ONE], [14 * ONE]))


def test_the_thresholds_exactly(small):
    at = lambda hq, sq, g: mm.movers([(22 * ONE, 14 * ONE, 0, 0, hq, sq, g)], 777)   # noqa: E731
    free = int(one(small, mm.NONE)[2][0])
    U2, rec, S = one(small, at(Q9, Q9 + (5 << 16), 1 << 20))               # q == hq: a hit
    assert (int(S[0]), rec.n_hit, rec.n_hit_moving) == (777, 1, 1)
    _, rec, S = one(small, at(Q9 - 1, Q9 - 1 + (5 << 16), 1 << 20))        # q == hq + 1: ((5 * 2^16 - 1) >> 16) 2^20 >> 16
    assert (int(S[0]), rec.n_hit) == (free + 64, 0)
    assert int(one(small, at(0, Q9 + 1, 1 << 32))[2][0]) == free           # q == sq - 1: (1 >> 16) g
    assert int(one(small, at(0, Q9 + ONE, 1 << 20))[2][0]) == free + 16    # a whole cell^2 inside
    assert int(one(small, at(0, Q9, 1 << 32))[2][0]) == free               # q == sq: nothing
    far = lambda hq: mm.movers([(18 * ONE + (1 << 29), 14 * ONE, 0, 0, hq, 1 << 40, 1 << 12)], 777)   # noqa: E731
    _, rec, S = one(small, far(0))                                         # 8192 cells away: q at the cap 2^40 == sq: nothing
    assert (int(S[0]), rec.n_hit) == (free, 0)
    _, rec, S = one(small, far(1 << 40))                                   # ... and == hq: a hit
    assert (int(S[0]), rec.n_hit_moving) == (777, 1)


def test_a_mover_on_the_robot_at_step_0(small):
    """Every sample hits at t = 0 (a step is at most two cells, the hit distance five): the wavefronts leave the loop after
    its first pass, and nothing but pen_hit_mv T and the terminal term with jm = 0 is added."""
    K, T, M = 257, 5, 4
    mv = mm.movers([(POSE[0], POSE[1], 0, 0, 25 << 16, 25 << 16, 0)], PEN_MV)
    _, rec, S = case(*small, K, T, M, mv)
    assert rec.n_hit == rec.n_hit_moving == K and rec.k_best == 0 and rec.den == K * WTAB[0]
    assert set(int(s) for s in S) == {PEN_MV * T + COSTS.w_goal * (M - 1)}


def test_a_state_that_hits_the_plane_and_a_mover_at_once(boxed):
    K, T, M = 257, 5, 4
    costs = COSTS._replace(r2=25)                                          # within 5 cells of the ring, whatever the step
    mv = mm.movers([(POSE[0], POSE[1], 0, 0, 25 << 16, 25 << 16, 0)], PEN_MV)
    _, rec, S = case(*boxed, K, T, M, mv, costs=costs)
    assert rec.n_hit == K and rec.n_hit_moving == 0
    assert set(int(s) for s in S) == {costs.pen_hit * T + costs.w_goal * (M - 1)}


def test_a_meeting_at_the_last_step_and_one_a_step_later(small):
    """Rule 14's t + 1.  The robot walks +x a cell a step from (16, 14), the mover -x a cell a step; hq = 0.  From (22, 14)
    they meet at (19, 14) after step 2 = T - 1; from (24, 14) they would meet after step 3 = T."""
    U = ((ONE, 0, 0),) * 3
    walk = lambda x: mm.movers([(x * ONE, 14 * ONE, -ONE, 0, 0, 0, 0)], 777)   # noqa: E731
    start = (16 * ONE, 14 * ONE, 0)
    path = ([30 * ONE], [14 * ONE])
    free = case(*small, 1, 3, 1, mm.NONE, pose=start, U=list(U), path=path)
    _, rec, S = case(*small, 1, 3, 1, walk(22), pose=start, U=list(U), path=path)
    assert rec.n_hit_moving == 1                                           # two steps' terms and pen_hit_mv (3 - 2)
    first_two = mm.step(small[1], 1, 9, MODEL, COSTS, *path, *start, list(U[:2]), 5)[2][0]
    assert int(S[0]) == int(first_two) + 777
    _, rec, S = case(*small, 1, 3, 1, walk(24), pose=start, U=list(U), path=path)
    assert rec.n_hit == 0 and int(S[0]) == int(free[2][0])


def test_extremes(small):
    cls, plane = small
    big, v = 1 << 36, 1 << 22
    corners = [(sx * big, sy * big, -sx * v, sy * v, 0, 1 << 40, 1 << 12) for sx in (-1, 1) for sy in (-1, 1)]
    near = list(zip(*movers_around(5, seed=3)[:7]))
    # 64 cells a step: one passes 2 cells ahead of the robot after its third step, one lands there from 192 cells up
    fast = [(POSE[0] + 2 * ONE - 3 * v, POSE[1], v, 0, ONE, 30 << 16, 5 * ONE),
            (POSE[0] + 2 * ONE, POSE[1] + ONE // 2 + 3 * v, 0, -v, 4 << 16, 30 << 16, 5 * ONE)]
    want = case(cls, plane, 65, 64, 9, mm.movers(corners + near + fast, PEN_MV))
    assert want[1].n_hit_moving > 0
    off = (-3 * ONE, 40 * ONE, 100)                                        # a robot standing off the map
    case(cls, plane, 65, 4, 3, movers_around(9, off, spread=4), pose=off)


def test_sixty_four_full_ramps_saturate(small):
    """64 movers on a ring 50 cells from the robot, sq = 2^40, g = 2^12: each adds just under 2^20 a step, the 64 just
    under 2^26, and after 17 steps every total is cut at 2^30; none can hit."""
    ring = [(POSE[0] + round(50 * ONE * math.cos(i / 64 * 2 * math.pi)), POSE[1] + round(50 * ONE * math.sin(i / 64 * 2 * math.pi)),
             (i % 3 - 1) * 1000, (i % 5 - 2) * 1000, 0, 1 << 40, 1 << 12) for i in range(64)]
    model = MODEL._replace(f_hi=2000)                                      # stays in its room
    _, rec, S = case(*small, 65, 33, 9, mm.movers(ring, 1 << 20), model=model, U=[(1000, 0, 10)] * 33)
    assert rec.n_hit == 0 and rec.s_min == rec.s_0 == 1 << 30 and rec.k_best == 0
    assert int(S.min()) == int(S.max()) == 1 << 30


def test_clearing_the_list(small):
    cls, plane = small
    K, T, M = 65, 8, 17
    px, py = straight_path(M)
    U = nominal(T)
    free = mp.step(plane, K, 4, MODEL, COSTS, px, py, *POSE, U, 1)
    free = (free[0], tuple(free[1]) + (0,), free[2])
    mv = movers_around(9)
    with open_map(cls) as m, kh.MppiContext(m, K, T, 4) as dev, kh.MppiContext(m, K, T, 4) as never:
        configure(dev, MODEL, COSTS, px, py, mv)
        configure(never, MODEL, COSTS, px, py)
        same(dev, mm.step(plane, K, 4, MODEL, COSTS, px, py, *POSE, U, 0, mv), *POSE, U, 0, "with the list")
        dev.set_movers()
        same(dev, free, *POSE, U, 1, "cleared")
        same(never, free, *POSE, U, 1, "never set")
        with pytest.raises(IndexError):                                    # a refused list leaves the old one (none) in place
            dev.set_movers([1 << 37], [0], [0], [0], [0], [1], [0], 5)
        same(dev, free, *POSE, U, 1, "after a refusal")
        dev.set_movers(*mv[:7], mv.pen_hit)                                # and a list can come back
        same(dev, mm.step(plane, K, 4, MODEL, COSTS, px, py, *POSE, U, 2, mv), *POSE, U, 2, "set again")


# ---- through the front end ----
def front_end(cfg, dt):
    from kompass_core.control import MPPI
    from kompass_core.models import AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry, RobotType
    robot = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER, geometry_params=np.array([0.1, 0.4]))
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=1000.0, max_decel=1000.0),
                          omega_limits=AngularCtrlLimits(max_vel=1.5, max_steer=0.7, max_acc=1000.0, max_decel=1000.0))
    return MPPI(robot, lim, cfg, control_time_step=dt), robot, lim


def test_a_window_shift_between_two_steps():
    """Two front ends over two maps of the same world, one of which moves its window by (3, -2) cells after the third step.
    Resolution and origin are powers of two, so every quantisation is exact and the two see the same integers but for the
    offset.  The robot and the mover stay more than the plane's reach from what the shift drops or brings in."""
    from kompass_core.control import MPPIConfig
    from kompass_core.mapping import WorldMap
    from kompass_core.models import RobotState
    res, dt, origin = 0.0625, 0.125, (-2.0, 1.0)
    cls = mp.scene_cls()
    at = lambda x, y: (origin[0] + x * res, origin[1] + y * res)           # noqa: E731
    path = np.array([at(30.0, 30.0), at(55.0, 30.0)])
    runs = []
    for shifting in (False, True):
        wm = WorldMap(mp.SCENE_W, mp.SCENE_H, res, origin=origin)
        wm.set_prior(cls)
        fe, _, _ = front_end(MPPIConfig(seed=5, samples=257, horizon=16), dt)
        fe.set_path(path)
        x, y = at(30.0, 30.0)
        state, out = RobotState(x=x, y=y, yaw=0.0, speed=0.0), []
        for n in range(6):
            if shifting and n == 3:
                wm.shift(3, -2)
            mx, my = at(40.0, 34.0 - 0.5 * n)                              # walks -y half a cell a step across the path
            assert fe.loop_step(current_state=state, local_map=wm, moving_obstacles=[(mx, my, 0.0, -0.5 * res / dt, 0.125)])
            i = fe.planner.last_inputs
            off = (3 * ONE, -2 * ONE) if shifting and n >= 3 else (0, 0)
            out.append((fe.linear_x_control, fe.angular_control, fe.record, fe.n_hit_moving, list(fe.planner.last_sequence),
                        i["tx"] + off[0], i["ty"] + off[1], i["movers"][0][0] + off[0], i["movers"][1][0] + off[1], i["movers"][2:]))
            vx, om = fe.linear_x_control[0], fe.angular_control[0]
            state = RobotState(x=state.x + vx * math.cos(state.yaw) * dt, y=state.y + vx * math.sin(state.yaw) * dt,
                               yaw=state.yaw + om * dt, speed=vx)
        runs.append(out)
    for n, (a, b) in enumerate(zip(*runs)):
        assert a == b, n
    assert sum(a[3] for a in runs[0]) > 0                                  # the mover does end samples on the way


def test_forty_steps_of_the_crossing_scene_through_the_front_end():
    """kompass_core.control.MPPI(..., moving_obstacles=...) over the scene against the statement driven with the inputs the
    front end quantised, the list included.  The mover is the crossing scene's: 0.1 m of radius at 0.05 m a cell makes
    hq = 25 << 16 and sq = 81 << 16 with the default margin of 4 cells and g = (200 * 65536) // 57 with the default
    weight.  The robot does not reach it in forty steps; the far end of its roll-outs does, which the test asserts."""
    import kompass_cpp
    from kompass_core.control import MPPIConfig
    from kompass_core.mapping import WorldMap
    from kompass_core.models import RobotState, RobotType
    cls = mp.scene_cls()
    plane = dref.dist2_plane(cls, mp.SCENE_REACH)
    res, dt = 0.05, 0.1
    wm = WorldMap(mp.SCENE_W, mp.SCENE_H, res, origin=ORIGIN)
    wm.set_prior(cls)
    cfg = MPPIConfig(seed=3)
    fe, robot, lim = front_end(cfg, dt)
    r32 = float(np.float32(res))
    pts = [(ORIGIN[0] + x * r32, ORIGIN[1] + y * r32) for x, y in mp.SCENE_VERTICES]
    fe.set_path(np.array(pts))
    q = kompass_cpp.control.MPPI.quantise(RobotType.to_kompass_cpp_lib(robot.robot_type), lim.to_kompass_cpp_lib(), dt, res,
                                          cfg.to_kompass_cpp())
    model = mp.Model(*q[:5], tuple(q[5]))
    costs = mp.scene_costs()
    v = -0.45 * r32 / dt                                                   # 0.45 cells a step towards -y
    state = RobotState(x=pts[0][0], y=pts[0][1], yaw=0.0, speed=0.0)
    prev, felt = None, 0
    for n in range(40):
        mover = (ORIGIN[0] + 85 * r32, ORIGIN[1] + 80 * r32 + n * v * dt, 0.0, v, 0.1)
        assert fe.loop_step(current_state=state, local_map=wm, moving_obstacles=np.array([mover]))
        i = fe.planner.last_inputs
        mv = mm.Movers(*[tuple(int(a) for a in col) for col in i["movers"][:7]], int(i["movers"][7]))
        assert (mv.vx, mv.hq, mv.sq, mv.g, mv.pen_hit) == ((0,), (mm.CROSS_HQ,), (mm.CROSS_SQ,), (mm.CROSS_G,), mm.CROSS_PEN)
        assert abs(mv.vy[0] - mm.CROSS_V[1]) <= 1 and abs(mv.oy[0] - (80 * ONE + n * mm.CROSS_V[1])) <= 64
        U = [tuple(i["u"][3 * k:3 * k + 3]) for k in range(cfg.horizon)]
        assert U == ([(0, 0, 0)] * cfg.horizon if prev is None else mp.shift(prev))
        wU, wrec, wS = mm.step(plane, cfg.samples, cfg.seed, model, costs, i["px"], i["py"], i["tx"], i["ty"], i["h"], U, n, mv)
        got = list(fe.planner.last_sequence)
        prev = [tuple(got[3 * k:3 * k + 3]) for k in range(cfg.horizon)]
        assert prev == wU, n
        assert fe.record + (fe.n_hit_moving,) == tuple(wrec), (n, fe.record, fe.n_hit_moving, tuple(wrec))
        assert np.array_equal(np.array(fe.planner.sample_costs(), np.int64), np.asarray(wS, np.int64)), n
        blind = mp.step(plane, cfg.samples, cfg.seed, model, costs, i["px"], i["py"], i["tx"], i["ty"], i["h"], U, n)[2]
        felt += int((np.asarray(blind) != np.asarray(wS)).any())
        vx, om = fe.linear_x_control[0], fe.angular_control[0]
        state = RobotState(x=state.x + vx * math.cos(state.yaw) * dt, y=state.y + vx * math.sin(state.yaw) * dt,
                           yaw=state.yaw + om * dt, speed=vx)
    assert felt > 0
    assert fe.loop_step(current_state=state, local_map=wm)                 # no list: the step of a controller without one
    i = fe.planner.last_inputs
    assert i["movers"][0] == [] and fe.n_hit_moving == 0
    U = [tuple(i["u"][3 * k:3 * k + 3]) for k in range(cfg.horizon)]
    want = mp.step(plane, cfg.samples, cfg.seed, model, costs, i["px"], i["py"], i["tx"], i["ty"], i["h"], U, 40)
    assert fe.record == tuple(want[1])
