"""Acceleration limits inside the MPPI roll-out on the device (kc_mppi_set_rates, kc_mppi_set_velocity; DESIGN.md 4.12
rules 25 to 29) against the statement tests/mppi_rates_ref.py: every S_k, the record, U' and, with a field, f0 and f_nom
bit for bit, with 1, 4 and 8 lanes a sample.  The statement's vectorised form is the reference;
tests/test_mppi_rates_cpu.py shows it equal to the loop form.  One reference a case, shared by the three roll-out variants.

Every test uses the 120 x 90 scene map of tests/mppi_ref.py at reach 8; the field's goal lies off the centre, at cell (97,
23)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import mppi_field_ref as mf  # noqa: E402
import mppi_movers_ref as mm  # noqa: E402
import mppi_rates_ref as mr  # noqa: E402
import mppi_ref as mp  # noqa: E402
import planner_clearance_ref as cref  # noqa: E402
import planner_ref as pref  # noqa: E402
import worldmap_dist_ref as dref  # noqa: E402
import worldmap_mcl_ref as mref  # noqa: E402
import worldmap_ref as ref  # noqa: E402

RES, ORIGIN = 0.05, (-0.33, 1.7)
W, H, REACH = mp.SCENE_W, mp.SCENE_H, mp.SCENE_REACH
OCC = ref.OCCUPIED
ONE = 1 << 16
GOAL, START, R2 = (97, 23), (10, 45), 9
PEN_D2 = [min(65535, 7 * (25 - d) + (d % 3)) for d in range(26)]
WTAB = [round(65536 * math.exp(-i / 8.0)) for i in range(128)]
MODEL = mp.Model(0, 2 * ONE, 0, 1500, 0, (mref.noise_scale(0.4 * ONE), 0, mref.noise_scale(400.0)))
OMNI = MODEL._replace(f_lo=-ONE, l_hi=ONE // 2, s=(MODEL.s[0], mref.noise_scale(0.2 * ONE), MODEL.s[2]))
CAR = OMNI._replace(l_hi=0, kq=3000, s=MODEL.s)                            # |H| <= (|F| 3000) >> 16: 1500 from F = 32768
COSTS = mp.Costs(2, PEN_D2, 11, 3000, 8, 300 << 16, 20, WTAB, 3)
POSE = (40 * ONE + 700, 50 * ONE - 300, 3000)                              # in the first room, the door ahead to the left
M = 17
PX = [round((40.0 + 0.9 * j) * ONE) for j in range(M)]
PY = [round((50.0 + 0.35 * j) * ONE) for j in range(M)]
WEIGHTS = (1 << 20, 32, 2)
RATES = mr.Rates(3000, 5000, 700, 300, 40, 25)                             # up != dn on every channel
V0 = (30000, -2000, -50)
STATE = r"\[kc -5\]"                                                        # KC_ERR_STATE


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


class Scene:
    """A class plane with its distance plane from the statement and the map that holds it; with `field`, the planner
    that solved on it and its field from the statement."""

    def __init__(self, cls, field=False, clearance=None):
        self.cls = cls
        self.plane = dref.dist2_plane(cls, REACH)
        self.map = kh.WorldMapContext(cls.shape[0], cls.shape[1], RES, ORIGIN)
        self.map.set_prior(cls)
        self.map.set_distance(REACH)
        self.planner = self.field = None
        if field:
            self.planner = kh.PlannerContext()
            self.planner.set_grid(cls)
            if clearance is None:
                self.field = pref.cost_field(pref.validity(cls, R2), GOAL)
            else:
                c2, weight10 = clearance
                table = cref.clearance_table(weight10, R2, c2)
                self.planner.set_clearance_cost(c2, table)
                self.field = cref.cost_field(pref.validity(cls, R2), cref.penalty(cref.clearance2(cls, c2), table), GOAL)
            self.planner.solve(START, GOAL, R2)
            assert np.array_equal(self.planner.field()[0], self.field)     # the statement's input is the device's own field

    def close(self):
        if self.planner is not None:
            self.planner.close()
        self.map.close()


def scene_fixture(make):
    @pytest.fixture(scope="module")
    def fx():
        s = make()
        yield s
        s.close()
    return fx


def boxed_cls():
    """The scene with a ring of occupied cells two cells around the cell (40, 50) of POSE."""
    c = mp.scene_cls()
    c[38, 48:53] = c[42, 48:53] = OCC
    c[38:43, 48] = c[38:43, 52] = OCC
    return c


scene = scene_fixture(lambda: Scene(mp.scene_cls(), field=True))
boxed = scene_fixture(lambda: Scene(boxed_cls()))
cleared = scene_fixture(lambda: Scene(mp.scene_cls(), field=True, clearance=(36, 50)))


def nominal(T, F=40000, L=0, Hh=120):
    return [(F + 500 * (t % 3), L, Hh - 40 * (t % 5)) for t in range(T)]


def movers_around(n, around=POSE, seed=0, spread=9):
    rng = np.random.default_rng(100 + seed + n)
    rows = [(around[0] + 2 * ONE, around[1] - 5 * ONE, 1000, -2000, ONE, 40 << 16, 7 * ONE)]
    for _ in range(n - 1):
        hq = (int(rng.integers(0, 4)) ** 2 << 16) + int(rng.integers(0, ONE))
        sq = hq + int(rng.integers(1, 40 * ONE))
        rows.append((around[0] + int(rng.integers(-spread * ONE, spread * ONE)), around[1] + int(rng.integers(-spread * ONE, spread * ONE)),
                     int(rng.integers(-ONE // 2, ONE // 2)), int(rng.integers(-ONE // 2, ONE // 2)), hq, sq, int(rng.integers(0, 30 * ONE))))
    return mm.movers(rows, 2500)


def configure(dev, model, costs, mv=None, path=(PX, PY)):
    dev.set_model(model.f_lo, model.f_hi, model.l_hi, model.h_hi, model.kq, model.s)
    dev.set_costs(costs.r2, costs.pen_d2, costs.pen_far, costs.pen_hit, costs.w_path, costs.qcap, costs.w_goal, costs.wtab,
                  costs.w_shift)
    if path[0] is not None:
        dev.set_path(*path)
    if mv is not None and len(mv.ox):
        dev.set_movers(*mv[:7], mv.pen_hit)


def same(dev, want, tx, ty, h, U, step, what="", field=False):
    """One device step with each roll-out variant against the statement's (U', Record, S, (f0, f_nom))."""
    wU, wrec, wS, wf = want
    for team in (1, 4, 8):
        dev.set_team(team)
        gU, grec = dev.step(tx, ty, h, U, step)
        gS = dev.costs()
        bad = np.flatnonzero(gS.astype(np.int64) != np.asarray(wS, np.int64))
        assert bad.size == 0, (what, team, bad[:5].tolist(), gS[bad[:5]].tolist(), [int(wS[i]) for i in bad[:5]])
        assert grec.as_tuple() + (int(grec.n_hit_moving),) == tuple(wrec), (what, team, grec.as_tuple(), grec.n_hit_moving, tuple(wrec))
        assert [tuple(int(v) for v in r) for r in gU] == list(wU), (what, team)
        if field:
            assert dev.last_field() == tuple(wf), (what, team, dev.last_field(), wf)


def statement(s, K, T, rates, v0, weights=None, mv=mm.NONE, model=MODEL, costs=COSTS, pose=POSE, U=None, step=5, seed=9, path=(PX, PY)):
    fld = None if weights is None else mf.Field(s.field, *weights)
    return mr.step(s.plane, K, seed, model, costs, *pose, nominal(T) if U is None else U, step, rates, v0, fld, mv, *path)


def case(s, K, T, rates=RATES, v0=V0, weights=None, mv=mm.NONE, model=MODEL, costs=COSTS, pose=POSE, U=None, step=5, seed=9, path=(PX, PY)):
    U = nominal(T) if U is None else U
    want = statement(s, K, T, rates, v0, weights, mv, model, costs, pose, U, step, seed, path)
    with kh.MppiContext(s.map, K, T, seed) as dev:
        configure(dev, model, costs, mv, path)
        if weights is not None:
            dev.set_field(s.planner, *weights)
        dev.set_rates(rates)
        dev.set_velocity(v0)
        same(dev, want, *pose, U, step, (K, T, tuple(rates), v0), field=weights is not None)
    return want


def differs(a, b):
    return [int(v) for v in a[2]] != [int(v) for v in b[2]]


# ---- shapes ----
@pytest.mark.parametrize("T", [1, 2, 64])
@pytest.mark.parametrize("K", [1, 3, 65, 1024])
def test_shapes(scene, K, T):
    got = case(scene, K, T)
    free = statement(scene, K, T, None, V0)
    if K >= 65 or T == 64:
        assert differs(got, free)                                          # the limits are felt
    if K >= 65 and T == 64:
        assert 0 < got[1].n_hit < K


# ---- the rates ----
def test_rate_1_on_every_channel(scene):
    """The limiter binds at every step of every sample: each moves as V0 says, to within T units a step."""
    got = case(scene, 257, 33, rates=mr.Rates(1, 1, 1, 1, 1, 1), v0=(50000, 3000, 90), model=OMNI)
    assert differs(got, statement(scene, 257, 33, None, (0, 0, 0), model=OMNI))


def test_rates_at_the_box_s_width_are_the_mode_off(scene):
    K, T = 257, 16
    U = nominal(T)
    wide = mr.box_rates(OMNI)
    off = mf.step(scene.plane, K, 9, OMNI, COSTS, *POSE, U, 5, None, mm.NONE, PX, PY)
    with kh.MppiContext(scene.map, K, T, 9) as dev, kh.MppiContext(scene.map, K, T, 9) as never:
        configure(dev, OMNI, COSTS)
        configure(never, OMNI, COSTS)
        same(never, off, *POSE, U, 5, "never had rates")
        dev.set_rates(wide)
        for v0 in ((0, 0, 0), (OMNI.f_lo, OMNI.l_hi, -OMNI.h_hi), (OMNI.f_hi, -OMNI.l_hi, OMNI.h_hi)):
            dev.set_velocity(v0)
            assert not differs(statement(scene, K, T, wide, v0, model=OMNI), off)
            same(dev, off, *POSE, U, 5, ("the box's width", v0))
        tight = wide._replace(h_dn=wide.h_dn // 8)                          # one channel below the width, from the box's corner
        dev.set_rates(tight)
        want = statement(scene, K, T, tight, (OMNI.f_hi, -OMNI.l_hi, OMNI.h_hi), model=OMNI)
        assert differs(want, off)
        same(dev, want, *POSE, U, 5, "H_dn below the width")


def test_up_and_dn_differ(scene):
    """The same two numbers the other way round give other costs: neither rate serves for both directions."""
    a = case(scene, 257, 32, rates=mr.Rates(6000, 500, 900, 100, 60, 5), model=OMNI)
    b = case(scene, 257, 32, rates=mr.Rates(500, 6000, 100, 900, 5, 60), model=OMNI)
    assert differs(a, b)


@pytest.mark.parametrize("v0", [(1 << 22, 1 << 22, 32767), (-(1 << 22), -(1 << 22), -32767), (3 * ONE, -ONE, 2000), (-2 * ONE, ONE, -1501)])
def test_v0_at_its_bounds_and_outside_the_box(scene, v0):
    """64 cells a step carries every sample off the map at once; three cells a step is outside OMNI's box (two forward,
    one back, half a cell sideways, 1500 of turn) and comes in at the rates."""
    got = case(scene, 65, 9, v0=v0, model=OMNI, rates=mr.Rates(9000, 7000, 5000, 4000, 300, 200))
    assert differs(got, statement(scene, 65, 9, mr.Rates(9000, 7000, 5000, 4000, 300, 200), (0, 0, 0), model=OMNI))


def test_a_car_whose_cone_binds_on_the_applied_f_while_f_falls(scene):
    """The car turns as hard as its cone allows at 40000 a step and is asked to slow to 2000 and go straight.  H_dn = 10
    would take 150 steps over that; the applied F falls by 6000 a step and its shrinking cone takes A_H down with it."""
    rates = mr.Rates(2000, 6000, 1, 1, 400, 10)
    U = [(2000, 0, 0)] * 16
    v0 = (40000, 0, 1500)
    A = mr.apply_rates(CAR, rates, v0, U)
    assert [a[0] for a in A[:7]] == [34000, 28000, 22000, 16000, 10000, 4000, 2000]
    assert A[0][2] == 1490 and [a[2] for a in A[1:7]] == [(a[0] * CAR.kq) >> 16 for a in A[1:7]] == [1281, 1007, 732, 457, 183, 91]
    assert A[7] == (2000, 0, 81)                                           # F has arrived: H_dn again
    got = case(scene, 257, 16, rates=rates, v0=v0, model=CAR, U=U)
    assert differs(got, statement(scene, 257, 16, None, v0, model=CAR, U=U))
    assert differs(got, statement(scene, 257, 16, rates, v0, model=CAR._replace(kq=0), U=U))   # the cone is felt


# ---- edges of the roll-out ----
def test_a_velocity_that_carries_every_sample_into_the_wall_at_step_0(scene):
    """Three cells from the wall of column 60, heading +x, asked to stand still: V0 is two cells a step and the robot
    sheds 1/16 cell a step, so the first state is a hit for every sample.  Without the mode nothing hits."""
    pose = (57 * ONE, 30 * ONE + 77, 0)
    U = [(0, 0, 0)] * 5
    quiet = MODEL._replace(s=(mref.noise_scale(0.01 * ONE), 0, 0))
    got = case(scene, 65, 5, rates=mr.Rates(4096, 4096, 1, 1, 50, 50), v0=(2 * ONE, 0, 0), model=quiet, pose=pose, U=U)
    assert got[1].n_hit == 65 and set(int(s) for s in got[2]) == {COSTS.pen_hit * 5 + COSTS.w_goal * (M - 1)}   # rule 7: jm = 0
    assert statement(scene, 65, 5, None, (0, 0, 0), model=quiet, pose=pose, U=U)[1].n_hit == 0


def test_a_boxed_in_pose_where_every_sample_hits_at_step_0(boxed):
    K, T = 257, 5
    costs = COSTS._replace(r2=25)
    got = case(boxed, K, T, costs=costs)
    assert got[1].n_hit == K and got[1].k_best == 0 and got[1].den == K * WTAB[0]


def test_a_robot_off_the_map(scene):
    got = case(scene, 65, 4, pose=(-3 * ONE, 40 * ONE, 100))
    assert got[1].n_hit == 0 and int(got[2][0]) > 0                        # FAR everywhere: pen_far and the path term alone


def test_the_total_is_cut_at_2_to_the_30(scene):
    """A robot that stands still far from a short path: 64 states of (qcap w_path) >> 16 = 2^24 each."""
    costs = COSTS._replace(w_path=1 << 16, qcap=1 << 24)
    still = MODEL._replace(f_hi=3000)
    got = case(scene, 65, 64, costs=costs, model=still, rates=mr.Rates(1, 1, 1, 1, 1, 1), v0=(0, 0, 0), U=[(1000, 0, 10)] * 64,
               pose=(20 * ONE, 20 * ONE, 0))
    assert got[1].n_hit == 0 and got[1].s_min == got[1].s_0 == 1 << 30 and int(got[2].max()) == 1 << 30


# ---- with the other terms ----
@pytest.mark.parametrize("N", [1, 64])
def test_with_movers(scene, N):
    U = nominal(33, 9000)
    mv = movers_around(N)
    got = case(scene, 65, 33, mv=mv, U=U)
    assert differs(got, statement(scene, 65, 33, RATES, V0, U=U))          # the list is felt
    if N == 1:
        assert differs(got, statement(scene, 65, 33, None, V0, mv=mv, U=U))   # and so are the limits
    assert got[1].n_hit_moving <= got[1].n_hit
    if N == 64:
        assert got[1].n_hit_moving > 0


@pytest.mark.parametrize("N", [0, 64])
def test_with_a_cost_field_attached(scene, N):
    mv = movers_around(N) if N else mm.NONE
    got = case(scene, 257, 32, weights=WEIGHTS, mv=mv, path=(None, None))
    free = statement(scene, 257, 32, None, V0, WEIGHTS, mv, path=(None, None))
    assert got[3][0] == free[3][0] == int(scene.field[40, 50])
    if N == 0:
        assert differs(got, free) and got[3][1] != free[3][1]              # f_nom: where the nominal sequence ends under the limits


def test_with_a_field_solved_with_the_clearance_cost(scene, cleared):
    assert not np.array_equal(cleared.field, scene.field)
    case(cleared, 257, 32, weights=WEIGHTS, path=(None, None))


# ---- the state a context keeps ----
def test_rates_set_cleared_and_set_again_and_the_velocity_between_steps(scene):
    K, T = 257, 16
    U = nominal(T)
    on = lambda rates, v0, step: statement(scene, K, T, rates, v0, U=U, step=step, seed=4)   # noqa: E731
    other = mr.Rates(500, 9000, 1, 1, 7, 300)
    with kh.MppiContext(scene.map, K, T, 4) as dev:
        configure(dev, MODEL, COSTS)
        dev.set_velocity(V0)                                               # no rates yet: it plays no part
        same(dev, on(None, V0, 0), *POSE, U, 0, "before any rates")
        dev.set_rates(RATES)
        same(dev, on(RATES, V0, 1), *POSE, U, 1, "set, with the velocity given before")
        dev.set_velocity((90000, 0, 700))
        same(dev, on(RATES, (90000, 0, 700), 2), *POSE, U, 2, "another velocity")
        same(dev, on(RATES, (90000, 0, 700), 3), *POSE, U, 3, "kept for the next step")
        with pytest.raises(ValueError):                                    # a refused call leaves both as they were
            dev.set_rates((1, 1, 1, 1, 0, 1))
        with pytest.raises(IndexError):
            dev.set_velocity((0, 0, 32768))
        same(dev, on(RATES, (90000, 0, 700), 4), *POSE, U, 4, "after two refusals")
        dev.set_rates(None)
        same(dev, on(None, V0, 5), *POSE, U, 5, "cleared")
        dev.set_rates(other)
        same(dev, on(other, (90000, 0, 700), 6), *POSE, U, 6, "set again: the velocity is still there")
        dev.set_velocity((0, 0, 0))
        same(dev, on(other, (0, 0, 0), 7), *POSE, U, 7, "at rest")


# ---- through the front end ----
def test_forty_closed_loop_steps_through_the_front_end(scene):
    """kompass_core.control.MPPI(acceleration_limits=True) over the scene against the statement driven with the inputs
    the front end quantised; the command is out[0] of kc_mppi_apply_rates over U', converted as controls() converts, and
    that integer triple is the next step's V0."""
    import kompass_cpp
    from kompass_core.control import MPPI, MPPIConfig
    from kompass_core.mapping import WorldMap
    from kompass_core.models import (AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry, RobotState,
                                     RobotType)
    res, dt = 0.05, 0.1
    wm = WorldMap(W, H, res, origin=ORIGIN)
    wm.set_prior(scene.cls)
    robot = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER, geometry_params=np.array([0.1, 0.4]))
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=0.3125, max_decel=0.5),
                          omega_limits=AngularCtrlLimits(max_vel=1.5, max_steer=0.7, max_acc=0.5, max_decel=0.7))
    cfg = MPPIConfig(seed=3, control_horizon=4, acceleration_limits=True)
    fe = MPPI(robot, lim, cfg, control_time_step=dt)
    r32 = float(np.float32(res))
    pts = [(ORIGIN[0] + x * r32, ORIGIN[1] + y * r32) for x, y in mp.SCENE_VERTICES]
    fe.set_path(np.array(pts))
    q = kompass_cpp.control.MPPI.quantise(RobotType.to_kompass_cpp_lib(robot.robot_type), lim.to_kompass_cpp_lib(), dt, res,
                                          cfg.to_kompass_cpp())
    model, rates = mp.Model(*q[:5], tuple(q[5])), mr.Rates(*q[6])
    lin, ang = dt * dt / r32 * 65536.0, dt * dt / (2 * math.pi) * 65536.0
    assert rates[:2] == (round(0.3125 * lin), round(0.5 * lin)) == (4096, 6554) and rates[4:] == (round(0.5 * ang), round(0.7 * ang))
    costs = mp.scene_costs()
    assert fe.last_velocity == (0, 0, 0)
    state = RobotState(x=pts[0][0], y=pts[0][1], yaw=0.0, speed=0.0)
    prev, v, x0, bound = None, (0, 0, 0), state.x, 0
    for n in range(40):
        assert fe.loop_step(current_state=state, local_map=wm)
        i = fe.planner.last_inputs
        U = [tuple(i["u"][3 * k:3 * k + 3]) for k in range(cfg.horizon)]
        assert i["step"] == n and i["limited"] and tuple(i["rates"]) == tuple(rates) and tuple(i["v0"]) == v
        assert U == ([(0, 0, 0)] * cfg.horizon if prev is None else mp.shift(prev))
        wU, wrec, wS, _ = mr.step(scene.plane, cfg.samples, cfg.seed, model, costs, i["tx"], i["ty"], i["h"], U, n, rates, v,
                                  px=i["px"], py=i["py"])
        got = list(fe.planner.last_sequence)
        prev = [tuple(got[3 * k:3 * k + 3]) for k in range(cfg.horizon)]
        assert prev == wU, n
        assert fe.record + (fe.n_hit_moving,) == tuple(wrec), (n, fe.record, tuple(wrec))
        assert np.array_equal(np.array(fe.planner.sample_costs(), np.int64), np.asarray(wS, np.int64)), n
        A = mr.apply_rates(model, rates, v, prev)                          # rule 28
        applied = list(fe.planner.last_applied)
        assert [tuple(applied[3 * k:3 * k + 3]) for k in range(cfg.horizon)] == A, n
        bound += A[0] != prev[0]
        v = A[0]
        assert fe.last_velocity == v
        vx, om = fe.linear_x_control, fe.angular_control
        cmd = fe.planner.controls(1)[0]
        assert len(vx) == len(om) == 4 and fe.linear_y_control == [0.0] * 4
        assert vx[0] == cmd[0] == v[0] / 65536.0 * r32 / dt and om[0] == cmd[2] == v[2] / 65536.0 * 2 * math.pi / dt
        assert vx[1] == A[1][0] / 65536.0 * r32 / dt                       # controls() shows the applied sequence
        path = fe.predicted_path()
        want = mp.rollout(A, i["tx"], i["ty"], i["h"])
        assert len(path) == cfg.horizon
        assert path[-1][0] == pytest.approx(ORIGIN[0] + want[-1][0] / 65536.0 * r32) and path[-1][1] == pytest.approx(
            ORIGIN[1] + want[-1][1] / 65536.0 * r32)
        state = RobotState(x=state.x + vx[0] * math.cos(state.yaw) * dt, y=state.y + vx[0] * math.sin(state.yaw) * dt,
                           yaw=state.yaw + om[0] * dt, speed=vx[0])
    assert state.x > x0 + 10 * r32                                         # it has driven
    assert bound >= 10                                                     # and the limits held it back on the way
    fe.planner.reset_sequence()
    assert fe.last_velocity == (0, 0, 0)
