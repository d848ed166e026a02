"""The grid planner's cost field in the MPPI controller on the device (kc_mppi_set_field; DESIGN.md 4.12 rules 19 to 24)
against the statement tests/mppi_field_ref.py: every S_k, the record, U', f0 and f_nom bit for bit, with 1, 4 and 8 lanes
a sample.  The statement's vectorised form is the reference; tests/test_mppi_field_cpu.py shows it equal to the loop
form.  One reference a case, shared by the three roll-out variants.

Every test uses the 120 x 90 scene map of tests/mppi_ref.py at reach 8 with the goal off the centre, at cell (97, 23):
a transposed index or a wrong row stride shows.  The planner's field is its own on the device (kc_planner_solve /
kc_planner_replan) and is shown equal to tests/planner_ref.py's before it serves as the statement's input."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import mppi_field_ref as mf  # noqa: E402
import mppi_movers_ref as mm  # noqa: E402
import mppi_ref as mp  # noqa: E402
import planner_clearance_ref as cref  # noqa: E402
import planner_ref as pref  # noqa: E402
import worldmap_dist_ref as dref  # noqa: E402
import worldmap_mcl_ref as mref  # noqa: E402
import worldmap_ref as ref  # noqa: E402

RES, ORIGIN = 0.05, (-0.33, 1.7)
W, H, REACH = mp.SCENE_W, mp.SCENE_H, mp.SCENE_REACH
OCC, EMP = ref.OCCUPIED, ref.EMPTY
ONE = 1 << 16
INF = mf.INF
GOAL, START, R2 = (97, 23), (10, 45), 9
PEN_D2 = [min(65535, 7 * (25 - d) + (d % 3)) for d in range(26)]
WTAB = [round(65536 * math.exp(-i / 8.0)) for i in range(128)]
MODEL = mp.Model(0, 2 * ONE, 0, 1500, 0, (mref.noise_scale(0.4 * ONE), 0, mref.noise_scale(400.0)))
COSTS = mp.Costs(2, PEN_D2, 11, 3000, 8, 300 << 16, 20, WTAB, 3)           # w_path, qcap, w_goal: the path mode's alone
POSE = (40 * ONE + 700, 50 * ONE - 300, 3000)                              # in the first room, the door ahead to the left
WEIGHTS = (1 << 20, 32, 2)
STATE = r"\[kc -5\]"                                                        # KC_ERR_STATE


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def field_of(cls, goal=GOAL, r2=R2):
    return pref.cost_field(pref.validity(cls, r2), goal)


def open_map(cls, reach=REACH):
    w, h = cls.shape
    m = kh.WorldMapContext(w, h, RES, ORIGIN)
    m.set_prior(cls)
    m.set_distance(reach)
    return m


class Scene:
    """A class plane with its distance plane and its field from the statements, and the map and planner that hold them."""

    def __init__(self, cls, goal=GOAL, r2=R2, clearance=None):
        self.cls, self.goal, self.r2 = cls, goal, r2
        self.plane = dref.dist2_plane(cls, REACH)
        self.map = open_map(cls)
        self.planner = kh.PlannerContext()
        self.planner.set_grid(cls)
        if clearance is None:
            self.field = field_of(cls, goal, r2)
        else:
            c2, weight10 = clearance
            table = cref.clearance_table(weight10, r2, c2)
            self.planner.set_clearance_cost(c2, table)
            self.field = cref.cost_field(pref.validity(cls, r2), cref.penalty(cref.clearance2(cls, c2), table), goal)
        self.planner.solve(START, goal, r2)
        assert np.array_equal(self.planner.field()[0], self.field)         # the statement's input is the device's own field

    def close(self):
        self.planner.close()
        self.map.close()


def scene_fixture(make):
    @pytest.fixture(scope="module")
    def fx():
        s = make()
        yield s
        s.close()
    return fx


def sealed_cls():
    """The scene with a sealed room I 20 .. 36, J 60 .. 80 in the first room: no walk leaves it."""
    c = mp.scene_cls()
    c[20, 60:81] = c[36, 60:81] = OCC
    c[20:37, 60] = c[20:37, 80] = OCC
    return c


def boxed_cls():
    """The scene with a ring of occupied cells two cells around the cell (40, 50) of POSE."""
    c = mp.scene_cls()
    c[38, 48:53] = c[42, 48:53] = OCC
    c[38:43, 48] = c[38:43, 52] = OCC
    return c


scene = scene_fixture(lambda: Scene(mp.scene_cls()))
sealed = scene_fixture(lambda: Scene(sealed_cls()))
boxed = scene_fixture(lambda: Scene(boxed_cls()))
cleared = scene_fixture(lambda: Scene(mp.scene_cls(), clearance=(36, 50)))


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


def configure(dev, model, costs, mv=None, path=None):
    dev.set_model(model.f_lo, model.f_hi, model.l_hi, model.h_hi, model.kq, model.s)
    dev.set_costs(costs.r2, costs.pen_d2, costs.pen_far, costs.pen_hit, costs.w_path, costs.qcap, costs.w_goal, costs.wtab,
                  costs.w_shift)
    if path is not None:
        dev.set_path(*path)
    if mv is not None:
        dev.set_movers(*mv[:7], mv.pen_hit)


def same(dev, want, tx, ty, h, U, step, what="", field=True):
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
        else:
            with pytest.raises(kh.KompassHipError, match=STATE):
                dev.last_field()


def case(s, K, T, weights=WEIGHTS, mv=mm.NONE, model=MODEL, costs=COSTS, pose=POSE, U=None, step=5, seed=9):
    """No path is ever set: rule 20."""
    U = nominal(T) if U is None else U
    want = mf.step(s.plane, K, seed, model, costs, *pose, U, step, mf.Field(s.field, *weights), mv)
    with kh.MppiContext(s.map, K, T, seed) as dev:
        configure(dev, model, costs, mv if len(mv.ox) else None)
        dev.set_field(s.planner, *weights)
        same(dev, want, *pose, U, step, (K, T, weights, len(mv.ox)))
    return want


# ---- shapes ----
@pytest.mark.parametrize("T", [1, 32, 64])
@pytest.mark.parametrize("K", [1, 7, 8, 9, 64, 1024])
def test_shapes(scene, K, T):
    _, rec, S, (f0, f_nom) = case(scene, K, T)
    assert f0 == int(scene.field[40, 50]) != int(scene.field[50, 40])       # the pose's cell, not its transpose
    if K >= 64 and T >= 32:
        assert 0 < rec.n_hit < K and len(set(int(v) for v in S)) > K // 2  # some hit the wall, the rest spread out


# ---- field edges ----
def test_rollouts_that_leave_the_map(scene):
    """64 cells a step from beside the east border, heading +x: the first state is outside, where d2 is FAR and fv is INF."""
    fast = MODEL._replace(f_hi=1 << 22)
    U = [(30 * ONE, 0, 0)] * 4
    pose = (100 * ONE, 20 * ONE + 9, 0)
    _, rec, S, (f0, f_nom) = case(scene, 65, 4, model=fast, pose=pose, U=U, weights=(5000, 256, 1))
    assert f0 == int(scene.field[100, 20]) and f_nom == 5000 and rec.n_hit < 65
    assert int(S[0]) == 4 * (COSTS.pen_far + 5000) + 5000
    _, _, _, (f0, f_nom) = case(scene, 65, 4, pose=(-3 * ONE, 40 * ONE, 100), weights=(5000, 256, 1))   # a robot off the map
    assert (f0, f_nom) == (INF, 5000)


def test_a_boxed_in_pose_where_every_sample_hits_at_step_0(boxed):
    K, T = 257, 5
    costs = COSTS._replace(r2=25)                                          # within 5 cells of the ring, whatever the step
    _, rec, S, (f0, f_nom) = case(boxed, K, T, costs=costs, weights=(7777, 32, 3))
    assert rec.n_hit == K and rec.k_best == 0 and rec.den == K * WTAB[0]
    assert (f0, f_nom) == (INF, 7777)                                      # rule 21: the pose's own cell, which no walk leaves
    assert set(int(s) for s in S) == {costs.pen_hit * T + 3 * 7777}


def test_a_pose_in_an_invalid_cell(scene):
    """Two cells from the wall of column 60: inside the planner's disc (r2 = 9), outside the controller's (r2 = 2)."""
    pose = (58 * ONE - 100, 30 * ONE + 77, 32768)                          # heading -x, away from the wall
    assert int(scene.plane[58, 30]) == 4 and int(scene.field[58, 30]) == INF
    _, rec, S, (f0, f_nom) = case(scene, 65, 9, pose=pose)
    assert f0 == INF and f_nom < WEIGHTS[0] and rec.n_hit < 65             # the nominal sequence walks out of it


def test_a_sealed_pocket_inside_the_map(sealed):
    pose = (28 * ONE + 5, 70 * ONE, 0)
    assert int(sealed.field[28, 70]) == INF and int(sealed.plane[28, 70]) > 25
    slow = MODEL._replace(f_hi=3000)                                       # stays in the pocket's middle
    _, rec, S, (f0, f_nom) = case(sealed, 65, 8, model=slow, pose=pose, U=[(1000, 0, 10)] * 8, weights=(6000, 256, 2))
    assert (f0, f_nom, rec.n_hit) == (INF, 6000, 0)
    assert set(int(s) for s in S) == {8 * (COSTS.pen_far + 6000) + 2 * 6000}


def test_fv_at_fcap_and_one_above_it(scene):
    """One sample, one step of one cell along +x from the cell (40, 50) to (41, 50)."""
    on_cell = (40 * ONE, 50 * ONE, 0)
    v = int(scene.field[41, 50])
    assert v != INF and v != int(scene.field[40, 50])
    for fcap, fc in ((v, v), (v - 1, v - 1), (v + 1, v)):                  # fv == fcap, fv == fcap + 1, fv == fcap - 1
        _, _, S, (f0, f_nom) = case(scene, 1, 1, pose=on_cell, U=[(ONE, 0, 0)], weights=(fcap, 256, 1))
        assert (f0, f_nom) == (int(scene.field[40, 50]), fc)
        assert int(S[0]) == COSTS.pen_far + fc + fc


def test_weights_that_drive_the_total_to_its_cap(sealed):
    pose = (28 * ONE + 5, 70 * ONE, 0)
    slow = MODEL._replace(f_hi=3000)
    _, rec, S, (f0, f_nom) = case(sealed, 65, 33, model=slow, pose=pose, U=[(1000, 0, 10)] * 33, weights=(1 << 24, 1 << 12, 64))
    assert rec.n_hit == 0 and rec.s_min == rec.s_0 == 1 << 30 and rec.k_best == 0 and f_nom == 1 << 24
    assert int(S.min()) == int(S.max()) == 1 << 30


# ---- movers, clearance ----
@pytest.mark.parametrize("N", [1, 64])
def test_movers_in_field_mode(scene, N):
    U = nominal(33, 9000)
    _, rec, S, _ = case(scene, 65, 33, mv=movers_around(N), U=U)
    free = mf.step(scene.plane, 65, 9, MODEL, COSTS, *POSE, U, 5, mf.Field(scene.field, *WEIGHTS))[2]
    assert (np.asarray(S) != np.asarray(free)).any()                       # the list is felt
    assert rec.n_hit_moving <= rec.n_hit
    if N == 64:
        assert rec.n_hit_moving > 0


def test_a_field_solved_with_the_clearance_cost(scene, cleared):
    assert not np.array_equal(cleared.field, scene.field)
    case(cleared, 257, 32)


# ---- replan: the field pointer follows the planner's buffers ----
def test_solve_replan_after_a_closed_door_and_a_moved_start(scene):
    K, T = 257, 16
    U = nominal(T)
    fld = lambda f: mf.Field(f, *WEIGHTS)                                  # noqa: E731
    closed = mp.scene_cls()
    closed[60, 52:62] = OCC
    shut_plane, shut_field = dref.dist2_plane(closed, REACH), field_of(closed)
    assert int(shut_field[40, 50]) == INF and int(scene.field[40, 50]) != INF
    with open_map(mp.scene_cls()) as m, kh.PlannerContext() as p, kh.MppiContext(m, K, T, 4) as dev:
        configure(dev, MODEL, COSTS)
        dev.set_field(p, *WEIGHTS)
        p.set_grid(mp.scene_cls())
        p.solve(START, GOAL, R2)
        seen = {p.field_device()[0]}
        same(dev, mf.step(scene.plane, K, 4, MODEL, COSTS, *POSE, U, 0, fld(scene.field)), *POSE, U, 0, "solved")
        m.set_prior(closed)                                                # the door shuts: the map and the planner's grid
        p.set_grid(closed)
        p.replan(START, GOAL, R2)
        assert p.replan_info()[0]                                          # a kept field, rolled back and relaxed
        assert np.array_equal(p.field()[0], shut_field)
        seen.add(p.field_device()[0])
        same(dev, mf.step(shut_plane, K, 4, MODEL, COSTS, *POSE, U, 1, fld(shut_field)), *POSE, U, 1, "door shut")
        p.replan((30, 60), GOAL, R2)                                       # the start alone: no pass, the same field
        seen.add(p.field_device()[0])
        same(dev, mf.step(shut_plane, K, 4, MODEL, COSTS, *POSE, U, 2, fld(shut_field)), *POSE, U, 2, "start moved")
        m.set_prior(mp.scene_cls())                                        # and open again
        p.set_grid(mp.scene_cls())
        p.replan(START, GOAL, R2)
        assert np.array_equal(p.field()[0], scene.field)
        seen.add(p.field_device()[0])
        same(dev, mf.step(scene.plane, K, 4, MODEL, COSTS, *POSE, U, 3, fld(scene.field)), *POSE, U, 3, "door open")
        f, w, h, stream = p.field_device()
        assert (w, h) == (W, H) and f != 0 and stream != 0
        print("field buffers seen:", len(seen))


# ---- detach ----
def test_detaching_gives_the_path_mode_of_before(scene):
    K, T, M = 257, 16, 17
    U = nominal(T)
    px = [round((40.0 + 0.9 * j) * ONE) for j in range(M)]
    py = [round((50.0 + 0.35 * j) * ONE) for j in range(M)]
    path = mm.step(scene.plane, K, 4, MODEL, COSTS, px, py, *POSE, U, 1) + ((None, None),)
    with kh.MppiContext(scene.map, K, T, 4) as dev, kh.MppiContext(scene.map, K, T, 4) as never:
        configure(dev, MODEL, COSTS, path=(px, py))
        configure(never, MODEL, COSTS, path=(px, py))
        same(dev, path, *POSE, U, 1, "before the attach", field=False)
        dev.set_field(scene.planner, *WEIGHTS)
        same(dev, mf.step(scene.plane, K, 4, MODEL, COSTS, *POSE, U, 1, mf.Field(scene.field, *WEIGHTS)), *POSE, U, 1, "attached")
        with pytest.raises(IndexError):                                    # a refused attach leaves the old one in place
            dev.set_field(scene.planner, (1 << 24) + 1, 32, 2)
        same(dev, mf.step(scene.plane, K, 4, MODEL, COSTS, *POSE, U, 1, mf.Field(scene.field, *WEIGHTS)), *POSE, U, 1, "after a refusal")
        dev.set_field(None)
        same(dev, path, *POSE, U, 1, "detached", field=False)
        same(never, path, *POSE, U, 1, "never attached", field=False)


# ---- KC_ERR_STATE ----
def test_a_step_without_a_disc_mode_goal_rooted_field_is_refused(scene):
    K, T = 9, 4
    U = nominal(T)
    cls = mp.scene_cls()
    known = cls.copy()
    known[100:, :] = ref.UNEXPLORED                                        # something to explore
    known[-1, :] = OCC
    with kh.PlannerContext() as p, kh.MppiContext(scene.map, K, T, 1) as dev:
        configure(dev, MODEL, COSTS)
        dev.set_field(p, *WEIGHTS)

        def refused(what):
            with pytest.raises(kh.KompassHipError, match=STATE):
                p.field_device()
            with pytest.raises(kh.KompassHipError, match=STATE):
                dev.step(*POSE, U, 0)

        def accepted():
            p.solve(START, GOAL, R2)
            same(dev, mf.step(scene.plane, K, 1, MODEL, COSTS, *POSE, U, 0, mf.Field(scene.field, *WEIGHTS)), *POSE, U, 0)

        refused("no grid")
        p.set_grid(cls)
        refused("before any solve")
        with pytest.raises(kh.KompassHipError, match=STATE):               # no step yet: no words either
            dev.last_field()
        accepted()
        p.set_oriented(16, 4, 10)
        p.solve_oriented(START, 0, GOAL)
        refused("an oriented solve")
        p.set_oriented(0)
        accepted()
        p.set_car(2)
        p.solve_car(START, 0, GOAL, -1, R2)
        refused("a car solve")
        p.set_car(0)
        accepted()
        p.set_grid(known)
        p.explore(START, R2)
        refused("explore")
        p.set_grid(cls)
        accepted()
        p.set_grid(cls[:, :-1].copy())                                     # 120 x 89
        p.solve(START, GOAL, R2)
        assert p.field_device()[1:3] == (W, H - 1)
        with pytest.raises(kh.KompassHipError, match=STATE):               # the shape is not the map's
            dev.step(*POSE, U, 0)
        p.set_grid(cls.T.copy())                                           # 90 x 120: as many cells, another stride
        p.solve((45, 10), (23, 97), R2)
        with pytest.raises(kh.KompassHipError, match=STATE):
            dev.step(*POSE, U, 0)
        p.set_grid(cls)
        accepted()


# ---- through the front end ----
def front_end(cfg, dt):
    from kompass_core.control import MPPI
    from kompass_core.models import AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry, RobotType
    robot = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER, geometry_params=np.array([0.1, 0.4]))
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=1000.0, max_decel=1000.0),
                          omega_limits=AngularCtrlLimits(max_vel=1.5, max_steer=0.7, max_acc=1000.0, max_decel=1000.0))
    return MPPI(robot, lim, cfg, control_time_step=dt), robot, lim


def grid_planner(radius):
    from kompass_core.models import Robot, RobotGeometry, RobotType
    from kompass_core.planning import GridPlanner
    return GridPlanner(Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER,
                             geometry_params=np.array([radius, 0.4])))


class Loop:
    """kompass_core.control.MPPI(..., cost_field=planner) beside the statement driven with the inputs the front end
    quantised: the plant applies the command, the statement is handed the map's own classes."""

    def __init__(self, res, origin, dt, cfg, seed_state):
        import kompass_cpp
        from kompass_core.mapping import WorldMap
        from kompass_core.models import RobotType
        self.res, self.origin, self.dt, self.cfg = res, origin, dt, cfg
        self.wm = WorldMap(W, H, res, origin=origin, hit=127, miss=127, e_min=-126, e_max=127)
        self.wm.set_prior(mp.scene_cls())
        self.fe, robot, lim = front_end(cfg, dt)
        self.gp = grid_planner(3.0 * res)                                  # r2 = 9
        q = kompass_cpp.control.MPPI.quantise(RobotType.to_kompass_cpp_lib(robot.robot_type), lim.to_kompass_cpp_lib(), dt, res,
                                              cfg.to_kompass_cpp())
        self.model = mp.Model(*q[:5], tuple(q[5]))
        self.costs = mp.scene_costs()
        self.state = seed_state
        self.prev, self.n = None, 0

    def at(self, x, y):
        """The world position a quarter cell beyond the centre of cell (x, y): the planner's truncation lands on the cell."""
        r = float(np.float32(self.res))
        o = self.wm.map_meta_data
        return (o["origin_x"] + (x + 0.25) * r, o["origin_y"] + (y + 0.25) * r)

    def step(self, goal_cell):
        from kompass_core.models import RobotState
        cfg = self.cfg
        assert self.fe.loop_step(current_state=self.state, local_map=self.wm, cost_field=self.gp)
        i = self.fe.planner.last_inputs
        assert i["field"] and i["px"] == []
        cls = np.asarray(self.wm.occupancy)
        plane = dref.dist2_plane(cls, mp.SCENE_REACH)
        assert self.gp.footprint_r2 == R2
        fld = mf.Field(field_of(cls, goal_cell), cfg.field_cap, cfg.field_run_weight, cfg.field_goal_weight)
        U = [tuple(i["u"][3 * k:3 * k + 3]) for k in range(cfg.horizon)]
        assert U == ([(0, 0, 0)] * cfg.horizon if self.prev is None else mp.shift(self.prev))
        wU, wrec, wS, (f0, f_nom) = mf.step(plane, cfg.samples, cfg.seed, self.model, self.costs, i["tx"], i["ty"], i["h"], U, self.n, fld)
        got = list(self.fe.planner.last_sequence)
        self.prev = [tuple(got[3 * k:3 * k + 3]) for k in range(cfg.horizon)]
        assert self.prev == wU, self.n
        assert self.fe.record + (self.fe.n_hit_moving,) == tuple(wrec), (self.n, self.fe.record, tuple(wrec))
        assert np.array_equal(np.array(self.fe.planner.sample_costs(), np.int64), np.asarray(wS, np.int64)), self.n
        assert (self.fe.field_at_robot, int(self.fe.planner.field_nominal)) == (f0, f_nom), self.n
        vx, om = self.fe.linear_x_control[0], self.fe.angular_control[0]
        s = self.state
        self.state = RobotState(x=s.x + vx * math.cos(s.yaw) * self.dt, y=s.y + vx * math.sin(s.yaw) * self.dt,
                                yaw=s.yaw + om * self.dt, speed=vx)
        self.n += 1
        return f0


def test_forty_steps_through_the_front_end():
    from kompass_core.control import MPPIConfig
    from kompass_core.models import RobotState
    loop = Loop(0.05, ORIGIN, 0.1, MPPIConfig(seed=3), None)
    sx, sy = loop.at(*START)
    gx, gy = loop.at(*GOAL)
    loop.state = RobotState(x=sx, y=sy, yaw=0.0, speed=0.0)
    loop.gp.setup_problem(None, sx, sy, 0.0, gx, gy, 0.0, grid=loop.wm)
    assert loop.gp.solve() is not None
    f = [loop.step(GOAL) for _ in range(40)]
    assert f[0] != INF and f[-1] < f[0] - 300                              # thirty cells' worth nearer the goal, by the field
    # the path mode comes back with cost_field=None: it asks for a path again
    assert not loop.fe.loop_step(current_state=loop.state, local_map=loop.wm)


def test_replan_and_window_shift_through_the_front_end():
    """Solve and step; shut the door through WorldMap.update and replan(map=world_map), then step; move the start only,
    then step; shift the window: a ValueError until the planner has read the map again."""
    from kompass_core.control import MPPIConfig
    from kompass_core.models import RobotState
    res, origin = 0.0625, (-2.0, 1.0)                                      # powers of two: every quantisation is exact
    loop = Loop(res, origin, 0.125, MPPIConfig(seed=5, samples=257, horizon=16), None)
    sx, sy = loop.at(40, 50)
    gx, gy = loop.at(*GOAL)
    loop.state = RobotState(x=sx, y=sy, yaw=0.0, speed=0.0)
    other = grid_planner(3.0 * res)                                        # a planner that never saw this map
    other.setup_problem(loop.wm.map_meta_data, sx, sy, 0.0, gx, gy, 0.0, grid=np.asarray(loop.wm.occupancy))
    assert other.solve() is not None
    with pytest.raises(ValueError, match="cost_field"):
        loop.fe.loop_step(current_state=loop.state, local_map=loop.wm, cost_field=other)
    loop.gp.setup_problem(None, sx, sy, 0.0, gx, gy, 0.0, grid=loop.wm)
    assert loop.gp.solve() is not None
    assert loop.step(GOAL) != INF
    # an occupied block of 15 x 15 cells over the door, fused into the map
    before = np.asarray(loop.wm.occupancy).copy()
    dx, dy = origin[0] + 60 * res, origin[1] + 56.5 * res
    assert loop.wm.update(RobotState(x=dx, y=dy, yaw=0.0), np.full((15, 15), 100, np.int32)) > 0
    after = np.asarray(loop.wm.occupancy)
    assert (after[60, 52:62] == OCC).all() and (before[60, 52:62] == EMP).all()
    assert loop.gp.replan(map=loop.wm) is None and loop.gp.replanned       # no path any more, from the kept field
    assert loop.step(GOAL) == INF                                          # cut off: the controller does not refuse
    assert loop.gp.replan(start=loop.at(30, 60)) is None and loop.gp.replanned
    assert loop.step(GOAL) == INF
    loop.wm.shift(3, -2)
    with pytest.raises(ValueError, match="cost_field"):
        loop.fe.loop_step(current_state=loop.state, local_map=loop.wm, cost_field=loop.gp)
    loop.gp.replan(map=loop.wm)
    assert not loop.gp.replanned                                           # rule 51: a full solve on the shifted window
    loop.step((GOAL[0] - 3, GOAL[1] + 2))


def test_a_planner_disc_below_the_hit_radius_is_warned_about_once(caplog):
    """The planner's r2 = 4 against the controller's hit r2 = 9: a cell the field holds valid can be a hit."""
    import logging
    from kompass_core.control import MPPIConfig
    from kompass_core.models import RobotState
    loop = Loop(0.0625, (-2.0, 1.0), 0.125, MPPIConfig(seed=1, samples=65, horizon=8), None)
    loop.gp = grid_planner(2.0 * 0.0625)
    sx, sy = loop.at(40, 50)
    gx, gy = loop.at(*GOAL)
    state = RobotState(x=sx, y=sy, yaw=0.0, speed=0.0)
    loop.gp.setup_problem(None, sx, sy, 0.0, gx, gy, 0.0, grid=loop.wm)
    assert loop.gp.solve() is not None and loop.gp.footprint_r2 == 4
    with caplog.at_level(logging.WARNING):
        for _ in range(3):
            assert loop.fe.loop_step(current_state=state, local_map=loop.wm, cost_field=loop.gp)
    assert sum("footprint r2 = 4 is below" in r.getMessage() for r in caplog.records) == 1
    assert loop.fe.field_at_robot == int(field_of(mp.scene_cls(), GOAL, 4)[40, 50])
