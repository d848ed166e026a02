"""A box footprint as a chain of discs inside the MPPI roll-out on the device (kc_mppi_set_footprint; DESIGN.md 4.12 rules
30 to 36) against the statement tests/mppi_box_ref.py: every S_k, the record, U' and, with a field, f0 and f_nom bit for
bit, with 1, 4 and 8 lanes a sample.  The statement's vectorised form is the reference; tests/test_mppi_box_cpu.py shows it
equal to the loop form.  One reference a case, shared by the three roll-out variants.

Every test uses the 120 x 90 scene map of tests/mppi_ref.py at reach 8; the field's goal lies off the centre, at cell (97,
23)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import mppi_box_ref as mb  # noqa: E402
import mppi_field_ref as mf  # noqa: E402
import mppi_movers_ref as mm  # noqa: E402
import mppi_rates_ref as mr  # noqa: E402
import mppi_ref as mp  # noqa: E402
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
QUIET = MODEL._replace(s=(0, 0, 0))                                        # every sample is the nominal sequence
COSTS = mp.Costs(2, PEN_D2, 11, 3000, 8, 300 << 16, 20, WTAB, 3)
POSE = (40 * ONE + 700, 50 * ONE - 300, 3000)                              # in the first room, the door ahead to the left
M = 17
PX = [round((40.0 + 0.9 * j) * ONE) for j in range(M)]
PY = [round((50.0 + 0.35 * j) * ONE) for j in range(M)]
WEIGHTS = (1 << 20, 32, 2)
RATES = mr.Rates(3000, 5000, 700, 300, 40, 25)
V0 = (30000, -2000, -50)
OFFS8 = tuple(round((-3.0 + 30.0 * i / 7.0) * ONE) for i in range(8))      # a rear-axle reference: from -3 to +27 cells
OFFS = {1: (5 * ONE,), 2: (-4 * ONE, 6 * ONE + 9), 3: OFFS8[:3], 5: OFFS8[::2] + (OFFS8[7],), 8: OFFS8}


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


class Scene:
    """A class plane with its distance plane from the statement and the map that holds it; with `field`, the planner
    that solved on it and its field from the statement."""

    def __init__(self, cls, field=False):
        self.cls = cls
        self.plane = dref.dist2_plane(cls, REACH)
        self.map = kh.WorldMapContext(cls.shape[0], cls.shape[1], RES, ORIGIN)
        self.map.set_prior(cls)
        self.map.set_distance(REACH)
        self.planner = self.field = None
        if field:
            self.planner = kh.PlannerContext()
            self.planner.set_grid(cls)
            self.field = pref.cost_field(pref.validity(cls, R2), GOAL)
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


def nominal(T, F=40000, L=0, Hh=120):
    return [(F + 500 * (t % 3), L, Hh - 40 * (t % 5)) for t in range(T)]


def movers_around(n, around=POSE, seed=0, spread=30):
    """spread 30: with 64 movers the samples end on one at different steps, not all at the first"""
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


def statement(s, K, T, offs, rates=None, v0=V0, weights=None, mv=mm.NONE, model=MODEL, costs=COSTS, pose=POSE, U=None, step=5, seed=9,
              path=(PX, PY), plane=None):
    fld = None if weights is None else mf.Field(s.field, *weights)
    return mb.step(s.plane if plane is None else plane, K, seed, model, costs, *pose, nominal(T) if U is None else U, step, offs, rates, v0,
                   fld, mv, *path)


def case(s, K, T, offs, rates=None, v0=V0, weights=None, mv=mm.NONE, model=MODEL, costs=COSTS, pose=POSE, U=None, step=5, seed=9,
         path=(PX, PY)):
    U = nominal(T) if U is None else U
    want = statement(s, K, T, offs, rates, v0, weights, mv, model, costs, pose, U, step, seed, path)
    with kh.MppiContext(s.map, K, T, seed) as dev:
        configure(dev, model, costs, mv, path)
        if weights is not None:
            dev.set_field(s.planner, *weights)
        if rates is not None:
            dev.set_rates(rates)
            dev.set_velocity(v0)
        dev.set_footprint(offs)
        same(dev, want, *pose, U, step, (K, T, len(offs)), field=weights is not None)
    return want


def differs(a, b):
    return [int(v) for v in a[2]] != [int(v) for v in b[2]]


# ---- the discs and the shapes ----
@pytest.mark.parametrize("nb", [1, 2, 3, 5, 8])
def test_disc_counts(scene, nb):
    """Three and five do not divide a team of four or eight: the last round of a team is part-filled."""
    got = case(scene, 200, 32, OFFS[nb])
    assert differs(got, statement(scene, 200, 32, ()))                     # the footprint is felt
    assert 0 < got[1].n_hit < 200


@pytest.mark.parametrize("T", [1, 8, 32])
@pytest.mark.parametrize("K", [1, 13, 64, 200])
def test_shapes(scene, K, T):
    """K TEAM is no multiple of 64 at most of these: the last wavefront is part-filled."""
    case(scene, K, T, OFFS[5])


def test_asymmetric_offsets_from_minus_3_to_plus_27_cells(scene):
    got = case(scene, 257, 16, OFFS8)
    mirrored = statement(scene, 257, 16, tuple(-o for o in OFFS8))
    assert differs(got, mirrored)                                          # the wall ahead is not behind


def test_the_fifth_disc_alone_hits(scene):
    """The robot stands still at cell (43, 30), heading +x, the wall of column 60 ahead: discs every four cells.  The
    fifth, at column 59, is one cell from the wall (d2 = 1 <= r2 = 2); the fourth, at 55, is 25 away and the pose's own
    cell 289 (FAR at reach 8)."""
    pose, U = (43 * ONE, 30 * ONE, 0), [(0, 0, 0)] * 4
    offs = tuple(4 * i * ONE for i in range(5))
    assert [mb.plane_at(scene.plane, x, y) for x, y in mb.centres(*pose, offs)] == [dref.FAR, dref.FAR, dref.FAR, 25, 1]
    got = case(scene, 65, 4, offs, model=QUIET, pose=pose, U=U)
    assert got[1].n_hit == 65 and set(int(s) for s in got[2]) == {COSTS.pen_hit * 4 + COSTS.w_goal * (M - 1)}
    assert case(scene, 65, 4, offs[:4], model=QUIET, pose=pose, U=U)[1].n_hit == 0
    assert case(scene, 65, 4, offs[4:], model=QUIET, pose=pose, U=U)[1].n_hit == 65   # and alone, as a team's first disc


def test_a_disc_leaves_the_map_while_the_pose_is_inside(scene):
    """Three cells from the border of column 0, heading -x: the disc eight cells ahead lies at column -5 and reads FAR,
    the one at the pose reads the border.  Rule 31 does not clamp a centre onto the map."""
    pose = (3 * ONE + 100, 40 * ONE, 32768)
    assert mp.cell(*mb.centres(*pose, (8 * ONE,))[0]) == (-5, 40)
    far = case(scene, 65, 6, (8 * ONE,), pose=pose, U=nominal(6, 3000, 0, 0), model=QUIET)
    both = case(scene, 65, 6, (0, 8 * ONE), pose=pose, U=nominal(6, 3000, 0, 0), model=QUIET)
    assert far[1].n_hit == 0 and int(far[2][0]) > 0 and differs(far, both)


def test_a_heading_that_wraps_within_the_horizon(scene):
    case(scene, 65, 6, OFFS[5], pose=(40 * ONE, 50 * ONE, 65500), U=nominal(6, 40000, 0, 300))
    case(scene, 65, 6, OFFS[5], pose=(40 * ONE, 50 * ONE, 20), U=nominal(6, 40000, 0, -300))


def test_offsets_at_the_bounds(scene):
    """+-2^22: 64 cells either way.  From the first room the far disc ahead lies beyond the wall, the one behind off the
    map."""
    got = case(scene, 65, 9, (-(1 << 22), 1 << 22))
    assert differs(got, statement(scene, 65, 9, ()))
    case(scene, 65, 9, (1 << 22, 0, -(1 << 22)), pose=(60 * ONE, 57 * ONE, 16384))     # in the door, along the wall


def test_a_boxed_in_pose_where_every_sample_hits_at_step_0(boxed):
    K, T = 257, 5
    got = case(boxed, K, T, OFFS[3], costs=COSTS._replace(r2=25))
    assert got[1].n_hit == K and got[1].k_best == 0 and got[1].den == K * WTAB[0]


def test_the_total_is_cut_at_2_to_the_30(scene):
    """A robot that stands still far from a short path: 64 states of (qcap w_path) >> 16 = 2^24 each."""
    costs = COSTS._replace(w_path=1 << 16, qcap=1 << 24)
    still = MODEL._replace(f_hi=3000)
    got = case(scene, 65, 64, (-2 * ONE, 0, 2 * ONE), costs=costs, model=still, U=[(1000, 0, 10)] * 64, pose=(20 * ONE, 20 * ONE, 0))
    assert got[1].n_hit == 0 and got[1].s_min == got[1].s_0 == 1 << 30 and int(got[2].max()) == 1 << 30


def test_one_disc_at_the_pose_is_the_mode_off(scene):
    K, T = 257, 16
    U = nominal(T)
    off = mr.step(scene.plane, K, 9, OMNI, COSTS, *POSE, U, 5, None, V0, None, mm.NONE, PX, PY)
    assert not differs(statement(scene, K, T, (0,), model=OMNI), off)
    with kh.MppiContext(scene.map, K, T, 9) as dev, kh.MppiContext(scene.map, K, T, 9) as never:
        configure(dev, OMNI, COSTS)
        configure(never, OMNI, COSTS)
        same(never, off, *POSE, U, 5, "never had a footprint")
        dev.set_footprint((0,))
        same(dev, off, *POSE, U, 5, "NB = 1, o = 0")
        dev.set_footprint((0, 0, 0, 0, 0, 0, 0, 0))
        same(dev, off, *POSE, U, 5, "eight discs at the pose")


# ---- with the other terms ----
@pytest.mark.parametrize("N", [1, 64])
def test_with_movers(scene, N):
    U = nominal(33, 9000)
    mv = movers_around(N)
    got = case(scene, 65, 33, OFFS8, mv=mv, U=U)
    assert differs(got, statement(scene, 65, 33, OFFS8, U=U))              # the list is felt
    assert differs(got, statement(scene, 65, 33, (), mv=mv, U=U))          # and so is the footprint
    assert got[1].n_hit_moving <= got[1].n_hit
    if N == 64:
        assert got[1].n_hit_moving > 0


def test_a_mover_that_only_a_rear_disc_reaches(scene):
    """A mover that stands still 7.5 cells behind the pose with a hit distance of two cells.  The rear disc, eight cells
    behind, is within it after the first step whatever the sample (the robot moves by 0 to 2 cells); the disc at the pose,
    at least 5.5 cells away, never is."""
    C, S = mref.headings()[POSE[2]]
    back = -(7 * ONE + ONE // 2)
    mv = mm.movers([(POSE[0] + ((C * back) >> 16), POSE[1] + ((S * back) >> 16), 0, 0, 4 * ONE, 9 * ONE, 7 * ONE)], 2500)
    got = case(scene, 65, 8, (-8 * ONE, 0), mv=mv)
    assert got[1].n_hit_moving == 65
    assert statement(scene, 65, 8, (0,), mv=mv)[1].n_hit_moving == 0


@pytest.mark.parametrize("N", [0, 64])
def test_with_a_cost_field_attached(scene, N):
    """Rule 33: the field is read at the pose's own cell, the plane under the discs."""
    mv = movers_around(N) if N else mm.NONE
    got = case(scene, 257, 32, OFFS8, weights=WEIGHTS, mv=mv, path=(None, None))
    free = statement(scene, 257, 32, (), weights=WEIGHTS, mv=mv, path=(None, None))
    assert got[3][0] == free[3][0] == int(scene.field[40, 50])
    assert differs(got, free)
    if N == 0:
        assert got[1].n_hit > free[1].n_hit


def test_with_rates(scene):
    """Rule 34: the discs turn with the heading the applied control produced."""
    got = case(scene, 257, 32, OFFS8, rates=RATES, model=OMNI)
    assert differs(got, statement(scene, 257, 32, OFFS8, model=OMNI))
    assert differs(got, statement(scene, 257, 32, (), rates=RATES, model=OMNI))


@pytest.mark.parametrize("nb", [3, 8])
def test_with_movers_a_field_and_rates_together(scene, nb):
    mv = movers_around(64)
    got = case(scene, 200, 32, OFFS[nb], rates=RATES, weights=WEIGHTS, mv=mv, model=OMNI, path=(None, None))
    assert differs(got, statement(scene, 200, 32, (), rates=RATES, weights=WEIGHTS, mv=mv, model=OMNI, path=(None, None)))


# ---- the state a context keeps ----
def test_a_footprint_set_cleared_and_set_again(scene):
    K, T = 257, 16
    U = nominal(T)
    on = lambda offs, step: statement(scene, K, T, offs, U=U, step=step, seed=4)   # noqa: E731
    with kh.MppiContext(scene.map, K, T, 4) as dev:
        configure(dev, MODEL, COSTS)
        same(dev, on((), 0), *POSE, U, 0, "before any footprint")
        dev.set_footprint(OFFS8)
        same(dev, on(OFFS8, 1), *POSE, U, 1, "set")
        same(dev, on(OFFS8, 2), *POSE, U, 2, "kept for the next step")
        with pytest.raises(IndexError):                                    # a refused call leaves the list as it was
            dev.set_footprint((0,) * 9)
        with pytest.raises(IndexError):
            dev.set_footprint((0, (1 << 22) + 1))
        same(dev, on(OFFS8, 3), *POSE, U, 3, "after two refusals")
        dev.set_footprint(())
        same(dev, on((), 4), *POSE, U, 4, "cleared: a context that never had one")
        dev.set_footprint(OFFS[3])
        same(dev, on(OFFS[3], 5), *POSE, U, 5, "a shorter list: the entries past it play no part")
        dev.set_footprint(None)
        same(dev, on((), 6), *POSE, U, 6, "cleared by None")


def fresh_map(cls):
    m = kh.WorldMapContext(cls.shape[0], cls.shape[1], RES, ORIGIN)
    m.set_prior(cls)
    m.set_distance(REACH)
    return m


def test_a_step_sees_an_update_under_a_front_disc(scene):
    """The plane is refreshed lazily: an update only marks its box.  A block of occupied cells appears in the door, 20 cells
    ahead of the pose and under the front discs."""
    K, T = 257, 8
    U = nominal(T)
    cls = scene.cls
    with fresh_map(cls) as m, kh.MppiContext(m, K, T, 4) as dev:
        configure(dev, MODEL, COSTS)
        dev.set_footprint(OFFS8)
        same(dev, mb.step(scene.plane, K, 4, MODEL, COSTS, *POSE, U, 0, OFFS8, px=PX, py=PY), *POSE, U, 0, "before")
        grid = np.full((3, 3), 100, np.int32)
        where = (ORIGIN[0] + 59.0 * m.resolution, ORIGIN[1] + 56.0 * m.resolution, 0.0)
        changed = [m.update(grid, where)[0] for _ in range(4)]
        assert changed[2] > 0
        now = np.ascontiguousarray(m.planes()[0])                          # the class plane alone: no refresh
        assert (now != cls).any()
        plane2 = dref.dist2_plane(now, REACH)
        want = mb.step(plane2, K, 4, MODEL, COSTS, *POSE, U, 1, OFFS8, px=PX, py=PY)
        assert differs(want, mb.step(scene.plane, K, 4, MODEL, COSTS, *POSE, U, 1, OFFS8, px=PX, py=PY))
        same(dev, want, *POSE, U, 1, "after the update")


def test_a_step_after_a_shift(scene):
    """The window moves by (3, -2) cells: the plane is wholly dirty, pose and path are given in the new offset."""
    K, T = 65, 8
    U = nominal(T)
    cls = scene.cls
    with fresh_map(cls) as m, kh.MppiContext(m, K, T, 4) as dev:
        configure(dev, MODEL, COSTS)
        dev.set_footprint(OFFS8)
        same(dev, mb.step(scene.plane, K, 4, MODEL, COSTS, *POSE, U, 2, OFFS8, px=PX, py=PY), *POSE, U, 2, "before")
        m.shift(3, -2)
        now = np.ascontiguousarray(m.planes()[0])
        assert (now[:W - 3, 2:] == cls[3:, :H - 2]).all()
        plane2 = dref.dist2_plane(now, REACH, 0)
        pose = (POSE[0] - 3 * ONE, POSE[1] + 2 * ONE, POSE[2])
        px, py = [x - 3 * ONE for x in PX], [y + 2 * ONE for y in PY]
        dev.set_path(px, py)
        same(dev, mb.step(plane2, K, 4, MODEL, COSTS, *pose, U, 3, OFFS8, px=px, py=py), *pose, U, 3, "after the shift")


# ---- through the front end ----
def test_forty_closed_loop_steps_through_the_front_end(scene):
    """kompass_core.control.MPPI(footprint="box") for a 0.7 x 0.2 m robot over the scene against the statement driven with
    the inputs the front end quantised: the offsets and the r2 of rule 36 at the map's resolution."""
    import kompass_cpp
    from kompass_core.control import MPPI, MPPIConfig
    from kompass_core.mapping import WorldMap
    from kompass_core.models import (AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry, RobotState,
                                     RobotType)
    res, dt = 0.05, 0.1
    wm = WorldMap(W, H, res, origin=ORIGIN)
    wm.set_prior(scene.cls)
    robot = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.BOX, geometry_params=np.array([0.7, 0.2, 0.4]))
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=5.0, max_decel=5.0),
                          omega_limits=AngularCtrlLimits(max_vel=1.5, max_steer=0.7, max_acc=5.0, max_decel=5.0))
    cfg = MPPIConfig(seed=3, control_horizon=4, footprint="box")
    fe = MPPI(robot, lim, cfg, control_time_step=dt)
    r32 = float(np.float32(res))
    pts = [(ORIGIN[0] + x * r32, ORIGIN[1] + y * r32) for x, y in mp.SCENE_VERTICES]
    fe.set_path(np.array(pts))
    q = kompass_cpp.control.MPPI.quantise(RobotType.to_kompass_cpp_lib(robot.robot_type), lim.to_kompass_cpp_lib(), dt, res,
                                          cfg.to_kompass_cpp())
    model = mp.Model(*q[:5], tuple(q[5]))
    offs, r2, rho = mb.cover(0.7 / (2.0 * r32), 0.2 / (2.0 * r32))         # a and b as footprintOf forms them; a / b = 3.5
    assert len(offs) == 4 and r2 == math.ceil((rho + 1.5) ** 2) == 18
    costs = mp.scene_costs()._replace(r2=r2)
    assert fe.footprint is None
    state = RobotState(x=pts[0][0], y=pts[0][1], yaw=0.0, speed=0.0)
    prev, x0 = None, state.x
    for n in range(40):
        assert fe.loop_step(current_state=state, local_map=wm)
        i = fe.planner.last_inputs
        U = [tuple(i["u"][3 * k:3 * k + 3]) for k in range(cfg.horizon)]
        assert i["step"] == n and list(i["offsets"]) == offs and i["r2"] == r2
        assert fe.footprint == ([o / 65536.0 for o in offs], r2)
        assert U == ([(0, 0, 0)] * cfg.horizon if prev is None else mp.shift(prev))
        wU, wrec, wS, _ = mb.step(scene.plane, cfg.samples, cfg.seed, model, costs, i["tx"], i["ty"], i["h"], U, n, offs,
                                  px=i["px"], py=i["py"])
        got = list(fe.planner.last_sequence)
        prev = [tuple(got[3 * k:3 * k + 3]) for k in range(cfg.horizon)]
        assert prev == wU, n
        assert fe.record + (fe.n_hit_moving,) == tuple(wrec), (n, fe.record, tuple(wrec))
        assert np.array_equal(np.array(fe.planner.sample_costs(), np.int64), np.asarray(wS, np.int64)), n
        vx, om = fe.linear_x_control, fe.angular_control
        state = RobotState(x=state.x + vx[0] * math.cos(state.yaw) * dt, y=state.y + vx[0] * math.sin(state.yaw) * dt,
                           yaw=state.yaw + om[0] * dt, speed=vx[0])
    assert state.x > x0 + 10 * r32                                         # it has driven
    fe.planner.clear_footprint()                                           # and back: hit_radius' r2, no offsets
    assert fe.loop_step(current_state=state, local_map=wm)
    i = fe.planner.last_inputs
    assert list(i["offsets"]) == [] and i["r2"] == 9 and fe.footprint == ([0.0], 9)
    U = [tuple(i["u"][3 * k:3 * k + 3]) for k in range(cfg.horizon)]
    wU, wrec, wS, _ = mb.step(scene.plane, cfg.samples, cfg.seed, model, mp.scene_costs(), i["tx"], i["ty"], i["h"], U, 40, (),
                              px=i["px"], py=i["py"])
    got = list(fe.planner.last_sequence)
    assert [tuple(got[3 * k:3 * k + 3]) for k in range(cfg.horizon)] == wU
    assert np.array_equal(np.array(fe.planner.sample_costs(), np.int64), np.asarray(wS, np.int64))


def front_end(cfg, params=(0.7, 0.2, 0.4)):
    from kompass_core.control import MPPI
    from kompass_core.models import AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry, RobotType
    robot = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.BOX, geometry_params=np.array(params))
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=5.0, max_decel=5.0),
                          omega_limits=AngularCtrlLimits(max_vel=1.5, max_steer=0.7, max_acc=5.0, max_decel=5.0))
    return MPPI(robot, lim, cfg, control_time_step=0.1)


def test_a_footprint_whose_r2_is_above_the_clearance_s_c2_is_refused(scene):
    """clearance = 4 cells: c2 = 16 below the 0.7 x 0.2 m box's r2 = 18.  A ValueError that names `clearance`, at the step
    (the offsets need the map's resolution); clearance = 4.25 (c2 = 18) passes."""
    from kompass_core.control import MPPIConfig
    from kompass_core.mapping import WorldMap
    from kompass_core.models import RobotState
    wm = WorldMap(W, H, 0.05, origin=ORIGIN)
    wm.set_prior(scene.cls)
    r32 = float(np.float32(0.05))
    pts = [(ORIGIN[0] + x * r32, ORIGIN[1] + y * r32) for x, y in mp.SCENE_VERTICES]
    state = RobotState(x=pts[0][0], y=pts[0][1], yaw=0.0, speed=0.0)
    fe = front_end(MPPIConfig(footprint="box", clearance=4.0, samples=64, horizon=8))
    fe.set_path(np.array(pts))
    with pytest.raises(ValueError, match="clearance"):
        fe.loop_step(current_state=state, local_map=wm)
    ok = front_end(MPPIConfig(footprint="box", clearance=4.25, samples=64, horizon=8))
    ok.set_path(np.array(pts))
    assert ok.loop_step(current_state=state, local_map=wm) and ok.footprint[1] == 18


def test_the_default_lanes_with_a_field_and_a_footprint(scene):
    """No set_team: the field mode without movers takes four lanes a sample, and eight while a footprint is set.  No result
    depends on it: both equal the statement."""
    K, T = 257, 16
    U = nominal(T)
    with kh.MppiContext(scene.map, K, T, 9) as dev:
        configure(dev, MODEL, COSTS, path=(None, None))
        dev.set_field(scene.planner, *WEIGHTS)
        for offs in (OFFS8, (), OFFS[3]):
            dev.set_footprint(offs)
            wU, wrec, wS, wf = statement(scene, K, T, offs, weights=WEIGHTS, path=(None, None))
            gU, grec = dev.step(*POSE, U, 5)
            assert np.array_equal(dev.costs().astype(np.int64), np.asarray(wS, np.int64)), len(offs)
            assert grec.as_tuple() + (int(grec.n_hit_moving),) == tuple(wrec) and [tuple(int(v) for v in r) for r in gU] == list(wU)
            assert dev.last_field() == tuple(wf)
