"""The grid planner's cost field in the MPPI controller (DESIGN.md 4.12 rules 19 to 24) without a device: the statement
tests/mppi_field_ref.py in its two forms against each other and, with no field, against tests/mppi_movers_ref.py; known
answers worked by hand; kc_mppi_check_field's order of refusals against the statement and the library; and the two
scenes of 4.12 in closed loop on the statement alone, the door and pillar and the trap."""
import numpy as np
import pytest

import kompass_hip as kh
import mppi_field_ref as mf
import mppi_movers_ref as mm
import mppi_ref as mp
import worldmap_dist_ref as dref
import worldmap_mcl_ref as mref

ONE = 1 << 16
FAR = dref.FAR
INF = mf.INF
BASE = mp.Costs(r2=1, pen_d2=[9, 7, 5, 3, 1], pen_far=2, pen_hit=1000, w_path=1 << 16, qcap=1 << 24, w_goal=10, wtab=[100, 25], w_shift=0)
QUIET = mp.Model(-ONE, ONE, ONE, 2000, 0, (0, 0, 0))


@pytest.fixture(scope="module")
def scene():
    cls = mp.scene_cls()
    return dref.dist2_plane(cls, mp.SCENE_REACH), mf.scene_field(cls)


@pytest.fixture(scope="module")
def trap():
    cls = mf.trap_cls()
    return dref.dist2_plane(cls, mp.SCENE_REACH), mf.scene_field(cls)


def same(a, b):
    assert a[0] == b[0] and tuple(a[1]) == tuple(b[1]) and [int(v) for v in a[2]] == [int(v) for v in b[2]] and tuple(a[3]) == tuple(b[3])


def some_movers(n, around, seed=1):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        hq = int(rng.integers(0, 6)) ** 2 << 16
        sq = hq + (int(rng.integers(1, 60)) << 16) + int(rng.integers(0, ONE))
        rows.append((around[0] + int(rng.integers(-12 * ONE, 12 * ONE)), around[1] + int(rng.integers(-12 * ONE, 12 * ONE)),
                     int(rng.integers(-ONE, ONE)), int(rng.integers(-ONE, ONE)), hq, sq, int(rng.integers(0, 40 * ONE))))
    return mm.movers(rows, 3000 + n)


# ---- the two forms ----
@pytest.mark.parametrize("N", [0, 3])
@pytest.mark.parametrize("weights", [(1 << 20, 32, 2), (700, 1 << 12, 64), (1 << 24, 0, 0)])
def test_the_two_forms_agree(scene, N, weights):
    """Three poses: in the first room, beside the door, and in a corner from where samples leave the map (fv = INF
    outside) and hit the border."""
    plane, f = scene
    m = mp.scene_model()._replace(f_lo=-ONE, l_hi=ONE // 2, kq=3000,
                                  s=(mp.scene_model().s[0], mref.noise_scale(0.2 * ONE), mp.scene_model().s[2]))
    U = [(60000 + 900 * t, -3000, 200 - 90 * t) for t in range(7)]
    fld = mf.Field(f, *weights)
    hits = 0
    for pose in ((40 * ONE + 500, 52 * ONE, 2000), (57 * ONE, 50 * ONE, 65000), (4 * ONE, 86 * ONE, 20000)):
        mv = some_movers(N, pose)
        a = mf.step_loop(plane, 41, 6, m, mp.scene_costs(), *pose, U, 9, fld, mv)
        b = mf.step(plane, 41, 6, m, mp.scene_costs(), *pose, U, 9, fld, mv)
        same(a, b)
        hits += a[1].n_hit
        assert a[3][0] == int(f[mp.cell(pose[0], pose[1])])
    assert hits > 0


def test_no_field_is_the_statement_of_rules_1_to_18(scene):
    plane, _ = scene
    px, py = mp.quantise_points(mp.polyline_points())
    m = mp.scene_model()
    U = [(60000 + 900 * t, 0, 200 - 90 * t) for t in range(7)]
    pose = (px[44], py[44], 2000)
    for mv in (mm.NONE, some_movers(3, pose)):
        want = mm.step(plane, 41, 6, m, mp.scene_costs(), px[40:75], py[40:75], *pose, U, 9, mv)
        for form in (mf.step_loop, mf.step):
            got = form(plane, 41, 6, m, mp.scene_costs(), *pose, U, 9, None, mv, px[40:75], py[40:75])
            assert got[0] == want[0] and tuple(got[1]) == tuple(want[1]) and got[3] == (None, None)
            assert [int(v) for v in got[2]] == [int(v) for v in want[2]]


# ---- known answers: K = 1 (no noise), heading 0 from cell (10, 10), one cell a step along +x ----
def one_sample(fplane, fcap, w_run, w_term, U, plane=None, pose=(10 * ONE, 10 * ONE, 0)):
    plane = np.full((40, 30), FAR, np.uint16) if plane is None else plane
    fld = mf.Field(fplane, fcap, w_run, w_term)
    a = mf.step_loop(plane, 1, 0, QUIET, BASE, *pose, U, 0, fld)
    b = mf.step(plane, 1, 0, QUIET, BASE, *pose, U, 0, fld)
    same(a, b)
    return int(a[2][0]), a[1], a[3]


def ramp():
    """f[I, J] = 1000 - 10 I + J: every cell its own value, so a transposed index shows."""
    return (1000 - 10 * np.arange(40)[:, None] + np.arange(30)[None, :]).astype(np.uint32)


def test_sums_by_hand():
    f = ramp()                                                             # f[10, 10] = 910, f[11, 10] = 900, f[12, 10] = 890
    U = [(ONE, 0, 0)] * 2
    S, rec, (f0, f_nom) = one_sample(f, 1 << 20, 32, 2, U)
    assert S == 2 * 2 + ((900 * 32) >> 8) + ((890 * 32) >> 8) + 2 * 890    # pen_far a state, rule 20 a state, rule 21 at the end
    assert (f0, f_nom, rec.n_hit) == (910, 890, 0)
    S, _, (f0, f_nom) = one_sample(f, 895, 256, 1, U)                      # the cap: fc = 895 at (11, 10), 890 at (12, 10)
    assert S == 4 + 895 + 890 + 890 and (f0, f_nom) == (910, 890)
    S, _, (f0, f_nom) = one_sample(f, 1, 1 << 12, 64, U)                   # fcap = 1: (1 * 4096) >> 8 = 16 a state
    assert S == 4 + 16 + 16 + 64 and (f0, f_nom) == (910, 1)
    S, _, _ = one_sample(f, 1 << 20, 1, 0, U)                              # (900 >> 8) + (890 >> 8): the shift floors
    assert S == 4 + 3 + 3


def test_cells_without_a_walk_and_cells_outside_cost_the_cap():
    f = ramp()
    f[11, 10] = INF                                                        # a cut-off cell on the way
    S, rec, (f0, f_nom) = one_sample(f, 5000, 256, 1, [(ONE, 0, 0)])
    assert S == 2 + 5000 + 5000 and (f0, f_nom) == (910, 5000)
    f[10, 10] = INF                                                        # the robot itself in one: f0 is not capped
    _, _, (f0, f_nom) = one_sample(f, 5000, 256, 1, [(0, 0, 0)])
    assert (f0, f_nom) == (INF, 5000)
    S, rec, (f0, f_nom) = one_sample(ramp(), 5000, 256, 1, [(ONE, 0, 0)] * 2, pose=(38 * ONE, 10 * ONE, 0))
    assert S == 2 * 2 + (1000 - 390 + 10) + 5000 + 5000 and (f0, f_nom) == (630, 5000)   # (39, 10), then outside the map
    S, rec, (f0, f_nom) = one_sample(ramp(), 5000, 256, 1, [(ONE, 0, 0)], pose=(-5 * ONE, 10 * ONE, 0))
    assert (f0, f_nom) == (INF, 5000)                                      # a pose outside the map


def test_a_hit_keeps_the_last_field_value_and_a_hit_at_step_0_the_pose_cell():
    f = ramp()
    plane = np.full((40, 30), FAR, np.uint16)
    plane[12, 10] = 0
    S, rec, (f0, f_nom) = one_sample(f, 1 << 20, 256, 3, [(ONE, 0, 0)] * 4, plane)
    assert S == 2 + 900 + 1000 * 3 + 3 * 900 and rec.n_hit == 1 and f_nom == 900   # hit at t = 1: fl is (11, 10)'s
    plane[11, 10] = 1
    S, rec, (f0, f_nom) = one_sample(f, 1 << 20, 256, 3, [(ONE, 0, 0)] * 4, plane)
    assert S == 1000 * 4 + 3 * 910 and rec.n_hit == 1 and (f0, f_nom) == (910, 910)  # hit at t = 0: the pose's own cell
    mv = mm.movers([(11 * ONE, 10 * ONE, 0, 0, ONE, ONE, 0)], 500)         # a mover ends it at t = 0 as well
    fld = mf.Field(f, 1 << 20, 256, 3)
    a = mf.step(np.full((40, 30), FAR, np.uint16), 1, 0, QUIET, BASE, 10 * ONE, 10 * ONE, 0, [(ONE, 0, 0)] * 4, 0, fld, mv)
    assert int(a[2][0]) == 500 * 4 + 3 * 910 and a[1].n_hit_moving == 1 and a[3] == (910, 910)


def test_the_total_is_cut_at_the_cap():
    f = np.full((40, 30), INF, np.uint32)
    S, rec, (f0, f_nom) = one_sample(f, 1 << 24, 1 << 12, 64, [(100, 0, 0)] * 64)
    assert S == rec.s_min == 1 << 30 and (f0, f_nom) == (INF, 1 << 24)     # 64 states of 2^28 and 2^30 at the end


def test_no_path_plays_a_part():
    """Rule 20: M is not looked at, w_path, qcap and w_goal neither."""
    f = ramp()
    fld = mf.Field(f, 1 << 20, 32, 2)
    plane = np.full((40, 30), FAR, np.uint16)
    a = mf.step(plane, 9, 1, QUIET, BASE, 10 * ONE, 10 * ONE, 0, [(ONE, 0, 0)] * 3, 0, fld)
    b = mf.step(plane, 9, 1, QUIET, BASE._replace(w_path=3, qcap=5 << 16, w_goal=77), 10 * ONE, 10 * ONE, 0, [(ONE, 0, 0)] * 3, 0, fld)
    same(a, b)


# ---- rule 23 ----
REFUSALS = [
    # each case breaks two rules; the earlier one in the documented order must answer
    ((0, (1 << 12) + 1, 0), ValueError, "fcap"),                           # fcap == 0 before w_run's range
    ((0, 0, 65), ValueError, "fcap"),                                      # ... and before w_term's
    (((1 << 24) + 1, (1 << 12) + 1, 0), IndexError, "fcap"),               # fcap's range before w_run's
    (((1 << 24) + 1, 0, 65), IndexError, "fcap"),
    ((5, (1 << 12) + 1, 65), IndexError, "w_run"),                         # w_run before w_term
    ((1 << 24, 1 << 12, 65), IndexError, "w_term"),                        # the bounds themselves pass: w_term alone is left
]


@pytest.mark.parametrize("args,exc,match", REFUSALS)
def test_check_field_refuses_in_the_documented_order(args, exc, match):
    with pytest.raises(exc, match=match):
        mf.check_field(*args)
    with pytest.raises(exc, match=match):
        kh.mppi_check_field(*args)


def test_check_field_accepts_the_bounds_themselves():
    for args in ((1, 0, 0), (1 << 24, 1 << 12, 64)):
        mf.check_field(*args)
        kh.mppi_check_field(*args)


def test_a_field_of_another_shape_is_a_state_error():
    plane = np.full((40, 30), FAR, np.uint16)
    for form in (mf.step_loop, mf.step):
        with pytest.raises(mp.StateError):
            form(plane, 1, 0, QUIET, BASE, 10 * ONE, 10 * ONE, 0, [(ONE, 0, 0)], 0, mf.Field(np.zeros((30, 40), np.uint32), 5, 1, 1))
        with pytest.raises(ValueError, match="fcap"):                      # the scalars' check comes before the shape's
            form(plane, 1, 0, QUIET, BASE, 10 * ONE, 10 * ONE, 0, [(ONE, 0, 0)], 0, mf.Field(np.zeros((30, 40), np.uint32), 0, 1, 1))


def test_the_front_end_s_defaults_are_the_scenes():
    from kompass_core.control import MPPIConfig
    cfg = MPPIConfig()
    assert (cfg.field_run_weight, cfg.field_goal_weight, cfg.field_cap) == (mf.FIELD_RUN, mf.FIELD_TERM, mf.FIELD_CAP) == (32, 2, 1 << 20)
    c = cfg.to_kompass_cpp()
    assert (c.field_run_weight, c.field_goal_weight, c.field_cap) == (32, 2, 1 << 20)
    with pytest.raises(ValueError):
        MPPIConfig(field_cap=0)
    with pytest.raises(ValueError):
        MPPIConfig(field_run_weight=(1 << 12) + 1)
    with pytest.raises(ValueError):
        MPPIConfig(field_goal_weight=65)


# ---- the two scenes in closed loop, on the statement alone ----
@pytest.mark.parametrize("seed", range(6))
def test_door_and_pillar_by_the_field(scene, seed):
    """Goal cell (110, 45), no path, the planner's r2 = 9.  Arrival within 1.5 cells inside 200 steps, d2 > 9 on every
    occupied cell.  Measured on this statement, seeds 0 to 5: 83, 88, 83, 89, 82, 83 steps; the smallest d2 26, 25, 25,
    25, 25, 25.  The path mode of tests/test_mppi_cpu.py needs 129 to 138 steps on this scene."""
    steps, d2_min, cells = mf.closed_loop(*scene, seed)
    print(f"door, seed {seed}: {steps} steps, smallest d2 {d2_min}, last cell {cells[-1]}")
    assert steps is not None and steps <= 200
    assert d2_min > 9


@pytest.mark.parametrize("seed", range(6))
def test_the_trap_by_the_field(trap, seed):
    """The U open towards the robot, between it and the goal.  The same two assertions.  Measured on this statement,
    seeds 0 to 5: 89, 98, 90, 92, 89, 96 steps; the smallest d2 25, 20, 25, 29, 25, 25."""
    steps, d2_min, cells = mf.closed_loop(*trap, seed)
    print(f"trap, seed {seed}: {steps} steps, smallest d2 {d2_min}, last cell {cells[-1]}")
    assert steps is not None and steps <= 200
    assert d2_min > 9


@pytest.mark.parametrize("seed", range(3))
def test_the_trap_holds_the_path_mode(trap, seed):
    """The path mode on the straight polyline from start to goal ends inside the U and does not arrive in 300 steps.
    Measured on this statement, seeds 0 to 2: the last cells (65, 46), (63, 45), (60, 44)."""
    steps, cells = mf.closed_loop_path(trap[0], seed)
    print(f"trap by the path, seed {seed}: {steps}, last cell {cells[-1]}")
    assert steps is None
    assert 45 <= cells[-1][0] < 70 and 30 < cells[-1][1] < 60             # inside the U
