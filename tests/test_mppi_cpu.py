"""The MPPI statement tests/mppi_ref.py on known answers worked by hand from the rules, its two forms
against each other, the closed loop on the statement alone, and the host-only entries of the library: kc_mppi_check's
order of refusals and the front end's quantisation.  No GPU."""
import math

import numpy as np
import pytest

import kompass_hip as kh
import mppi_ref as mp
import worldmap_dist_ref as dref
import worldmap_mcl_ref as mref
from worldmap_ref import EMPTY, OCCUPIED

ONE = 1 << 16
FAR = dref.FAR


def open_plane(w=40, h=30, value=FAR):
    return np.full((w, h), value, np.uint16)


WT2 = [100, 25]
BASE = mp.Costs(r2=1, pen_d2=[9, 7, 5, 3, 1], pen_far=2, pen_hit=1000, w_path=1 << 16, qcap=1 << 24, w_goal=10, wtab=WT2, w_shift=0)
QUIET = mp.Model(-ONE, ONE, ONE, 2000, 0, (0, 0, 0))


def test_k1_is_the_nominal_sequence_and_the_hand_sum():
    """One sample: eps = 0, U' = clampU(U).  Heading 0, (C, S) = (65536, 0): F = 3/4 cell a step along +x from (10, 10).
    Plane FAR everywhere: pen_far = 2 a step.  Path points (10, 10), (11.5, 10): after step 0 at x = 10.75 the nearer is
    point 1, q = (0.75 * 256)^2 = 36864, term (q * 2^16) >> 16 = 36864, jm = 1; after step 1 at x = 11.5 q = 0.  The cone
    is off; H = 70000 is clamped to 2000 in U' only (U_in itself must respect the bounds, so the test uses 2000).
    S = 2 + 36864 + 2 + 0 + w_goal (2 - 1 - 1) = 36868."""
    px, py = [10 * ONE, 11 * ONE + ONE // 2], [10 * ONE, 10 * ONE]
    U = [(3 * ONE // 4, 0, 0), (3 * ONE // 4, 0, 0)]
    for f in (mp.step_loop, mp.step):
        out, rec, S = f(open_plane(), 1, 5, QUIET, BASE, px, py, 10 * ONE, 10 * ONE, 0, U, 0)
        assert out == U and list(S) == [36868]
        assert rec == mp.Record(36868, 0, 36868, 100, 0, 0)
    tight = QUIET._replace(f_hi=ONE // 2, h_hi=50)
    out, rec, _ = mp.step_loop(open_plane(), 1, 5, tight, BASE, px, py, 10 * ONE, 10 * ONE, 0, [(3 * ONE // 4, 0, 900)] * 2, 0)
    assert out == [(ONE // 2, 0, 50)] * 2                                  # U' = clampU(U)


def test_two_samples_and_a_two_entry_table():
    """K = 2, T = 1: sample 0 is U, sample 1 is U + eps.  With w_shift = 0 and wtab = [100, 25] the worse sample (by more
    than 0) weighs 25: U' = U + floor((2 * 25 * d + 125) / 250) for the better nominal, d = X_1 - U; the other way round
    U + floor((2 * 100 * d + 125) / 250)."""
    m = QUIET._replace(s=(mref.noise_scale(0.3 * ONE), 0, mref.noise_scale(300.0)))
    px, py = [12 * ONE], [10 * ONE]
    U = [(ONE // 2, 0, 0)]
    seen = set()
    for step in range(12):
        key = mp.sample_key(7, step)
        X1 = mp.sample(m, key, U, 1, 0)
        out, rec, S = mp.step_loop(open_plane(), 2, 7, m, BASE, px, py, 10 * ONE, 10 * ONE, 0, U, step)
        assert rec.den == 125 and rec.s_0 == S[0] and S[0] != S[1]
        w1 = 25 if S[0] < S[1] else 100
        want = tuple(U[0][c] + (2 * w1 * (X1[c] - U[0][c]) + 125) // 250 for c in range(3))
        assert out == [mp.clamp_u(m, *want)] and rec.k_best == (0 if S[0] < S[1] else 1)
        seen.add(rec.k_best)
        assert mp.step(open_plane(), 2, 7, m, BASE, px, py, 10 * ONE, 10 * ONE, 0, U, step)[0] == out
    assert seen == {0, 1}


def test_the_cone_takes_the_magnitude_of_a_reverse_step():
    m = mp.Model(-ONE, ONE, 0, 3000, 1000, (0, 0, 0))
    assert mp.clamp_u(m, -40000, 5, 3000) == (-40000, 0, (40000 * 1000) >> 16)   # 610
    assert mp.clamp_u(m, -40000, 0, -3000) == (-40000, 0, -610)
    assert mp.clamp_u(m, -2 * ONE, 0, 3000) == (-ONE, 0, 1000)                    # the cone sees the clamped F
    assert mp.clamp_u(m, 0, 0, 77) == (0, 0, 0)                                   # standing still, a car cannot turn
    out, _, _ = mp.step_loop(open_plane(), 1, 0, m, BASE, [0], [0], 10 * ONE, 10 * ONE, 0, [(-40000, 0, 3000)], 0)
    assert out == [(-40000, 0, 610)]


def test_heading_wraps_from_65535():
    assert mp.advance(0, 0, 65535, 0, 0, 3)[2] == 2
    assert mp.advance(0, 0, 1, 0, 0, -3)[2] == 65534
    C, S = mref.headings()[65535]
    assert (C, S) == (65536, -6)
    tx, ty, h = mp.advance(5 * ONE, 5 * ONE, 65535, ONE, 0, 1)
    assert (tx, ty, h) == (6 * ONE, 5 * ONE - 6, 0)                       # the heading BEFORE the step turns the step


def test_a_hit_at_step_0():
    """The robot's first step lands on a cell with d2 = 1 <= r2: pen_hit T, nothing else but the terminal term with
    jm = 0, whatever the path says."""
    plane = open_plane()
    plane[11, 10] = 1
    px, py = [30 * ONE, 11 * ONE, 12 * ONE], [10 * ONE] * 3
    U = [(ONE, 0, 0)] * 5
    for f in (mp.step_loop, mp.step):
        _, rec, S = f(plane, 1, 0, QUIET, BASE, px, py, 10 * ONE, 10 * ONE, 0, U, 0)
        assert list(S) == [1000 * 5 + 10 * 2] and rec.n_hit == 1
    plane[11, 10], plane[12, 10] = FAR, 0                                  # a hit at step 1 keeps step 0's jm = 1
    _, rec, S = mp.step_loop(plane, 1, 0, QUIET, BASE, px, py, 10 * ONE, 10 * ONE, 0, U, 0)
    assert list(S) == [2 + 0 + 1000 * 4 + 10 * (2 - 1)]


def test_saturation_at_2_to_the_30():
    """pen_hit = 2^20 and T = 64 give 2^26 for a hit at step 0; the cap is reached by the path term: qcap = 2^40 and
    w_path = 1 add 2^24 a step far from the path, 64 steps 2^30, and the total is cut there."""
    c = BASE._replace(pen_hit=1 << 20, w_path=1, qcap=1 << 40, w_goal=1 << 20)
    far = ([5000 * ONE, 5001 * ONE], [4000 * ONE] * 2)
    U = [(100, 0, 0)] * 64
    for f in (mp.step_loop, mp.step):
        _, rec, S = f(open_plane(), 3, 1, QUIET, c, *far, 10 * ONE, 10 * ONE, 0, U, 0)
        assert list(S) == [1 << 30] * 3 and rec.s_min == 1 << 30 and rec.k_best == 0 and rec.den == 300
    _, rec, S = mp.step_loop(open_plane(value=0), 1, 1, QUIET, c, *far, 10 * ONE, 10 * ONE, 0, U, 0)
    assert list(S) == [(1 << 26) + (1 << 20)]


def test_ties_of_the_path_search_at_the_cap_go_to_the_lowest_index():
    """Every point beyond the cap has the same key but for j: jm = 0, and the terminal term is w_goal (M - 1)."""
    c = BASE._replace(qcap=4 << 16, w_path=1 << 10)                         # two cells
    px, py = [20 * ONE, 30 * ONE, 25 * ONE], [10 * ONE] * 3
    for f in (mp.step_loop, mp.step):
        _, _, S = f(open_plane(), 1, 0, QUIET, c, px, py, 10 * ONE, 10 * ONE, 0, [(0, 0, 0)], 0)
        assert list(S) == [2 + (((4 << 16) << 10) >> 16) + 10 * 2]
    px = [20 * ONE, 11 * ONE, 11 * ONE]                                     # an exact tie below the cap: the lower index
    _, _, S = mp.step_loop(open_plane(), 1, 0, QUIET, c, px, py, 10 * ONE, 10 * ONE, 0, [(0, 0, 0)], 0)
    assert list(S) == [2 + ((256 * 256) << 10 >> 16) + 10 * 1]


def test_the_two_forms_agree():
    cls = mp.scene_cls()
    plane = dref.dist2_plane(cls, mp.SCENE_REACH)
    px, py = mp.quantise_points(mp.polyline_points())
    m = mp.scene_model()._replace(f_lo=-ONE, l_hi=ONE // 2, kq=3000, s=(mp.scene_model().s[0], mref.noise_scale(0.2 * ONE), mp.scene_model().s[2]))
    U = [(60000 + 900 * t, -3000, 200 - 90 * t) for t in range(7)]
    for pose in ((px[44], py[44], 2000), (57 * ONE, 50 * ONE, 65000), (2 * ONE, 88 * ONE, 20000)):
        a = mp.step_loop(plane, 41, 6, m, mp.scene_costs(), px[40:75], py[40:75], *pose, U, 9)
        b = mp.step(plane, 41, 6, m, mp.scene_costs(), px[40:75], py[40:75], *pose, U, 9)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == [int(v) for v in b[2]]
    assert a[1].n_hit > 0


# ---- rule 12 ----
LIM = (0, ONE, 0, 1000, 0)
S3 = (1, 2, 3)
GOOD = (2, [5, 4, 3, 2, 1], 100, 8, 1 << 20, 7, [10, 5], 1)            # r2, pen_d2, pen_hit, w_path, qcap, w_goal, wtab, w_shift


def with_cost(**kw):
    names = ("r2", "pen_d2", "pen_hit", "w_path", "qcap", "w_goal", "wtab", "w_shift")
    d = dict(zip(names, GOOD))
    d.update(kw)
    return tuple(d[n] for n in names)


def ref_check(K, T, M, limits=None, s=None, costs=None, reach=0):
    model = None if limits is None else mp.Model(*limits, tuple(s))
    c = None if costs is None else mp.Costs(costs[0], costs[1], 0, *costs[2:])
    mp.check(K, T, M, model, c, reach)


REFUSALS = [
    # each case breaks two rules; the earlier one in the documented order must answer
    (dict(K=0, T=65), ValueError),                                          # no sample, before too many steps
    (dict(K=65537, T=65), IndexError),
    (dict(K=65537, limits=(1, 0, 0, 0, 0)), IndexError),                    # counts before limits
    (dict(T=65, M=0), ValueError),
    (dict(M=257, limits=(1, 0, 0, 0, 0)), IndexError),
    (dict(limits=(1, 0, 0, 40000, 0)), ValueError),                         # an empty box before H_hi's range
    (dict(limits=(0, ONE, -1, 0, 1 << 25)), ValueError),
    (dict(limits=(0, (1 << 22) + 1, 0, 40000, 0)), IndexError),
    (dict(limits=(0, ONE, 0, 32768, 0), s=(-1, 0, 0)), IndexError),         # the limits before the scales
    (dict(limits=(0, ONE, 0, 10, (1 << 24) + 1), s=(-1, 0, 0)), IndexError),
    (dict(s=(0, -1, 0), costs=with_cost(pen_d2=[1])), ValueError),          # the scales before the costs
    (dict(costs=with_cost(pen_d2=[1], pen_hit=1 << 21)), ValueError),       # the table's length before pen_hit
    (dict(costs=with_cost(pen_d2=[0] * 4097, r2=5000)), IndexError),
    (dict(costs=with_cost(r2=5, pen_hit=1 << 21)), ValueError),             # r2 > c2 before pen_hit
    (dict(costs=with_cost(pen_hit=(1 << 20) + 1, w_path=1 << 17)), IndexError),
    (dict(costs=with_cost(w_path=(1 << 16) + 1, wtab=[])), IndexError),
    (dict(costs=with_cost(qcap=(1 << 40) + 1, wtab=[])), IndexError),
    (dict(costs=with_cost(qcap=1 << 40, w_path=2, wtab=[])), IndexError),   # (qcap >> 16) w_path = 2^25
    (dict(costs=with_cost(w_goal=(1 << 20) + 1, wtab=[])), IndexError),
    (dict(costs=with_cost(wtab=[]), reach=255), IndexError),                # the reach before the weight table
    (dict(costs=with_cost(wtab=[]), reach=1), ValueError),                  # c2 = 4 > reach^2 = 1
    (dict(costs=with_cost(wtab=[0])), ValueError),
    (dict(costs=with_cost(wtab=[1] * 4097, w_shift=31)), IndexError),       # the table's length before the shift
    (dict(costs=with_cost(wtab=[5, 6], w_shift=31)), ValueError),
    (dict(costs=with_cost(wtab=[(1 << 20) + 1, 6])), ValueError),
    (dict(costs=with_cost(wtab=[5, 6])), ValueError),
]


@pytest.mark.parametrize("case,exc", REFUSALS)
def test_check_refuses_in_the_documented_order(case, exc):
    a = dict(K=8, T=4, M=3, limits=LIM, s=S3, costs=GOOD, reach=0)
    a.update(case)
    with pytest.raises(exc):
        ref_check(a["K"], a["T"], a["M"], a["limits"], a["s"], a["costs"], a["reach"])
    with pytest.raises(exc):
        kh.mppi_check(a["K"], a["T"], a["M"], a["limits"], a["s"], a["costs"], a["reach"])


def test_check_accepts_the_bounds_themselves():
    edge = with_cost(pen_d2=[0] * 4096, r2=4095, pen_hit=1 << 20, w_path=1, qcap=1 << 40, w_goal=1 << 20, wtab=[1 << 20] * 4096, w_shift=30)
    for costs, reach in ((GOOD, 2), (edge, 64), (with_cost(w_path=1 << 16, qcap=1 << 24), 0)):
        kh.mppi_check(65536, 64, 256, (-(1 << 22), 1 << 22, 1 << 22, 32767, 1 << 24), (0, 0, 2 ** 31 - 1), costs, reach)
        ref_check(65536, 64, 256, (-(1 << 22), 1 << 22, 1 << 22, 32767, 1 << 24), (0, 0, 2 ** 31 - 1), costs, reach)
    kh.mppi_check(1, 1, 1)


# ---- the closed loop on the statement alone ----
@pytest.fixture(scope="module")
def scene_plane():
    cls = mp.scene_cls()
    assert cls.shape == (120, 90) and (cls[60, 52:62] == EMPTY).all() and cls[60, 51] == cls[60, 62] == OCCUPIED
    return dref.dist2_plane(cls, mp.SCENE_REACH)


def test_scene_path_is_as_described():
    pts = mp.polyline_points()
    assert len(pts) == 41 + 20 + 41 + 1 and pts[0] == (10.0, 45.0) and pts[41] == (50.0, 56.5) and pts[-1] == (110.0, 45.0)
    c = mp.scene_costs()
    assert c.pen_d2[0] == 60 and c.pen_d2[49] == 0 and len(c.pen_d2) == 50 and c.wtab[0] == 65535 and len(c.wtab) == 256
    mp.check(mp.SCENE_K, mp.SCENE_T, mp.SCENE_WINDOW, mp.scene_model(), c, mp.SCENE_REACH)


@pytest.mark.parametrize("seed", range(6))
def test_closed_loop_reaches_the_goal_clear_of_every_obstacle(scene_plane, seed):
    """Within 1.5 cells of the last point in at most 200 steps, every occupied cell with d2 > 9.  Measured on this
    statement: 130, 129, 138, 131, 129, 135 steps for seeds 0 to 5, the smallest d2 on the way 13 or 16."""
    steps, d2_min, cells = mp.closed_loop(scene_plane, seed)
    print(f"seed {seed}: {steps} steps, smallest d2 {d2_min}")
    assert steps is not None and steps <= 200
    assert d2_min > 9
    cross = [(a, b) for a, b in zip(cells, cells[1:]) if a[0] < 60 <= b[0]]  # up to two cells a step: column 60 may be skipped
    assert len(cross) == 1 and all(52 <= J <= 61 for _, J in cross[0])     # through the door, once


# ---- the front end's host side ----
def test_front_end_quantises_the_scene_and_refuses_other_maps():
    import kompass_cpp
    from kompass_core.control import MPPI, MPPIConfig
    from kompass_core.models import (AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry, RobotState,
                                     RobotType)
    cfg = MPPIConfig()
    t = kompass_cpp.control.MPPI.costs_of(cfg.to_kompass_cpp())
    assert mp.Costs(t[0], list(t[1]), t[2], t[3], t[4], t[5], t[6], list(t[7]), t[8]) == mp.scene_costs()
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=2.0, max_decel=2.0),
                          vy_limits=LinearCtrlLimits(max_vel=0.5, max_acc=2.0, max_decel=2.0),
                          omega_limits=AngularCtrlLimits(max_vel=1.5, max_steer=0.7, max_acc=2.0, max_decel=2.0))
    r = float(np.float32(0.05))
    want_s = (mref.noise_scale(0.5 * ONE), mref.noise_scale(0.5 * ONE), mref.noise_scale(cfg.sigma_turn / (2 * math.pi) * 65536.0))
    for kind, l_hi, kq, s1 in ((RobotType.DIFFERENTIAL_DRIVE, 0, 0, 0), (RobotType.OMNI, round(0.5 * 0.1 / r * 65536.0), 0, want_s[1]),
                               (RobotType.ACKERMANN, 0, round(65536.0 / (2 * math.pi * 0.5 / r)), 0)):
        q = kompass_cpp.control.MPPI.quantise(RobotType.to_kompass_cpp_lib(kind), lim.to_kompass_cpp_lib(), 0.1, 0.05, cfg.to_kompass_cpp())
        assert tuple(q[:5]) == (0, round(1.0 * 0.1 / r * 65536.0), l_hi, round(1.5 * 0.1 / (2 * math.pi) * 65536.0), kq), kind
        assert tuple(q[5]) == (want_s[0], s1, want_s[2])
    back = MPPIConfig(allow_reverse=True).to_kompass_cpp()
    assert kompass_cpp.control.MPPI.quantise(RobotType.to_kompass_cpp_lib(RobotType.OMNI), lim.to_kompass_cpp_lib(), 0.1, 0.05, back)[0] == -131072
    robot = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER, geometry_params=np.array([0.1, 0.4]))
    fe = MPPI(robot, lim, cfg, control_time_step=0.1)
    assert fe.linear_x_control == [0.0] and fe.angular_control == [0.0] and not fe.path
    with pytest.raises(TypeError, match="WorldMap"):
        fe.loop_step(current_state=RobotState(x=0.0, y=0.0, yaw=0.0), local_map=np.zeros((5, 5)))
    with pytest.raises(TypeError, match="WorldMap"):
        fe.loop_step(current_state=RobotState(x=0.0, y=0.0, yaw=0.0))
    with pytest.raises(ValueError):
        MPPI(robot, lim, MPPIConfig(hit_radius=9.0, clearance=7.0), control_time_step=0.1)    # r2 above c2
    with pytest.raises((ValueError, IndexError)):
        MPPIConfig(samples=70000)
