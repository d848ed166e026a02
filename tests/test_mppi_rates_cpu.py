"""Acceleration limits inside the MPPI roll-out (DESIGN.md 4.12 rules 25 to 29) without a device: the statement
tests/mppi_rates_ref.py in its two forms against each other; with no rates, and with rates at the box's width, against
tests/mppi_field_ref.py; known answers of rule 26 worked by hand; kc_mppi_check_rates' order of refusals and
kc_mppi_apply_rates against the statement and the library; and the door-and-pillar scene in closed loop on the statement
alone, under a robot that obeys the rates."""
import numpy as np
import pytest

import kompass_hip as kh
import mppi_field_ref as mf
import mppi_movers_ref as mm
import mppi_rates_ref as mr
import mppi_ref as mp
import worldmap_dist_ref as dref
import worldmap_mcl_ref as mref

ONE = 1 << 16


@pytest.fixture(scope="module")
def scene():
    cls = mp.scene_cls()
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


def car():
    """Reverse, a lateral channel and a cone: every branch of rule 26."""
    b = mp.scene_model()
    return b._replace(f_lo=-ONE, l_hi=ONE // 2, kq=3000, s=(b.s[0], mref.noise_scale(0.2 * ONE), b.s[2]))


U7 = [(60000 + 900 * t, -3000, 200 - 90 * t) for t in range(7)]
POSES = ((40 * ONE + 500, 52 * ONE, 2000), (57 * ONE, 50 * ONE, 65000), (4 * ONE, 86 * ONE, 20000))


# ---- the two forms ----
@pytest.mark.parametrize("field", [False, True])
@pytest.mark.parametrize("N", [0, 3])
@pytest.mark.parametrize("rates,v0", [((1, 1, 1, 1, 1, 1), (0, 0, 0)), ((4096, 9000, 700, 300, 50, 20), (50000, -20000, -300)),
                                      ((1 << 23, 1 << 23, 1 << 23, 1 << 23, 65535, 65535), (1 << 22, -(1 << 22), 32767)),
                                      ((3000, 1 << 23, 1, 1 << 23, 1, 65535), (-(1 << 22), 1 << 22, -32767))])
def test_the_two_forms_agree(scene, field, N, rates, v0):
    """Three poses: in the first room, beside the door, and in a corner from where samples leave the map."""
    plane, f = scene
    px, py = mp.quantise_points(mp.polyline_points())
    fld = mf.Field(f, 1 << 20, 32, 2) if field else None
    hits = 0
    for pose in POSES:
        mv = some_movers(N, pose)
        a = mr.step_loop(plane, 41, 6, car(), mp.scene_costs(), *pose, U7, 9, rates, v0, fld, mv, px[30:70], py[30:70])
        b = mr.step(plane, 41, 6, car(), mp.scene_costs(), *pose, U7, 9, rates, v0, fld, mv, px[30:70], py[30:70])
        same(a, b)
        hits += a[1].n_hit
    if v0 != (0, 0, 0):
        assert hits > 0


@pytest.mark.parametrize("field", [False, True])
def test_no_rates_and_rates_at_the_box_s_width_are_rules_1_to_24(scene, field):
    """Rule 27's last sentence.  One below the width on one channel is felt: the bound is tight."""
    plane, f = scene
    px, py = mp.quantise_points(mp.polyline_points())
    fld = mf.Field(f, 1 << 20, 32, 2) if field else None
    m = car()
    wide = mr.box_rates(m)
    assert wide == (m.f_hi - m.f_lo,) * 2 + (2 * m.l_hi,) * 2 + (2 * m.h_hi,) * 2
    felt = 0
    for pose in POSES:
        mv = some_movers(2, pose)
        want = mf.step(plane, 41, 6, m, mp.scene_costs(), *pose, U7, 9, fld, mv, px[30:70], py[30:70])
        for form in (mr.step_loop, mr.step):
            same(form(plane, 41, 6, m, mp.scene_costs(), *pose, U7, 9, None, (5, 6, 7), fld, mv, px[30:70], py[30:70]), want)
            for v0 in ((0, 0, 0), (m.f_lo, m.l_hi, 0), (m.f_hi, -m.l_hi, 0)):     # H0 = 0: inside the cone whatever F0 is
                same(form(plane, 41, 6, m, mp.scene_costs(), *pose, U7, 9, wide, v0, fld, mv, px[30:70], py[30:70]), want)
        tight = wide._replace(f_up=wide.f_up // 4)
        got = mr.step(plane, 41, 6, m, mp.scene_costs(), *pose, U7, 9, tight, (m.f_lo, 0, 0), fld, mv, px[30:70], py[30:70])
        felt += [int(v) for v in got[2]] != [int(v) for v in want[2]]
    assert felt > 0


# ---- rule 26 by hand ----
BOX = mp.Model(-1000, 1000, 500, 200, 0, (0, 0, 0))
CONE = BOX._replace(kq=1 << 13)                                            # |H| <= |F| / 8


def applied(m, rates, v0, U):
    """The statement and the library, which must agree -> [A[t]]"""
    want = mr.apply_rates(m, rates, v0, U)
    got = kh.mppi_apply_rates(m[:5], rates, v0, U)
    assert got.dtype == np.int32 and [tuple(int(v) for v in r) for r in got] == want
    return want


def test_rule_26_by_hand():
    # up != dn: F rises by 300 a step and falls by 100; L the other way round; H by 1
    r = (300, 100, 50, 400, 1, 1)
    U = [(1000, -500, 200)] * 4 + [(0, 500, -200)] * 3
    assert applied(BOX, r, (0, 0, 0), U) == [(300, -400, 1), (600, -500, 2), (900, -500, 3), (1000, -500, 4),
                                            (900, -450, 3), (800, -400, 2), (700, -350, 1)]
    # V0 outside the box: it comes in at dn (or up), the box plays no part in rule 26
    assert applied(BOX, r, (1 << 22, -(1 << 22), -32767), [(1000, 0, 0)] * 2) == [
        ((1 << 22) - 100, -(1 << 22) + 50, -32766), ((1 << 22) - 200, -(1 << 22) + 100, -32765)]
    # a negative value rising towards zero takes up, falling away from zero takes dn: the rates are signed, not by magnitude
    assert applied(BOX, r, (-1000, 0, 0), [(0, 0, 0), (0, 0, 0), (-1000, 0, 0)]) == [(-700, 0, 0), (-400, 0, 0), (-500, 0, 0)]
    # a target inside one step is met, not overshot
    assert applied(BOX, r, (0, 0, 0), [(299, -399, 1), (300, 0, 0)]) == [(299, -399, 1), (300, -349, 0)]


def test_the_cone_binds_on_the_applied_f():
    """kq = 2^13: |A_H| <= |A_F| >> 3.  X asks for F = 1000 and H = 100, inside its own cone (125); the applied F is 80 a
    step, so the cone of the applied F binds; then F falls and the shrinking cone takes H down faster than H_dn = 1."""
    r = (80, 400, 1, 1, 60, 1)
    U = [(1000, 0, 100)] * 3 + [(0, 0, 100)] * 2
    assert applied(CONE, r, (0, 0, 0), U) == [(80, 0, 10), (160, 0, 20), (240, 0, 30), (0, 0, 0), (0, 0, 0)]
    # the value behind the cone is the next p: from 30, not from the 60 + 60 + 60 the limiter alone would have reached
    assert applied(CONE, (80, 100, 1, 1, 60, 1), (0, 0, 0), U)[3:] == [(140, 0, 17), (40, 0, 5)]
    assert applied(CONE, r, (-800, 0, -100), [(-800, 0, -100)]) == [(-800, 0, -100)]          # |F| counts, and H's sign is kept
    assert applied(CONE._replace(kq=0), r, (0, 0, 0), U[:1]) == [(80, 0, 60)]                # no cone without kq


def test_rate_1_moves_by_one_a_step():
    got = applied(BOX, (1, 1, 1, 1, 1, 1), (5, -5, 0), [(1000, 500, -200)] * 64)
    assert got == [(5 + t, -5 + t, -t) for t in range(1, 65)]


def test_apply_rates_refuses_what_the_step_and_the_checks_refuse():
    ok = ((0, 1000, 0, 100, 0), (1, 1, 1, 1, 1, 1), (0, 0, 0))
    kh.mppi_apply_rates(*ok, [(0, 0, 0)] * 64)
    with pytest.raises(ValueError):
        kh.mppi_apply_rates(*ok, [])                                       # no step
    with pytest.raises(IndexError):
        kh.mppi_apply_rates(*ok, [(0, 0, 0)] * 65)
    with pytest.raises(ValueError):
        kh.mppi_apply_rates((5, 4, 0, 0, 0), ok[1], ok[2], [(0, 0, 0)])    # an empty box
    with pytest.raises(ValueError):
        kh.mppi_apply_rates(ok[0], (1, 1, 0, 1, 1, 1), ok[2], [(0, 0, 0)])
    with pytest.raises(IndexError):
        kh.mppi_apply_rates(ok[0], ok[1], (0, 0, 32768), [(0, 0, 0)])
    with pytest.raises(IndexError):
        kh.mppi_apply_rates(*ok, [(0, 0, 0), ((1 << 22) + 1, 0, 0)])
    with pytest.raises(ValueError):
        kh.mppi_apply_rates(ok[0], None, ok[2], [(0, 0, 0)])               # NULL rates: nothing to apply


# ---- rule 29 ----
BIG, TURN = (1 << 23) + 1, 65536
REFUSALS = [
    # each case breaks two rules; the earlier one in the documented order must answer
    (((0, 1, 1, 1, 1, 0), None), ValueError, "rate 0"),                    # a rate below 1, in index order
    (((1, 1, 1, 0, -5, 1), None), ValueError, "rate 3"),
    (((BIG, 1, 1, 1, 1, 0), None), ValueError, "rate 5"),                  # below 1 anywhere before above the cap anywhere
    (((1, 1, 1, 1, TURN, 0), None), ValueError, "rate 5"),
    (((1, BIG, 1, BIG, 1, 1), None), IndexError, "rate 1"),                # F and L rates in index order
    (((1, 1, 1, BIG, TURN, 1), None), IndexError, "rate 3"),               # an F or L rate before an H rate
    (((1, 1, 1, 1, TURN, TURN), None), IndexError, "rate 4"),
    (((1, 1, 1, 1, 1, TURN), (BIG, 0, 0)), IndexError, "rate 5"),          # the rates before v0
    (((0, 1, 1, 1, 1, 1), (0, 0, 40000)), ValueError, "rate 0"),
    (((1, 1, 1, 1, 1, 1), ((1 << 22) + 1, 0, 32768)), IndexError, r"V0\[0\]"),   # F0, L0 before H0
    (((1, 1, 1, 1, 1, 1), (0, -(1 << 22) - 1, -32768)), IndexError, r"V0\[1\]"),
    (((1 << 23, 1 << 23, 1 << 23, 1 << 23, 65535, 65535), (1 << 22, -(1 << 22), -32768)), IndexError, "H0"),   # the bounds pass
]


@pytest.mark.parametrize("args,exc,match", REFUSALS)
def test_check_rates_refuses_in_the_documented_order(args, exc, match):
    with pytest.raises(exc, match=match):
        mr.check_rates(*args)
    with pytest.raises(exc, match=match):
        kh.mppi_check_rates(*args)


def test_check_rates_accepts_the_bounds_and_null_rates_whatever_v0_is():
    for args in (((1, 1, 1, 1, 1, 1), None), ((1 << 23, 1 << 23, 1 << 23, 1 << 23, 65535, 65535), (1 << 22, -(1 << 22), -32767)),
                 (None, None), (None, (1 << 30, 0, 1 << 20))):
        mr.check_rates(*args)
        kh.mppi_check_rates(*args)


def test_the_statement_s_steps_check_the_rates():
    plane = np.full((40, 30), dref.FAR, np.uint16)
    for form in (mr.step_loop, mr.step):
        with pytest.raises(ValueError, match="rate 2"):
            form(plane, 1, 0, BOX, mp.scene_costs(), 0, 0, 0, [(0, 0, 0)], 0, (1, 1, 0, 1, 1, 1), px=[0], py=[0])
        with pytest.raises(IndexError, match="H0"):
            form(plane, 1, 0, BOX, mp.scene_costs(), 0, 0, 0, [(0, 0, 0)], 0, (1, 1, 1, 1, 1, 1), (0, 0, 32768), px=[0], py=[0])


# ---- the front end's arithmetic ----
def test_the_front_end_forms_the_rates_where_it_forms_the_box():
    import math

    import kompass_cpp
    from kompass_core.control import MPPIConfig
    from kompass_core.models import AngularCtrlLimits, LinearCtrlLimits, RobotCtrlLimits, RobotType
    assert MPPIConfig().acceleration_limits is False and MPPIConfig().to_kompass_cpp().acceleration_limits is False
    cfg = MPPIConfig(acceleration_limits=True)
    assert cfg.to_kompass_cpp().acceleration_limits is True
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=2.0, max_decel=3.0),
                          vy_limits=LinearCtrlLimits(max_vel=0.5, max_acc=0.7, max_decel=0.0),
                          omega_limits=AngularCtrlLimits(max_vel=1.5, max_steer=0.7, max_acc=2.5, max_decel=1e9))
    r, dt = float(np.float32(0.05)), 0.1
    kind = RobotType.to_kompass_cpp_lib(RobotType.OMNI)
    q = kompass_cpp.control.MPPI.quantise(kind, lim.to_kompass_cpp_lib(), dt, 0.05, cfg.to_kompass_cpp())
    lin, ang = dt * dt / r * 65536.0, dt * dt / (2 * math.pi) * 65536.0
    assert tuple(q[6]) == (round(2.0 * lin), round(3.0 * lin), round(0.7 * lin), 1, round(2.5 * ang), 65535)   # clamped into rule 25's range
    mr.check_rates(tuple(q[6]))
    big = kompass_cpp.control.MPPI.quantise(kind, lim.to_kompass_cpp_lib(), 10.0, 0.05, cfg.to_kompass_cpp())
    assert tuple(big[6])[:2] == (1 << 23, 1 << 23)
    off = kompass_cpp.control.MPPI.quantise(kind, lim.to_kompass_cpp_lib(), dt, 0.05, MPPIConfig().to_kompass_cpp())
    assert tuple(off[:6]) == tuple(q[:6])                                  # the box and the scales do not depend on the mode


# ---- the closed loop, on the statement alone ----
@pytest.mark.parametrize("seed", range(6))
def test_door_and_pillar_under_the_limits(scene, seed):
    """The robot obeys F_up = F_dn = 4096 (1/16 cell a step^2) and H_up = H_dn = 50 and moves by v = rule 26(v, U'[0]);
    the controller knows the rates and v.  Arrival within 1.5 cells inside 200 steps, d2 > 9 on every occupied cell.
    Measured on this statement, seeds 0 to 5: 155, 146, 131, 135, 139, 148 steps; the smallest d2 13, 13, 10, 10, 13,
    13."""
    steps, d2_min, cells = mr.closed_loop_limited(scene[0], seed, mr.SCENE_RATES, aware=True)
    print(f"limited, aware, seed {seed}: {steps} steps, smallest d2 {d2_min}, last cell {cells[-1]}")
    assert steps is not None and steps <= 200
    assert d2_min > 9


def test_the_scene_bites_the_step_that_does_not_know_the_limits(scene):
    """The step of rules 1 to 12 under the same robot: its U'[0] passes through rule 26 behind the step.  On at least
    four of the six seeds it comes to d2 <= 9 or does not arrive in 200 steps.  Measured on this statement, seeds 0 to 5:
    no arrival in 200 steps on any; the smallest d2 1, 2, 0, 0, 10, 0; the last cells (82, 55), (105, 46), (103, 49),
    (109, 40), (93, 51), (105, 41)."""
    bitten = 0
    for seed in range(6):
        steps, d2_min, cells = mr.closed_loop_limited(scene[0], seed, mr.SCENE_RATES, aware=False)
        print(f"limited, not aware, seed {seed}: {steps} steps, smallest d2 {d2_min}, last cell {cells[-1]}")
        bitten += steps is None or d2_min <= 9
    assert bitten >= 4
