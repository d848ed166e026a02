"""A box footprint as a chain of discs inside the MPPI roll-out (DESIGN.md 4.12 rules 30 to 36) without a device: the
statement tests/mppi_box_ref.py in its two forms against each other and, with no offsets or with the one offset 0, against
tests/mppi_rates_ref.py; kc_mppi_check_footprint's order of refusals; rule 36's cover against hand values, in the
statement and in Control::MPPI::footprintOf; the cover theorem against an exact oriented-rectangle test; and the
corridor with an L-turn in closed loop on the statement alone."""
import math

import numpy as np
import pytest

import kompass_hip as kh
import mppi_box_ref as mb
import mppi_field_ref as mf
import mppi_movers_ref as mm
import mppi_rates_ref as mr
import mppi_ref as mp
import worldmap_dist_ref as dref
import worldmap_mcl_ref as mref
from worldmap_ref import OCCUPIED

ONE = 1 << 16


@pytest.fixture(scope="module")
def scene():
    cls = mp.scene_cls()
    return dref.dist2_plane(cls, mp.SCENE_REACH), mf.scene_field(cls), cls == OCCUPIED


@pytest.fixture(scope="module")
def corridor():
    cls = mb.corridor_cls()
    return dref.dist2_plane(cls, mb.L_REACH), cls == OCCUPIED


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
    b = mp.scene_model()
    return b._replace(f_lo=-ONE, l_hi=ONE // 2, kq=3000, s=(b.s[0], mref.noise_scale(0.2 * ONE), b.s[2]))


U7 = [(60000 + 900 * t, -3000, 200 - 90 * t) for t in range(7)]
POSES = ((40 * ONE + 500, 52 * ONE, 2000), (57 * ONE, 50 * ONE, 65000), (4 * ONE, 86 * ONE, 20000))
RATES, V0 = (4096, 9000, 700, 300, 50, 20), (50000, -20000, -300)
OFFSETS = {1: (0,), 3: (-3 * ONE, 5 * ONE + 77, 12 * ONE), 8: tuple(round((-3 + 30 * i / 7) * ONE) for i in range(8)),
           2: (-(1 << 22), 1 << 22)}


# ---- the two forms ----
@pytest.mark.parametrize("field", [False, True])
@pytest.mark.parametrize("N", [0, 3])
@pytest.mark.parametrize("rates", [None, RATES])
@pytest.mark.parametrize("nb", [1, 3, 8, 2])
def test_the_two_forms_agree(scene, field, N, rates, nb):
    """Three poses: in the first room, beside the door, and in a corner from where discs and samples leave the map."""
    plane, f, _ = scene
    px, py = mp.quantise_points(mp.polyline_points())
    fld = mf.Field(f, 1 << 20, 32, 2) if field else None
    for pose in POSES:
        mv = some_movers(N, pose)
        a = mb.step_loop(plane, 41, 6, car(), mp.scene_costs(), *pose, U7, 9, OFFSETS[nb], rates, V0, fld, mv, px[30:70], py[30:70])
        b = mb.step(plane, 41, 6, car(), mp.scene_costs(), *pose, U7, 9, OFFSETS[nb], rates, V0, fld, mv, px[30:70], py[30:70])
        same(a, b)


@pytest.mark.parametrize("field", [False, True])
@pytest.mark.parametrize("rates", [None, RATES])
def test_no_offsets_and_the_one_offset_0_are_rules_1_to_29(scene, field, rates):
    """The mode off is mppi_rates_ref's own step; NB = 1 with o = 0 is the same numbers through rule 31.  A second disc is
    felt."""
    plane, f, _ = scene
    px, py = mp.quantise_points(mp.polyline_points())
    fld = mf.Field(f, 1 << 20, 32, 2) if field else None
    felt = 0
    for pose in POSES:
        mv = some_movers(2, pose)
        want = mr.step(plane, 41, 6, car(), mp.scene_costs(), *pose, U7, 9, rates, V0, fld, mv, px[30:70], py[30:70])
        for form in (mb.step_loop, mb.step):
            same(form(plane, 41, 6, car(), mp.scene_costs(), *pose, U7, 9, (), rates, V0, fld, mv, px[30:70], py[30:70]), want)
            same(form(plane, 41, 6, car(), mp.scene_costs(), *pose, U7, 9, (0,), rates, V0, fld, mv, px[30:70], py[30:70]), want)
        got = mb.step(plane, 41, 6, car(), mp.scene_costs(), *pose, U7, 9, (0, 9 * ONE), rates, V0, fld, mv, px[30:70], py[30:70])
        felt += [int(v) for v in got[2]] != [int(v) for v in want[2]]
    assert felt > 0


def test_rule_31_by_hand():
    """Heading 16384 is +y: (C, S) = (0, 65536).  The centres turn with the heading, are not clamped, and the rounding is
    rule 4's."""
    assert mref.headings()[16384] == (0, 65536) and mref.headings()[0] == (65536, 0)
    assert mb.centres(5 * ONE, 7 * ONE, 0, (-3 * ONE, 2 * ONE + 1)) == [(2 * ONE, 7 * ONE), (7 * ONE + 1, 7 * ONE)]
    assert mb.centres(5 * ONE, 7 * ONE, 16384, (-3 * ONE, 2 * ONE + 1)) == [(5 * ONE, 4 * ONE), (5 * ONE, 9 * ONE + 1)]
    C, S = mref.headings()[8192]
    assert mb.centres(1 << 36, -(1 << 36), 8192, (1 << 22,)) == [((1 << 36) + ((C << 22) + (1 << 15) >> 16), -(1 << 36) + ((S << 22) + (1 << 15) >> 16))]
    plane = np.full((20, 20), dref.FAR, np.uint16)
    plane[2, 7], plane[7, 7] = 5, 9
    assert mb.plane_min(plane, 5 * ONE, 7 * ONE, 0, (-3 * ONE, 2 * ONE)) == 5
    assert mb.plane_min(plane, 5 * ONE, 7 * ONE, 0, (2 * ONE,)) == 9
    assert mb.plane_min(plane, 5 * ONE, 7 * ONE, 0, (-6 * ONE, 15 * ONE)) == dref.FAR      # both off the map


# ---- rule 35 ----
BIG = (1 << 22) + 1
REFUSALS = [
    # each case breaks two rules; the earlier one in the documented order must answer
    ((None, 9), IndexError, "discs"),                                      # the count before the null array
    (((BIG,) * 9, None), IndexError, "discs"),                             # the count before an offset
    (((0, BIG, -BIG), None), IndexError, "offset 1"),                      # offsets in index order
    (((-BIG, 0, 0, 0, 0, 0, 0, BIG), None), IndexError, "offset 0"),
    ((None, 8), ValueError, "null"),                                       # a null array at the cap: the count passes
]


@pytest.mark.parametrize("args,exc,match", REFUSALS)
def test_check_footprint_refuses_in_the_documented_order(args, exc, match):
    with pytest.raises(exc, match=match):
        mb.check_footprint(*args)
    with pytest.raises(exc, match=match):
        kh.mppi_check_footprint(*args)


def test_check_footprint_accepts_the_bounds_and_no_discs_whatever_else_is_given():
    for args in (((), None), (None, 0), ((BIG, BIG), 0), ((0,), None), ((1 << 22, -(1 << 22)) * 4, None)):
        mb.check_footprint(*args)
        kh.mppi_check_footprint(*args)


def test_the_statement_s_steps_check_the_footprint():
    plane = np.full((40, 30), dref.FAR, np.uint16)
    box = mp.Model(-1000, 1000, 500, 200, 0, (0, 0, 0))
    for form in (mb.step_loop, mb.step):
        with pytest.raises(IndexError, match="discs"):
            form(plane, 1, 0, box, mp.scene_costs(), 0, 0, 0, [(0, 0, 0)], 0, (0,) * 9, px=[0], py=[0])
        with pytest.raises(IndexError, match="offset 1"):
            form(plane, 1, 0, box, mp.scene_costs(), 0, 0, 0, [(0, 0, 0)], 0, (0, BIG), px=[0], py=[0])


# ---- rule 36 ----
def test_the_cover_by_hand():
    """1.5 x 0.2 m at 0.05 m: a = 15, b = 2; n = ceil(7.5) = 8, s = 3.75, rho^2 = 4 + 1.875^2 = 7.515625, (rho + 1.5)^2 =
    17.99: r2 = 18.  The first centre at -15 + 1.875 = -13.125 cells."""
    offs, r2, rho = mb.cover(15.0, 2.0)
    assert len(offs) == 8 and rho * rho == pytest.approx(7.515625, abs=1e-12) and r2 == 18
    assert offs == [round((-13.125 + 3.75 * i) * 65536) for i in range(8)] and offs[0] == -860160 and offs[1] - offs[0] == 245760
    assert mb.cover(3.0, 3.0) == ([0], math.ceil((math.sqrt(18.0) + 1.5) ** 2), math.sqrt(18.0))     # a square: one disc at the pose
    assert len(mb.cover(3.0, 4.0)[0]) == 1                                 # wider than long
    offs, r2, rho = mb.cover(50.0, 2.0)                                    # the cap of 8: links of 12.5, a larger rho
    assert len(offs) == 8 and rho == pytest.approx(math.hypot(2.0, 6.25)) and r2 == math.ceil((rho + 1.5) ** 2)
    assert mb.cover(15.0, 2.0, margin=0.0)[1] == 8                         # ceil(7.515625)
    mb.check_footprint(mb.cover(63.0, 1.0)[0])


def test_footprint_of_is_the_cover():
    import kompass_cpp
    fo = kompass_cpp.control.MPPI.footprint_of
    r = float(np.float32(0.05))                                            # the resolution is a float in the class
    offs, r2, rho = fo(1.5, 0.2, 0.05)
    want = mb.cover(1.5 / (2.0 * r), 0.2 / (2.0 * r))                    # a and b as footprintOf forms them
    assert (list(offs), r2) == (want[0], want[1]) and rho == pytest.approx(want[2], rel=1e-12)
    assert len(offs) == 8 and r2 == 18 and rho * rho == pytest.approx(7.515625, rel=1e-6)
    assert (offs[1] - offs[0]) / 65536.0 == pytest.approx(3.75, rel=1e-6)
    offs, r2, rho = fo(0.3, 0.3, 0.05)
    assert list(offs) == [0] and r2 == math.ceil((rho + 1.5) ** 2) and rho == pytest.approx(math.sqrt(18.0), rel=1e-6)
    assert fo(1.5, 0.2, 0.05, 0.0)[1] == 8
    for length, width, res in ((0.6, 0.2, 0.05), (0.4, 0.2, 0.05), (0.8, 0.1, 0.05), (0.9, 0.3, 0.1), (1.2, 0.4, 0.025), (0.7, 0.2, 0.05),
                               (0.35, 0.07, 0.02), (2.0, 0.25, 0.04)):     # whole ratios among them: one formula, one rounding
        rr = float(np.float32(res))
        offs, r2, rho = fo(length, width, res)
        want = mb.cover(length / (2.0 * rr), width / (2.0 * rr))
        assert (list(offs), r2) == (want[0], want[1]) and rho == pytest.approx(want[2], rel=1e-12), (length, width, res)
    for bad in ((0.0, 0.2, 0.05, 1.5), (1.5, -1.0, 0.05, 1.5), (1.5, 0.2, 0.0, 1.5), (1.5, 0.2, 0.05, -0.1), (float("nan"), 0.2, 0.05, 1.5)):
        with pytest.raises(ValueError):
            fo(*bad)
    with pytest.raises(IndexError):
        fo(10.0, 0.2, 0.05)                                                # the outer discs beyond 64 cells


def test_the_front_end_takes_the_box_from_the_robot():
    from kompass_core.control import MPPI, MPPIConfig
    from kompass_core.models import (AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry, RobotType)
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=2.0, max_decel=3.0),
                          omega_limits=AngularCtrlLimits(max_vel=1.5, max_steer=0.7, max_acc=2.5, max_decel=2.5))
    assert MPPIConfig().footprint == "disc" and MPPIConfig().footprint_margin == 1.5
    assert MPPIConfig(footprint="box", footprint_margin=2.0).to_kompass_cpp().footprint_margin == 2.0
    with pytest.raises(ValueError):
        MPPIConfig(footprint="car")
    box = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.BOX, geometry_params=np.array([1.5, 0.2, 0.4]))
    can = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER, geometry_params=np.array([0.1, 0.4]))
    assert MPPI(box, lim, MPPIConfig(footprint="box")).planner.has_box_footprint
    assert not MPPI(box, lim, MPPIConfig()).planner.has_box_footprint
    assert MPPI(box, lim, MPPIConfig(footprint="box")).footprint is None   # before a step
    with pytest.raises(ValueError, match="BOX"):
        MPPI(can, lim, MPPIConfig(footprint="box"))


def test_movers_of_takes_the_discs_reach_in_the_place_of_hit_radius():
    import kompass_cpp
    cfg = kompass_cpp.control.MPPIConfig()
    ob = [kompass_cpp.control.MovingObstacle(1.0, 2.0, 0.1, 0.0, 0.25)]
    mo = kompass_cpp.control.MPPI.movers_of
    plain = mo(ob, 0.1, 0.05, 0.0, 0.0, 0.0, 0.0, cfg)
    assert mo(ob, 0.1, 0.05, 0.0, 0.0, 0.0, 0.0, cfg, -1.0) == plain
    rho = mb.cover(15.0, 2.0)[2]
    got = mo(ob, 0.1, 0.05, 0.0, 0.0, 0.0, 0.0, cfg, rho + 1.5)
    r = float(np.float32(0.05))
    hit = rho + 1.5 + 0.25 / r
    assert got[4] == [round(hit * hit * 65536.0)] and got[5] == [round((hit + cfg.mover_margin) ** 2 * 65536.0)]
    assert got[:4] == plain[:4] and got[4] != plain[4]


# ---- the cover theorem ----
def test_no_state_that_is_not_a_hit_overlaps_an_occupied_cell(scene):
    """sqrt(r2) >= rho + 1.5 > rho + sqrt(2): whenever rule 31 reports no hit, no part of the box overlaps any part of an
    occupied cell.  6000 seeded poses on the door-and-pillar scene: 3000 anywhere on the map, 3000 within a box length of
    the wall, the door, the pillar and the border (clamped onto the map: the pose on it, its discs free to leave it).  Two
    boxes: the showcase's 30 x 4 cells and a 9 x 5 one (n = 2).  Without exception among the states that have at least one
    disc's cell on the map, those with other discs off it included.  Set aside are exactly the states all of whose discs'
    cells lie off the map: rule 31 reads FAR for each, the plane is not looked at once, and such a state is no hit whatever
    lies under the box (a pose in the border's corner with every centre outside).  On this generator they are 41 and 32 of
    the 6000."""
    plane, _, occ = scene
    rng = np.random.default_rng(7)
    near = ((60, 57), (60, 40), (90, 45), (3, 45), (60, 86), (117, 3))
    for (a, b), most_blind in (((15.0, 2.0), 41), ((4.5, 2.5), 32)):
        offs, r2, rho = mb.cover(a, b)
        assert math.sqrt(r2) >= rho + math.sqrt(2.0) and r2 <= mp.SCENE_REACH ** 2
        free = hits = blind = partly = 0
        for n in range(6000):
            if n < 3000:
                x, y = rng.uniform(0.0, mp.SCENE_W - 1), rng.uniform(0.0, mp.SCENE_H - 1)
            else:
                cx, cy = near[n % len(near)]
                x, y = cx + rng.uniform(-a - 4, a + 4), cy + rng.uniform(-a - 4, a + 4)
                x, y = min(max(x, 0.0), mp.SCENE_W - 1.0), min(max(y, 0.0), mp.SCENE_H - 1.0)
            tx, ty, h = round(x * ONE), round(y * ONE), int(rng.integers(0, 65536))
            on = [0 <= I < mp.SCENE_W and 0 <= J < mp.SCENE_H for I, J in (mp.cell(dx, dy) for dx, dy in mb.centres(tx, ty, h, offs))]
            if not any(on):
                assert mb.plane_min(plane, tx, ty, h, offs) == dref.FAR      # the plane was not looked at
                blind += 1
                continue
            partly += not all(on)
            if mb.plane_min(plane, tx, ty, h, offs) <= r2:
                hits += 1
                continue
            free += 1
            assert mb.overlaps(occ, tx, ty, h, a, b) == [], (a, b, tx, ty, h)
        print(f"box {a} x {b}: {free} free, {hits} hits, {partly} of them with a disc off the map, {blind} with every disc off it")
        assert free > 1000 and hits > 1000 and partly >= 100 and blind <= most_blind


def test_the_exact_overlap_test_by_hand():
    occ = np.zeros((40, 40), bool)
    occ[20, 20] = True                                                     # the square [19.5, 20.5]^2
    box = lambda x, y, h: mb.overlaps(occ, round(x * ONE), round(y * ONE), h, 15.0, 2.0)   # noqa: E731
    assert box(4.4, 20.0, 0) == [] and box(4.6, 20.0, 0) == [(20, 20)]     # the front end reaches x + 15
    assert box(20.0, 17.4, 0) == [] and box(20.0, 17.6, 0) == [(20, 20)]   # the side reaches y + 2
    assert box(20.0, 4.4, 16384) == [] and box(20.0, 4.6, 16384) == [(20, 20)]
    # at 45 degrees the square's corner (19.5, 19.5) leads: the box's side lies 2 from its axis, the corner sqrt(2) / 2 from the centre
    d = (2.0 + math.sqrt(0.5)) * math.sqrt(2.0)
    assert box(20.0 + d - 0.01, 20.0, 8192) == [(20, 20)] and box(20.0 + d + 0.01, 20.0, 8192) == []


# ---- the closed loop, on the statement alone ----
@pytest.mark.parametrize("seed", range(6))
def test_the_box_drives_the_corridor_and_its_l_turn(corridor, seed):
    """A 30 x 4-cell box (a = 15, b = 2: eight discs, r2 = 18) down a corridor 22 cells between its walls' centres that
    turns left by 90 degrees into another; the path is chamfered over 15 cells (the box's centre cannot follow a sharp
    corner) and ends 27 cells before the border.  mppi_ref's scene model and costs, K = 512, T = 32.  Arrival within 1.5
    cells inside 200 steps (the bound of every closed-loop scene of 4.12) and no overlap of the box with an occupied cell at
    any state the robot is in, by the exact test.  Measured on this statement, seeds 0 to 5: 138, 147, 129, 152, 131, 133
    steps, no overlap."""
    plane, occ = corridor
    offs, r2, _ = mb.cover(mb.BOX_A, mb.BOX_B)
    steps, bad, hits = mb.closed_loop(plane, occ, seed, offs, r2)
    print(f"box, seed {seed}: {steps} steps, {len(bad)} overlapping states, n_hit at most {max(hits)}")
    assert steps is not None and steps <= 200
    assert bad == []


def test_the_circumscribed_disc_is_boxed_in_from_the_first_step(corridor):
    """The disc around the whole box: radius hypot(15, 2) = 15.13, r2 = ceil(16.63^2) = 277.  The corridor's centre line
    is 11 cells from either wall: every sample of every step hits at its first state, and the robot never leaves.  Seeds 0
    to 5, 20 steps each."""
    plane, occ = corridor
    r2 = math.ceil((math.hypot(mb.BOX_A, mb.BOX_B) + mb.MARGIN) ** 2)
    assert r2 == 277
    for seed in range(6):
        steps, _, hits = mb.closed_loop(plane, occ, seed, [0], r2, max_steps=20)
        assert steps is None and set(hits) == {mb.L_K}


def test_the_disc_of_the_half_width_lets_the_box_s_ends_into_the_walls(corridor):
    """hit_radius = b + margin = 3.5 cells (r2 = 12), what a user sets today, on the path a planner hands a disc: the sharp
    L by (80, 20).  The roll-out does not know where the box's ends are, and at least one state the robot is in overlaps an
    occupied cell.  Seeds in order until one shows it.  Measured on this statement, seeds 0 to 5: 102, 14, 11, 79, 15 and 3
    overlapping states (arrival on four seeds, in 178, 173, 172 and 146 steps).  On the chamfered path of the test above
    the same disc arrives on all six seeds (127 to 133 steps) without an overlap: there the clearance term holds the robot
    on the centre line and the path is one the box can follow."""
    plane, occ = corridor
    r2 = round((mb.BOX_B + mb.MARGIN) ** 2)
    assert r2 == 12
    count = 0
    for seed in range(6):
        steps, bad, _ = mb.closed_loop(plane, occ, seed, [0], r2, vertices=mb.L_SHARP)
        print(f"half-width disc on the sharp path, seed {seed}: {steps} steps, {len(bad)} overlapping states")
        count += len(bad)
        if count:
            break
    assert count >= 1
