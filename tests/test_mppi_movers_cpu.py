"""Moving obstacles in the MPPI controller (DESIGN.md 4.12 rules 13 to 18) without a device: the statement
tests/mppi_movers_ref.py in its two forms against each other and, with no mover, against tests/mppi_ref.py; known answers
worked by hand; kc_mppi_check_movers' order of refusals; the front end's quantisation; and the crossing scene in closed
loop on the statement alone."""
import math

import numpy as np
import pytest

import kompass_hip as kh
import mppi_movers_ref as mm
import mppi_ref as mp
import worldmap_dist_ref as dref
import worldmap_mcl_ref as mref

ONE = 1 << 16
FAR = dref.FAR
WT2 = [100, 25]
BASE = mp.Costs(r2=1, pen_d2=[9, 7, 5, 3, 1], pen_far=2, pen_hit=1000, w_path=1 << 16, qcap=1 << 24, w_goal=10, wtab=WT2, w_shift=0)
QUIET = mp.Model(-ONE, ONE, ONE, 2000, 0, (0, 0, 0))


def open_plane(w=40, h=30, value=FAR):
    return np.full((w, h), value, np.uint16)


@pytest.fixture(scope="module")
def scene_plane():
    return dref.dist2_plane(mp.scene_cls(), mp.SCENE_REACH)


def some_movers(n, around, seed=1):
    """n movers within a dozen cells of a place, some near enough to hit, with unlike radii and gains."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        hq = int(rng.integers(0, 6)) ** 2 << 16
        sq = hq + (int(rng.integers(1, 60)) << 16) + int(rng.integers(0, ONE))
        rows.append((around[0] + int(rng.integers(-12 * ONE, 12 * ONE)), around[1] + int(rng.integers(-12 * ONE, 12 * ONE)),
                     int(rng.integers(-ONE, ONE)), int(rng.integers(-ONE, ONE)), hq, sq, int(rng.integers(0, 40 * ONE))))
    return mm.movers(rows, 3000 + n)


def same(a, b):
    assert a[0] == b[0] and tuple(a[1]) == tuple(b[1]) and [int(v) for v in a[2]] == [int(v) for v in b[2]]


# ---- the two forms ----
@pytest.mark.parametrize("N", [0, 1, 3, 9])
def test_the_two_forms_agree(scene_plane, N):
    px, py = mp.quantise_points(mp.polyline_points())
    m = mp.scene_model()._replace(f_lo=-ONE, l_hi=ONE // 2, kq=3000,
                                  s=(mp.scene_model().s[0], mref.noise_scale(0.2 * ONE), mp.scene_model().s[2]))
    U = [(60000 + 900 * t, -3000, 200 - 90 * t) for t in range(7)]
    moving = 0
    for pose in ((px[44], py[44], 2000), (57 * ONE, 50 * ONE, 65000), (2 * ONE, 88 * ONE, 20000)):
        mv = some_movers(N, pose)
        a = mm.step_loop(scene_plane, 41, 6, m, mp.scene_costs(), px[40:75], py[40:75], *pose, U, 9, mv)
        b = mm.step(scene_plane, 41, 6, m, mp.scene_costs(), px[40:75], py[40:75], *pose, U, 9, mv)
        same(a, b)
        moving += a[1].n_hit_moving
        assert a[1].n_hit_moving <= a[1].n_hit
    assert moving == 0 if N == 0 else moving > 0 or N < 9                  # the larger lists do reach rule 16's hit


def test_no_mover_is_the_statement_of_rules_1_to_12(scene_plane):
    """Both forms with N = 0 against mppi_ref.step, on the cases of tests/test_mppi_cpu.py: the hand sums, the hit at
    step 0, the saturation, the ties at the cap, and the scene's three poses."""
    px, py = [10 * ONE, 11 * ONE + ONE // 2], [10 * ONE, 10 * ONE]
    U2 = [(3 * ONE // 4, 0, 0)] * 2
    hit = open_plane()
    hit[11, 10] = 1
    sat = BASE._replace(pen_hit=1 << 20, w_path=1, qcap=1 << 40, w_goal=1 << 20)
    far = ([5000 * ONE, 5001 * ONE], [4000 * ONE] * 2)
    ties = BASE._replace(qcap=4 << 16, w_path=1 << 10)
    noisy = QUIET._replace(s=(mref.noise_scale(0.3 * ONE), 0, mref.noise_scale(300.0)))
    cases = [(open_plane(), 1, 5, QUIET, BASE, px, py, 10 * ONE, 10 * ONE, 0, U2, 0),
             (open_plane(), 2, 7, noisy, BASE, [12 * ONE], [10 * ONE], 10 * ONE, 10 * ONE, 0, [(ONE // 2, 0, 0)], 3),
             (hit, 1, 0, QUIET, BASE, [30 * ONE, 11 * ONE, 12 * ONE], [10 * ONE] * 3, 10 * ONE, 10 * ONE, 0, [(ONE, 0, 0)] * 5, 0),
             (open_plane(), 3, 1, QUIET, sat, *far, 10 * ONE, 10 * ONE, 0, [(100, 0, 0)] * 64, 0),
             (open_plane(), 1, 0, QUIET, ties, [20 * ONE, 30 * ONE, 25 * ONE], [10 * ONE] * 3, 10 * ONE, 10 * ONE, 0, [(0, 0, 0)], 0)]
    sx, sy = mp.quantise_points(mp.polyline_points())
    m = mp.scene_model()._replace(f_lo=-ONE, l_hi=ONE // 2, kq=3000,
                                  s=(mp.scene_model().s[0], mref.noise_scale(0.2 * ONE), mp.scene_model().s[2]))
    U = [(60000 + 900 * t, -3000, 200 - 90 * t) for t in range(7)]
    for pose in ((sx[44], sy[44], 2000), (57 * ONE, 50 * ONE, 65000), (2 * ONE, 88 * ONE, 20000)):
        cases.append((scene_plane, 41, 6, m, mp.scene_costs(), sx[40:75], sy[40:75], *pose, U, 9))
    for c in cases:
        want = mp.step(*c)
        for f in (mm.step_loop, mm.step):
            got = f(*c)
            assert got[0] == want[0] and tuple(got[1]) == tuple(want[1]) + (0,)
            assert [int(v) for v in got[2]] == [int(v) for v in want[2]]


# ---- known answers ----
def one_sample(mv, U, plane=None, px=(30 * ONE,), py=(10 * ONE,), costs=BASE):
    """K = 1 (no noise), heading 0 from (10, 10): F is a step along +x.  -> (S_0, Record) of both forms, shown equal."""
    plane = open_plane() if plane is None else plane
    a = mm.step_loop(plane, 1, 0, QUIET, costs, list(px), list(py), 10 * ONE, 10 * ONE, 0, U, 0, mv)
    b = mm.step(plane, 1, 0, QUIET, costs, list(px), list(py), 10 * ONE, 10 * ONE, 0, U, 0, mv)
    same(a, b)
    return a[2][0], a[1]


def test_thresholds_by_hand():
    """One step of one cell along +x to (11, 10); the mover stands still 3 cells beyond at (14, 10): dx = -3 * 256,
    q = 9 * 65536 exactly.  The rest of the sum: pen_far = 2, the path point 19 cells away at the cap qcap = 2^24: 2^24
    w_path >> 16 = 2^24, w_goal (M - 1 - 0) = 0."""
    rest = 2 + (1 << 24)
    q = 9 << 16
    U = [(ONE, 0, 0)]
    at = lambda hq, sq, g: mm.movers([(14 * ONE, 10 * ONE, 0, 0, hq, sq, g)], 777)   # noqa: E731
    assert one_sample(at(q, q + (5 << 16), 1 << 20), U) == (777, mm.Record(777, 0, 777, 100, 1, 0, 1))      # q == hq: a hit
    S, rec = one_sample(at(q - 1, q - 1 + (5 << 16), 1 << 20), U)          # q == hq + 1: the ramp's top less one 2^-16
    assert S == rest + ((((5 << 16) - 1) >> 16) * (1 << 20) >> 16) == rest + 64 and rec.n_hit == 0
    S, _ = one_sample(at(0, q + 1, 1 << 32), U)                            # q == sq - 1: (1 >> 16) g = 0
    assert S == rest
    S, _ = one_sample(at(0, q + ONE, 1 << 20), U)                          # a whole cell^2 inside: 1 * 2^20 >> 16
    assert S == rest + 16
    S, rec = one_sample(at(0, q, 1 << 32), U)                              # q == sq: nothing
    assert S == rest and rec.n_hit_moving == 0


def test_the_mover_moves_before_it_is_met():
    """Rule 14: after step t the mover has taken t + 1 steps.  It walks -x one cell a step from (14, 10) while the robot
    walks +x one cell a step from (10, 10): after step 0 they stand at (13, 10) and (11, 10), after step 1 both at (12,
    10).  hq = 0: a hit at t = 1 exactly: S = the rest of step 0 + pen_hit_mv (T - 1) + w_goal (M - 1 - jm)."""
    mv = mm.movers([(14 * ONE, 10 * ONE, -ONE, 0, 0, 0, 0)], 500)
    S, rec = one_sample(mv, [(ONE, 0, 0)] * 3)
    assert S == 2 + (1 << 24) + 500 * 2 and rec.n_hit_moving == 1
    S, rec = one_sample(mv, [(ONE, 0, 0)])                                 # T = 1: the meeting would be at step T
    assert S == 2 + (1 << 24) and rec.n_hit == 0


def test_a_static_hit_wins_the_tie():
    plane = open_plane()
    plane[11, 10] = 0
    mv = mm.movers([(11 * ONE, 10 * ONE, 0, 0, ONE, ONE, 0)], 500)
    S, rec = one_sample(mv, [(ONE, 0, 0)] * 4, plane)
    assert S == 1000 * 4 and rec.n_hit == 1 and rec.n_hit_moving == 0


# ---- rule 18 ----
GOOD = [(5 * ONE, 6 * ONE, 100, -100, 4 << 16, 20 << 16, 1000), (-7 * ONE, 0, 0, 0, 0, 1 << 40, 1 << 12)]
BIG = 1 << 36


def rows_with(i, **kw):
    names = ("ox", "oy", "vx", "vy", "hq", "sq", "g")
    rows = [list(r) for r in GOOD]
    for k, v in kw.items():
        rows[i][names.index(k)] = v
    return rows


def two(a, b):
    """Two broken movers: row 0 from a, row 1 from b."""
    return [rows_with(0, **a)[0], rows_with(1, **b)[1]]


REFUSALS = [
    # each case breaks two rules; the earlier one in the documented order must answer
    (dict(rows=[GOOD[0]] * 65, null=("g",)), IndexError, "movers"),         # the count before a null array
    (dict(rows=[GOOD[0]] * 65, pen=(1 << 20) + 1), IndexError, "movers"),
    (dict(rows=GOOD, null=("vx",), pen=(1 << 20) + 1), ValueError, "array"),  # a null array before pen_hit_mv
    (dict(rows=rows_with(0, hq=5, sq=4), pen=(1 << 20) + 1), IndexError, "pen_hit_mv"),   # pen_hit_mv before the movers
    (dict(rows=rows_with(0, ox=BIG + 1, vx=(1 << 22) + 1)), IndexError, "mover 0: a position"),
    (dict(rows=rows_with(0, oy=-BIG - 1, hq=5, sq=4)), IndexError, "mover 0: a position"),
    (dict(rows=rows_with(0, vy=-(1 << 22) - 1, hq=5, sq=4)), IndexError, "mover 0: a velocity"),
    (dict(rows=rows_with(0, hq=(1 << 41) + 1, sq=1 << 41)), ValueError, "mover 0: hq"),   # hq > sq before sq's range
    (dict(rows=rows_with(0, sq=(1 << 40) + 1, g=(1 << 32) + 1)), IndexError, "mover 0: sq"),
    (dict(rows=rows_with(0, hq=0, sq=1 << 40, g=(1 << 32) + 1)), IndexError, "mover 0: g"),   # the gain before the top
    (dict(rows=rows_with(0, hq=0, sq=1 << 40, g=1 << 13)), IndexError, "mover 0: the ramp"),  # 2^24 2^13 >> 16 = 2^21
    (dict(rows=two(dict(g=(1 << 32) + 1), dict(ox=BIG + 1))), IndexError, "mover 0: g"),    # mover by mover, in index order
    (dict(rows=two(dict(hq=5, sq=4), dict(ox=BIG + 1))), ValueError, "mover 0: hq"),
    (dict(rows=two(dict(), dict(vx=1 << 23, hq=5, sq=4))), IndexError, "mover 1: a velocity"),
]


@pytest.mark.parametrize("case,exc,match", REFUSALS)
def test_check_movers_refuses_in_the_documented_order(case, exc, match):
    rows, pen, null = case["rows"], case.get("pen", 100), case.get("null", ())
    cols = dict(zip(("ox", "oy", "vx", "vy", "hq", "sq", "g"), zip(*rows)))
    with pytest.raises(exc, match=match):                                  # the statement: a missing array is an empty one
        mm.check_movers(mm.Movers(*[() if k in null else cols[k] for k in cols], pen))
    with pytest.raises(exc, match=match):
        kh.mppi_check_movers(*[None if k in null else cols[k] for k in cols], pen, n=len(rows))


def test_check_movers_accepts_the_bounds_themselves_and_an_empty_list():
    edge = [(BIG, -BIG, 1 << 22, -(1 << 22), 1 << 40, 1 << 40, 1 << 32), (-BIG, BIG, 0, 0, 0, 1 << 40, 1 << 12)]
    cols = list(zip(*(edge * 32)))
    kh.mppi_check_movers(*cols, 1 << 20)
    mm.check_movers(mm.movers(edge * 32, 1 << 20))
    kh.mppi_check_movers((), (), (), (), (), (), (), (1 << 20) + 1)         # N = 0 is never an error
    kh.mppi_check_movers(None, None, None, None, None, None, None, 1 << 30, n=0)
    mm.check_movers(mm.NONE._replace(pen_hit=1 << 30))


# ---- the front end's host side ----
def want_movers(obs, dt, res, ox, oy, hit_radius, margin, weight):
    r = float(np.float32(res))
    rows = []
    for x, y, vx, vy, rad in obs:
        hit = hit_radius + rad / r
        hq, sq = round(hit * hit * 65536.0), round((hit + margin) * (hit + margin) * 65536.0)
        rows.append((round((x - ox) / r * 65536.0), round((y - oy) / r * 65536.0), round(vx * dt / r * 65536.0),
                     round(vy * dt / r * 65536.0), hq, sq, math.floor(weight * 65536.0 / (((sq - hq) >> 16) + 1))))
    return rows


def test_front_end_quantises_the_movers():
    import kompass_cpp
    from kompass_core.control import MPPIConfig
    M = kompass_cpp.control.MPPI
    cfg = MPPIConfig()
    assert (cfg.mover_margin, cfg.mover_weight, cfg.mover_hit_penalty) == (4.0, 200.0, 4000)
    c = cfg.to_kompass_cpp()
    obs = [(1.234, -0.777, 0.31, -0.45, 0.25), (3.0, 2.0, 0.0, 0.0, 0.0), (-2.5, 7.125, -1.2, 0.6, 0.4)]
    mk = lambda o: [kompass_cpp.control.MovingObstacle(*v) for v in o]     # noqa: E731
    for origin in ((0.0, 0.0), (-0.33, 1.7), (-0.33 + 3 * 0.05, 1.7 - 2 * 0.05)):   # the last: the window shifted by (3, -2) cells
        got = M.movers_of(mk(obs), 0.1, 0.05, *origin, 0.0, 0.0, c)
        want = want_movers(obs, 0.1, 0.05, *origin, cfg.hit_radius, cfg.mover_margin, cfg.mover_weight)
        assert [tuple(r) for r in zip(*got[:7])] == want and got[7] == 4000 and got[8] == 0
        mm.check_movers(mm.movers(want, got[7]))
    a = M.movers_of(mk(obs), 0.1, 0.05, -0.33, 1.7, 0.0, 0.0, c)
    b = M.movers_of(mk(obs), 0.1, 0.05, -0.33 + 3 * 0.05, 1.7 - 2 * 0.05, 0.0, 0.0, c)
    r32 = float(np.float32(0.05))
    assert all(abs(x0 - x1 - 3 * 0.05 / r32 * ONE) <= 1 for x0, x1 in zip(a[0], b[0]))       # three cells, to a rounding
    assert a[2:7] == b[2:7]                                                # what does not depend on the origin
    # a person of 0.25 m at 0.05 m a cell: hit inside 3 + 5 = 8 cells, soft from 12
    assert a[4][0] == 64 << 16 and a[5][0] == 144 << 16 and a[6][0] == (200 * 65536) // 81
    with pytest.raises(IndexError, match="moving obstacle 1"):             # 2^20 cells are 52 km at this resolution
        M.movers_of(mk([obs[0], (60000.0, 0.0, 0.0, 0.0, 0.1)]), 0.1, 0.05, 0.0, 0.0, 0.0, 0.0, c)
    with pytest.raises(IndexError, match="moving obstacle 2"):             # 64 cells a step are 32 m/s here
        M.movers_of(mk([obs[0], obs[1], (0.0, 0.0, 0.0, -40.0, 0.1)]), 0.1, 0.05, 0.0, 0.0, 0.0, 0.0, c)
    with pytest.raises(IndexError, match="moving obstacle 0"):
        M.movers_of(mk([(0.0, 0.0, 0.0, 0.0, 250.0)]), 0.1, 0.05, 0.0, 0.0, 0.0, 0.0, c)     # a soft distance above 4096 cells
    # 65 obstacles on a line from the robot: the farthest, given first, is the one left out, the rest keep their order
    many = [(10.0 + 0.1 * (65 - i), 1.0, 0.0, 0.0, 0.1) for i in range(65)]
    got = M.movers_of(mk(many), 0.1, 0.05, 0.0, 0.0, 10.0, 1.0, c)
    assert got[8] == 1 and len(got[0]) == 64
    assert [tuple(r) for r in zip(*got[:7])] == want_movers(many[1:], 0.1, 0.05, 0.0, 0.0, cfg.hit_radius, cfg.mover_margin, cfg.mover_weight)
    o = M.from_tracked_box([1.0, 2.0, 0.9], [0.6, 0.8, 1.8], [0.5, -0.25, 0.0])
    assert (o.x, o.y, o.vx, o.vy) == (1.0, 2.0, 0.5, -0.25) and o.radius == pytest.approx(0.5)


def test_front_end_takes_the_three_forms_of_a_list():
    from kompass_core.control.mppi import _moving_obstacles

    class Person:
        x, y, vx, vy, radius = 1.0, 2.0, 0.5, -0.5, 0.3

    for given in ([(1.0, 2.0, 0.5, -0.5, 0.3)], np.array([[1.0, 2.0, 0.5, -0.5, 0.3]]), [Person()]):
        o, = _moving_obstacles(given)
        assert (o.x, o.y, o.vx, o.vy, o.radius) == (1.0, 2.0, 0.5, -0.5, 0.3)
    assert _moving_obstacles(None) == [] and _moving_obstacles([]) == [] and _moving_obstacles(np.zeros((0, 5))) == []
    with pytest.raises(ValueError):
        _moving_obstacles(np.zeros((2, 4)))
    with pytest.raises(ValueError):
        _moving_obstacles([(1.0, 2.0, 3.0)])


# ---- the crossing scene in closed loop, on the statement alone ----
@pytest.mark.parametrize("seed", range(6))
def test_the_seeing_controller_passes_the_crossing_mover(scene_plane, seed):
    """The mover walks down column 85 at 0.45 cells a step and crosses the path in the far room.  Arrival within 200 steps,
    q > hq at every step, every occupied cell with d2 > 9.  Measured on this statement, seeds 0 to 5: 144, 144, 146, 147,
    146, 155 steps; the smallest q - hq 85.6, 86.9, 81.3, 87.8, 75.2, 92.4 cells^2; the smallest d2 13 or 16."""
    steps, d2_min, margin = mm.closed_loop(scene_plane, seed, mm.crossing_mover())
    print(f"seed {seed}: {steps} steps, smallest d2 {d2_min}, smallest q - hq {margin / 65536.0:.1f} cells^2")
    assert steps is not None and steps <= 200
    assert margin > 0
    assert d2_min > 9


def test_the_blind_controller_walks_into_it(scene_plane):
    """The same runs with the controller given no mover: at least four of the six seeds come inside hq, so the scene tests
    something.  Measured: q - hq of -10.8, -9.9, +28.9, -15.7, -12.0, -5.9 cells^2 for seeds 0 to 5."""
    margins = [mm.closed_loop(scene_plane, seed, mm.crossing_mover(), seeing=False)[2] for seed in range(6)]
    print("blind: " + ", ".join(f"{m / 65536.0:+.1f}" for m in margins))
    assert sum(m <= 0 for m in margins) >= 4
