"""The world map's virtual laser scan (DESIGN.md 4.11 rules 20 to 27) without a GPU: the library's two host-only entries
(kc_worldmap_scan_table, kc_worldmap_scan_check) against the Python statement tests/worldmap_scan_ref.py, and the
statement itself against a straight wall's closed form and a 7 x 5 map whose hit cells are written out by hand."""
import math

import numpy as np
import pytest

import kompass_hip as kh
import worldmap_ref as ref
import worldmap_scan_ref as sref

F32 = np.float32
OCC, UNK, EMP = ref.OCCUPIED, ref.UNEXPLORED, ref.EMPTY


# ---- rule 21 ---------------------------------------------------------------------------------------------------------
def table_both(angles):
    got = kh.worldmap_scan_table(angles)
    want = sref.scan_table(angles)
    assert got.dtype == np.int32 and got.shape == (len(angles), 2)
    assert (got.astype(np.int64) == want).all(), [a for a, g, w in zip(angles, got, want) if tuple(g) != tuple(w)][:5]
    return got


def test_table_on_seeded_angles():
    r = np.random.default_rng(21)
    table_both(r.uniform(-math.pi, math.pi, 4000))
    table_both(r.uniform(-50.0, 50.0, 2000))
    table_both(r.uniform(-1e-6, 1e-6, 200))


def test_table_on_multiples_of_quarter_pi_zeros_and_large_angles():
    quarter = [k * (math.pi / 4) for k in range(-16, 17)]
    assert quarter[0] == -4 * math.pi and quarter[-1] == 4 * math.pi
    t = table_both(quarter)
    assert tuple(t[16]) == (1 << 30, 0)                                    # angle 0
    assert tuple(t[18]) == (0, 1 << 30) and tuple(t[20]) == (-(1 << 30), 0)  # pi / 2, pi: the tiny cos / sin round to 0
    assert t[17][0] == t[17][1] == 759250125                               # pi / 4: dx == dy under yaw 0
    assert tuple(table_both([0.0, -0.0])[1]) == (1 << 30, 0)
    r = np.random.default_rng(22)
    table_both(list(1e6 + r.uniform(-1.0, 1.0, 500)) + [1e6, -1e6])
    assert np.abs(t.astype(np.int64)).max() <= 1 << 30


def test_table_refuses_a_non_finite_angle_and_writes_nothing():
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            kh.worldmap_scan_table([0.1, bad, 0.2])
        with pytest.raises(ValueError):
            sref.scan_table([0.1, bad, 0.2])
    assert kh.worldmap_scan_table([]).shape == (0, 2)


# ---- rules 20, 21 and 25: the refusals --------------------------------------------------------------------------------
def check_both(*args):
    got, want = kh.worldmap_scan_check(*args), sref.scan_check(*args)
    assert got == want, (args, got, want)
    return got


def test_every_refusal_of_the_scan_check():
    assert check_both(0.05, 1, 360, 10.0, 0) == 200
    assert check_both(0.05, 1, 360, 10.0, kh.SCAN_UNKNOWN_BLOCKS) == 200
    for f in (kh.worldmap_scan_check, sref.scan_check):
        for poses, beams in [(0, 360), (1, 0), (0, 0)]:
            with pytest.raises(ValueError):
                f(0.05, poses, beams, 10.0, 0)
        f(0.05, 1, 65536, 10.0, 0)
        f(0.05, 64, 65536, 10.0, 0)                                        # exactly 2^22 rays
        f(0.05, 1 << 22, 1, 10.0, 0)
        for poses, beams in [(1, 65537), (65, 65536), ((1 << 22) + 1, 1), (4195, 1000)]:
            with pytest.raises(IndexError):
                f(0.05, poses, beams, 10.0, 0)
        for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError):
                f(0.05, 1, 360, bad, 0)
        with pytest.raises(IndexError):
            f(0.05, 1, 360, 102.5, 0)                                      # 2050 cells
        f(0.05, 1, 360, 102.4, 0)                                          # 2048 cells at float32(0.05)
        for flags in (2, 3, 4, 1 << 31):
            with pytest.raises(ValueError):
                f(0.05, 1, 360, 10.0, flags)
        for res in (0.0, -0.05, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                f(res, 1, 360, 10.0, 0)
        # the order: counts before range_max before flags
        with pytest.raises(ValueError):
            f(0.05, 0, 360, 1000.0, 0)
        with pytest.raises(IndexError):
            f(0.05, 1, 65537, float("nan"), 0)
        with pytest.raises(IndexError):
            f(0.05, 1, 360, 1000.0, 2)


@pytest.mark.parametrize("res,mult", [(0.05, 64), (0.05, 1), (0.25, 40), (0.1, 128), (0.05, 2048)])
def test_radius_at_and_around_a_whole_number_of_cells(res, mult):
    r = F32(res)
    exact = F32(r * F32(mult))
    assert float(exact) / float(r) == mult, "the case must be an exact multiple in float"
    below, above = np.nextafter(exact, F32(0)), np.nextafter(exact, F32(np.inf))
    assert check_both(res, 1, 8, float(exact), 0) == mult
    assert check_both(res, 1, 8, float(below), 0) == mult
    if mult < sref.MAX_RADIUS:
        assert check_both(res, 1, 8, float(above), 0) == mult + 1
    else:
        for f in (kh.worldmap_scan_check, sref.scan_check):
            with pytest.raises(IndexError):
                f(res, 1, 8, float(above), 0)


# ---- the statement against a straight wall ---------------------------------------------------------------------------
def test_statement_recovers_a_straight_wall_within_a_millimetre():
    """A wall of occupied cells along I = 205 of a 210 x 420 map at 0.05 m; its near face is the plane x = origin_x +
    204.5 cells.  Poses by seed at 0.5 to 5 m from the face, beams at up to 60 degrees of incidence, so up to 10 m.

    The bound.  Cq and Sq are each within 2^-17 of cos and sin (half a unit of 16 fraction bits), so the walked
    direction is within sqrt(2) 2^-17 = 1.1e-5 rad of the beam's and its length within the same fraction of 1; rule 21's
    2^-31 is nothing beside that.  At distance d and incidence i the face is met at d cos(i) / cos(i + da): the error is
    d da tan(i) <= 10 m x 1.1e-5 x tan(60 deg) = 0.19 mm, the length adds d x 1.1e-5 = 0.11 mm, the pose's 2^-17 cell
    is 4e-7 m, double rounding less.  0.3 mm in all: 1 mm holds with margin."""
    res, origin = 0.05, (-1.3, 2.2)
    W, H, wall = 210, 420, 205
    cls = np.full((W, H), EMP, np.int8)
    cls[wall, :] = OCC
    r = float(F32(res))
    face = origin[0] + (wall - 0.5) * r
    rng = np.random.default_rng(2024)
    worst = 0.0
    for _ in range(20):
        perp = rng.uniform(0.5, 5.0)
        x, y = face - perp, origin[1] + (210 + rng.uniform(-10, 10)) * r
        yaw = rng.uniform(-math.pi, math.pi)
        world_dir = rng.uniform(-math.pi / 3, math.pi / 3, 24)             # the incidence, from the wall's normal
        angles = world_dir - yaw
        ranges, cells = sref.scan(cls, res, origin, [(x, y, yaw)], angles, 10.5)
        want = perp / np.cos(world_dir)
        assert want.max() <= 10.0 and (cells[0] % W == wall).all()
        worst = max(worst, float(np.abs(ranges[0] - want).max()))
    print(f"worst deviation from the closed form: {worst * 1e3:.4f} mm")
    assert worst <= 1e-3


# ---- the statement on a 7 x 5 map written out by hand ----------------------------------------------------------------
# resolution 0.25 and origin (0, 0): every number below is exact in binary.  Cell (I, J) spans [I - 1/2, I + 1/2) cells.
#   J=4  . . . . . . .
#   J=3  . . . . . . .
#   J=2  . ? . # . . #        # occupied, ? never observed
#   J=1  . . . . # . .
#   J=0  . . . . . # .
#        0 1 2 3 4 5 6  = I
RES7 = 0.25
DIAG = 759250125  # lrint(cos(pi / 4) 2^30) = lrint(sin(pi / 4) 2^30)


def map7():
    cls = np.full((7, 5), EMP, np.int8)
    for cell in [(3, 2), (6, 2), (4, 1), (5, 0)]:
        cls[cell] = OCC
    cls[1, 2] = UNK
    return cls


def one_beam(cells_xy, angle, range_max, flags=0, real=None):
    """The pose in cells (so (3, 2) is that cell's centre), yaw 0 -> (range, hit cell as (I, J) or None)."""
    x, y = cells_xy[0] * RES7, cells_xy[1] * RES7
    ranges, cells = sref.scan(map7(), RES7, (0.0, 0.0), [(x, y, 0.0)], [angle], range_max, flags,
                              None if real is None else [real])
    c = int(cells[0, 0])
    return float(ranges[0, 0]), (None if c < 0 else (c % 7, c // 7))


def diag_range(e):
    return (float(e) * 16384.0 / float(DIAG)) * RES7


PI = math.pi
HAND = [
    # a beam at exactly 45 degrees from the corner (1/2, 1/2) of cell (1, 1): dx == dy, fx = fy = 0, every step ties and
    # x goes first: (2, 1), (2, 2), (3, 2).  The ray runs through the corner of (3, 2) and hits it on its 2nd x step
    ((0.5, 0.5), PI / 4, 2.0, 0, diag_range(2 * 65536), (3, 2)),
    # axis-aligned: dy == 0 from the centre of (0, 2) through the never-observed (1, 2); dx == 0 from (3, 0) upwards;
    # dy == 0 backwards from (5, 2)
    ((0.0, 2.0), 0.0, 2.0, 0, 2.5 * RES7, (3, 2)),
    ((3.0, 0.0), PI / 2, 2.0, 0, 1.5 * RES7, (3, 2)),
    ((5.0, 2.0), PI, 2.0, 0, 1.5 * RES7, (3, 2)),
    ((3.0, 4.0), -PI / 2, 2.0, 0, 1.5 * RES7, (3, 2)),
    # rule 25: with the flag the never-observed cell ends the first of those beams
    ((0.0, 2.0), 0.0, 2.0, sref.UNKNOWN_BLOCKS, 0.5 * RES7, (1, 2)),
    # a start on the boundary between (3, 2) and (4, 2), fx == 0: backwards the first step has e = 0, forwards 65536
    ((3.5, 2.0), PI, 2.0, 0, 0.0, (3, 2)),
    ((3.5, 2.0), 0.0, 2.0, 0, 2.0 * RES7, (6, 2)),
    # a start inside a blocking cell
    ((6.0, 2.0), 1.234, 2.0, 0, 0.0, (6, 2)),
    ((6.2, 1.9), -2.0, 2.0, 0, 0.0, (6, 2)),
    # a start outside the map looking in, and looking away
    ((-2.0, 2.0), 0.0, 2.0, 0, 4.5 * RES7, (3, 2)),
    ((-2.0, 2.0), PI, 2.0, 0, 2.0, None),
    # the diagonal gap between (5, 0) and (4, 1), whose shared corner is (4.5, 0.5): from the corner (3.5, -0.5) at 45
    # degrees the ray runs exactly through it and ends in (5, 0), the x step of the tie; from the centre of (5, 1) at 225
    # degrees it ends in (4, 1) alike
    ((3.5, -0.5), PI / 4, 2.0, 0, diag_range(65536), (5, 0)),
    ((5.0, 1.0), 5 * PI / 4, 2.0, 0, diag_range(32768), (4, 1)),
    # a hit at exactly range_max counts (2.5 cells of 0.25 m = 0.625 m, exact); one float lower it does not
    ((0.0, 2.0), 0.0, 0.625, 0, 0.625, (3, 2)),
    ((0.0, 2.0), 0.0, float(np.nextafter(F32(0.625), F32(0))), 0, float(np.nextafter(F32(0.625), F32(0))), None),
    # nothing on the way: range_max
    ((0.0, 4.0), 0.0, 5.0, 0, 5.0, None),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_written_map(case):
    start, angle, range_max, flags, want_r, want_cell = HAND[case]
    got_r, got_cell = one_beam(start, angle, range_max, flags)
    assert got_cell == want_cell and got_r == want_r, (HAND[case], got_r, got_cell)


def test_hand_written_direction_is_the_diagonal():
    """what the 45 degree cases rest on: under yaw 0 the direction is the table's entry, and both are DIAG"""
    t = sref.scan_table([PI / 4, 5 * PI / 4])
    assert t.tolist() == [[DIAG, DIAG], [-DIAG, -DIAG]]
    assert ref.quantise_pose(RES7, (0.0, 0.0), 0.5 * RES7, 0.5 * RES7, 0.0) == (65536, 0, 32768, 32768)
    assert (65536 * DIAG + (1 << 15)) >> 16 == DIAG


# ---- rule 27 -----------------------------------------------------------------------------------------------------------
def test_merge_with_a_present_scan():
    v = 2.5 * RES7                                                         # the map's range of this beam
    for real, want in [(float("nan"), v), (float("inf"), v), (-float("inf"), v), (0.3, 0.3), (0.7, v), (v, v),
                       (math.nextafter(v, 0.0), math.nextafter(v, 0.0)), (0.0, 0.0)]:
        got, cell = one_beam((0.0, 2.0), 0.0, 2.0, 0, real=real)
        assert got == want and cell == (3, 2), (real, got)
        assert sref.merge(real, v) == want
    # a beam without a hit: the present range below range_max wins, the cell stays -1
    assert one_beam((0.0, 4.0), 0.0, 5.0, 0, real=1.5) == (1.5, None)
    assert one_beam((0.0, 4.0), 0.0, 5.0, 0, real=7.0) == (5.0, None)
