"""The world map's obstacle window (DESIGN.md 4.11 rules 16 to 19): the library's host-only kc_worldmap_window against the
numpy statement tests/worldmap_points_ref.py, every refusal of rule 16, and the statement itself on a map written out by
hand.  No GPU needed."""
import math

import numpy as np
import pytest

import kompass_hip as kh
import worldmap_points_ref as pref
import worldmap_ref as ref

F32 = np.float32


def both(res, origin, x, y, rng):
    got = kh.worldmap_window(res, origin, x, y, rng)
    want = pref.window(res, origin, x, y, rng)
    assert got == want, (res, origin, x, y, rng, got, want)
    return got


@pytest.mark.parametrize("res,origin", [(0.05, (-0.33, 1.7)), (0.1, (0.1, -0.7)), (0.25, (0.0, 0.0)),
                                        (0.05, (1e5 + 0.1, -3e4 - 0.3)), (1.0 / 3.0, (-1.0 / 3.0, 2.0 / 7.0))])
def test_window_on_seeded_positions(res, origin):
    r = np.random.default_rng(5)
    rr = float(F32(res))
    for _ in range(200):
        x, y = origin[0] + r.uniform(-400, 400), origin[1] + r.uniform(-400, 400)     # negative offsets too
        both(res, origin, x, y, float(r.uniform(0.01, 50.0)))
    # exactly on cell centres and cell boundaries (the half-way cases of the shift), either side of the origin
    for ci, cj in [(0, 0), (3, -4), (-7, 2), (1000, -1000)]:
        for fi, fj in [(0.0, 0.0), (0.5, 0.5), (-0.5, 0.5), (0.5, -0.5), (0.25, -0.75)]:
            x, y = origin[0] + (ci + fi) * rr, origin[1] + (cj + fj) * rr
            both(res, origin, x, y, 3.0)
            both(res, origin, math.nextafter(x, math.inf), math.nextafter(y, -math.inf), 3.0)


def test_half_cells_round_up_on_exact_arithmetic():
    # resolution 0.25 and these offsets are exact in binary: tx is exactly (c + 1/2) 2^16, and (tx + 2^15) >> 16 is c + 1
    assert both(0.25, (0.0, 0.0), 0.125, -0.125, 1.0)[:2] == (1, 0)
    assert both(0.25, (0.0, 0.0), -0.375, 0.625, 1.0)[:2] == (-1, 3)
    assert both(0.25, (1.0, -2.0), 1.0, -2.0, 1.0)[:2] == (0, 0)
    assert both(0.25, (1.0, -2.0), 0.0, 0.0, 1.0)[:2] == (-4, 8)


@pytest.mark.parametrize("res,mult", [(0.05, 64), (0.05, 1), (0.25, 40), (0.1, 128), (0.05, 2048)])
def test_radius_at_and_around_a_whole_number_of_cells(res, mult):
    r = F32(res)
    exact = F32(r * F32(mult))
    assert float(exact) / float(r) == mult, "the case must be an exact multiple in float"
    below, above = np.nextafter(exact, F32(0)), np.nextafter(exact, F32(np.inf))
    assert both(res, (0.0, 0.0), 0.0, 0.0, float(exact))[2] == mult
    assert both(res, (0.0, 0.0), 0.0, 0.0, float(below))[2] == mult
    if mult < pref.MAX_RADIUS:
        assert both(res, (0.0, 0.0), 0.0, 0.0, float(above))[2] == mult + 1
    else:
        for f in (kh.worldmap_window, pref.window):
            with pytest.raises(IndexError):
                f(res, (0.0, 0.0), 0.0, 0.0, float(above))


def test_every_refusal_of_rule_16():
    ok = (0.05, (0.0, 0.0), 1.0, 2.0, 10.0)
    both(*ok)
    for f in (kh.worldmap_window, pref.window):
        for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError):
                f(0.05, (0.0, 0.0), 1.0, 2.0, bad)
        with pytest.raises(IndexError):
            f(0.05, (0.0, 0.0), 1.0, 2.0, 102.5)                         # 2050 cells
        f(0.05, (0.0, 0.0), 1.0, 2.0, 102.4)                             # 2048 cells at float32(0.05)
        far = 0.05 * (2 ** 20 + 2)
        for x, y in [(far, 0.0), (0.0, -far), (-far, far)]:
            with pytest.raises(IndexError):
                f(0.05, (0.0, 0.0), x, y, 10.0)
        f(0.05, (0.0, 0.0), 0.05 * (2 ** 20 - 2), -0.05 * (2 ** 20 - 2), 10.0)
        for x, y in [(float("nan"), 0.0), (0.0, float("inf"))]:
            with pytest.raises(ValueError):
                f(0.05, (0.0, 0.0), x, y, 10.0)
        with pytest.raises(ValueError):
            f(0.05, (float("nan"), 0.0), 0.0, 0.0, 10.0)
        for res in (0.0, -0.05, float("nan")):
            with pytest.raises(ValueError):
                f(res, (0.0, 0.0), 0.0, 0.0, 10.0)


def test_statement_on_a_map_written_out_by_hand():
    """7 x 5 cells of 0.5 m, cell (0, 0) centred on (1, -2), the robot in cell (3, 2), range 1 m: Rc = 2."""
    O, E, U = ref.OCCUPIED, ref.EMPTY, ref.UNEXPLORED
    rows = [  # rows[J][I], J = 0 first
        [O, O, O, O, O, O, O],
        [O, O, E, O, O, O, O],
        [O, O, O, E, U, O, O],
        [O, O, O, O, O, O, O],
        [O, O, O, O, O, O, O],
    ]
    cls = np.array(rows, np.int8).T
    assert cls.shape == (7, 5)
    res, origin = 0.5, (1.0, -2.0)
    assert both(res, origin, 2.5, -1.0, 1.0) == (3, 2, 2)
    xyz, n, bounds = pref.worldmap_points_ref(cls, res, origin, 2.5, -1.0, 1.0)
    cells = [(3, 0), (3, 1), (4, 1), (1, 2), (2, 2), (5, 2), (2, 3), (3, 3), (4, 3), (3, 4)]   # (I, J), by (J, I)
    want = np.array([[1.0 + 0.5 * i, -2.0 + 0.5 * j, 0.0] for i, j in cells], np.float32)
    assert n == 10 and bounds == (1, 5, 0, 4)
    assert xyz.dtype == np.float32 and xyz.tobytes() == want.tobytes()
    assert pref.sort_points(xyz[::-1], res, origin).tobytes() == want.tobytes()
    # Rc = 0 (a range below one cell is still one cell: ceil): the robot's own cell alone, empty here
    assert pref.window(res, origin, 2.5, -1.0, 0.4)[2] == 1
    # the robot outside the map: the disc is clipped, here to column I = 6
    xyz, n, bounds = pref.worldmap_points_ref(cls, res, origin, 1.0 + 0.5 * 8, -1.0, 1.0)
    assert n == 1 and bounds == (6, 6, 2, 2) and xyz.tolist() == [[4.0, -1.0, 0.0]]
    # far outside: nothing, which is no error
    assert pref.worldmap_points_ref(cls, res, origin, 50.0, 50.0, 1.0)[1:] == (0, (-1, -1, -1, -1))


def test_rule_18_rounds_product_and_sum_once_each():
    """An origin that no float holds and a resolution whose double differs from the literal: the point is the float of
    origin + I * (double)(float)resolution, not of anything evaluated in float."""
    res, origin = 0.05, (-0.33, 1.7)
    r = float(F32(res))
    I = np.arange(0, 2000, 37)
    pts = pref.cell_points(res, origin, I, I[::-1])
    for k, i in enumerate(I):
        assert pts[k, 0] == F32(origin[0] + float(i) * r)
        assert pts[k, 1] == F32(origin[1] + float(I[::-1][k]) * r)
    in_float = (F32(origin[0]) + I.astype(np.float32) * F32(res)).astype(np.float32)
    assert (in_float != pts[:, 0]).any(), "the case must tell double from float evaluation"
