"""Scan integration without a GPU (DESIGN.md 4.11 rules 52 to 56): known answers of the statement
tests/worldmap_integrate_ref.py, the argument that rule 23's box never cuts a crossing, the host-only entries
kc_worldmap_quantise_ranges and kc_worldmap_integrate_check, and the statement's consistency with the virtual scan."""
import math

import numpy as np
import pytest

import kompass_hip as kh
import worldmap_integrate_ref as iref
import worldmap_ref as ref
import worldmap_scan_ref as sref

MISS, HIT = iref.MISS, iref.HIT
CELL = 65536


def centre_pose(i, j, yaw=0.0):
    """The quantised pose at the centre of cell (i, j): rule 20's fractions are fx = fy = 2^15."""
    return round(math.cos(yaw) * 65536.0), round(math.sin(yaw) * 65536.0), i * CELL, j * CELL


def marks_of(W, H, pose, angles, zq, Rc, flags=0):
    return iref.mark_plane(W, H, pose, sref.scan_table(angles), zq, Rc, Rc * CELL, flags)


def cells_with(marks):
    return {(int(i), int(j)): int(marks[i, j]) for i, j in np.argwhere(marks != 0)}


def test_axis_beam_from_a_cell_centre():
    """From a centre the cells along +x are entered at q = 1/2, 3/2, 5/2, 7/2 cells.  Rule 53 crosses a step with q_s <= z,
    so a range of 3.5 cells less one unit of q ends in the third cell ahead: three MISS (the start cell and two more) and
    one HIT.  At 3.5 cells exactly the fourth cell is entered at the range itself and takes the HIT: four MISS and one
    HIT.  Both are pinned, the boundary being the point of the case."""
    pose = centre_pose(5, 4)
    below = cells_with(marks_of(16, 9, pose, [0.0], [7 * CELL // 2 - 1], 8))
    assert below == {(5, 4): MISS, (6, 4): MISS, (7, 4): MISS, (8, 4): HIT}
    at = cells_with(marks_of(16, 9, pose, [0.0], [7 * CELL // 2], 8))
    assert at == {(5, 4): MISS, (6, 4): MISS, (7, 4): MISS, (8, 4): MISS, (9, 4): HIT}
    # the other three directions, by the yaw and by the beam angle
    assert cells_with(marks_of(16, 9, centre_pose(5, 4, math.pi), [0.0], [3 * CELL // 2 - 1], 8)) == {(5, 4): MISS, (4, 4): HIT}
    assert cells_with(marks_of(16, 9, pose, [math.pi / 2], [3 * CELL // 2], 8)) == {(5, 4): MISS, (5, 5): MISS, (5, 6): HIT}
    assert cells_with(marks_of(16, 9, pose, [-math.pi / 2], [CELL], 8)) == {(5, 4): MISS, (5, 3): HIT}


def test_zero_range_marks_the_start_cell():
    pose = centre_pose(3, 2)
    for a in (0.0, 1.0, -2.5):
        assert cells_with(marks_of(8, 8, pose, [a], [0], 4)) == {(3, 2): HIT}
    # and the limits of rule 54: -1 says nothing, ZMAX nothing without the flag and MISS along the whole range with it
    assert cells_with(marks_of(8, 8, pose, [0.0], [-1], 4, iref.CLEAR_NO_RETURN)) == {}
    assert cells_with(marks_of(8, 8, pose, [0.0], [4 * CELL], 4)) == {}
    assert cells_with(marks_of(8, 8, pose, [0.0], [4 * CELL], 4, iref.CLEAR_NO_RETURN)) == {(i, 2): MISS for i in range(3, 8)}


def test_exact_diagonal_visits_the_x_side_neighbour_first():
    pose = centre_pose(2, 2)
    t = sref.scan_table([math.pi / 4])
    assert t[0][0] == t[0][1]                                  # the exact diagonal: every step ties
    cells = iref.walk(pose, t[0], 3)
    assert [(i, j) for i, j, _ in cells[:5]] == [(2, 2), (3, 2), (3, 3), (4, 3), (4, 4)]
    assert cells[1][2] == cells[2][2]                          # the y step follows at the same distance
    half_diag = cells[1][2]                                    # sqrt(1/2) cell
    got = cells_with(marks_of(8, 8, pose, [math.pi / 4], [half_diag], 3))
    assert got == {(2, 2): MISS, (3, 2): MISS, (3, 3): HIT}
    assert cells_with(marks_of(8, 8, pose, [math.pi / 4], [half_diag - 1], 3)) == {(2, 2): HIT}


def test_a_hit_beats_a_miss_in_the_observation():
    m = iref.IntegrateRef(8, 8, 0.25)
    pose = centre_pose(1, 1)
    marks, changed, box = m.integrate(pose, [0.0, 0.0], [2 * CELL, 4 * CELL], 2.0)
    assert marks[3, 1] == MISS | HIT and marks[5, 1] == HIT and marks[4, 1] == MISS
    assert m.cls[3, 1] == ref.OCCUPIED and m.cls[5, 1] == ref.OCCUPIED and m.cls[4, 1] == ref.EMPTY
    assert m.evidence[3, 1] == 3 and m.evidence[2, 1] == -1      # rule 5 once a cell, however many beams
    assert (changed, box) == (5, (1, 1, 5, 1))


@pytest.mark.parametrize("Rc", [1, 64, 2048])
def test_the_box_never_cuts_a_crossing(Rc):
    """crossed() asserts that q never decreases and that the step leaving rule 23's box has q > ZMAX.  ZMAX is the largest
    Rc allows (Rc cells); the starts include fx = 0 looking along -x, where the first step is entered at q = 0, and yaws at
    which |dx| exceeds 2^30."""
    zmax = Rc * CELL
    angles = [0.0, math.pi / 2, math.pi, -math.pi / 2, math.pi / 4, 3 * math.pi / 4, 1e-9, math.pi - 1e-9, 0.3, 2.0, -1.1, 3.0]
    table = sref.scan_table(angles)
    longest = 0
    for yaw in (0.0, math.pi / 4, -math.pi / 4, 1.234):
        cq, sq = round(math.cos(yaw) * 65536.0), round(math.sin(yaw) * 65536.0)
        for tx, ty in ((0, 0), (CELL // 2, CELL // 2), (CELL // 2 - 1, 7 * CELL + CELL // 2), (-3 * CELL + 12345, 54321)):
            for t in table:
                cells = iref.crossed((cq, sq, tx, ty), t, Rc, zmax, zmax)
                longest = max(longest, len(cells))
                I0, J0 = (tx + CELL // 2) >> 16, (ty + CELL // 2) >> 16
                assert all(abs(i - I0) <= Rc + 1 and abs(j - J0) <= Rc + 1 for i, j in cells)
    assert Rc + 1 <= longest <= 2 * (Rc + 2) + 2                 # the kernel's loop bound


def test_a_walk_can_be_entered_in_front_of_any_step_of_its_dominant_axis():
    """What lets the mark kernel share a beam among lanes: the walk merges the x steps at EX_m = ex + m
    2^16 with the y steps at EY_n, x step m before y step n iff EX_m |dy| <= EY_n |dx|.  In front of x step m0 exactly n0 =
    ceil(T / (2^16 |dx|)) y steps are made, T = EX_m0 |dy| - ey |dx| (0 for T <= 0); in front of y step n0 exactly m0 =
    floor(T / (2^16 |dy|)) + 1 x steps, T = EY_n0 |dx| - ex |dy| (0 for T < 0 or dx == 0).  Checked against the statement's
    walk for every step of seeded beams, ties and boundary starts included."""
    rng = np.random.default_rng(8)
    angles = np.concatenate([np.arange(8) * math.pi / 4, rng.uniform(-math.pi, math.pi, 24)])
    table = sref.scan_table(angles)
    Rc = 40
    for yaw, (tx, ty) in ((0.0, (0, 0)), (0.0, (CELL // 2, CELL // 2)), (math.pi / 4, (CELL // 2 - 1, 123)), (2.2, (-777, 31000))):
        cq, sq = round(math.cos(yaw) * 65536.0), round(math.sin(yaw) * 65536.0)
        X0, Y0 = tx + CELL // 2, ty + CELL // 2
        I0, J0, fx, fy = X0 >> 16, Y0 >> 16, X0 & 0xFFFF, Y0 & 0xFFFF
        for t in table:
            ac, as_ = int(t[0]), int(t[1])
            dx = (cq * ac - sq * as_ + (1 << 15)) >> 16
            dy = (sq * ac + cq * as_ + (1 << 15)) >> 16
            adx, ady = abs(dx), abs(dy)
            ex = CELL - fx if dx > 0 else fx
            ey = CELL - fy if dy > 0 else fy
            steps = iref.walk((cq, sq, tx, ty), t, Rc)                    # the cells; a step changes I or J by one
            made = [(abs(i - I0), abs(j - J0)) for i, j, _ in steps]     # (x steps, y steps) made on arrival
            for (m, n), (m1, n1) in zip(made, made[1:]):
                if m1 == m + 1:                                          # the step ahead is x step m: n y steps are made
                    T = (ex + m * CELL) * ady - ey * adx
                    assert n == (-(-T // (CELL * adx)) if T > 0 else 0), (yaw, t, m, n)
                else:                                                    # y step n: m x steps are made
                    T = (ey + n * CELL) * adx - ex * ady
                    assert m == (T // (CELL * ady) + 1 if dx != 0 and T >= 0 else 0), (yaw, t, m, n)


def test_quantiser_hand_values():
    res, rmax = 0.25, 10.0                                       # ZMAX = 40 cells
    zmax = 40 * CELL
    r = [float("nan"), -0.0, 0.0, -1e-300, -math.inf, 0.3, 0.5, 1.0, 10.0, math.nextafter(10.0, 0.0), 11.0, math.inf, 1e-7]
    want = [-1, 0, 0, -1, -1, -1, 2 * CELL, 4 * CELL, zmax, zmax, zmax, zmax, 0]
    got = kh.worldmap_quantise_ranges(r, res, rmax, range_min=0.0)
    want0 = list(want)
    want0[5] = round(0.3 / 0.25 * 65536.0)
    assert got.dtype == np.int32 and got.tolist() == want0
    want_min = list(want)
    want_min[1] = want_min[2] = want_min[12] = -1                # below range_min = 0.5, -0.0 included
    assert kh.worldmap_quantise_ranges(r, res, rmax, range_min=0.5).tolist() == want_min
    assert iref.quantise_ranges(r, res, rmax).tolist() == want0 and iref.quantise_ranges(r, res, rmax, 0.5).tolist() == want_min
    assert kh.worldmap_integrate_check(res, len(r), rmax) == (40, zmax) == iref.integrate_check(res, len(r), rmax)


def test_quantiser_against_the_statement_on_seeded_ranges():
    rng = np.random.default_rng(5)
    r = np.concatenate([rng.uniform(-1.0, 12.0, 500), [np.nan, np.inf, -np.inf, 0.0, 7.3]])
    for res, rmax, rmin in ((0.05, 10.0, 0.0), (0.05, 7.3, 0.12), (0.1, 3.3, 0.0), (0.013, 9.99, 1.0)):
        assert kh.worldmap_quantise_ranges(r, res, rmax, rmin).tolist() == iref.quantise_ranges(r, res, rmax, rmin).tolist()
        assert kh.worldmap_integrate_check(res, len(r), rmax) == iref.integrate_check(res, len(r), rmax)
    for bad in (dict(range_min=-0.1), dict(range_min=float("nan")), dict(range_max=0.0), dict(range_max=float("inf"))):
        with pytest.raises(ValueError):
            kh.worldmap_quantise_ranges([1.0], 0.05, **{"range_max": 5.0, **bad})
    with pytest.raises(IndexError):
        kh.worldmap_quantise_ranges([1.0], 0.05, 103.0)          # Rc = 2060
    with pytest.raises(ValueError):
        kh.worldmap_quantise_ranges([], 0.05, 5.0)


def test_refusal_order_of_the_check():
    """counts, range_max, flags, zq: every call is wrong in its own place and in every later one"""
    nan, ok = float("nan"), 5.0
    zmax = kh.worldmap_integrate_check(0.05, 3, ok)[1]
    bad_zq = [0, zmax + 1, -2]
    with pytest.raises(ValueError, match="at least one"):
        kh.worldmap_integrate_check(0.05, 0, nan, 6, bad_zq)
    with pytest.raises(IndexError, match="beams"):
        kh.worldmap_integrate_check(0.05, 65537, nan, 6)
    with pytest.raises(ValueError, match="range_max"):
        kh.worldmap_integrate_check(0.05, 3, nan, 6, bad_zq)
    with pytest.raises(IndexError, match="2048"):
        kh.worldmap_integrate_check(0.05, 3, 103.0, 6, bad_zq)
    with pytest.raises(ValueError, match="flag"):
        kh.worldmap_integrate_check(0.05, 3, ok, 6, bad_zq)
    with pytest.raises(ValueError, match="flag"):
        kh.worldmap_integrate_check(0.05, 3, ok, 2, [0, 0, 0])
    with pytest.raises(ValueError, match="quantised range 1 "):
        kh.worldmap_integrate_check(0.05, 3, ok, 1, bad_zq)
    with pytest.raises(ValueError, match="quantised range 2 "):
        kh.worldmap_integrate_check(0.05, 3, ok, 0, [0, zmax, -2])
    assert kh.worldmap_integrate_check(0.05, 3, ok, 1, [-1, 0, zmax]) == (100, zmax)
    assert kh.worldmap_integrate_check(0.05, 65536, ok, 0) == (100, zmax)
    for args in ((0.05, 0, ok), (0.05, 65537, ok), (0.05, 3, nan), (0.05, 3, 103.0), (0.05, 3, ok, 2), (0.05, 3, ok, 0, bad_zq)):
        with pytest.raises((ValueError, IndexError)) as lib_err:
            kh.worldmap_integrate_check(*args)
        with pytest.raises(type(lib_err.value)):
            iref.integrate_check(*args)


def seeded_room(W=120, H=90, seed=3):
    rng = np.random.default_rng(seed)
    cls = np.full((W, H), ref.EMPTY, np.int8)
    cls[0, :] = cls[-1, :] = cls[:, 0] = cls[:, -1] = ref.OCCUPIED
    for _ in range(14):
        i, j = int(rng.integers(8, W - 12)), int(rng.integers(8, H - 12))
        cls[i:i + int(rng.integers(1, 5)), j:j + int(rng.integers(1, 5))] = ref.OCCUPIED
    return cls


def test_consistency_with_the_virtual_scan():
    """Scan the prior, quantise the ranges, integrate them into an empty map.  A range r of rule 24 quantises to q_s or q_s
    + 1 (it is e 2^30 / a within two roundings), so wherever the walk stays 2 units of q inside the hit cell (q_{s+1} >=
    q_s + 2) the HIT lies on exactly that cell.  No cell that is empty in the prior becomes occupied."""
    res, origin, rmax = 0.05, (-1.0, 0.5), 4.0
    prior = seeded_room()
    W, H = prior.shape
    angles = -math.pi + np.arange(90) * (2 * math.pi / 90) + 0.0071
    table = sref.scan_table(angles)
    m = iref.IntegrateRef(W, H, res, origin)
    r = float(np.float32(res))
    checked = 0
    for k, (ci, cj, yaw) in enumerate([(60.3, 45.2, 0.3), (20.0, 70.5, -1.9), (100.71, 12.13, 2.4), (33.5, 33.5, 0.0)]):
        if prior[int(round(ci)), int(round(cj))] != ref.EMPTY:
            continue
        q = ref.quantise_pose(res, origin, origin[0] + ci * r, origin[1] + cj * r, yaw)
        ranges, cells = sref.scan_pose(prior, res, q, table, rmax)
        zq = iref.quantise_ranges(ranges, res, rmax)
        Rc, zmax = iref.integrate_check(res, len(angles), rmax)
        for b in range(len(angles)):
            if cells[b] < 0:
                assert zq[b] == zmax
                continue
            hit = (int(cells[b]) % W, int(cells[b]) // W)
            steps = iref.walk(q, table[b], Rc)
            s = [(i, j) for i, j, _ in steps].index(hit)
            if s > 0 and steps[s + 1][2] >= steps[s][2] + 2:
                one = iref.mark_plane(W, H, q, table[b:b + 1], zq[b:b + 1], Rc, zmax)
                assert [tuple(c) for c in np.argwhere(one & HIT)] == [hit], (k, b)
                checked += 1
        m.integrate(q, angles, zq, rmax, iref.CLEAR_NO_RETURN)
    assert checked > 200
    assert not np.any((m.cls == ref.OCCUPIED) & (prior == ref.EMPTY))
    assert np.any(m.cls == ref.OCCUPIED) and np.any(m.cls == ref.EMPTY)
