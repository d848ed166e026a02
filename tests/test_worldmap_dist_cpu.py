"""The world map's distance plane without a device (DESIGN.md 4.11 rules 42 and 43): the statement
tests/worldmap_dist_ref.py on maps a reader can check by hand, against the planner's clear2 (the same definition, on
purpose), and its dirty-box bookkeeping against a full recompute."""
import numpy as np
import pytest

import kompass_hip as kh
import planner_clearance_ref as cref
import worldmap_dist_ref as dref
from worldmap_ref import EMPTY, OCCUPIED, UNEXPLORED

FAR = dref.FAR


def empty(w, h):
    return np.full((w, h), EMPTY, np.int8)


def test_constants_are_the_librarys():
    assert (kh.WORLDMAP_DIST_FAR, kh.WORLDMAP_DIST_UNKNOWN_BLOCKS, kh.WORLDMAP_DIST_MAX_REACH) == (FAR, dref.UNKNOWN_BLOCKS, dref.MAX_REACH)
    assert FAR == cref.CLEAR_FAR and dref.MAX_REACH ** 2 == cref.MAX_C2 < FAR


def test_one_occupied_cell():
    c = empty(9, 7)
    c[4, 3] = OCCUPIED
    d = dref.dist2_plane(c, 3)
    for i in range(9):
        for j in range(7):
            d2 = (i - 4) ** 2 + (j - 3) ** 2
            assert d[i, j] == (d2 if d2 <= 9 else FAR), (i, j)
    assert d[4, 3] == 0 and d[7, 3] == 9 and d[6, 5] == 8 and d[7, 4] == FAR        # 9 + 1 is beyond reach 3
    assert d.dtype == np.uint16


def test_a_wall_at_the_maps_edge():
    c = empty(8, 6)
    c[0, :] = OCCUPIED
    d = dref.dist2_plane(c, 4)
    for i in range(8):
        assert (d[i, :] == (i * i if i <= 4 else FAR)).all(), i
    c = empty(8, 6)
    c[:, 5] = OCCUPIED                                           # the far edge along J
    d = dref.dist2_plane(c, 2)
    assert (d[:, 5] == 0).all() and (d[:, 4] == 1).all() and (d[:, 3] == 4).all() and (d[:, :3] == FAR).all()


def test_reach_one_sees_the_four_neighbours_only():
    c = empty(5, 5)
    c[2, 2] = OCCUPIED
    d = dref.dist2_plane(c, 1)
    want = np.full((5, 5), FAR, np.uint16)
    want[2, 2] = 0
    want[1, 2] = want[3, 2] = want[2, 1] = want[2, 3] = 1           # the diagonal neighbours lie at 2 > 1
    assert (d == want).all()


def test_reach_larger_than_the_map():
    c = empty(6, 4)
    c[5, 3] = OCCUPIED
    d = dref.dist2_plane(c, 254)
    for i in range(6):
        for j in range(4):
            assert d[i, j] == (5 - i) ** 2 + (3 - j) ** 2
    assert (dref.dist2_plane(c, 7) == d).all() and dref.dist2_plane(c, 5)[0, 0] == FAR      # 25 + 9 > 25


def test_no_occupied_cell_is_far_everywhere():
    for c in (empty(7, 5), np.full((7, 5), UNEXPLORED, np.int8)):
        assert (dref.dist2_plane(c, 3) == FAR).all()
    assert (dref.dist2_plane(np.full((7, 5), UNEXPLORED, np.int8), 3, dref.UNKNOWN_BLOCKS) == 0).all()


def test_unknown_cells_block_with_the_flag_only():
    c = empty(9, 3)
    c[1, 1] = UNEXPLORED
    c[7, 1] = OCCUPIED
    plain, flagged = dref.dist2_plane(c, 2), dref.dist2_plane(c, 2, dref.UNKNOWN_BLOCKS)
    assert plain[1, 1] == FAR and plain[3, 1] == FAR and plain[5, 1] == 4 and plain[7, 1] == 0
    assert flagged[1, 1] == 0 and flagged[3, 1] == 4 and flagged[0, 0] == 2 and flagged[5, 1] == 4
    assert (flagged[4:, :] == plain[4:, :]).all()


def test_plane_form_equals_cell_form():
    rng = np.random.default_rng(5)
    c = rng.choice(np.array([EMPTY, EMPTY, EMPTY, EMPTY, UNEXPLORED, OCCUPIED], np.int8), (13, 11))
    for reach, flags in ((1, 0), (3, 1), (5, 0), (20, 1)):
        d = dref.dist2_plane(c, reach, flags)
        for i in range(13):
            for j in range(11):
                assert d[i, j] == dref.dist2_cell(c, i, j, reach, flags), (reach, flags, i, j)


def test_equals_the_planners_clear2():
    """The definition is clear2's on purpose: the same plane from the planner's statement, whose `allow_unknown` is the
    absence of KC_WORLDMAP_DIST_UNKNOWN_BLOCKS."""
    grid, _, _ = cref.doorway_scene()
    grid = grid.copy()
    grid[60:70, 5:9] = -1
    for reach in (1, 4, 9):
        for flags, allow_unknown in ((0, True), (dref.UNKNOWN_BLOCKS, False)):
            assert (dref.dist2_plane(grid.astype(np.int8), reach, flags) == cref.clearance2(grid, reach * reach, allow_unknown)).all()


def test_refusals_of_the_reach_and_flags():
    for reach, flags, exc in ((-1, 0, IndexError), (255, 0, IndexError), (255, 2, IndexError), (3, 2, ValueError), (0, 1, ValueError)):
        with pytest.raises(exc):
            dref.check(reach, flags)
    dref.check(0)
    dref.check(254, 1)
    with pytest.raises(IndexError):
        dref.dist2_plane(empty(3, 3), 0)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("reach,flags", [(1, 0), (4, 1), (9, 0)])
def test_partial_refresh_equals_full_recompute(seed, reach, flags):
    """Seeded sequences of box changes, some refreshed at once, some merged first, one that changes nothing."""
    rng = np.random.default_rng(100 + seed)
    W, H = 47, 33
    c = rng.choice(np.array([EMPTY] * 8 + [UNEXPLORED, OCCUPIED], np.int8), (W, H))
    m = dref.DistRef(c, reach, flags)
    assert m.refresh() == (0, 0, W - 1, H - 1) and m.last_full and (m.plane == dref.dist2_plane(c, reach, flags)).all()
    assert m.refresh() is None and m.last_box == (-1, -1, -1, -1)
    partial = 0
    for k in range(12):
        i0, j0 = int(rng.integers(0, W)), int(rng.integers(0, H))
        i1, j1 = min(W - 1, i0 + int(rng.integers(0, 7))), min(H - 1, j0 + int(rng.integers(0, 7)))
        if k == 5:
            m.mark(0, (-1, -1, -1, -1))                          # an update that changed nothing
        else:
            old = c[i0:i1 + 1, j0:j1 + 1].copy()
            c[i0:i1 + 1, j0:j1 + 1] = rng.choice(np.array([EMPTY, UNEXPLORED, OCCUPIED], np.int8), old.shape)
            diff = np.argwhere(c[i0:i1 + 1, j0:j1 + 1] != old)
            if len(diff):
                m.mark(len(diff), (i0 + diff[:, 0].min(), j0 + diff[:, 1].min(), i0 + diff[:, 0].max(), j0 + diff[:, 1].max()))
        if k % 3 != 1:                                           # every third change waits for the next: merged boxes
            box = m.refresh()
            partial += box is not None and not m.last_full
            assert (m.plane == dref.dist2_plane(c, reach, flags)).all(), (k, box)
    assert (m.field() == dref.dist2_plane(c, reach, flags)).all() and partial >= 3
    m.mark_all()
    assert m.refresh() == (0, 0, W - 1, H - 1)
