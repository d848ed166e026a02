"""The any-angle rules of the grid planner (rules 9 to 12) as tests/planner_shortcut_ref.py states
them, against hand values: the touched cells of a segment, the selection on an empty grid, on the doorway scene with
and without the clearance cost and on seeded clutter, and the presence of every layer.  No GPU needed."""
import math

import numpy as np
import pytest

import planner_clearance_ref as cref
import planner_ref as ref
import planner_shortcut_ref as sref


@pytest.mark.parametrize("a, b, count", [((0, 0), (2, 1), 4), ((0, 0), (2, 2), 7), ((0, 0), (3, 1), 6), ((5, 5), (2, 7), 6),
                                         ((0, 0), (0, 4), 5), ((2, 3), (37, 20), 54)])
def test_touched_cells_by_hand(a, b, count):
    t = sref.touched(a, b)
    assert len(t) == count
    cells = set(map(tuple, t.tolist()))
    assert len(cells) == count and a in cells and b in cells
    assert cells == set(map(tuple, sref.touched(b, a).tolist()))          # symmetric in a and b
    # at most three touched cells in a column of the major axis
    major = 0 if abs(b[0] - a[0]) >= abs(b[1] - a[1]) else 1
    assert np.bincount(t[:, major] - t[:, major].min()).max() <= 3


def test_touched_cells_of_short_segments():
    assert set(map(tuple, sref.touched((0, 0), (2, 1)).tolist())) == {(0, 0), (1, 0), (1, 1), (2, 1)}
    assert sref.touched((4, 4), (4, 4)).tolist() == [[4, 4]]
    assert set(map(tuple, sref.touched((7, 2), (8, 2)).tolist())) == {(7, 2), (8, 2)}
    # a single diagonal step touches its two orthogonal neighbours: rule 3's corner rule
    for di, dj in ((1, 1), (-1, 1), (-1, -1), (1, -1)):
        got = set(map(tuple, sref.touched((3, 3), (3 + di, 3 + dj)).tolist()))
        assert got == {(3, 3), (3 + di, 3 + dj), (3 + di, 3), (3, 3 + dj)}
    # symmetry over every direction of a window
    for dx in range(-9, 10):
        for dy in range(-9, 10):
            a, b = (20, 30), (20 + dx, 30 + dy)
            assert set(map(tuple, sref.touched(a, b).tolist())) == set(map(tuple, sref.touched(b, a).tolist()))


def _kept_segments_clear(valid, cells, keep, clear2=None):
    m = None if clear2 is None else sref.walk_min_clear2(cells, clear2)
    for s, t in zip(keep[:-1], keep[1:]):
        assert t > s
        assert t == s + 1 or sref.segment_clear(valid, cells[s], cells[t], clear2, m), (s, t)


def test_empty_grid():
    valid = ref.validity(np.zeros((40, 30), np.int32), 0)
    cells = ref.walk(valid, ref.cost_field(valid, (37, 20)), (2, 3))
    assert len(cells) == 36
    assert sref.select(valid, cells, 64) == [0, 35]
    assert sref.select(valid, cells, 8) == [0, 8, 16, 24, 32, 35]
    assert sref.select(valid, cells, 1) == list(range(36))
    assert sref.select(valid, cells[:1], 64) == [0]                       # n = 1 returns its one cell
    assert sref.select(valid, cells[:2], 64) == [0, 1]
    r = sref.shortcut(valid, cells, 64)
    assert r["count"] == 2 and r["min_clear2"] == sref.CLEAR_FAR and r["cells"].tolist() == [[2, 3], [37, 20]]
    assert r["length"] == math.sqrt(35 * 35 + 17 * 17)
    assert sref.length_metres(r["cells"], 0.05) == np.float32(float(np.float32(0.05)) * math.sqrt(35 * 35 + 17 * 17))
    for span in (0, sref.MAX_SPAN + 1):
        with pytest.raises(AssertionError):
            sref.select(valid, cells, span)


def test_doorway_scene_plain():
    grid, start, goal = cref.doorway_scene()
    valid = ref.validity(grid, 4)
    cells = ref.walk(valid, ref.cost_field(valid, goal), start)
    assert len(cells) == 94 and round(sref.length_cells(cells), 3) == 114.539
    r16, r128 = sref.shortcut(valid, cells, 16), sref.shortcut(valid, cells, 128)
    assert (r16["count"], r128["count"]) == (10, 5)
    assert round(r128["length"], 3) == 108.393
    assert r128["indices"][0] == 0 and r128["indices"][-1] == 93
    for r in (r16, r128):
        _kept_segments_clear(valid, cells, r["indices"].tolist())
        np.testing.assert_array_equal(r["cells"], cells[r["indices"]])


def test_doorway_scene_with_the_clearance_cost():
    grid, start, goal = cref.doorway_scene()
    p = cref.plan(grid, start, goal, 4, 100, 40)
    valid, clear2, cells = p["valid"], p["clear2"], p["cells"]
    assert len(cells) == 122 and round(sref.length_cells(cells), 3) == 142.539 and p["min_clear2"] == 81
    r16, r128 = sref.shortcut(valid, cells, 16, clear2), sref.shortcut(valid, cells, 128, clear2)
    assert (r16["count"], r128["count"]) == (11, 9)
    assert round(r128["length"], 3) == 138.251
    assert r16["min_clear2"] == 81 and r128["min_clear2"] == 81          # rule 10: the distance is not given back
    for r in (r16, r128):
        _kept_segments_clear(valid, cells, r["indices"].tolist(), clear2)
    # on validity alone the shortcut comes as close as squared distance 5
    plain = sref.select(valid, cells, 128)
    assert sref.min_touched_clear2(cells, plain, clear2) == 5


def _clutter_walk(shape, density, seed):
    rng = np.random.default_rng(seed)
    grid = np.where(rng.random(shape) < density, 100, 0).astype(np.int32)
    valid = ref.validity(grid, 0)
    free = np.argwhere(valid)
    goal = tuple(int(v) for v in free[rng.integers(len(free))])
    field = ref.cost_field(valid, goal)
    reach = np.where(field == ref.INF, 0, field)
    start = tuple(int(v) for v in np.unravel_index(np.argmax(reach), reach.shape))
    return grid, valid, ref.walk(valid, field, start)


def test_largest_clear_index_is_not_the_first_failure():
    """A blocked line of sight to p[t] says nothing about p[t + 1]: on clutter the two scans keep different cells."""
    grid, valid, cells = _clutter_walk((130, 97), 0.15, 1)
    assert len(cells) > 60
    a = sref.select(valid, cells, 64)
    b = sref.select_first_failure(valid, cells, 64)
    assert a != b and len(a) < len(b)
    _kept_segments_clear(valid, cells, a)
    _kept_segments_clear(valid, cells, b)
    # the rule's own property: no later index of the window is clear
    for s, t in zip(a[:-1], a[1:]):
        for u in range(t + 1, min(len(cells) - 1, s + 64) + 1):
            assert not sref.segment_clear(valid, cells[s], cells[u])


@pytest.mark.parametrize("span", [1, 2, 17, 64, 1024])
def test_every_kept_segment_is_clear(span):
    for shape, density, seed in [((64, 64), 0.02, 3), ((130, 97), 0.15, 4), ((65, 300), 0.35, 5)]:
        grid, valid, cells = _clutter_walk(shape, density, seed)
        clear2 = cref.clearance2(grid, 36)
        for c2 in (None, clear2):
            keep = sref.select(valid, cells, span, c2)
            assert keep[0] == 0 and keep[-1] == len(cells) - 1 and all(0 < t - s <= span for s, t in zip(keep[:-1], keep[1:]))
            _kept_segments_clear(valid, cells, keep, c2)
            if c2 is not None:
                assert sref.min_touched_clear2(cells, keep, c2) >= sref.walk_min_clear2(cells, c2)
        if span == 1:
            assert keep == list(range(len(cells)))
        assert sref.length_cells(cells[keep]) <= sref.length_cells(cells) + 1e-9   # the triangle inequality


def test_shortcut_is_present_in_every_layer():
    import inspect
    from pathlib import Path

    import kompass_cpp
    import kompass_hip as kh
    from kompass_core.planning import GridPlanner

    header = (Path(__file__).resolve().parent.parent / "include" / "kompass_hip.h").read_text()
    L = kh.lib()
    for name in ("kc_planner_shortcut", "kc_planner_get_shortcut"):
        assert name + "(" in header and hasattr(L, name) and name in kh.SIGNATURES, name
    assert "#define KC_PLANNER_MAX_SPAN 1024" in header and kh.PLAN_MAX_SPAN == sref.MAX_SPAN == 1024
    assert hasattr(kh.PlannerContext, "shortcut")
    assert inspect.signature(kh.PlannerContext.shortcut).parameters["max_span"].default == 128
    cls = kompass_cpp.planning.GridPlanner
    for name in ("get_any_angle_solution", "get_any_angle_cells", "get_any_angle_length"):
        assert hasattr(cls, name), name
    par = inspect.signature(GridPlanner.__init__).parameters
    assert par["any_angle"].default is False and par["max_span"].default == 128   # off by default
    assert isinstance(GridPlanner.any_angle_length, property)
