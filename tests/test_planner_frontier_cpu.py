"""The exploration rules (rules 21 to 26) as tests/planner_frontier_ref.py states them, on grids worked
by hand; the argument checks of the paths that need no device; and the new entries in the built library.  No GPU
needed."""
import ctypes

import numpy as np
import pytest

import planner_frontier_ref as fref
import planner_ref as ref

INF = ref.INF
U, O = ref.UNEXPLORED, ref.OCCUPIED


def ragged(shape, density, seed, blobs=3):
    """A seeded grid with ragged frontiers: occupied clutter at `density`, unknown speckle, and blobs of unknown."""
    rng = np.random.default_rng(seed)
    w, h = shape
    grid = np.where(rng.random(shape) < density, O, 0).astype(np.int32)
    grid[rng.random(shape) < 0.04] = U
    ii, jj = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
    for _ in range(blobs):
        ci, cj, r = rng.integers(0, w), rng.integers(0, h), rng.integers(1, max(2, min(max(w, h) // 3, 24)))
        grid[(ii - ci) ** 2 + (jj - cj) ** 2 <= r * r * (0.6 + 0.8 * rng.random(shape))] = U
    return grid


def serpentine(w, h):
    """Even rows free, odd rows unknown except one free link cell at alternating ends: one long frontier."""
    g = np.zeros((w, h), np.int32)
    g[:, 1::2] = U
    for j in range(1, h, 2):
        g[w - 1 if (j // 2) % 2 == 0 else 0, j] = 0
    return g


def test_by_hand_one_wall_of_unknown():
    """5 x 3, the column i = 4 unknown, the robot at (0, 1): the frontier is the column i = 3, three cells, label
    3 + 0 * 5; the entry is (3, 1) at cost 30; the centroid sums are 9 and 3."""
    g = np.zeros((5, 3), np.int32)
    g[4, :] = U
    out = fref.explore(g, (0, 1))
    assert out["status"] == ref.FOUND and out["components"] == 1
    want = np.full((5, 3), INF, np.uint32)
    want[3, :] = 3
    np.testing.assert_array_equal(out["labels"], want)
    assert out["frontiers"] == [dict(size=3, sum_i=9, sum_j=3, entry=(3, 1), cost=30, root=3)]
    np.testing.assert_array_equal(out["paths"][0], [[0, 1], [1, 1], [2, 1], [3, 1]])
    assert not out["valid"][4].any() and out["valid"][:4].all()                # rule 21: unknown cells are not valid
    assert (out["field"][4] == INF).all()
    # min_cost = 30 keeps (3, 1); 31 drops it and leaves the corner cells at 34
    assert fref.explore(g, (0, 1), min_cost=30)["frontiers"][0]["entry"] == (3, 1)
    cut = fref.explore(g, (0, 1), min_cost=31)
    # (3, 0) and (3, 2) are not 8-connected once (3, 1) is dropped: two components of one cell each
    assert cut["components"] == 2 and [r["root"] for r in cut["frontiers"]] == [3, 13]
    assert [r["entry"] for r in cut["frontiers"]] == [(3, 0), (3, 2)] and all(r["cost"] == 34 for r in cut["frontiers"])
    assert fref.explore(g, (0, 1), min_cost=31, min_size=2)["status"] == fref.NO_FRONTIER


def test_by_hand_inflation_and_unknown():
    """Rule 21 against rule 2: with r2 = 1 an occupied cell takes its four neighbours, an unknown cell takes none, so the
    cells beside the unknown stay frontier cells whatever a solve's allow_unknown would say."""
    g = np.zeros((7, 5), np.int32)
    g[6, :] = U
    g[3, 2] = O
    valid = fref.explore_validity(g, 1)
    assert not valid[3, 2] and not valid[2, 2] and not valid[4, 2] and not valid[3, 1] and not valid[3, 3]
    assert valid[5, :].all() and not valid[6, :].any()
    assert not ref.validity(g, 1, allow_unknown=False)[5, :].any()             # the solve's map would lose them
    out = fref.explore(g, (0, 0), r2=1)
    assert out["components"] == 1 and out["frontiers"][0]["size"] == 5 and out["frontiers"][0]["root"] == 5
    # the entry: (5, 0) along the bottom row at 50; nothing crosses the unknown column
    assert out["frontiers"][0]["entry"] == (5, 0) and out["frontiers"][0]["cost"] == 50
    assert fref.path_cost(out["paths"][0]) == 50


def test_by_hand_diagonal_join_and_orthogonal_rule():
    """Two frontier cells that touch only by a corner are one frontier (rule 24); a cell whose only unknown neighbour is
    diagonal is no frontier cell (rule 23)."""
    g = np.zeros((4, 4), np.int32)
    g[1, 0] = U       # makes (0, 0) and (2, 0) and (1, 1) frontier cells
    out = fref.explore(g, (3, 3))
    front = out["labels"] != INF
    assert sorted(map(tuple, np.argwhere(front))) == [(0, 0), (1, 1), (2, 0)]
    assert not front[0, 1] and not front[2, 1]                                 # diagonal to the unknown cell only
    assert out["components"] == 1 and (out["labels"][front] == 0).all()
    rec = out["frontiers"][0]
    assert rec["size"] == 3 and rec["sum_i"] == 3 and rec["sum_j"] == 1 and rec["entry"] == (1, 1) and rec["cost"] == 28


def tie_grids():
    """(grid, robot) twice: two frontiers symmetric about the robot; one frontier with two cheapest cells."""
    two = np.zeros((9, 5), np.int32)
    two[0, :] = U
    two[8, :] = U
    one = np.zeros((5, 3), np.int32)
    one[0, :] = U
    one[2, 1] = O          # in front of the robot: (1, 1) costs 40, (1, 0) and (1, 2) cost 30 round either side
    return (two, (4, 2)), (one, (3, 1))


def test_by_hand_tie_goes_to_the_smaller_flat_index():
    """Two frontiers symmetric about the robot at equal cost: the order goes by the entry's flat index; within a
    frontier two cheapest cells tie to the smaller index."""
    (two, robot2), (one, robot1) = tie_grids()
    a, b = fref.explore(two, robot2)["frontiers"]
    assert a["cost"] == b["cost"] == 30 and a["entry"] == (1, 2) and b["entry"] == (7, 2) and (a["root"], b["root"]) == (1, 7)
    out = fref.explore(one, robot1)
    assert out["field"][1, 0] == out["field"][1, 2] == 30 and out["field"][1, 1] == 40
    assert out["frontiers"] == [dict(size=3, sum_i=3, sum_j=3, entry=(1, 0), cost=30, root=1)]


def test_statuses():
    g = np.zeros((6, 6), np.int32)
    g[5, :] = U
    g[0, 0] = O
    assert fref.explore(g, (5, 2))["status"] == ref.START_INVALID              # on an unknown cell
    assert fref.explore(g, (0, 0))["status"] == ref.START_INVALID              # on an occupied cell
    assert fref.explore(g, (1, 0), r2=1)["status"] == ref.START_INVALID        # inside the inflation
    for cell in [(-1, 0), (6, 0), (0, 6), (3, -1)]:
        out = fref.explore(g, cell)
        assert out["status"] == ref.START_OUTSIDE and out["components"] == 0 and out["frontiers"] == []
        assert (out["field"] == INF).all() and (out["labels"] == INF).all()
    assert fref.explore(np.zeros((6, 6), np.int32), (2, 2))["status"] == fref.NO_FRONTIER
    assert fref.explore(np.zeros((6, 6), np.int32), (2, 2))["components"] == 0
    with pytest.raises(ValueError):
        fref.explore(g, (2, 2), min_size=0)


def test_serpentine_is_one_component():
    g = serpentine(64, 64)
    out = fref.explore(g, (0, 0), paths=False)
    assert out["components"] == 1 and out["frontiers"][0]["root"] == 0
    assert out["frontiers"][0]["size"] > 2000
    assert out["frontiers"][0]["entry"] == (0, 0) and out["frontiers"][0]["cost"] == 0


@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (5, 3), (37, 29), (65, 65)])
@pytest.mark.parametrize("seed", [1, 2])
def test_labels_are_the_component_minimum_on_ragged_grids(shape, seed):
    """The flood fill against the rule's own words: every frontier cell's label is a frontier cell of its component, no
    smaller index is 8-connected to it, neighbours share a label, and the records add up."""
    g = ragged(shape, 0.1, seed)
    free = np.argwhere(fref.explore_validity(g, 0))
    robot = tuple(int(v) for v in free[len(free) // 2]) if len(free) else (0, 0)
    out = fref.explore(g, robot)
    lab, w = out["labels"], shape[0]
    front = lab != INF
    for i, j in np.argwhere(front):
        assert lab[i, j] <= i + j * w and front[lab[i, j] % w, lab[i, j] // w] and lab[lab[i, j] % w, lab[i, j] // w] == lab[i, j]
        for di, dj in ref.NEIGHBOURS:
            ni, nj = i + di, j + dj
            if 0 <= ni < shape[0] and 0 <= nj < shape[1] and front[ni, nj]:
                assert lab[ni, nj] == lab[i, j]
    assert out["components"] == len(np.unique(lab[front]))
    assert sum(r["size"] for r in out["frontiers"]) == int(front.sum())
    keys = [(r["cost"], r["entry"][0] + r["entry"][1] * w) for r in out["frontiers"]]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    for r, path in zip(out["frontiers"], out["paths"]):
        assert tuple(path[0]) == robot and tuple(path[-1]) == r["entry"] and fref.path_cost(path) == r["cost"]
        ref.check_path(out["valid"], path, robot, r["entry"])


# ---- the built library and the paths that need no device --------------------------------------------------------
def test_the_library_has_the_entries():
    import kompass_hip as kh
    lib = kh.lib()
    for name in ("kc_planner_explore", "kc_planner_get_frontiers", "kc_planner_get_frontier_path", "kc_planner_get_frontier_labels",
                 "kc_planner_explore_info"):
        assert hasattr(lib, name), name
    assert kh.PLAN_NO_FRONTIER == fref.NO_FRONTIER == 6
    assert kh.PLAN_FRONTIER_DTYPE.itemsize == 40
    # a null context is refused before anything else
    cell = (ctypes.c_int32 * 2)(0, 0)
    st = ctypes.c_int(-1)
    assert lib.kc_planner_explore(None, cell, 0, 0, 1, ctypes.byref(st), None, None, None, None) != 0
    n = ctypes.c_size_t(0)
    assert lib.kc_planner_get_frontiers(None, None, 0, ctypes.byref(n)) != 0
    assert lib.kc_planner_get_frontier_path(None, 0, None, 0, ctypes.byref(n)) != 0
    assert lib.kc_planner_get_frontier_labels(None, None, 0) != 0
    assert lib.kc_planner_explore_info(None, None, None, None) != 0


def test_min_distance_to_cost_needs_no_device():
    import kompass_cpp
    conv = kompass_cpp.planning.GridPlanner.min_distance_to_cost
    assert conv(0.0, 0.05) == 0 and conv(1.0, 0.05) == 200 and conv(0.152, 0.05) == 30 and conv(0.147, 0.05) == 29
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            conv(bad, 0.05)
    with pytest.raises(IndexError):
        conv(1e9, 0.05)
    for name in ("explore", "get_frontiers", "get_frontier_solution", "get_frontier_path_cells", "get_frontier_labels", "get_components"):
        assert hasattr(kompass_cpp.planning.GridPlanner, name), name


def test_front_end_has_the_surface():
    from kompass_core import planning
    for name in ("find_frontiers", "explore", "frontier_path", "components"):
        assert hasattr(planning.GridPlanner, name), name
    assert planning.Frontier._fields == ("entry", "entry_cell", "centroid", "cost", "size", "root")
