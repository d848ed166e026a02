"""Rule 19's claim and rule 20's start state as tests/planner_replan_ref.py states them, against the
fresh fields of planner_ref.py and planner_clearance_ref.py: every cell whose old value lies below the rollback
threshold keeps it in the new grid's field, and the relaxation from the rollback state ends in that field.  This is
what makes the device test meaningful: the device is compared with a fresh solve, and this file says a replan may be.
No GPU needed."""
import numpy as np
import pytest

import planner_clearance_ref as cref
import planner_ref as ref
import planner_replan_ref as rref

# the shapes and cost sets of test_planner_clearance_gpu.py (which a test without a device cannot import): one tile,
# tile edges both ways, one cell wide; (r2, c2, weight10, allow_unknown)
SHAPES = [(64, 64), (130, 97), (65, 300), (257, 63), (1, 90)]
COSTS = [(0, 9, 10, True), (1, 36, 25, False), (5, 5, 40, True), (4, 100, 3000, True)]
ROUNDS = ("anywhere", "beside the goal", "the start and a tile edge", "freed only")


def clutter(shape, density, seed):
    rng = np.random.default_rng(seed)
    grid = np.where(rng.random(shape) < density, 100, 0).astype(np.int32)
    grid[rng.random(shape) < 0.05] = -1
    return grid


def maps(grid, r2, unknown, cost=None):
    """(valid, pen): pen is None without a clearance cost, cost = (c2, table)."""
    valid = ref.validity(grid, r2, unknown)
    if cost is None:
        return valid, None
    return valid, cref.penalty(cref.clearance2(grid, cost[0], unknown), cost[1])


def field_of(valid, pen, goal):
    return ref.cost_field(valid, goal) if pen is None else cref.cost_field(valid, pen, goal)


def pick_pair(valid, pen, rng):
    """(start, goal, field): a random valid cell as the goal, the cell farthest from it as the start; None without a
    valid cell."""
    idx = np.argwhere(valid)
    if not len(idx):
        return None
    goal = tuple(int(v) for v in idx[rng.integers(len(idx))])
    f = field_of(valid, pen, goal)
    reach = np.where(f == ref.INF, 0, f)
    start = tuple(int(v) for v in np.unravel_index(np.argmax(reach), reach.shape))
    return start, goal, f


def flip(grid, rng, occupy, free):
    """`occupy` free cells become occupied and `free` occupied cells free, at random (fewer where there are fewer)."""
    g = grid.copy()
    for value, to, k in ((0, 100, occupy), (100, 0, free)):
        idx = np.argwhere(grid == value)
        if len(idx) and k:
            pick = idx[rng.choice(len(idx), size=min(k, len(idx)), replace=False)]
            g[pick[:, 0], pick[:, 1]] = to
    return g


def flipped(grid, kind, start, goal, rng):
    """The new grid of one round: 1 to 40 cells flipped each way, and the round's own cells."""
    w, h = grid.shape
    if kind == "anywhere":
        return flip(grid, rng, int(rng.integers(1, 41)), int(rng.integers(1, 41)))
    if kind == "freed only":
        return flip(grid, rng, 0, int(rng.integers(1, 41)))
    if kind == "beside the goal":
        g = flip(grid, rng, int(rng.integers(1, 6)), int(rng.integers(1, 6)))
        for di, dj in ref.NEIGHBOURS:
            i, j = goal[0] + di, goal[1] + dj
            if 0 <= i < w and 0 <= j < h and grid[i, j] != 100:
                g[i, j] = 100
                break
        return g
    g = flip(grid, rng, int(rng.integers(1, 41)), int(rng.integers(1, 41)))
    g[start] = 100
    for y in rng.integers(0, h, 3):           # one flip on each side of the tile edge at 63 / 64, where the grid has one
        if w > 64:
            g[63, y] = 100 - g[63, y] if g[63, y] in (0, 100) else 100
            g[64, h - 1 - y] = 100 - g[64, h - 1 - y] if g[64, h - 1 - y] in (0, 100) else 100
        elif h > 64:
            g[0, 63] = 100 - g[0, 63] if g[0, 63] in (0, 100) else 100
            g[w - 1, 64] = 100 - g[w - 1, 64] if g[w - 1, 64] in (0, 100) else 100
    return g


def check_claim(old, valid_old, pen_old, grid_new, goal, r2, unknown, cost):
    """Rule 19 and rule 20 on one pair of grids -> (T, touched cells)."""
    valid_new, pen_new = maps(grid_new, r2, unknown, cost)
    fresh = field_of(valid_new, pen_new, goal)
    t = rref.touched(valid_old, valid_new, pen_old, pen_new)
    T = rref.threshold(old, t)
    below = old < np.uint32(min(T, ref.INF)) if T != ref.INF else old != ref.INF
    np.testing.assert_array_equal(fresh[below], old[below])            # the claim: old < T keeps its value
    if T == ref.INF:
        np.testing.assert_array_equal(fresh, old)                      # rule 20: the field is kept as it is
    state = rref.rollback(old, valid_new, T, goal)
    assert (state >= fresh).all() and (state[~valid_new] == ref.INF).all()
    np.testing.assert_array_equal(rref.settle(state, valid_new, pen_new), fresh)
    # a tile that is not listed holds final values only
    on = rref.active_tiles(state, valid_new, goal)
    final = np.repeat(np.repeat(~on, 64, axis=0), 64, axis=1)[:old.shape[0], :old.shape[1]]
    np.testing.assert_array_equal(state[final], fresh[final])
    return T, int(t.sum())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("density", [0.03, 0.15])
@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("penalties", [False, True])
def test_values_below_the_threshold_are_final(shape, density, cost, penalties):
    r2, c2, wt, unknown = cost
    rng = np.random.default_rng(hash((shape, int(density * 100), r2, penalties)) % 2 ** 32)
    grid = clutter(shape, density, rng.integers(2 ** 31))
    table = (c2, cref.clearance_table(wt, r2, c2)) if penalties else None
    valid_old, pen_old = maps(grid, r2, unknown, table)
    pair = pick_pair(valid_old, pen_old, rng)
    if pair is None:                      # no valid cell, no goal, no kept field: nothing to state
        assert not valid_old.any()
        return
    start, goal, old = pair
    assert old[goal] == 0
    seen = [check_claim(old, valid_old, pen_old, flipped(grid, kind, start, goal, rng), goal, r2, unknown, table)
            for kind in ROUNDS]
    assert all(n > 0 or T == ref.INF for T, n in seen)


def test_by_hand():
    """A 7 x 5 corridor, goal at the left end: blocking (4, 2) touches one cell of value 40 whose smallest neighbour
    holds 30, so T = 40; freeing the wall cell (2, 1) gives T = 20, its diagonal neighbour's 10 plus the 10 of the bound."""
    g = np.full((7, 5), 100, np.int32)
    g[:, 2] = 0
    valid = ref.validity(g, 0)
    old = ref.cost_field(valid, (0, 2))
    np.testing.assert_array_equal(old[:, 2], 10 * np.arange(7))
    new = g.copy()
    new[4, 2] = 100
    t = rref.touched(valid, ref.validity(new, 0))
    assert t.sum() == 1 and t[4, 2] and rref.candidate(old, (4, 2)) == 40 and rref.threshold(old, t) == 40
    state = rref.rollback(old, ref.validity(new, 0), 40, (0, 2))
    np.testing.assert_array_equal(state[:, 2], [0, 10, 20, 30, ref.INF, ref.INF, ref.INF])
    np.testing.assert_array_equal(rref.settle(state, ref.validity(new, 0)), ref.cost_field(ref.validity(new, 0), (0, 2)))
    new = g.copy()
    new[2, 1] = 0
    t = rref.touched(valid, ref.validity(new, 0))
    assert t.sum() == 1 and rref.threshold(old, t) == 20          # old(2, 1) is INF, (1, 2) holds 10: no corner rule here
    # nothing touched: 100 -> 90 blocks neither before nor after, -1 -> 0 passes both ways with unknown cells allowed
    same = g.copy()
    same[0, 0] = 90
    assert rref.threshold(old, rref.touched(valid, ref.validity(same, 0))) == ref.INF
    # penalties: a cell valid in both maps whose penalty differs is touched
    pen_a, pen_b = np.zeros((7, 5), np.uint32), np.zeros((7, 5), np.uint32)
    pen_b[5, 2] = 3
    t = rref.touched(valid, valid, pen_a, pen_b)
    assert t.sum() == 1 and t[5, 2] and rref.threshold(old, t) == 50
    pen_b[5, 0] = 7                                                # an invalid cell's penalty does not count
    assert rref.touched(valid, valid, pen_a, pen_b).sum() == 1


def test_a_freed_orthogonal_neighbour_allows_a_diagonal():
    """The third case of the lower bound: (1, 1) -> (0, 0) is a diagonal the blocked (1, 0) forbids.  Freeing it lowers
    old(1, 1) = 20 to 14, and T = old(0, 0) + 10 = 10 lies below both."""
    g = np.zeros((3, 3), np.int32)
    g[1, 0] = 100
    valid = ref.validity(g, 0)
    old = ref.cost_field(valid, (0, 0))
    assert old[1, 1] == 20
    new = np.zeros((3, 3), np.int32)
    out = rref.replan(old, valid, ref.validity(new, 0), (0, 0))
    assert out["T"] == 10 and out["touched"].sum() == 1
    assert out["field"][1, 1] == 14
    np.testing.assert_array_equal(out["field"], ref.octile(3, 3, (0, 0)))
