"""The grid planner's exploration rules (rules 21 to 26) as a plain CPU statement over planner_ref.py:
numpy for the maps, its heap Dijkstra for the field, a flood fill in ascending flat index for the components, its
neighbour order for the paths.  Written from the rules, not from the kernels: the kernels iterate labels to a fixed point and
add into records with atomics, this visits every component once and sums with numpy.

A grid is g[i, j] of (width, height) cells as in planner_ref.py; the flat index of a cell is i + j * width."""
import numpy as np

import planner_ref as ref

INF = ref.INF
NO_FRONTIER = 6
ORTHOGONAL = ref.NEIGHBOURS[:4]


# ---- rule 21 ----------------------------------------------------------------------------------------------------
def explore_validity(grid, r2):
    """Only occupied cells inflate; an unknown cell is not explore-valid itself."""
    g = np.asarray(grid)
    return ref.validity(g, r2, allow_unknown=True) & (g != ref.UNEXPLORED)


# ---- rule 23 ----------------------------------------------------------------------------------------------------
def frontier_cells(grid, valid, field, min_cost=0):
    g = np.asarray(grid)
    unknown = g == ref.UNEXPLORED
    beside = np.zeros(g.shape, bool)
    for di, dj in ORTHOGONAL:
        beside |= ref._shift(unknown, di, dj)  # cells outside the grid are not unknown
    f = np.asarray(field).astype(np.int64)
    return np.asarray(valid, bool) & (f >= int(min_cost)) & (f < INF) & beside


# ---- rule 24 ----------------------------------------------------------------------------------------------------
def label(front):
    """uint32 [width, height]: the smallest flat index of each frontier cell's 8-connected component, INF elsewhere."""
    fr = np.asarray(front, bool)
    w, h = fr.shape
    lab = np.full((w, h), INF, np.uint32)
    jj, ii = np.nonzero(fr.T)  # ascending flat index: j is the slow one
    for i0, j0 in zip(ii.tolist(), jj.tolist()):
        if lab[i0, j0] != INF:
            continue
        root = i0 + j0 * w  # the first unlabelled cell in flat order is its component's smallest
        lab[i0, j0] = root
        stack = [(i0, j0)]
        while stack:
            i, j = stack.pop()
            for di, dj in ref.NEIGHBOURS:
                ni, nj = i + di, j + dj
                if 0 <= ni < w and 0 <= nj < h and fr[ni, nj] and lab[ni, nj] == INF:
                    lab[ni, nj] = root
                    stack.append((ni, nj))
    return lab


# ---- rule 25 ----------------------------------------------------------------------------------------------------
def records(labels, field, min_size=1):
    """(components, the kept frontiers' records sorted by (cost, entry flat index)); a record is a dict of size, sum_i,
    sum_j, entry (i, j), cost, root."""
    lab = np.asarray(labels)
    w, h = lab.shape
    ii, jj = np.nonzero(lab != INF)
    roots = lab[ii, jj].astype(np.int64)
    out = []
    uniq = np.unique(roots)
    for root in uniq.tolist():
        m = roots == root
        ci, cj = ii[m].astype(np.int64), jj[m].astype(np.int64)
        if len(ci) < min_size:
            continue
        key = (field[ci, cj].astype(np.int64) << 32) | (ci + cj * w)
        k = int(np.argmin(key))
        out.append(dict(size=int(len(ci)), sum_i=int(ci.sum()), sum_j=int(cj.sum()), entry=(int(ci[k]), int(cj[k])),
                        cost=int(field[ci[k], cj[k]]), root=int(root)))
    out.sort(key=lambda r: (r["cost"], r["entry"][0] + r["entry"][1] * w))
    return len(uniq), out


# ---- rule 26 ----------------------------------------------------------------------------------------------------
def walk_down(valid, field, start):
    """From `start` to the cell whose field is 0: at each cell the allowed neighbour with the smallest field + step,
    the first in rule 4's order among equals; that minimum is the cell's own field.  (n, 2) int32 cells."""
    w, h = valid.shape
    i, j = int(start[0]), int(start[1])
    cells = [(i, j)]
    while field[i, j] != 0:
        best, step = None, None
        for di, dj in ref.NEIGHBOURS:
            ni, nj = i + di, j + dj
            if not (0 <= ni < w and 0 <= nj < h) or not valid[ni, nj]:
                continue
            if di and dj and not (valid[ni, j] and valid[i, nj]):
                continue
            f = int(field[ni, nj]) + (ref.DIAGONAL if di and dj else ref.STRAIGHT)
            if best is None or f < best:
                best, step = f, (ni, nj)
        assert best == int(field[i, j]), "the walk is off the field"
        i, j = step
        cells.append(step)
    return np.array(cells, np.int32).reshape(-1, 2)


def frontier_path(valid, field, entry):
    """The walk from the entry cell down to the robot's cell, reversed: robot first."""
    return walk_down(valid, field, entry)[::-1].copy()


def path_cost(cells):
    d = np.abs(np.diff(np.asarray(cells, np.int64), axis=0))
    return int(np.where(d.sum(axis=1) == 2, ref.DIAGONAL, ref.STRAIGHT).sum()) if len(d) else 0


def explore(grid, robot, r2=0, min_cost=0, min_size=1, paths=True):
    """The whole statement: dict(status, valid, field, labels, components, frontiers, paths)."""
    if min_size < 1:
        raise ValueError("min_size must be at least 1")
    g = np.asarray(grid)
    w, h = g.shape
    valid = explore_validity(g, r2)
    ri, rj = int(robot[0]), int(robot[1])
    inside = 0 <= ri < w and 0 <= rj < h
    field = ref.cost_field(valid, (ri, rj))  # all INF for a robot outside the grid or on a cell that is not valid
    labels = label(frontier_cells(g, valid, field, min_cost))
    components, kept = records(labels, field, min_size)
    if not inside:
        status = ref.START_OUTSIDE
    elif not valid[ri, rj]:
        status = ref.START_INVALID
    else:
        status = ref.FOUND if kept else NO_FRONTIER
    out = dict(status=status, valid=valid, field=field, labels=labels, components=components, frontiers=kept, paths=None)
    if paths:
        out["paths"] = [frontier_path(valid, field, r["entry"]) for r in kept]
    return out
