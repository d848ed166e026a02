"""The grid planner's clearance rules (rules 6 to 8) as a plain CPU statement beside planner_ref.py,
which supplies blocking, validity, the allowed steps and the status.  Written from the rules, not from the kernels:
the clearance field is the disc test offset by offset (the kernels take two passes over rows and columns), the
penalised field is a heap Dijkstra (the kernels relax tiles), the walk looks at one neighbour after the other.

Arrays are [width, height] as in planner_ref."""
import heapq
import math

import numpy as np

import planner_ref as ref

CLEAR_FAR = 0xFFFF
MAX_C2 = 254 * 254
INF = ref.INF


# ---- rule 6: the clearance field ------------------------------------------------------------------------------
def clearance2(grid, c2, allow_unknown=True):
    """clear2[i, j]: the smallest (bi - i)^2 + (bj - j)^2 over blocking cells when that is <= c2, CLEAR_FAR
    otherwise; cells outside the grid do not block.  uint16."""
    assert 0 <= c2 <= MAX_C2
    b = ref.blocking(grid, allow_unknown)
    out = np.full(b.shape, CLEAR_FAR, np.uint16)
    r = math.isqrt(int(c2))
    for di in range(-r, r + 1):
        for dj in range(-r, r + 1):
            d2 = di * di + dj * dj
            if d2 <= c2:
                hit = ref._shift(b, di, dj) & (out > d2)
                out[hit] = d2
    return out


# ---- rule 7: the penalty and the penalised field ----------------------------------------------------------------
def clearance_table(weight10, r2, c2):
    """pen_by_d2[0 .. c2]: 0 up to the footprint (d2 <= r2), then weight10 at its edge falling linearly in d2 to 0 at
    c2, in integers (the division truncates); all zero when the reach does not pass the footprint."""
    t = np.zeros(int(c2) + 1, np.uint32)
    if c2 > r2:
        for d2 in range(int(r2) + 1, int(c2) + 1):
            t[d2] = int(weight10) * (int(c2) - d2) // (int(c2) - int(r2))
    return t


def penalty(clear2, table):
    """pen[cell] = table[clear2[cell]], 0 for CLEAR_FAR cells.  uint32."""
    c = np.asarray(clear2)
    t = np.asarray(table, np.uint32)
    far = c == CLEAR_FAR
    assert (c[~far] < len(t)).all()
    return np.where(far, np.uint32(0), t[np.where(far, 0, c)]).astype(np.uint32)


def cost_field(valid, pen, goal):
    """field[goal] = 0, field[a] = pen[a] + min over allowed steps a -> b of (step + field[b]): a step pays for the
    cell it leaves.  Heap Dijkstra from the goal, relaxing d[c] + step + pen[a] into the neighbour a (the allowed
    steps are symmetric).  uint32 [width, height], INF where no walk arrives."""
    v = np.asarray(valid, bool)
    w, h = v.shape
    gi, gj = int(goal[0]), int(goal[1])
    if not (0 <= gi < w and 0 <= gj < h) or not v[gi, gj]:
        return np.full((w, h), INF, np.uint32)
    masks = ref.move_masks(v).reshape(-1).tolist()
    p = np.asarray(pen, np.uint32).reshape(-1).tolist()
    steps = [(di * h + dj, ref.STRAIGHT if not (di and dj) else ref.DIAGONAL) for di, dj in ref.NEIGHBOURS]
    dist = [INF] * (w * h)
    g = gi * h + gj
    dist[g] = 0
    heap = [(0, g)]
    pop, push = heapq.heappop, heapq.heappush
    while heap:
        d, c = pop(heap)
        if d != dist[c]:
            continue
        m = masks[c]
        for q in range(8):
            if m >> q & 1:
                off, cost = steps[q]
                a = c + off
                nd = d + cost + p[a]
                if nd < dist[a]:
                    dist[a] = nd
                    push(heap, (nd, a))
    assert max(d for d in dist if d != INF) < INF
    return np.array(dist, np.uint32).reshape(w, h)


# ---- rule 8: the walk -------------------------------------------------------------------------------------------
def walk(valid, field, pen, start):
    """From `start`, the allowed neighbour b with the smallest field[b] + step, the first in NEIGHBOURS among equals,
    until the cell whose field is 0; that minimum is field[c] - pen[c] at every cell.  (n, 2) int32 cells."""
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
        assert best is not None and best == int(field[i, j]) - int(pen[i, j]), "the walk left the field's own steps"
        i, j = step
        cells.append(step)
    return np.array(cells, np.int32).reshape(-1, 2)


def path_length(cells):
    """The steps alone, 10 straight and 14 diagonal."""
    d = np.abs(np.diff(np.asarray(cells, np.int64).reshape(-1, 2), axis=0))
    assert len(d) == 0 or d.max() <= 1
    return int(np.where(d.sum(axis=1) == 2, ref.DIAGONAL, ref.STRAIGHT).sum()) if len(d) else 0


def path_cost(cells, pen):
    """The steps plus the penalty of every cell left (all but the last)."""
    c = np.asarray(cells, np.int64).reshape(-1, 2)
    return path_length(c) + int(np.asarray(pen, np.uint64)[c[:-1, 0], c[:-1, 1]].sum())


def path_clearance(cells, clear2):
    """The smallest clear2 along the path, both ends included."""
    c = np.asarray(cells, np.int64).reshape(-1, 2)
    return int(np.asarray(clear2)[c[:, 0], c[:, 1]].min())


def plan(grid, start, goal, r2, c2, weight10, allow_unknown=True, table=None):
    """The whole statement in cells: dict(status, valid, clear2, pen, field, cells, cost, length, min_clear2)."""
    g = np.asarray(grid)
    valid = ref.validity(g, r2, allow_unknown)
    clear2 = clearance2(g, c2, allow_unknown)
    pen = penalty(clear2, clearance_table(weight10, r2, c2) if table is None else table)
    field = cost_field(valid, pen, goal)
    st = ref.status(valid, field, start, goal)
    out = dict(status=st, valid=valid, clear2=clear2, pen=pen, field=field, cells=None, cost=None, length=None,
               min_clear2=None)
    if st == ref.FOUND:
        cells = walk(valid, field, pen, start)
        out.update(cells=cells, cost=int(field[start[0], start[1]]), length=path_length(cells),
                   min_clear2=path_clearance(cells, clear2))
    return out


def doorway_scene():
    """A 96 x 80 room cut in two by a wall with a 20-cell doorway, a block in front of it: (grid, start, goal)."""
    grid = np.zeros((96, 80), np.int32)
    grid[48, :30] = grid[48, 50:] = 100
    grid[20:30, 20:60] = 100
    return grid, (5, 40), (90, 70)
