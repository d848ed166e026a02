"""The grid planner's rules as a plain CPU statement: numpy for the maps, a heap Dijkstra for the
cost field, a loop for the walk.  Written from the five rules, not from the kernels: validity is the disc test
offset by offset, the field is Dijkstra (the kernels relax tiles), the walk looks at one neighbour after the other.

A grid is an array g[i, j] of (width, height) cells; i runs along x.  Cell values are the mapper's: 100 occupied,
-1 unexplored, anything else free."""
import heapq
import math

import numpy as np

INF = 0xFFFFFFFF
OCCUPIED, UNEXPLORED = 100, -1
STRAIGHT, DIAGONAL = 10, 14
# the order the walk breaks ties in: E, N, W, S, NE, NW, SW, SE
NEIGHBOURS = ((1, 0), (0, 1), (-1, 0), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1))
FOUND, START_OUTSIDE, GOAL_OUTSIDE, START_INVALID, GOAL_INVALID, UNREACHABLE = range(6)
CYLINDER, BOX, SPHERE = 0, 1, 2


# ---- rule 2: the footprint ------------------------------------------------------------------------------------
def footprint_radius(shape, dims):
    """The circumscribed horizontal radius: the cylinder's or sphere's radius, half the box's diagonal (the dims as
    the float32 the classes hold, the arithmetic in double)."""
    d = [float(np.float32(v)) for v in dims]
    if shape == BOX:
        return 0.5 * math.sqrt(d[0] * d[0] + d[1] * d[1])
    return d[0]


def radius_to_r2(radius, resolution):
    """R2 = floor((radius / resolution)^2 * (1 + 2^-20)), in double: the 2^-20 keeps a radius that is a whole number
    of cells up to float32 rounding (0.3f / 0.05f = 5.99999998) at that number."""
    r = float(radius) / float(np.float32(resolution))
    return int(math.floor(r * r * (1.0 + 2.0 ** -20)))


def _shift(a, di, dj, fill=False):
    """out[i, j] = a[i + di, j + dj], `fill` outside."""
    out = np.full_like(a, fill)
    w, h = a.shape
    i0, i1 = max(0, -di), min(w, w - di)
    j0, j1 = max(0, -dj), min(h, h - dj)
    if i0 < i1 and j0 < j1:
        out[i0:i1, j0:j1] = a[i0 + di:i1 + di, j0 + dj:j1 + dj]
    return out


def blocking(grid, allow_unknown=True):
    g = np.asarray(grid)
    b = g == OCCUPIED
    if not allow_unknown:
        b |= g == UNEXPLORED
    return b


def validity(grid, r2, allow_unknown=True):
    """valid[i, j]: no blocking cell (bi, bj) with (bi - i)^2 + (bj - j)^2 <= r2; outside the grid nothing blocks."""
    b = blocking(grid, allow_unknown)
    bad = np.zeros_like(b)
    r = math.isqrt(int(r2))
    for di in range(-r, r + 1):
        for dj in range(-r, r + 1):
            if di * di + dj * dj <= r2:
                bad |= _shift(b, di, dj)
    return ~bad


# ---- rule 3: the cost field -----------------------------------------------------------------------------------
def move_masks(valid):
    """bit q of mask[i, j]: a step from (i, j) to its neighbour NEIGHBOURS[q] is allowed (both cells valid, and for
    a diagonal both orthogonal neighbours between them)."""
    v = np.asarray(valid, bool)
    m = np.zeros(v.shape, np.uint8)
    for q, (di, dj) in enumerate(NEIGHBOURS):
        ok = v & _shift(v, di, dj)
        if di and dj:
            ok &= _shift(v, di, 0) & _shift(v, 0, dj)
        m |= ok.astype(np.uint8) << q
    return m


def cost_field(valid, goal):
    """Dijkstra from the goal cell over the allowed steps (they are symmetric): uint32 [width, height], INF where
    no walk arrives; all INF when the goal is outside the grid or invalid."""
    v = np.asarray(valid, bool)
    w, h = v.shape
    field = np.full((w, h), INF, np.uint32)
    gi, gj = int(goal[0]), int(goal[1])
    if not (0 <= gi < w and 0 <= gj < h) or not v[gi, gj]:
        return field
    masks = move_masks(v).reshape(-1).tolist()
    steps = [(di * h + dj, STRAIGHT if not (di and dj) else DIAGONAL) for di, dj in NEIGHBOURS]
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
                nd = d + cost
                if nd < dist[c + off]:
                    dist[c + off] = nd
                    push(heap, (nd, c + off))
    return np.array(dist, np.uint32).reshape(w, h)


def octile(width, height, goal):
    """The field of an empty grid in closed form."""
    di = np.abs(np.arange(width)[:, None] - goal[0])
    dj = np.abs(np.arange(height)[None, :] - goal[1])
    return (DIAGONAL * np.minimum(di, dj) + STRAIGHT * np.abs(di - dj)).astype(np.uint32)


# ---- rule 4: the path -----------------------------------------------------------------------------------------
def status(valid, field, start, goal):
    w, h = valid.shape
    inside = lambda c: 0 <= c[0] < w and 0 <= c[1] < h
    if not inside(start):
        return START_OUTSIDE
    if not inside(goal):
        return GOAL_OUTSIDE
    if not valid[start[0], start[1]]:
        return START_INVALID
    if not valid[goal[0], goal[1]]:
        return GOAL_INVALID
    return UNREACHABLE if field[start[0], start[1]] == INF else FOUND


def walk(valid, field, start):
    """Steepest descent from `start`: the allowed neighbour with the smallest field value, the first in NEIGHBOURS
    among equals, until the cell whose field is 0.  (n, 2) int32 cells."""
    w, h = valid.shape
    i, j = int(start[0]), int(start[1])
    cells = [(i, j)]
    while field[i, j] != 0:
        best, step = None, None
        for di, dj in NEIGHBOURS:
            ni, nj = i + di, j + dj
            if not (0 <= ni < w and 0 <= nj < h) or not valid[ni, nj]:
                continue
            if di and dj and not (valid[ni, j] and valid[i, nj]):
                continue
            f = int(field[ni, nj])
            if best is None or f < best:
                best, step = f, (ni, nj)
        assert best is not None and best < int(field[i, j]), "the walk found no descending neighbour"
        i, j = step
        cells.append(step)
    return np.array(cells, np.int32).reshape(-1, 2)


def simplify(cells):
    """Drop the interior cells of straight runs: a cell goes when the step into it equals the step out of it."""
    c = np.asarray(cells, np.int64).reshape(-1, 2)
    if len(c) < 3:
        return c.astype(np.int32)
    d = np.diff(c, axis=0)
    keep = np.ones(len(c), bool)
    keep[1:-1] = np.any(d[1:] != d[:-1], axis=1)
    return c[keep].astype(np.int32)


def check_path(valid, cells, start, goal):
    """Every cell valid, consecutive cells neighbours under the corner rule, the ends where they belong."""
    c = np.asarray(cells)
    assert tuple(c[0]) == tuple(start) and tuple(c[-1]) == tuple(goal)
    assert valid[c[:, 0], c[:, 1]].all()
    d = np.diff(c, axis=0)
    assert (np.abs(d).max(axis=1) == 1).all() if len(d) else True
    diag = np.nonzero((d[:, 0] != 0) & (d[:, 1] != 0))[0]
    for k in diag:
        assert valid[c[k + 1, 0], c[k, 1]] and valid[c[k, 0], c[k + 1, 1]], f"step {k} cuts a corner"


# ---- rule 5: world <-> cell, the mapper's pair anchored at the map's origin --------------------------------------
def world_to_cell(x, origin, resolution):
    """localToGrid (mapping/local_mapper.h:210-222) with the central point at the origin: (int)((x - origin) /
    resolution) in float32, truncated towards zero; None for what no int holds."""
    with np.errstate(all="ignore"):
        q = (np.float32(x) - np.float32(origin)) / np.float32(resolution)
    if not np.isfinite(q) or abs(float(q)) >= 2.0 ** 30:
        return None
    return int(q)


def cell_to_world(i, origin, resolution):
    """Its inverse as kc_dwa_set_grid_device uses it: origin + i * resolution, float32."""
    return np.float32(origin) + np.float32(i) * np.float32(resolution)


def cost_in_metres(field_value, resolution):
    return np.float32(field_value) * np.float32(resolution) / np.float32(10.0)


def plan(grid, origin, resolution, start_xy, goal_xy, radius, allow_unknown=True, do_simplify=False):
    """The whole statement: dict(status, valid, field, cells, points, cost)."""
    g = np.asarray(grid)
    w, h = g.shape
    r2 = radius_to_r2(radius, resolution)
    valid = validity(g, r2, allow_unknown)
    s = (world_to_cell(start_xy[0], origin[0], resolution), world_to_cell(start_xy[1], origin[1], resolution))
    t = (world_to_cell(goal_xy[0], origin[0], resolution), world_to_cell(goal_xy[1], origin[1], resolution))
    s = tuple(-1 if v is None else v for v in s)
    t = tuple(-1 if v is None else v for v in t)
    field = cost_field(valid, t)
    st = status(valid, field, s, t)
    out = dict(status=st, valid=valid, field=field, cells=None, points=None, cost=None, start=s, goal=t, r2=r2)
    if st == FOUND:
        cells = walk(valid, field, s)
        if do_simplify:
            cells = simplify(cells)
        out["cells"] = cells
        out["points"] = np.stack([cell_to_world(cells[:, 0], origin[0], resolution),
                                  cell_to_world(cells[:, 1], origin[1], resolution)], 1).astype(np.float32)
        out["cost"] = cost_in_metres(field[s], resolution)
    return out
