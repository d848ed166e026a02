"""The oriented box footprint of the grid planner (rules 13 to 18) as a plain CPU statement: numpy
for the maps, a heap Dijkstra over the states (k, i, j) for the field, a loop for the walk.  Written from the rules,
not from the kernels: validity is the mask test offset by offset, the field is Dijkstra (the kernels relax tiles of
four layers), the walk looks at one transition after the other.

Grids are g[i, j] of (width, height) cells as in planner_ref.py; maps by class are [4, width, height]."""
import heapq
import math

import numpy as np

import planner_ref as ref

INF = ref.INF
# rule 13: the length axis of class k; the two step directions of a class are this one (the first of the two in rule
# 4's order E, N, W, S, NE, NW, SW, SE) and its opposite
CLASS_DIR = ((1, 0), (1, 1), (0, 1), (-1, 1))
STEP_COST = (ref.STRAIGHT, ref.DIAGONAL, ref.STRAIGHT, ref.DIAGONAL)
DIRECTION_CLASS = (0, 2, 0, 2, 1, 3, 1, 3)   # of ref.NEIGHBOURS


def _lround(x):
    """C's lround: halves away from zero."""
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def orientation_class(yaw):
    return ((_lround(float(yaw) / (math.pi / 4.0)) % 4) + 4) % 4


def box_a2_b2(dims, margin, resolution):
    """A2, B2 of rule 14 from the box's float32 dimensions, rule 2's formula."""
    x, y = float(np.float32(dims[0])), float(np.float32(dims[1]))
    m = float(np.float32(margin))
    return ref.radius_to_r2(x / 2.0 + m, resolution), ref.radius_to_r2(y / 2.0 + m, resolution)


def oriented_mask(k, a2, b2):
    """Rule 14's offsets (di, dj) of class k, in integers."""
    r = math.isqrt(a2 + b2)   # T2 contains every mask (rule 15)
    out = []
    for di in range(-r, r + 1):
        for dj in range(-r, r + 1):
            s, d = (di + dj) ** 2, (dj - di) ** 2
            if k == 0:
                ok = di * di <= a2 and dj * dj <= b2
            elif k == 2:
                ok = dj * dj <= a2 and di * di <= b2
            elif k == 1:
                ok = s <= 2 * a2 and d <= 2 * b2
            elif k == 3:
                ok = d <= 2 * a2 and s <= 2 * b2
            else:
                raise ValueError(f"class {k} is outside 0 .. 3")
            if ok:
                out.append((di, dj))
    return out


def oriented_validity(grid, a2, b2, allow_unknown=True):
    """valid[k, i, j]: no blocking cell at (i, j) + o for any o of mask k; outside the grid nothing blocks."""
    b = ref.blocking(grid, allow_unknown)
    out = np.zeros((4,) + b.shape, bool)
    for k in range(4):
        bad = np.zeros_like(b)
        for di, dj in oriented_mask(k, a2, b2):
            bad |= ref._shift(b, di, dj)
        out[k] = ~bad
    return out


def turn_validity(grid, a2, b2, allow_unknown=True):
    """Rule 15: rule 2's disc test with r2 = T2 = A2 + B2."""
    return ref.validity(grid, a2 + b2, allow_unknown)


def transitions(valid, turn, i, j, k, turn10):
    """The allowed transitions out of the valid state (i, j, k) in rule 17's order: (cost, (ni, nj, nk))."""
    _, w, h = valid.shape
    out = []
    if not valid[k, i, j]:
        return out
    di, dj = CLASS_DIR[k]
    for sgn in (1, -1):
        ni, nj = i + sgn * di, j + sgn * dj
        if 0 <= ni < w and 0 <= nj < h and valid[k, ni, nj]:
            out.append((STEP_COST[k], (ni, nj, k)))
    if turn[i, j]:
        out.append((turn10, (i, j, (k + 1) % 4)))
        out.append((turn10, (i, j, (k + 3) % 4)))
    return out


def state_field(valid, turn, goal, turn10):
    """Rule 16 by Dijkstra from the goal's valid states (moves and turns are symmetric): uint32 [4, width, height]."""
    _, w, h = valid.shape
    n = w * h
    dist = [INF] * (4 * n)
    gi, gj = int(goal[0]), int(goal[1])
    if not (0 <= gi < w and 0 <= gj < h):
        return np.array(dist, np.uint32).reshape(4, w, h)
    v = valid.reshape(-1).tolist()
    t = turn.reshape(-1).tolist()
    heap = []
    for k in range(4):
        if valid[k, gi, gj]:
            dist[k * n + gi * h + gj] = 0
            heap.append((0, k * n + gi * h + gj))
    heapq.heapify(heap)
    step = [di * h + dj for di, dj in CLASS_DIR]
    while heap:
        d, s = heapq.heappop(heap)
        if d != dist[s]:
            continue
        k, c = divmod(s, n)
        i, j = divmod(c, h)
        di, dj = CLASS_DIR[k]
        for sgn in (1, -1):
            ni, nj = i + sgn * di, j + sgn * dj
            if 0 <= ni < w and 0 <= nj < h:
                q = s + sgn * step[k]
                if v[q] and d + STEP_COST[k] < dist[q]:
                    dist[q] = d + STEP_COST[k]
                    heapq.heappush(heap, (dist[q], q))
        if t[c]:
            for nk in ((k + 1) % 4, (k + 3) % 4):
                q = nk * n + c
                if d + turn10 < dist[q]:
                    dist[q] = d + turn10
                    heapq.heappush(heap, (dist[q], q))
    return np.array(dist, np.uint32).reshape(4, w, h)


def status(valid, field, start, k0, goal):
    _, w, h = valid.shape
    inside = lambda c: 0 <= c[0] < w and 0 <= c[1] < h
    if not inside(start):
        return ref.START_OUTSIDE
    if not inside(goal):
        return ref.GOAL_OUTSIDE
    if not valid[k0, start[0], start[1]]:
        return ref.START_INVALID
    if not valid[:, goal[0], goal[1]].any():
        return ref.GOAL_INVALID
    return ref.UNREACHABLE if field[k0, start[0], start[1]] == INF else ref.FOUND


def walk(valid, turn, field, start, k0, turn10):
    """Rule 17: (n, 3) int32 states (i, j, k) and the costs of the transitions taken."""
    i, j, k = int(start[0]), int(start[1]), int(k0)
    states, costs = [(i, j, k)], []
    while field[k, i, j] != 0:
        best, nxt, paid = None, None, None
        for cost, (ni, nj, nk) in transitions(valid, turn, i, j, k, turn10):
            f = int(field[nk, ni, nj])
            if f != INF and (best is None or f + cost < best):
                best, nxt, paid = f + cost, (ni, nj, nk), cost
        assert best is not None and best == int(field[k, i, j]), "the walk left the field"
        i, j, k = nxt
        states.append(nxt)
        costs.append(paid)
    return np.array(states, np.int32).reshape(-1, 3), costs


def collapse(states):
    """Rule 18: the walk's cells with the repeated cell of a turn dropped."""
    s = np.asarray(states).reshape(-1, 3)
    keep = np.ones(len(s), bool)
    keep[1:] = np.any(s[1:, :2] != s[:-1, :2], axis=1)
    return s[keep, :2].astype(np.int32)


def plan(grid, start, k0, goal, a2, b2, turn10, allow_unknown=True):
    """The whole statement in cells: dict(status, valid, turn, field, states, cells, cost)."""
    g = np.asarray(grid)
    valid = oriented_validity(g, a2, b2, allow_unknown)
    turn = turn_validity(g, a2, b2, allow_unknown)
    field = state_field(valid, turn, goal, turn10)
    st = status(valid, field, start, k0, goal)
    out = dict(status=st, valid=valid, turn=turn, field=field, states=None, cells=None, cost=INF, step_costs=None)
    if st == ref.FOUND:
        out["states"], out["step_costs"] = walk(valid, turn, field, start, k0, turn10)
        out["cells"] = collapse(out["states"])
        out["cost"] = int(field[k0, start[0], start[1]])
    return out


# ---- the issue's scenes -----------------------------------------------------------------------------------------
BIG_BOX, SMALL_BOX = (1.5, 0.2, 0.3), (0.3, 0.1, 0.2)
RES = 0.05


def corridor_scene():
    g = np.full((72, 70), ref.OCCUPIED, np.int32)
    g[:, 30:37] = 0
    return g, (2, 33), (69, 33)


def l_scene(bay=True):
    g = np.full((72, 70), ref.OCCUPIED, np.int32)
    g[0:51, 30:37] = 0
    g[44:51, 30:70] = 0
    if bay:
        g[30:65, 16:51] = 0
    return g, (2, 33), (47, 66)


def clutter_scene(unknown=False):
    """72 x 70, Bernoulli(0.01) drawn row by row (an image [j, i] of 70 rows and 72 columns), the two corners
    cleared; `unknown` sets some free cells to UNEXPLORED."""
    rng = np.random.default_rng(7)
    img = np.where(rng.random((70, 72)) < 0.01, ref.OCCUPIED, 0).astype(np.int32)
    img[0:8, 0:8] = 0
    img[60:70, 60:72] = 0
    if unknown:
        u = np.random.default_rng(8).random((70, 72)) < 0.01
        u[0:8, 0:8] = False
        u[60:70, 60:72] = False
        img[u & (img == 0)] = ref.UNEXPLORED
    return np.ascontiguousarray(img.T), (3, 3), (68, 66)
