"""The grid planner's car motion (rules 27 to 36) as a plain CPU statement: numpy for the maps, a
heap Dijkstra over the states (h, i, j) for the field, a loop for the walk.  Written from the rules, not from the
kernels: a unit step is tested cell by cell, an arc is the conjunction of its 2 n unit steps, the field is Dijkstra
(the kernels relax tiles of one heading layer each), the walk looks at one primitive after the other.

The graph is directed (a left arc has no inverse unless reverse is on, and then at another cost), so the Dijkstra
runs from the goal states over *predecessors*; forward_cost() is the independent check from the start.

Grids are g[i, j] of (width, height) cells as in planner_ref.py; maps by heading are [8, width, height]."""
import heapq
import math

import numpy as np

import planner_oriented_ref as oref
import planner_ref as ref

INF = ref.INF
# rule 27: heading h is the direction the robot's front points: E, NE, N, NW, W, SW, S, SE
D = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
S, L, R, B, BL, BR = range(6)          # rule 30's primitives, in the order they are tried and ranked
MOVE_NAMES = ("S", "L", "R", "B", "BL", "BR")
ARC = 24                               # cost of an arc per turn cell: n straight and n diagonal steps
MAX_TURN_CELLS = 8
MAX_REVERSE_WEIGHT = 16
TAN_PI_8 = 0.41421356237309503
ANY = -1                               # the goal heading "any"


def step(h):
    return ref.DIAGONAL if h & 1 else ref.STRAIGHT


def heading_class(yaw):
    """Rule 27: rule 13's formula with 8 in place of 4."""
    return ((oref._lround(float(yaw) / (math.pi / 4.0)) % 8) + 8) % 8


def turn_cells(radius, resolution):
    """Rule 31: n = max(1, ceil(R_min / resolution * tan(pi / 8))), the arguments as the float32 the class holds."""
    return max(1, int(math.ceil(float(np.float32(radius)) / float(np.float32(resolution)) * TAN_PI_8)))


def state_validity(grid, r2=0, box=None, allow_unknown=True):
    """Rule 28: valid[h, i, j].  box = (A2, B2) takes rule 14's masks by h & 3, otherwise rule 2's disc for every h."""
    if box is None:
        v = ref.validity(grid, r2, allow_unknown)
        return np.stack([v] * 8)
    v4 = oref.oriented_validity(grid, box[0], box[1], allow_unknown)
    return np.stack([v4[h & 3] for h in range(8)])


def unit_steps(valid, disc):
    """Rule 29: ok[s][h, i, j] for s = +1 / -1: the unit step from (i, j, h) along s * D[h] is allowed.  A cell
    outside the grid is never stepped on (the shifts fill with False)."""
    out = {}
    for s in (1, -1):
        ok = np.zeros_like(valid)
        for h in range(8):
            di, dj = s * D[h][0], s * D[h][1]
            a = valid[h] & ref._shift(valid[h], di, dj)
            if disc and (h & 1):       # rule 3's corner rule; the box's swept cells lie in one end's footprint
                a &= ref._shift(valid[h], di, 0) & ref._shift(valid[h], 0, dj)
            ok[h] = a
        out[s] = ok
    return out


def _legs(h, prim, n):
    """The two legs of an arc out of heading h: ((sign, heading of leg 1), (sign, heading of leg 2))."""
    if prim == L:
        return (1, h), (1, (h + 1) & 7)
    if prim == R:
        return (1, h), (1, (h + 7) & 7)
    if prim == BL:
        return (-1, h), (-1, (h + 7) & 7)
    return (-1, h), (-1, (h + 1) & 7)


def target(i, j, h, prim, n):
    """Where primitive `prim` out of (i, j, h) ends."""
    if prim == S:
        return i + D[h][0], j + D[h][1], h
    if prim == B:
        return i - D[h][0], j - D[h][1], h
    (s1, h1), (s2, h2) = _legs(h, prim, n)
    return i + n * (s1 * D[h1][0] + s2 * D[h2][0]), j + n * (s1 * D[h1][1] + s2 * D[h2][1]), h2


def cost_of(h, prim, n, rw):
    c = step(h) if prim in (S, B) else ARC * n
    return c * rw if prim >= B else c


def moves_map(valid, disc, n, rw):
    """Rule 30: uint8 [8, width, height], bit p set where primitive p is allowed out of the state."""
    ok = unit_steps(valid, disc)
    m = np.zeros(valid.shape, np.uint8)
    for h in range(8):
        m[h] |= ok[1][h].astype(np.uint8) << S
        if rw:
            m[h] |= ok[-1][h].astype(np.uint8) << B
        for prim in ((L, R, BL, BR) if rw else (L, R)):
            (s1, h1), (s2, h2) = _legs(h, prim, n)
            a = np.ones(valid.shape[1:], bool)
            for k in range(n):         # the step that leaves the cell k steps along leg 1
                a &= ref._shift(ok[s1][h1], k * s1 * D[h1][0], k * s1 * D[h1][1])
            ci, cj = n * s1 * D[h1][0], n * s1 * D[h1][1]
            for k in range(n):         # ... and along leg 2 from the corner cell, in the new heading
                a &= ref._shift(ok[s2][h2], ci + k * s2 * D[h2][0], cj + k * s2 * D[h2][1])
            m[h] |= a.astype(np.uint8) << prim
    return m


def goal_states(valid, goal, hg):
    _, w, hh = valid.shape
    gi, gj = int(goal[0]), int(goal[1])
    if not (0 <= gi < w and 0 <= gj < hh):
        return []
    return [(h, gi, gj) for h in (range(8) if hg == ANY else (hg,)) if valid[h, gi, gj]]


def state_field(valid, moves, goal, hg, n, rw):
    """Rule 32 by Dijkstra from the goal states over predecessors: uint32 [8, width, height]."""
    _, w, hh = valid.shape
    dist = np.full(valid.shape, INF, np.uint64)
    heap = []
    for st in goal_states(valid, goal, hg):
        dist[st] = 0
        heap.append((0, st))
    heapq.heapify(heap)
    mv = moves.tolist()
    d = dist.tolist()
    while heap:
        c, (h, i, j) = heapq.heappop(heap)
        if c != d[h][i][j]:
            continue
        # a predecessor is a state whose primitive `prim` ends here: its heading follows from the primitive
        for prim, hs in ((S, h), (L, (h + 7) & 7), (R, (h + 1) & 7), (B, h), (BL, (h + 1) & 7), (BR, (h + 7) & 7)):
            ti, tj, _ = target(0, 0, hs, prim, n)
            pi, pj = i - ti, j - tj
            if not (0 <= pi < w and 0 <= pj < hh) or not (mv[hs][pi][pj] >> prim & 1):
                continue
            nc = c + cost_of(hs, prim, n, rw)
            if nc < d[hs][pi][pj]:
                d[hs][pi][pj] = nc
                heapq.heappush(heap, (nc, (hs, pi, pj)))
    return np.array(d, np.uint64).astype(np.uint32)


def forward_cost(valid, moves, start, h0, goal, hg, n, rw):
    """The cheapest sequence of primitives from (start, h0) to a goal state, by Dijkstra from the start; INF if none."""
    goals = set(goal_states(valid, goal, hg))
    mv = moves.tolist()
    s0 = (int(h0), int(start[0]), int(start[1]))
    best = {s0: 0}
    heap = [(0, s0)]
    while heap:
        c, st = heapq.heappop(heap)
        if c != best[st]:
            continue
        if st in goals:
            return c
        h, i, j = st
        for prim in range(6):
            if mv[h][i][j] >> prim & 1:
                ti, tj, th = target(i, j, h, prim, n)
                nc = c + cost_of(h, prim, n, rw)
                if nc < best.get((th, ti, tj), INF):
                    best[(th, ti, tj)] = nc
                    heapq.heappush(heap, (nc, (th, ti, tj)))
    return INF


def status(valid, field, start, h0, goal, hg):
    _, w, hh = valid.shape
    inside = lambda c: 0 <= c[0] < w and 0 <= c[1] < hh
    if not inside(start):
        return ref.START_OUTSIDE
    if not inside(goal):
        return ref.GOAL_OUTSIDE
    if not valid[h0, start[0], start[1]]:
        return ref.START_INVALID
    if not goal_states(valid, goal, hg):
        return ref.GOAL_INVALID
    return ref.UNREACHABLE if field[h0, start[0], start[1]] == INF else ref.FOUND


def walk(moves, field, start, h0, n, rw):
    """Rule 33: (m, 3) int32 states (i, j, h), the (m - 1) primitive ids and the costs paid."""
    i, j, h = int(start[0]), int(start[1]), int(h0)
    states, prims, costs, seen = [(i, j, h)], [], [], {(i, j, h)}
    while field[h, i, j] != 0:
        best = None
        for prim in range(6):
            if moves[h, i, j] >> prim & 1:
                ti, tj, th = target(i, j, h, prim, n)
                f = int(field[th, ti, tj])
                c = cost_of(h, prim, n, rw)
                if f != INF and (best is None or f + c < best[0]):   # ties go to the first in rule 30's order
                    best = (f + c, prim, c, (ti, tj, th))
        assert best is not None and best[0] == int(field[h, i, j]), "the walk left the field"
        i, j, h = best[3]
        assert (i, j, h) not in seen, "a state came twice"
        seen.add((i, j, h))
        states.append((i, j, h))
        prims.append(best[1])
        costs.append(best[2])
    return np.array(states, np.int32).reshape(-1, 3), np.array(prims, np.int32), costs


def expand(states, prims, n):
    """Rule 34: every unit step of every primitive, first leg then second: (cells (k, 2) int32, the heading the robot
    holds at each of them (k,) int32; the corner cell of an arc is listed once, with the first leg's heading)."""
    s = np.asarray(states).reshape(-1, 3)
    i, j, h = (int(v) for v in s[0])
    cells, heads = [(i, j)], [h]
    for prim in (int(p) for p in prims):
        if prim in (S, B):
            legs = (((1 if prim == S else -1), h, 1),)
        else:
            (s1, h1), (s2, h2) = _legs(h, prim, n)
            legs = ((s1, h1, n), (s2, h2, n))
        for sg, hl, count in legs:
            for _ in range(count):
                i, j = i + sg * D[hl][0], j + sg * D[hl][1]
                cells.append((i, j))
                heads.append(hl)
            h = hl
    return np.array(cells, np.int32).reshape(-1, 2), np.array(heads, np.int32)


def check_range(n, rw, cells):
    """Rules 31 and 32: what the solve refuses."""
    return 1 <= n <= MAX_TURN_CELLS and 0 <= rw <= MAX_REVERSE_WEIGHT and ARC * n * max(rw, 1) * 8 * cells <= 0xFFFFFFFE


def plan(grid, start, h0, goal, hg, n, rw, r2=0, box=None, allow_unknown=True):
    """The whole statement in cells: dict(status, valid, moves, field, states, prims, cells, heads, cost, step_costs)."""
    g = np.asarray(grid)
    valid = state_validity(g, r2, box, allow_unknown)
    moves = moves_map(valid, box is None, n, rw)
    field = state_field(valid, moves, goal, hg, n, rw)
    st = status(valid, field, start, h0, goal, hg)
    out = dict(status=st, valid=valid, moves=moves, field=field, states=None, prims=None, cells=None, heads=None, cost=INF,
               step_costs=None)
    if st == ref.FOUND:
        out["states"], out["prims"], out["step_costs"] = walk(moves, field, start, h0, n, rw)
        out["cells"], out["heads"] = expand(out["states"], out["prims"], n)
        out["cost"] = int(field[h0, start[0], start[1]])
    return out


# ---- the issue's scenes -----------------------------------------------------------------------------------------
def dead_end_scene():
    """40 x 21, a corridor closed at both ends: free cells i 2 .. 37, j 8 .. 12."""
    g = np.full((40, 21), ref.OCCUPIED, np.int32)
    g[2:38, 8:13] = 0
    return g, (20, 10), (5, 10)


def free_scene():
    return np.zeros((40, 30), np.int32), (20, 10), (5, 10)
