"""The grid planner's replan rules (rules 19 and 20) as a plain CPU statement beside planner_ref.py and
planner_clearance_ref.py, which supply validity, the penalty, the allowed steps and the fresh fields and are not
changed.  Written from the rules, not from the kernels: the touched cells are an array comparison, the threshold
looks at one neighbour after the other, and where the kernels relax the tiles of a list, `settle` is a heap Dijkstra
that starts from every finite value of the rollback state at once.

Arrays are [width, height] as in planner_ref.  The kept field is one whose goal was a valid cell (old[goal] == 0):
rule 19's proof starts there, and the planner keeps no other."""
import heapq

import numpy as np

import planner_ref as ref

INF = ref.INF


# ---- rule 19: the rollback threshold ----------------------------------------------------------------------------
def touched(valid_old, valid_new, pen_old=None, pen_new=None):
    """bool [width, height]: the validity differs, or (with penalties) the cell is valid in both maps and its
    penalty differs."""
    vo, vn = np.asarray(valid_old, bool), np.asarray(valid_new, bool)
    t = vo != vn
    if pen_old is not None:
        t |= vo & vn & (np.asarray(pen_old) != np.asarray(pen_new))
    return t


def candidate(old_field, cell):
    """min(old(c), min over the 8 neighbours u inside the grid of old(u) + 10), INF terms left out: validity and the
    corner rule are ignored on purpose, it is a lower bound."""
    w, h = old_field.shape
    i, j = cell
    best = int(old_field[i, j])
    for di, dj in ref.NEIGHBOURS:
        ni, nj = i + di, j + dj
        if 0 <= ni < w and 0 <= nj < h and old_field[ni, nj] != INF:
            best = min(best, int(old_field[ni, nj]) + ref.STRAIGHT)
    return best


def threshold(old_field, touched_cells):
    """T = min over touched cells of candidate(c); INF when no cell is touched (or no candidate is finite)."""
    f = np.asarray(old_field)
    return min((candidate(f, (int(i), int(j))) for i, j in np.argwhere(touched_cells)), default=INF)


# ---- rule 20: the replan ------------------------------------------------------------------------------------------
def rollback(old_field, valid_new, T, goal):
    """The start state of the relaxation: old(c) where the cell is valid in the new map and old(c) < T, INF elsewhere,
    0 at the goal where it is valid."""
    f, v = np.asarray(old_field, np.uint32), np.asarray(valid_new, bool)
    out = np.where(v & (f < np.uint32(min(T, INF))), f, np.uint32(INF)).astype(np.uint32)
    w, h = f.shape
    if 0 <= goal[0] < w and 0 <= goal[1] < h and v[goal[0], goal[1]]:
        out[goal[0], goal[1]] = 0
    return out


def active_tiles(state, valid_new, goal, tile=64):
    """bool [tiles_x, tiles_y]: the tile's halo region (the tile and one cell around it) holds a valid cell that the
    rollback put to INF.  Every cell of a tile that is not listed is final."""
    v = np.asarray(valid_new, bool)
    w, h = v.shape
    may_change = v & (np.asarray(state) == INF)
    tx, ty = -(-w // tile), -(-h // tile)
    out = np.zeros((tx, ty), bool)
    for a in range(tx):
        for b in range(ty):
            out[a, b] = may_change[max(0, a * tile - 1):(a + 1) * tile + 1, max(0, b * tile - 1):(b + 1) * tile + 1].any()
    return out


def settle(state, valid, pen=None):
    """The fixed point of rule 3's (rule 7's with `pen`) relaxation from `state`: every finite value is a source, a
    value only ever falls.  Equals the fresh field when `state` lies between it and the initial state."""
    v = np.asarray(valid, bool)
    w, h = v.shape
    masks = ref.move_masks(v).reshape(-1).tolist()
    p = [0] * (w * h) if pen is None else np.asarray(pen, np.uint32).reshape(-1).tolist()
    steps = [(di * h + dj, ref.STRAIGHT if not (di and dj) else ref.DIAGONAL) for di, dj in ref.NEIGHBOURS]
    dist = np.asarray(state, np.uint32).reshape(-1).tolist()
    heap = [(d, c) for c, d in enumerate(dist) if d != INF]
    heapq.heapify(heap)
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
    return np.array(dist, np.uint32).reshape(w, h)


def replan(old_field, valid_old, valid_new, goal, pen_old=None, pen_new=None):
    """The whole statement: dict(touched, T, state, field, relaxed).  `field` is the new grid's field, `relaxed` whether
    rule 20 had anything to relax (T != INF)."""
    t = touched(valid_old, valid_new, pen_old, pen_new)
    T = threshold(old_field, t)
    if T == INF:
        return dict(touched=t, T=T, state=None, field=np.asarray(old_field, np.uint32), relaxed=False)
    state = rollback(old_field, valid_new, T, goal)
    return dict(touched=t, T=T, state=state, field=settle(state, valid_new, pen_new), relaxed=True)
