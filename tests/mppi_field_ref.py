"""The grid planner's cost field in the MPPI controller (DESIGN.md 4.12 rules 19 to 24, include/kompass_hip.h
kc_mppi_set_field) as a statement, in two forms.  Rules 1 to 12 are tests/mppi_ref.py's and rules 13 to 18
tests/mppi_movers_ref.py's; they are used from there, not restated: the checks, the samples, rule 4's advance, rule 2's
clamp, rule 14's q and the loop form's update.  With no field both forms are mppi_movers_ref's own.

step_loop is the literal one: Python ints, a loop a sample, a step, a mover.  step is the same over all samples at once
in numpy int64 (every value stays below 2^63 by the rules' bounds); its roll-out loop is mppi_movers_ref.step's with rule
20 in the place of rule 6 and rule 21 in the place of rule 7.  Fields are arrays f[I, J] of shape (W, H), as the planes.

Both return (U', Record, S, (f0, f_nom)); the last is (None, None) with no field."""
from collections import namedtuple

import numpy as np

import mppi_movers_ref as mm
import mppi_ref as mp
from worldmap_dist_ref import FAR
from worldmap_ref import MAX_OFFSET

INF = 0xFFFFFFFF                                                          # rule 19: no walk reaches the goal
MAX_FCAP, MAX_W_RUN, MAX_W_TERM = 1 << 24, 1 << 12, 64

Field = namedtuple("Field", "plane fcap w_run w_term")                    # rule 19's plane [W, H] and rules 19 to 21's scalars


# ---- rule 23: kc_mppi_check_field, in the library's order.  ValueError: KC_ERR_INVALID, IndexError: KC_ERR_RANGE ----
def check_field(fcap, w_run, w_term):
    if fcap == 0:
        raise ValueError("fcap = 0")
    if fcap > MAX_FCAP:
        raise IndexError("fcap above 2^24")
    if w_run > MAX_W_RUN:
        raise IndexError("w_run above 2^12")
    if w_term > MAX_W_TERM:
        raise IndexError("w_term above 64")


def check_shape(fld, plane):
    """A step's own refusal, behind the plane's: the field's shape is the map's."""
    if np.asarray(fld.plane).shape != np.asarray(plane).shape:
        raise mp.StateError("the field's shape is not the map's")


# ---- rule 19 ----
def fv(f, I, J):
    W, H = f.shape
    return int(f[I, J]) if 0 <= I < W and 0 <= J < H else INF


# ---- rules 20 and 21 around mppi_ref's rules 4, 5 and 8 and mppi_movers_ref's rules 14 to 16, for one sample ----
def sample_cost(plane, m, c, mv, fld, tx, ty, h, X):
    """-> (S_k, hit, hit by a mover, fl)"""
    W, Hh = plane.shape
    T, c2, N = len(X), len(c.pen_d2) - 1, len(mv.ox)
    total = 0
    fl = min(fv(fld.plane, *mp.cell(tx, ty)), fld.fcap)                   # rule 21: the pose's own cell
    for t in range(T):
        tx, ty, h = mp.advance(tx, ty, h, *X[t])
        I, J = mp.cell(tx, ty)
        d2 = int(plane[I, J]) if 0 <= I < W and 0 <= J < Hh else FAR
        if d2 <= c.r2:
            return min(total + c.pen_hit * (T - t) + fld.w_term * fl, mp.S_CAP), True, False, fl
        q = [mm.mover_q(mv, i, t, tx, ty) for i in range(N)]
        if any(q[i] <= mv.hq[i] for i in range(N)):
            return min(total + mv.pen_hit * (T - t) + fld.w_term * fl, mp.S_CAP), True, True, fl
        for i in range(N):
            if q[i] < mv.sq[i]:
                total += (((mv.sq[i] - q[i]) >> 16) * mv.g[i]) >> 16
        total += c.pen_d2[d2] if d2 <= c2 else c.pen_far
        fl = min(fv(fld.plane, I, J), fld.fcap)                           # rule 20
        total += (fl * fld.w_run) >> 8
    return min(total + fld.w_term * fl, mp.S_CAP), False, False, fl


def step_loop(plane, K, seed, m, c, tx, ty, h, U, step, fld=None, mv=mm.NONE, px=None, py=None):
    """One kc_mppi_step, literally.  fld None: the path mode over (px, py)."""
    if fld is None:
        return mm.step_loop(plane, K, seed, m, c, px, py, tx, ty, h, U, step, mv) + ((None, None),)
    T = len(U)
    mp.check(K, T, 1, m, c)                                               # rule 20: M plays no part
    mm.check_movers(mv)
    check_field(fld.fcap, fld.w_run, fld.w_term)
    mp.check_step(K, T, tx, ty, h, U, step)
    check_shape(fld, plane)
    key = mp.sample_key(seed, step)
    Xs = [[mp.sample(m, key, U, k, t) for t in range(T)] for k in range(K)]
    got = [sample_cost(plane, m, c, mv, fld, tx, ty, h, Xs[k]) for k in range(K)]
    S = [g[0] for g in got]
    out, s_min, k_best, den = mp.update(m, c, U, Xs, S)
    rec = mm.Record(s_min, k_best, S[0], den, sum(g[1] for g in got), step, sum(g[2] for g in got))
    return out, rec, S, (fv(fld.plane, *mp.cell(tx, ty)), got[0][3])      # rule 22


# ---- the vectorised form ----
def step(plane, K, seed, m, c, tx, ty, h, U, step, fld=None, mv=mm.NONE, px=None, py=None):
    """The same over all samples at once -> (U' as a list of tuples, Record, S int64 [K], (f0, f_nom))."""
    if fld is None:
        return mm.step(plane, K, seed, m, c, px, py, tx, ty, h, U, step, mv) + ((None, None),)
    T, N = len(U), len(mv.ox)
    mp.check(K, T, 1, m, c)
    mm.check_movers(mv)
    check_field(fld.fcap, fld.w_run, fld.w_term)
    mp.check_step(K, T, tx, ty, h, U, step)
    check_shape(fld, plane)
    plane = np.asarray(plane)
    f = np.asarray(fld.plane).astype(np.int64)
    W, Hh = plane.shape
    heads = mp._heads()
    X = mp.samples_v(m, mp.sample_key(seed, step), U, K)
    pen = np.array(list(c.pen_d2) + [c.pen_far], np.int64)
    c2 = len(c.pen_d2) - 1
    OX, OY, VX, VY, HQ, SQ, G = (np.array(a, np.int64)[None, :] if i < 4 else np.array(a, np.uint64).astype(np.int64)[None, :]
                                 for i, a in enumerate(mv[:7]))
    TX, TY, Hd = np.full(K, tx, np.int64), np.full(K, ty, np.int64), np.full(K, h, np.int64)
    alive = np.ones(K, bool)
    moving = np.zeros(K, bool)
    total = np.zeros(K, np.int64)
    f0 = fv(fld.plane, *mp.cell(tx, ty))
    fl = np.full(K, min(f0, fld.fcap), np.int64)
    for t in range(T):
        C, S = heads[Hd, 0], heads[Hd, 1]
        F, L, H = X[:, t, 0], X[:, t, 1], X[:, t, 2]
        TX = np.where(alive, np.clip(TX + ((C * F - S * L + (1 << 15)) >> 16), -MAX_OFFSET, MAX_OFFSET), TX)
        TY = np.where(alive, np.clip(TY + ((S * F + C * L + (1 << 15)) >> 16), -MAX_OFFSET, MAX_OFFSET), TY)
        Hd = np.where(alive, (Hd + H) & 0xFFFF, Hd)
        I, J = (TX + (1 << 15)) >> 16, (TY + (1 << 15)) >> 16
        inside = (I >= 0) & (I < W) & (J >= 0) & (J < Hh)
        Ic, Jc = np.where(inside, I, 0), np.where(inside, J, 0)
        d2 = np.where(inside, plane[Ic, Jc].astype(np.int64), FAR)
        hit = alive & (d2 <= c.r2)
        total += np.where(hit, c.pen_hit * (T - t), 0)
        alive &= ~hit
        if N:                                                             # rules 14 and 16
            dx, dy = (TX[:, None] - (OX + (t + 1) * VX)) >> 8, (TY[:, None] - (OY + (t + 1) * VY)) >> 8
            q = np.minimum(dx * dx + dy * dy, mm.MAX_Q)
            mhit = alive & (q <= HQ).any(axis=1)
            total += np.where(mhit, mv.pen_hit * (T - t), 0)
            alive &= ~mhit
            moving |= mhit
            soft = np.where(q < SQ, (((SQ - q) >> 16) * G) >> 16, 0).sum(axis=1)
            total += np.where(alive, soft, 0)
        if not alive.any():
            break
        total += np.where(alive, pen[np.minimum(d2, c2 + 1)], 0)
        fc = np.minimum(np.where(inside, f[Ic, Jc], INF), fld.fcap)      # rules 19 and 20
        fl = np.where(alive, fc, fl)
        total += np.where(alive, (fc * fld.w_run) >> 8, 0)
    S = np.minimum(total + fld.w_term * fl, mp.S_CAP)                     # rules 21 and 8
    # rules 8 to 11, as mppi_ref.step has them
    s_min = int(S.min())
    k_best = int(np.argmin(S))
    wt = np.array(c.wtab, np.int64)
    w = wt[np.minimum((S - s_min) >> c.w_shift, len(wt) - 1)]
    den = int(w.sum())
    Ua = np.array(U, np.int64).reshape(T, 3)
    num = (w[:, None, None] * (X - Ua[None])).sum(axis=0)
    new = mp._clamp_u_v(m, Ua + (2 * num + den) // (2 * den))
    rec = mm.Record(s_min, k_best, int(S[0]), den, int(K - alive.sum()), step, int(moving.sum()))
    return [tuple(int(v) for v in r) for r in new], rec, S, (f0, int(fl[0]))


# ---- the two scenes of DESIGN.md 4.12 ----
ONE = 1 << 16
SCENE_START, SCENE_GOAL, SCENE_R2 = (10, 45), (110, 45), 9
FIELD_CAP, FIELD_RUN, FIELD_TERM = 1 << 20, 32, 2                         # MPPIConfig's field_cap, field_run_weight, field_goal_weight


def trap_cls():
    """int8 [W, H]: the border, and a U open towards the robot: its bottom at I = 70, its arms at J = 30 and J = 60."""
    from worldmap_ref import EMPTY, OCCUPIED
    c = np.full((mp.SCENE_W, mp.SCENE_H), EMPTY, np.int8)
    c[0, :] = c[-1, :] = OCCUPIED
    c[:, 0] = c[:, -1] = OCCUPIED
    c[70, 30:61] = OCCUPIED
    c[45:71, 30] = OCCUPIED
    c[45:71, 60] = OCCUPIED
    return c


def scene_field(cls, goal=SCENE_GOAL, r2=SCENE_R2):
    """The planner's field of a class plane (tests/planner_ref.py: the disc of r2, unknown cells allowed)."""
    import planner_ref as pref
    return pref.cost_field(pref.validity(cls, r2), goal)


def closed_loop(plane, fplane, seed, K=mp.SCENE_K, T=mp.SCENE_T, max_steps=200, start=SCENE_START, goal=SCENE_GOAL,
                fcap=FIELD_CAP, w_run=FIELD_RUN, w_term=FIELD_TERM):
    """mppi_ref.closed_loop in field mode: no path; the goal test is 1.5 cells around the goal cell's centre.
    -> (steps taken or None, smallest d2 of an occupied cell, the cells)."""
    m, c = mp.scene_model(), mp.scene_costs()
    fld = Field(fplane, fcap, w_run, w_term)
    tx, ty, h = start[0] * ONE, start[1] * ONE, 0
    U = [(0, 0, 0)] * T
    cells, d2_min = [], FAR
    for n in range(max_steps):
        new = step(plane, K, seed, m, c, tx, ty, h, U, n, fld)[0]
        tx, ty, h = mp.advance(tx, ty, h, *new[0])
        U = mp.shift(new)
        I, J = mp.cell(tx, ty)
        cells.append((I, J))
        d2_min = min(d2_min, int(plane[I, J]))
        if (tx - goal[0] * ONE) ** 2 + (ty - goal[1] * ONE) ** 2 <= (3 << 15) ** 2:
            return n + 1, d2_min, cells
    return None, d2_min, cells


def closed_loop_path(plane, seed, vertices=(SCENE_START, SCENE_GOAL), K=mp.SCENE_K, T=mp.SCENE_T, max_steps=300):
    """mppi_ref.closed_loop (the path mode) over another polyline: the straight one from start to goal by default.
    -> (steps taken or None, the cells)."""
    m, c = mp.scene_model(), mp.scene_costs()
    px, py = mp.quantise_points(mp.polyline_points(tuple((float(x), float(y)) for x, y in vertices)))
    tx, ty, h = px[0], py[0], 0
    U = [(0, 0, 0)] * T
    cells = []
    for n in range(max_steps):
        wx, wy = mp.window_from(px, py, tx, ty)
        new = mp.step(plane, K, seed, m, c, wx, wy, tx, ty, h, U, n)[0]
        tx, ty, h = mp.advance(tx, ty, h, *new[0])
        U = mp.shift(new)
        cells.append(mp.cell(tx, ty))
        if (tx - px[-1]) ** 2 + (ty - py[-1]) ** 2 <= (3 << 15) ** 2:
            return n + 1, cells
    return None, cells
