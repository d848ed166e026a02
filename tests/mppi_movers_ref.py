"""Moving obstacles in the MPPI controller (DESIGN.md 4.12 rules 13 to 18, include/kompass_hip.h kc_mppi_set_movers) as a
statement, in two forms.  Rules 1 to 12 are tests/mppi_ref.py's and are used from there, not restated: the checks, the
samples, rule 4's advance, rule 2's clamp and the loop form's update.

step_loop is the literal one: Python ints, a loop a sample, a step, a mover.  step is the same over all samples at once
in numpy int64 (every value stays below 2^63 by the rules' bounds); its roll-out loop is mppi_ref.step's with rule 16
between rule 5's test and rule 5's penalty, and tests/test_mppi_movers_cpu.py shows both forms equal to mppi_ref.step
when there is no mover and equal to each other when there are some."""
from collections import namedtuple

import numpy as np

import mppi_ref as mp
from worldmap_dist_ref import FAR
from worldmap_ref import MAX_OFFSET

MAX_MOVERS, MAX_POS, MAX_VEL, MAX_Q, MAX_GAIN, MAX_TOP, MAX_PEN_HIT = 64, 1 << 36, 1 << 22, 1 << 40, 1 << 32, 1 << 20, 1 << 20

Movers = namedtuple("Movers", "ox oy vx vy hq sq g pen_hit")              # rule 13: seven lists of N entries, one penalty
Record = namedtuple("Record", "s_min k_best s_0 den n_hit step n_hit_moving")   # rule 17; [:6] is mppi_ref.Record
NONE = Movers((), (), (), (), (), (), (), 0)


def movers(rows, pen_hit):
    """[(OX, OY, VX, VY, hq, sq, g)] -> Movers"""
    cols = list(zip(*rows)) if len(rows) else [()] * 7
    return Movers(*[tuple(int(v) for v in c) for c in cols], int(pen_hit))


def advanced(mv, n=1):
    """The list n control steps later, as a plant hands it on."""
    return mv._replace(ox=tuple(x + n * v for x, v in zip(mv.ox, mv.vx)), oy=tuple(y + n * v for y, v in zip(mv.oy, mv.vy)))


# ---- rule 18: kc_mppi_check_movers, in the library's order.  ValueError: KC_ERR_INVALID, IndexError: KC_ERR_RANGE ----
def check_movers(mv):
    n = len(mv.ox)
    if n == 0:
        return
    if n > MAX_MOVERS:
        raise IndexError("movers")
    if any(len(c) != n for c in mv[1:7]):
        raise ValueError("one entry a mover in every array")
    if mv.pen_hit > MAX_PEN_HIT:
        raise IndexError("pen_hit_mv above 2^20")
    for i in range(n):
        if abs(mv.ox[i]) > MAX_POS or abs(mv.oy[i]) > MAX_POS:
            raise IndexError(f"mover {i}: a position beyond 2^36")
        if abs(mv.vx[i]) > MAX_VEL or abs(mv.vy[i]) > MAX_VEL:
            raise IndexError(f"mover {i}: a velocity beyond 2^22")
        if mv.hq[i] > mv.sq[i]:
            raise ValueError(f"mover {i}: hq above sq")
        if mv.sq[i] > MAX_Q:
            raise IndexError(f"mover {i}: sq above 2^40")
        if mv.g[i] > MAX_GAIN:
            raise IndexError(f"mover {i}: g above 2^32")
        if (((mv.sq[i] - mv.hq[i]) >> 16) * mv.g[i]) >> 16 > MAX_TOP:
            raise IndexError(f"mover {i}: the ramp's top above 2^20")


# ---- rule 14 ----
def mover_q(mv, i, t, tx, ty):
    """q_i against the state after step t"""
    dx = (tx - (mv.ox[i] + (t + 1) * mv.vx[i])) >> 8
    dy = (ty - (mv.oy[i] + (t + 1) * mv.vy[i])) >> 8
    return min(dx * dx + dy * dy, MAX_Q)


# ---- rules 15 and 16 around mppi_ref's rules 4 to 8, for one sample ----
def sample_cost(plane, m, c, mv, px, py, tx, ty, h, X):
    """-> (S_k, hit, hit by a mover)"""
    W, Hh = plane.shape
    T, M, c2, N = len(X), len(px), len(c.pen_d2) - 1, len(mv.ox)
    total, jm = 0, 0
    for t in range(T):
        tx, ty, h = mp.advance(tx, ty, h, *X[t])
        I, J = mp.cell(tx, ty)
        d2 = int(plane[I, J]) if 0 <= I < W and 0 <= J < Hh else FAR
        if d2 <= c.r2:                                                    # rule 5's test comes first: a static hit wins
            return min(total + c.pen_hit * (T - t) + c.w_goal * (M - 1 - jm), mp.S_CAP), True, False
        q = [mover_q(mv, i, t, tx, ty) for i in range(N)]
        if any(q[i] <= mv.hq[i] for i in range(N)):                       # rule 16: frozen, nothing more from 5, 6 and 16
            return min(total + mv.pen_hit * (T - t) + c.w_goal * (M - 1 - jm), mp.S_CAP), True, True
        for i in range(N):
            if q[i] < mv.sq[i]:
                total += (((mv.sq[i] - q[i]) >> 16) * mv.g[i]) >> 16
        total += c.pen_d2[d2] if d2 <= c2 else c.pen_far
        best = min((min(((tx - px[j]) >> 8) ** 2 + ((ty - py[j]) >> 8) ** 2, c.qcap) << 8) | j for j in range(M))   # rule 6
        total += ((best >> 8) * c.w_path) >> 16
        jm = best & 0xFF
    return min(total + c.w_goal * (M - 1 - jm), mp.S_CAP), False, False


def step_loop(plane, K, seed, m, c, px, py, tx, ty, h, U, step, mv=NONE):
    """One kc_mppi_step with the list mv set, literally -> (U', Record, [S_k])."""
    T = len(U)
    mp.check(K, T, len(px), m, c)
    check_movers(mv)
    mp.check_step(K, T, tx, ty, h, U, step)
    key = mp.sample_key(seed, step)
    Xs = [[mp.sample(m, key, U, k, t) for t in range(T)] for k in range(K)]
    got = [sample_cost(plane, m, c, mv, px, py, tx, ty, h, Xs[k]) for k in range(K)]
    S = [g[0] for g in got]
    out, s_min, k_best, den = mp.update(m, c, U, Xs, S)
    return out, Record(s_min, k_best, S[0], den, sum(g[1] for g in got), step, sum(g[2] for g in got)), S


# ---- the vectorised form ----
def step(plane, K, seed, m, c, px, py, tx, ty, h, U, step, mv=NONE):
    """The same over all samples at once -> (U' as a list of tuples, Record, S int64 [K])."""
    T, M, N = len(U), len(px), len(mv.ox)
    mp.check(K, T, M, m, c)
    check_movers(mv)
    mp.check_step(K, T, tx, ty, h, U, step)
    plane = np.asarray(plane)
    W, Hh = plane.shape
    heads = mp._heads()
    X = mp.samples_v(m, mp.sample_key(seed, step), U, K)
    PX, PY = np.array(px, np.int64)[None, :], np.array(py, np.int64)[None, :]
    jidx = np.arange(M, dtype=np.int64)[None, :]
    pen = np.array(list(c.pen_d2) + [c.pen_far], np.int64)
    c2 = len(c.pen_d2) - 1
    OX, OY, VX, VY, HQ, SQ, G = (np.array(a, np.int64)[None, :] if i < 4 else np.array(a, np.uint64).astype(np.int64)[None, :]
                                 for i, a in enumerate(mv[:7]))           # all below 2^63
    TX, TY, Hd = np.full(K, tx, np.int64), np.full(K, ty, np.int64), np.full(K, h, np.int64)
    alive = np.ones(K, bool)
    moving = np.zeros(K, bool)
    total, jm = np.zeros(K, np.int64), np.zeros(K, np.int64)
    for t in range(T):
        C, S = heads[Hd, 0], heads[Hd, 1]
        F, L, H = X[:, t, 0], X[:, t, 1], X[:, t, 2]
        TX = np.where(alive, np.clip(TX + ((C * F - S * L + (1 << 15)) >> 16), -MAX_OFFSET, MAX_OFFSET), TX)
        TY = np.where(alive, np.clip(TY + ((S * F + C * L + (1 << 15)) >> 16), -MAX_OFFSET, MAX_OFFSET), TY)
        Hd = np.where(alive, (Hd + H) & 0xFFFF, Hd)
        I, J = (TX + (1 << 15)) >> 16, (TY + (1 << 15)) >> 16
        inside = (I >= 0) & (I < W) & (J >= 0) & (J < Hh)
        d2 = np.where(inside, plane[np.where(inside, I, 0), np.where(inside, J, 0)].astype(np.int64), FAR)
        hit = alive & (d2 <= c.r2)
        total += np.where(hit, c.pen_hit * (T - t), 0)
        alive &= ~hit
        if N:                                                             # rules 14 and 16
            dx, dy = (TX[:, None] - (OX + (t + 1) * VX)) >> 8, (TY[:, None] - (OY + (t + 1) * VY)) >> 8
            q = np.minimum(dx * dx + dy * dy, MAX_Q)
            mhit = alive & (q <= HQ).any(axis=1)
            total += np.where(mhit, mv.pen_hit * (T - t), 0)
            alive &= ~mhit
            moving |= mhit
            soft = np.where(q < SQ, (((SQ - q) >> 16) * G) >> 16, 0).sum(axis=1)
            total += np.where(alive, soft, 0)
        if not alive.any():
            break
        a = np.flatnonzero(alive)
        total[a] += pen[np.minimum(d2[a], c2 + 1)]
        dx, dy = (TX[a, None] - PX) >> 8, (TY[a, None] - PY) >> 8
        key = ((np.minimum(dx * dx + dy * dy, c.qcap) << 8) | jidx).min(axis=1)
        total[a] += ((key >> 8) * c.w_path) >> 16
        jm[a] = key & 0xFF
    S = np.minimum(total + c.w_goal * (M - 1 - jm), mp.S_CAP)
    # rules 8 to 11, as mppi_ref.step has them
    s_min = int(S.min())
    k_best = int(np.argmin(S))
    wt = np.array(c.wtab, np.int64)
    w = wt[np.minimum((S - s_min) >> c.w_shift, len(wt) - 1)]
    den = int(w.sum())
    Ua = np.array(U, np.int64).reshape(T, 3)
    num = (w[:, None, None] * (X - Ua[None])).sum(axis=0)
    new = mp._clamp_u_v(m, Ua + (2 * num + den) // (2 * den))
    rec = Record(s_min, k_best, int(S[0]), den, int(K - alive.sum()), step, int(moving.sum()))
    return [tuple(int(v) for v in r) for r in new], rec, S


# ---- the crossing scene of DESIGN.md 4.12 ----
ONE = 1 << 16
CROSS_START = (85 * ONE, 80 * ONE)
CROSS_V = (0, round(-0.45 * 65536))
CROSS_HQ, CROSS_SQ, CROSS_G, CROSS_PEN = 25 << 16, 81 << 16, (200 * 65536) // 57, 4000


def crossing_mover(start=CROSS_START, v=CROSS_V, hq=CROSS_HQ, sq=CROSS_SQ, g=CROSS_G, pen=CROSS_PEN):
    return movers([(start[0], start[1], v[0], v[1], hq, sq, g)], pen)


def closed_loop(plane, seed, mv, seeing=True, K=mp.SCENE_K, T=mp.SCENE_T, max_steps=200):
    """mppi_ref.closed_loop with one list of movers walking beside it: each step the controller is handed the list at its
    present place (or nothing when not `seeing`), then the plant advances the robot by the first control and every mover
    by its V.  -> (steps taken or None, smallest d2, smallest q - hq over the movers after each plant step)."""
    m, c = mp.scene_model(), mp.scene_costs()
    px, py = mp.quantise_points(mp.polyline_points())
    tx, ty, h = px[0], py[0], 0
    U = [(0, 0, 0)] * T
    d2_min, margin = FAR, None
    for n in range(max_steps):
        wx, wy = mp.window_from(px, py, tx, ty)
        new = step(plane, K, seed, m, c, wx, wy, tx, ty, h, U, n, mv if seeing else NONE)[0]
        tx, ty, h = mp.advance(tx, ty, h, *new[0])
        mv = advanced(mv)
        U = mp.shift(new)
        I, J = mp.cell(tx, ty)
        d2_min = min(d2_min, int(plane[I, J]))
        for i in range(len(mv.ox)):                                       # t = -1: the list where it stands now
            here = mover_q(mv, i, -1, tx, ty) - mv.hq[i]
            margin = here if margin is None else min(margin, here)
        if (tx - px[-1]) ** 2 + (ty - py[-1]) ** 2 <= (3 << 15) ** 2:
            return n + 1, d2_min, margin
    return None, d2_min, margin
