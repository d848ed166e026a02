"""Acceleration limits inside the MPPI roll-out (DESIGN.md 4.12 rules 25 to 29, include/kompass_hip.h kc_mppi_set_rates) as
a statement, in two forms.  Rules 1 to 12 are tests/mppi_ref.py's, rules 13 to 18 tests/mppi_movers_ref.py's and rules 19
to 24 tests/mppi_field_ref.py's; they are used from there, not restated: the checks, the samples, rule 4's advance, the
costs of a sample and the loop form's update.  With no rates both forms are mppi_field_ref's own.

step_loop is the literal one: Python ints.  It draws every X_k as mppi_ref does, turns each into its applied sequence A_k
by rule 26 and hands A_k to the sample costs of the statements above in the place of X_k (rule 27: the state moves by A);
the update is handed X_k (rule 10 blends X).  step is the same over all samples at once in numpy int64; only the loop the
rules sit in is written again, with rule 26 between rule 3 and rule 4.

Both return (U', Record, S, (f0, f_nom)) as mppi_field_ref's do."""
from collections import namedtuple

import numpy as np

import mppi_field_ref as mf
import mppi_movers_ref as mm
import mppi_ref as mp
from worldmap_dist_ref import FAR
from worldmap_ref import MAX_OFFSET

MAX_RATE, MAX_TURN_RATE = 1 << 23, 65535
MAX_V0, MAX_H0 = 1 << 22, 32767

Rates = namedtuple("Rates", "f_up f_dn l_up l_dn h_up h_dn")               # rule 25
STILL = (0, 0, 0)


# ---- rule 29: kc_mppi_check_rates, in the library's order.  ValueError: KC_ERR_INVALID, IndexError: KC_ERR_RANGE ----
def check_rates(rates=None, v0=None):
    if rates is None:
        return
    for i, r in enumerate(rates):
        if r < 1:
            raise ValueError(f"rate {i} is below 1")
    for i in range(4):
        if rates[i] > MAX_RATE:
            raise IndexError(f"rate {i}, an F or L rate, is above 2^23")
    for i in range(4, 6):
        if rates[i] > MAX_TURN_RATE:
            raise IndexError(f"rate {i}, an H rate, is above 65535")
    if v0 is not None:
        check_v0(v0)


def check_v0(v0):
    for i in range(2):
        if abs(v0[i]) > MAX_V0:
            raise IndexError(f"V0[{i}] is beyond 2^22")
    if abs(v0[2]) > MAX_H0:
        raise IndexError("H0 is beyond 32767")


def box_rates(m):
    """The box's width on every channel: from a V0 inside the box, A = X (rule 27).  At least 1, as rule 25 asks."""
    return Rates(*[max(1, w) for w in (m.f_hi - m.f_lo,) * 2 + (2 * m.l_hi,) * 2 + (2 * m.h_hi,) * 2])


# ---- rule 26 ----
def lim(p, x, up, dn):
    return min(p + up, x) if p < x else max(p - dn, x)


def apply_one(m, R, prev, X):
    """A[t] from A[t - 1] = prev and X[t]"""
    F = lim(prev[0], X[0], R[0], R[1])
    L = lim(prev[1], X[1], R[2], R[3])
    H = lim(prev[2], X[2], R[4], R[5])
    if m.kq > 0:
        cone = (abs(F) * m.kq) >> 16
        H = max(-cone, min(cone, H))
    return F, L, H


def apply_rates(m, R, v0, X):
    """Rule 28, kc_mppi_apply_rates: rule 26 over a sequence -> [A[t]]"""
    out, prev = [], tuple(v0)
    for x in X:
        prev = apply_one(m, R, prev, x)
        out.append(prev)
    return out


# ---- the loop form ----
def step_loop(plane, K, seed, m, c, tx, ty, h, U, step, rates=None, v0=STILL, fld=None, mv=mm.NONE, px=None, py=None):
    """One kc_mppi_step with the rates set (None: the mode is off), literally."""
    if rates is None:
        return mf.step_loop(plane, K, seed, m, c, tx, ty, h, U, step, fld, mv, px, py)
    T = len(U)
    mp.check(K, T, 1 if fld is not None else len(px), m, c)
    mm.check_movers(mv)
    if fld is not None:
        mf.check_field(fld.fcap, fld.w_run, fld.w_term)
    check_rates(rates, v0)
    mp.check_step(K, T, tx, ty, h, U, step)
    if fld is not None:
        mf.check_shape(fld, plane)
    key = mp.sample_key(seed, step)
    Xs = [[mp.sample(m, key, U, k, t) for t in range(T)] for k in range(K)]
    As = [apply_rates(m, rates, v0, X) for X in Xs]                        # rule 26
    if fld is not None:                                                   # rule 27: the costs of A_k
        got = [mf.sample_cost(plane, m, c, mv, fld, tx, ty, h, A) for A in As]
        words = (mf.fv(fld.plane, *mp.cell(tx, ty)), got[0][3])
    else:
        got = [mm.sample_cost(plane, m, c, mv, px, py, tx, ty, h, A) for A in As]
        words = (None, None)
    S = [g[0] for g in got]
    out, s_min, k_best, den = mp.update(m, c, U, Xs, S)                    # rule 10 blends X_k
    rec = mm.Record(s_min, k_best, S[0], den, sum(g[1] for g in got), step, sum(g[2] for g in got))
    return out, rec, S, words


# ---- the vectorised form ----
def _lim_v(p, x, up, dn):
    return np.where(p < x, np.minimum(p + up, x), np.maximum(p - dn, x))


def step(plane, K, seed, m, c, tx, ty, h, U, step, rates=None, v0=STILL, fld=None, mv=mm.NONE, px=None, py=None):
    """The same over all samples at once -> (U' as a list of tuples, Record, S int64 [K], (f0, f_nom))."""
    if rates is None:
        return mf.step(plane, K, seed, m, c, tx, ty, h, U, step, fld, mv, px, py)
    field = fld is not None
    T, N = len(U), len(mv.ox)
    M = 1 if field else len(px)
    mp.check(K, T, M, m, c)
    mm.check_movers(mv)
    if field:
        mf.check_field(fld.fcap, fld.w_run, fld.w_term)
    check_rates(rates, v0)
    mp.check_step(K, T, tx, ty, h, U, step)
    if field:
        mf.check_shape(fld, plane)
    plane = np.asarray(plane)
    W, Hh = plane.shape
    heads = mp._heads()
    X = mp.samples_v(m, mp.sample_key(seed, step), U, K)
    pen = np.array(list(c.pen_d2) + [c.pen_far], np.int64)
    c2 = len(c.pen_d2) - 1
    OX, OY, VX, VY, HQ, SQ, G = (np.array(a, np.int64)[None, :] if i < 4 else np.array(a, np.uint64).astype(np.int64)[None, :]
                                 for i, a in enumerate(mv[:7]))
    TX, TY, Hd = np.full(K, tx, np.int64), np.full(K, ty, np.int64), np.full(K, h, np.int64)
    AF, AL, AH = (np.full(K, v, np.int64) for v in v0)                    # rule 26: A[-1] = V0
    alive = np.ones(K, bool)
    moving = np.zeros(K, bool)
    total, jm = np.zeros(K, np.int64), np.zeros(K, np.int64)
    if field:
        f = np.asarray(fld.plane).astype(np.int64)
        f0 = mf.fv(fld.plane, *mp.cell(tx, ty))
        fl = np.full(K, min(f0, fld.fcap), np.int64)
    else:
        PX, PY = np.array(px, np.int64)[None, :], np.array(py, np.int64)[None, :]
        jidx = np.arange(M, dtype=np.int64)[None, :]
    for t in range(T):
        AF = _lim_v(AF, X[:, t, 0], rates[0], rates[1])                   # rule 26
        AL = _lim_v(AL, X[:, t, 1], rates[2], rates[3])
        AH = _lim_v(AH, X[:, t, 2], rates[4], rates[5])
        if m.kq > 0:
            cone = (np.abs(AF) * m.kq) >> 16
            AH = np.maximum(-cone, np.minimum(cone, AH))
        C, S = heads[Hd, 0], heads[Hd, 1]
        TX = np.where(alive, np.clip(TX + ((C * AF - S * AL + (1 << 15)) >> 16), -MAX_OFFSET, MAX_OFFSET), TX)   # rule 27
        TY = np.where(alive, np.clip(TY + ((S * AF + C * AL + (1 << 15)) >> 16), -MAX_OFFSET, MAX_OFFSET), TY)
        Hd = np.where(alive, (Hd + AH) & 0xFFFF, Hd)
        I, J = (TX + (1 << 15)) >> 16, (TY + (1 << 15)) >> 16
        inside = (I >= 0) & (I < W) & (J >= 0) & (J < Hh)
        Ic, Jc = np.where(inside, I, 0), np.where(inside, J, 0)
        d2 = np.where(inside, plane[Ic, Jc].astype(np.int64), FAR)
        hit = alive & (d2 <= c.r2)
        total += np.where(hit, c.pen_hit * (T - t), 0)
        alive &= ~hit
        if N:
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
        if field:
            fc = np.minimum(np.where(inside, f[Ic, Jc], mf.INF), fld.fcap)
            fl = np.where(alive, fc, fl)
            total += np.where(alive, (fc * fld.w_run) >> 8, 0)
        else:
            a = np.flatnonzero(alive)
            dx, dy = (TX[a, None] - PX) >> 8, (TY[a, None] - PY) >> 8
            key = ((np.minimum(dx * dx + dy * dy, c.qcap) << 8) | jidx).min(axis=1)
            total[a] += ((key >> 8) * c.w_path) >> 16
            jm[a] = key & 0xFF
    S = np.minimum(total + (fld.w_term * fl if field else c.w_goal * (M - 1 - jm)), mp.S_CAP)
    s_min = int(S.min())
    k_best = int(np.argmin(S))
    wt = np.array(c.wtab, np.int64)
    w = wt[np.minimum((S - s_min) >> c.w_shift, len(wt) - 1)]
    den = int(w.sum())
    Ua = np.array(U, np.int64).reshape(T, 3)
    num = (w[:, None, None] * (X - Ua[None])).sum(axis=0)                 # rule 10: X, not A
    new = mp._clamp_u_v(m, Ua + (2 * num + den) // (2 * den))
    rec = mm.Record(s_min, k_best, int(S[0]), den, int(K - alive.sum()), step, int(moving.sum()))
    return [tuple(int(v) for v in r) for r in new], rec, S, ((f0, int(fl[0])) if field else (None, None))


# ---- the closed-loop scene of DESIGN.md 4.12 under a robot that obeys the rates ----
SCENE_RATES = Rates(4096, 4096, 1, 1, 50, 50)                             # 1/16 cell a step^2; the scene has no lateral channel


def closed_loop_limited(plane, seed, rates=SCENE_RATES, aware=True, K=mp.SCENE_K, T=mp.SCENE_T, max_steps=200):
    """mppi_ref.closed_loop with a robot that moves by v = rule 26(v, U'[0]) from v = 0.  aware: the controller is told
    the rates and v (rules 25 to 27); not aware: it is the step of rules 1 to 12, and its U'[0] passes through the same
    robot.  -> (steps taken or None, smallest d2 of an occupied cell, the cells)."""
    m, c = mp.scene_model(), mp.scene_costs()
    px, py = mp.quantise_points(mp.polyline_points())
    tx, ty, h = px[0], py[0], 0
    U = [(0, 0, 0)] * T
    v = STILL
    cells, d2_min = [], FAR
    for n in range(max_steps):
        wx, wy = mp.window_from(px, py, tx, ty)
        new = step(plane, K, seed, m, c, tx, ty, h, U, n, rates if aware else None, v, px=wx, py=wy)[0]
        v = apply_one(m, rates, v, new[0])
        tx, ty, h = mp.advance(tx, ty, h, *v)
        U = mp.shift(new)
        I, J = mp.cell(tx, ty)
        cells.append((I, J))
        d2_min = min(d2_min, int(plane[I, J]))
        if (tx - px[-1]) ** 2 + (ty - py[-1]) ** 2 <= (3 << 15) ** 2:
            return n + 1, d2_min, cells
    return None, d2_min, cells
