"""A box footprint as a chain of discs on the distance plane, inside the MPPI roll-out (DESIGN.md 4.12 rules 30 to 36,
include/kompass_hip.h kc_mppi_set_footprint) as a statement, in two forms.  Rules 1 to 12 are tests/mppi_ref.py's, rules 13
to 18 tests/mppi_movers_ref.py's, rules 19 to 24 tests/mppi_field_ref.py's and rules 25 to 29 tests/mppi_rates_ref.py's; they
are used from there, not restated: the checks, the samples, rule 4's advance, rule 26's applied control and the loop
form's update.  With no offsets both forms are mppi_rates_ref's own.

step_loop is the literal one: Python ints, a loop a sample, a step, a disc, a mover.  step is the same over all samples
at once in numpy int64 (every value stays below 2^63 by the rules' bounds); its roll-out loop is mppi_rates_ref.step's
with rule 31's minimum over the discs in the place of rule 5's one lookup and rule 32's in the place of rule 14's q.

Both return (U', Record, S, (f0, f_nom)) as mppi_rates_ref's do.

cover() is rule 36, the front end's doubles; rectangle_overlaps_cell() and overlaps() are the exact geometry the cover
theorem is tested against: no rule, only a yardstick."""
import math

import numpy as np

import mppi_field_ref as mf
import mppi_movers_ref as mm
import mppi_rates_ref as mr
import mppi_ref as mp
import worldmap_mcl_ref as mref
from worldmap_dist_ref import FAR
from worldmap_ref import MAX_OFFSET

MAX_DISCS, MAX_DISC_OFFSET = 8, 1 << 22                                   # rule 30
MARGIN = 1.5                                                              # rule 36: sqrt(2) rounded up to half a cell


# ---- rule 35: kc_mppi_check_footprint, in the library's order.  ValueError: KC_ERR_INVALID, IndexError: KC_ERR_RANGE ----
def check_footprint(offsets, n=None):
    """offsets None: a NULL array; n: the count handed over, len(offsets) by default."""
    n = (0 if offsets is None else len(offsets)) if n is None else n
    if n == 0:
        return
    if n > MAX_DISCS:
        raise IndexError("discs above 8")
    if offsets is None:
        raise ValueError("a null array of offsets")
    for i in range(n):
        if abs(offsets[i]) > MAX_DISC_OFFSET:
            raise IndexError(f"offset {i} beyond 2^22")


# ---- rule 31 ----
def centres(tx, ty, h, offs):
    """The disc centres of the state (tx, ty, h): h is the heading after the step."""
    C, S = mref.headings()[h]
    return [(tx + ((C * o + (1 << 15)) >> 16), ty + ((S * o + (1 << 15)) >> 16)) for o in offs]


def plane_at(plane, x, y):
    W, Hh = plane.shape
    I, J = mp.cell(x, y)
    return int(plane[I, J]) if 0 <= I < W and 0 <= J < Hh else FAR


def plane_min(plane, tx, ty, h, offs):
    """dm of a state"""
    return min(plane_at(plane, x, y) for x, y in centres(tx, ty, h, offs))


# ---- rule 32 ----
def mover_q(mv, i, t, cs):
    """Rule 14's q against every disc centre, the least"""
    return min(mm.mover_q(mv, i, t, x, y) for x, y in cs)


# ---- rules 31 and 32 around the rules of the four statements, for one sample ----
def sample_cost(plane, m, c, mv, fld, px, py, tx, ty, h, A, offs):
    """A: the controls the state moves by (X_k, or A_k under rates) -> (S_k, hit, hit by a mover, fl or None)"""
    field = fld is not None
    T, c2, N = len(A), len(c.pen_d2) - 1, len(mv.ox)
    M = 0 if field else len(px)
    total, jm = 0, 0
    fl = min(mf.fv(fld.plane, *mp.cell(tx, ty)), fld.fcap) if field else None

    def end():
        return fld.w_term * fl if field else c.w_goal * (M - 1 - jm)
    for t in range(T):
        tx, ty, h = mp.advance(tx, ty, h, *A[t])
        cs = centres(tx, ty, h, offs)                                     # rule 31: by the heading after the step
        dm = min(plane_at(plane, x, y) for x, y in cs)
        if dm <= c.r2:
            return min(total + c.pen_hit * (T - t) + end(), mp.S_CAP), True, False, fl
        q = [mover_q(mv, i, t, cs) for i in range(N)]
        if any(q[i] <= mv.hq[i] for i in range(N)):
            return min(total + mv.pen_hit * (T - t) + end(), mp.S_CAP), True, True, fl
        for i in range(N):
            if q[i] < mv.sq[i]:
                total += (((mv.sq[i] - q[i]) >> 16) * mv.g[i]) >> 16
        total += c.pen_d2[dm] if dm <= c2 else c.pen_far
        if field:                                                         # rule 33: the field at the pose's own cell
            fl = min(mf.fv(fld.plane, *mp.cell(tx, ty)), fld.fcap)
            total += (fl * fld.w_run) >> 8
        else:
            best = min((min(((tx - px[j]) >> 8) ** 2 + ((ty - py[j]) >> 8) ** 2, c.qcap) << 8) | j for j in range(M))
            total += ((best >> 8) * c.w_path) >> 16
            jm = best & 0xFF
    return min(total + end(), mp.S_CAP), False, False, fl


def _checks(plane, K, m, c, tx, ty, h, U, step, offs, rates, v0, fld, mv, px):
    T = len(U)
    mp.check(K, T, 1 if fld is not None else len(px), m, c)
    mm.check_movers(mv)
    if fld is not None:
        mf.check_field(fld.fcap, fld.w_run, fld.w_term)
    mr.check_rates(rates, v0)
    check_footprint(offs)
    mp.check_step(K, T, tx, ty, h, U, step)
    if fld is not None:
        mf.check_shape(fld, plane)


def step_loop(plane, K, seed, m, c, tx, ty, h, U, step, offs=(), rates=None, v0=mr.STILL, fld=None, mv=mm.NONE, px=None, py=None):
    """One kc_mppi_step with the footprint set (none: the mode is off), literally."""
    if len(offs) == 0:
        return mr.step_loop(plane, K, seed, m, c, tx, ty, h, U, step, rates, v0, fld, mv, px, py)
    _checks(plane, K, m, c, tx, ty, h, U, step, offs, rates, v0, fld, mv, px)
    T = len(U)
    key = mp.sample_key(seed, step)
    Xs = [[mp.sample(m, key, U, k, t) for t in range(T)] for k in range(K)]
    As = Xs if rates is None else [mr.apply_rates(m, rates, v0, X) for X in Xs]   # rule 34: the discs turn with what was applied
    got = [sample_cost(plane, m, c, mv, fld, px, py, tx, ty, h, A, offs) for A in As]
    S = [g[0] for g in got]
    out, s_min, k_best, den = mp.update(m, c, U, Xs, S)
    rec = mm.Record(s_min, k_best, S[0], den, sum(g[1] for g in got), step, sum(g[2] for g in got))
    words = (mf.fv(fld.plane, *mp.cell(tx, ty)), got[0][3]) if fld is not None else (None, None)
    return out, rec, S, words


# ---- the vectorised form ----
def step(plane, K, seed, m, c, tx, ty, h, U, step, offs=(), rates=None, v0=mr.STILL, fld=None, mv=mm.NONE, px=None, py=None):
    """The same over all samples at once -> (U' as a list of tuples, Record, S int64 [K], (f0, f_nom))."""
    if len(offs) == 0:
        return mr.step(plane, K, seed, m, c, tx, ty, h, U, step, rates, v0, fld, mv, px, py)
    _checks(plane, K, m, c, tx, ty, h, U, step, offs, rates, v0, fld, mv, px)
    field = fld is not None
    T, N = len(U), len(mv.ox)
    M = 1 if field else len(px)
    plane = np.asarray(plane)
    W, Hh = plane.shape
    heads = mp._heads()
    X = mp.samples_v(m, mp.sample_key(seed, step), U, K)
    pen = np.array(list(c.pen_d2) + [c.pen_far], np.int64)
    c2 = len(c.pen_d2) - 1
    OX, OY, VX, VY, HQ, SQ, G = (np.array(a, np.int64)[None, :] if i < 4 else np.array(a, np.uint64).astype(np.int64)[None, :]
                                 for i, a in enumerate(mv[:7]))
    O = np.array(offs, np.int64)[None, :]
    TX, TY, Hd = np.full(K, tx, np.int64), np.full(K, ty, np.int64), np.full(K, h, np.int64)
    AF, AL, AH = (np.full(K, v, np.int64) for v in v0)
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
        if rates is None:
            AF, AL, AH = X[:, t, 0], X[:, t, 1], X[:, t, 2]
        else:                                                             # rule 26
            AF = mr._lim_v(AF, X[:, t, 0], rates[0], rates[1])
            AL = mr._lim_v(AL, X[:, t, 1], rates[2], rates[3])
            AH = mr._lim_v(AH, X[:, t, 2], rates[4], rates[5])
            if m.kq > 0:
                cone = (np.abs(AF) * m.kq) >> 16
                AH = np.maximum(-cone, np.minimum(cone, AH))
        C, S = heads[Hd, 0], heads[Hd, 1]
        TX = np.where(alive, np.clip(TX + ((C * AF - S * AL + (1 << 15)) >> 16), -MAX_OFFSET, MAX_OFFSET), TX)
        TY = np.where(alive, np.clip(TY + ((S * AF + C * AL + (1 << 15)) >> 16), -MAX_OFFSET, MAX_OFFSET), TY)
        Hd = np.where(alive, (Hd + AH) & 0xFFFF, Hd)
        C, S = heads[Hd, 0], heads[Hd, 1]                                 # rule 31: the pair of the new heading
        CX = TX[:, None] + ((C[:, None] * O + (1 << 15)) >> 16)           # [K, NB]
        CY = TY[:, None] + ((S[:, None] * O + (1 << 15)) >> 16)
        DI, DJ = (CX + (1 << 15)) >> 16, (CY + (1 << 15)) >> 16
        din = (DI >= 0) & (DI < W) & (DJ >= 0) & (DJ < Hh)
        d2 = np.where(din, plane[np.where(din, DI, 0), np.where(din, DJ, 0)].astype(np.int64), FAR).min(axis=1)   # dm
        hit = alive & (d2 <= c.r2)
        total += np.where(hit, c.pen_hit * (T - t), 0)
        alive &= ~hit
        if N:                                                             # rule 32
            dx = (CX[:, :, None] - (OX + (t + 1) * VX)[:, None, :]) >> 8   # [K, NB, N]
            dy = (CY[:, :, None] - (OY + (t + 1) * VY)[:, None, :]) >> 8
            q = np.minimum(dx * dx + dy * dy, mm.MAX_Q).min(axis=1)
            mhit = alive & (q <= HQ).any(axis=1)
            total += np.where(mhit, mv.pen_hit * (T - t), 0)
            alive &= ~mhit
            moving |= mhit
            soft = np.where(q < SQ, (((SQ - q) >> 16) * G) >> 16, 0).sum(axis=1)
            total += np.where(alive, soft, 0)
        if not alive.any():
            break
        total += np.where(alive, pen[np.minimum(d2, c2 + 1)], 0)
        if field:                                                         # rule 33
            I, J = (TX + (1 << 15)) >> 16, (TY + (1 << 15)) >> 16
            inside = (I >= 0) & (I < W) & (J >= 0) & (J < Hh)
            fc = np.minimum(np.where(inside, f[np.where(inside, I, 0), np.where(inside, J, 0)], mf.INF), fld.fcap)
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


# ---- rule 36: the front end's cover, host doubles ----
def cover(a, b, margin=MARGIN):
    """A box of half-length a and half-width b (cells) -> (offsets in 16 fraction bits, r2, rho)"""
    n = min(MAX_DISCS, max(1, math.ceil(a / b)))
    s = 2.0 * a / n
    offs = [round((-a + s / 2 + i * s) * 65536.0) for i in range(n)]
    rho = math.sqrt(b * b + (s / 2) ** 2)
    return offs, math.ceil((rho + margin) ** 2), rho


# ---- exact geometry: an oriented rectangle against a cell's closed unit square, by separating axes ----
def rectangle_overlaps_cell(x, y, th, a, b, I, J):
    """x, y: the rectangle's centre in cells; th: radians; a, b: half-length (along th) and half-width; the cell (I, J)
    covers [I - 0.5, I + 0.5] x [J - 0.5, J + 0.5]."""
    c, s = math.cos(th), math.sin(th)
    dx, dy = I - x, J - y
    if abs(dx) > abs(a * c) + abs(b * s) + 0.5 or abs(dy) > abs(a * s) + abs(b * c) + 0.5:   # the world's axes
        return False
    half = 0.5 * (abs(c) + abs(s))                                        # the square on either body axis
    return abs(dx * c + dy * s) <= a + half and abs(-dx * s + dy * c) <= b + half


def overlaps(occ, tx, ty, h, a, b, shift=0.0):
    """The occupied cells of occ [W, H] (bool) that the box of the state (tx, ty, h) overlaps; shift: the box's centre
    along its forward axis from the pose, in cells (0: the pose is the centre).  Exact to the doubles' rounding."""
    th = h / 65536.0 * 2.0 * math.pi
    x, y = tx / 65536.0 + shift * math.cos(th), ty / 65536.0 + shift * math.sin(th)
    r = int(math.ceil(math.hypot(a, b) + 1.0))
    I0, J0 = int(round(x)), int(round(y))
    out = []
    for I in range(max(0, I0 - r), min(occ.shape[0], I0 + r + 1)):
        for J in range(max(0, J0 - r), min(occ.shape[1], J0 + r + 1)):
            if occ[I, J] and rectangle_overlaps_cell(x, y, th, a, b, I, J):
                out.append((I, J))
    return out


# ---- the corridor with an L-turn of DESIGN.md 4.12: a 30 x 4-cell box, the pose at its centre ----
BOX_A, BOX_B = 15.0, 2.0                                                  # half-length, half-width: 1.5 x 0.2 m at 0.05 m
L_WIDTH = 22                                                              # between the walls' cell centres
L_REACH = 18                                                              # the circumscribed disc's r2 = 277 <= 18^2
L_VERTICES = ((25.0, 20.0), (65.0, 20.0), (80.0, 35.0), (80.0, 62.0))     # chamfered, and short of the border by the box
L_SHARP = ((25.0, 20.0), (80.0, 20.0), (80.0, 62.0))                     # what a planner that takes the robot for a disc hands over
L_K, L_T = 512, 32


def corridor_cls():
    """int8 [120, 90]: the border; a corridor along J = 20 between walls at J = 9 and J = 31, turning at I = 80 into a
    corridor along I = 80 between walls at I = 69 and I = 91."""
    from worldmap_ref import EMPTY, OCCUPIED
    c = np.full((mp.SCENE_W, mp.SCENE_H), EMPTY, np.int8)
    c[0, :] = c[-1, :] = OCCUPIED
    c[:, 0] = c[:, -1] = OCCUPIED
    lo, hi = 20 - L_WIDTH // 2, 20 + L_WIDTH // 2                         # 9, 31
    left, right = 80 - L_WIDTH // 2, 80 + L_WIDTH // 2                    # 69, 91
    c[0:right + 1, lo] = OCCUPIED
    c[0:left + 1, hi] = OCCUPIED
    c[left, hi:] = OCCUPIED
    c[right, lo:] = OCCUPIED
    return c


def corridor_costs(r2):
    """mppi_ref.scene_costs with the table drawn out to L_REACH^2 (it is zero from d2 = 49 on) and the r2 given"""
    c = mp.scene_costs()
    pen = list(c.pen_d2) + [0] * (L_REACH * L_REACH + 1 - len(c.pen_d2))
    return c._replace(r2=r2, pen_d2=pen)


def closed_loop(plane, occ, seed, offs, r2, K=L_K, T=L_T, max_steps=200, a=BOX_A, b=BOX_B, vertices=L_VERTICES):
    """mppi_ref.closed_loop over the L with the footprint given (one offset 0: a disc at the pose).  After every plant
    step the exact overlap test runs on the state the robot is in.  -> (steps taken or None, the states that overlap an
    occupied cell, n_hit of every step)."""
    m, c = mp.scene_model(), corridor_costs(r2)
    px, py = mp.quantise_points(mp.polyline_points(vertices))
    tx, ty, h = px[0], py[0], 0
    U = [(0, 0, 0)] * T
    bad, hits = [], []
    for n in range(max_steps):
        wx, wy = mp.window_from(px, py, tx, ty)
        new, rec, _, _ = step(plane, K, seed, m, c, tx, ty, h, U, n, offs, px=wx, py=wy)
        hits.append(rec.n_hit)
        tx, ty, h = mp.advance(tx, ty, h, *new[0])
        U = mp.shift(new)
        if overlaps(occ, tx, ty, h, a, b):
            bad.append((n, tx, ty, h))
        if (tx - px[-1]) ** 2 + (ty - py[-1]) ** 2 <= (3 << 15) ** 2:
            return n + 1, bad, hits
    return None, bad, hits
