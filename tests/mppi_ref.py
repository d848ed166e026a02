"""The MPPI controller over the world map's distance plane (include/kompass_hip.h kc_mppi_*) as a
statement, in two forms.

step_loop is the literal one: Python ints, a loop a sample, a loop a step, a loop a path point; Python's >> on int is
arithmetic, its int has no width, // floors, round() rounds half to even as lrint does.

step is the same over all samples at once in numpy int64 / uint64 (whose arithmetic wraps as the library's does, whose >>
on int64 is arithmetic and whose // floors); every value stays below 2^63 by the rules' bounds, so it is exact.  It
serves as a reference because tests/test_mppi_cpu.py shows it equal to step_loop.

math.cos / math.sin enter through rule 29's heading table (worldmap_mcl_ref.headings) and nowhere else.  Planes are
arrays m[I, J] of shape (W, H), as worldmap_ref's."""
import math
from collections import namedtuple

import numpy as np

import worldmap_mcl_ref as mref
from worldmap_dist_ref import FAR, MAX_REACH
from worldmap_ref import MAX_OFFSET

M64 = mref.M64
MAX_SAMPLES, MAX_HORIZON, MAX_PATH, MAX_TABLE = 65536, 64, 256, 4096
MAX_DISP, MAX_TURN, MAX_KQ = 1 << 22, 32767, 1 << 24
MAX_PEN_HIT, MAX_W_PATH, MAX_QCAP, MAX_PATH_TERM, MAX_W_GOAL = 1 << 20, 1 << 16, 1 << 40, 1 << 24, 1 << 20
S_CAP = 1 << 30

Model = namedtuple("Model", "f_lo f_hi l_hi h_hi kq s")                   # rule 2's limits, rule 3's scales s[3]
Costs = namedtuple("Costs", "r2 pen_d2 pen_far pen_hit w_path qcap w_goal wtab w_shift")
Record = namedtuple("Record", "s_min k_best s_0 den n_hit step")          # rule 11


class StateError(RuntimeError):
    """KC_ERR_STATE"""


# ---- rule 12: kc_mppi_check, in the library's order.  ValueError: KC_ERR_INVALID, IndexError: KC_ERR_RANGE ----
def check(K, T, M, model=None, costs=None, reach=0):
    if K == 0 or T == 0 or M == 0:
        raise ValueError("no sample, no step or no path point")
    if K > MAX_SAMPLES:
        raise IndexError("samples")
    if T > MAX_HORIZON:
        raise IndexError("horizon")
    if M > MAX_PATH:
        raise IndexError("path window")
    if model is not None:
        if model.f_lo > model.f_hi or model.l_hi < 0 or model.h_hi < 0 or model.kq < 0:
            raise ValueError("an empty or negative limit")
        if abs(model.f_lo) > MAX_DISP or abs(model.f_hi) > MAX_DISP or model.l_hi > MAX_DISP:
            raise IndexError("a displacement limit above 2^22")
        if model.h_hi > MAX_TURN:
            raise IndexError("H_hi above 32767")
        if model.kq > MAX_KQ:
            raise IndexError("kq above 2^24")
        if len(model.s) != 3 or any(v < 0 for v in model.s):
            raise ValueError("a noise scale is negative")
    if costs is not None:
        n = len(costs.pen_d2)
        if n < 2:
            raise ValueError("pen_d2 needs c2 + 1 >= 2 entries")
        if n > MAX_TABLE:
            raise IndexError("pen_d2 too long")
        if costs.r2 > n - 1:
            raise ValueError("r2 above c2")
        if costs.pen_hit > MAX_PEN_HIT:
            raise IndexError("pen_hit above 2^20")
        if costs.w_path > MAX_W_PATH:
            raise IndexError("w_path above 2^16")
        if costs.qcap > MAX_QCAP:
            raise IndexError("qcap above 2^40")
        if (costs.qcap >> 16) * costs.w_path > MAX_PATH_TERM:
            raise IndexError("(qcap >> 16) w_path above 2^24")
        if costs.w_goal > MAX_W_GOAL:
            raise IndexError("w_goal above 2^20")
        if reach != 0:
            if not 1 <= reach <= MAX_REACH:
                raise IndexError("reach outside 1 .. 254")
            if n - 1 > reach * reach:
                raise ValueError("c2 above reach^2")
        w = costs.wtab
        if len(w) == 0:
            raise ValueError("an empty weight table")
        if len(w) > MAX_TABLE:
            raise IndexError("weight table too long")
        if not 0 <= costs.w_shift <= 30:
            raise ValueError("w_shift outside 0 .. 30")
        if not 1 <= w[0] <= 1 << 20:
            raise ValueError("wtab[0] outside 1 .. 2^20")
        if any(w[i] > w[i - 1] for i in range(1, len(w))):
            raise ValueError("the weight table increases")


def check_step(K, T, tx, ty, h, U, step):
    """kc_mppi_step's own refusals of its arguments, in its order."""
    if abs(tx) > MAX_OFFSET or abs(ty) > MAX_OFFSET:
        raise IndexError("the pose lies more than 2^20 cells from the origin")
    if not 0 <= h <= 65535:
        raise IndexError("heading outside 0 .. 65535")
    if len(U) != T:
        raise ValueError("one control a step")
    for F, L, H in U:
        if abs(F) > MAX_DISP or abs(L) > MAX_DISP or abs(H) > MAX_TURN:
            raise IndexError("a control of the sequence is outside rule 2's bounds")
    if not 0 <= step <= 0xFFFFFFFF:
        raise IndexError("step is a uint32")


# ---- rule 2 ----
def clamp_u(m, F, L, H):
    F = max(m.f_lo, min(m.f_hi, F))
    L = max(-m.l_hi, min(m.l_hi, L))
    H = max(-m.h_hi, min(m.h_hi, H))
    if m.kq > 0:
        lim = (abs(F) * m.kq) >> 16
        H = max(-lim, min(lim, H))
    return F, L, H


# ---- rule 3 ----
def sample_key(seed, step):
    return mref.mix64(((seed & M64) ^ (step << 32)) & M64)


def sample(m, key, U, k, t):
    """X_k[t]"""
    e = [0, 0, 0]
    if k != 0:
        e = [mref.noise(mref.mix64(key ^ ((k << 8) | (3 * t + c))), m.s[c]) for c in range(3)]
    return clamp_u(m, U[t][0] + e[0], U[t][1] + e[1], U[t][2] + e[2])


# ---- rule 4 ----
def advance(tx, ty, h, F, L, H):
    C, S = mref.headings()[h]
    tx = mref.clamp(tx + ((C * F - S * L + (1 << 15)) >> 16))
    ty = mref.clamp(ty + ((S * F + C * L + (1 << 15)) >> 16))
    return tx, ty, (h + H) & 0xFFFF


def cell(tx, ty):
    """Rule 1"""
    return (tx + (1 << 15)) >> 16, (ty + (1 << 15)) >> 16


def rollout(U, tx, ty, h):
    """The states after each step of a sequence: what predicted_path() shows."""
    out = []
    for F, L, H in U:
        tx, ty, h = advance(tx, ty, h, F, L, H)
        out.append((tx, ty, h))
    return out


# ---- rules 5 to 8 for one sample ----
def sample_cost(plane, m, c, px, py, tx, ty, h, X):
    """-> (S_k, hit).  X: the sample's T controls."""
    W, Hh = plane.shape
    T, M, c2 = len(X), len(px), len(c.pen_d2) - 1
    total, jm, hit = 0, 0, False
    for t in range(T):
        tx, ty, h = advance(tx, ty, h, *X[t])
        I, J = cell(tx, ty)
        d2 = int(plane[I, J]) if 0 <= I < W and 0 <= J < Hh else FAR
        if d2 <= c.r2:                                                    # rule 5: frozen, nothing more from 5 and 6
            total += c.pen_hit * (T - t)
            hit = True
            break
        total += c.pen_d2[d2] if d2 <= c2 else c.pen_far
        best = None
        for j in range(M):                                                # rule 6
            q = ((tx - px[j]) >> 8) ** 2 + ((ty - py[j]) >> 8) ** 2
            key = (min(q, c.qcap) << 8) | j
            if best is None or key < best:
                best = key
        total += ((best >> 8) * c.w_path) >> 16
        jm = best & 0xFF
    total += c.w_goal * (M - 1 - jm)                                      # rule 7
    return min(total, S_CAP), hit


def update(m, c, U, Xs, S):
    """Rules 8 to 11 from all samples' controls Xs[k][t] and costs S[k] -> (U', s_min, k_best, den)."""
    s_min = min(S)
    k_best = S.index(s_min)
    EW = len(c.wtab)
    w = [c.wtab[min((s - s_min) >> c.w_shift, EW - 1)] for s in S]
    den = sum(w)
    out = []
    for t in range(len(U)):
        new = []
        for ch in range(3):
            num = sum(w[k] * (Xs[k][t][ch] - U[t][ch]) for k in range(len(S)))
            new.append(U[t][ch] + (2 * num + den) // (2 * den))
        out.append(clamp_u(m, *new))
    return out, s_min, k_best, den


def step_loop(plane, K, seed, m, c, px, py, tx, ty, h, U, step):
    """One kc_mppi_step, literally -> (U', Record, [S_k])."""
    T = len(U)
    check(K, T, len(px), m, c)
    check_step(K, T, tx, ty, h, U, step)
    key = sample_key(seed, step)
    Xs = [[sample(m, key, U, k, t) for t in range(T)] for k in range(K)]
    S, n_hit = [], 0
    for k in range(K):
        s, hit = sample_cost(plane, m, c, px, py, tx, ty, h, Xs[k])
        S.append(s)
        n_hit += int(hit)
    out, s_min, k_best, den = update(m, c, U, Xs, S)
    return out, Record(s_min, k_best, S[0], den, n_hit, step), S


# ---- the vectorised form ----
_U = np.uint64


def _mix64_v(x):
    with np.errstate(over="ignore"):
        z = x + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def _clamp_u_v(m, X):
    F = np.clip(X[..., 0], m.f_lo, m.f_hi)
    L = np.clip(X[..., 1], -m.l_hi, m.l_hi)
    H = np.clip(X[..., 2], -m.h_hi, m.h_hi)
    if m.kq > 0:
        lim = (np.abs(F) * m.kq) >> 16
        H = np.maximum(-lim, np.minimum(lim, H))
    return np.stack([F, L, H], axis=-1)


def samples_v(m, key, U, K):
    """X [K, T, 3] int64"""
    Ua = np.array(U, np.int64).reshape(-1, 3)
    T = Ua.shape[0]
    ctr = (np.arange(K, dtype=_U)[:, None] << _U(8)) | np.arange(3 * T, dtype=_U)[None, :]
    v = _mix64_v(_U(key) ^ ctr)
    g = ((v & _U(0xFFFF)) + ((v >> _U(16)) & _U(0xFFFF)) + ((v >> _U(32)) & _U(0xFFFF)) + (v >> _U(48))).astype(np.int64) - 131070
    s = np.tile(np.array(m.s, np.int64), T)[None, :]
    eps = ((g * s + (1 << 15)) >> 16).reshape(K, T, 3)
    eps[0] = 0
    return _clamp_u_v(m, Ua[None] + eps)


_HEADS = None


def _heads():
    global _HEADS
    if _HEADS is None:
        _HEADS = np.array(mref.headings(), np.int64)
    return _HEADS


def step(plane, K, seed, m, c, px, py, tx, ty, h, U, step):
    """One kc_mppi_step over all samples at once -> (U' as a list of tuples, Record, S int64 [K])."""
    T, M = len(U), len(px)
    check(K, T, M, m, c)
    check_step(K, T, tx, ty, h, U, step)
    plane = np.asarray(plane)
    W, Hh = plane.shape
    heads = _heads()
    X = samples_v(m, sample_key(seed, step), U, K)
    PX, PY = np.array(px, np.int64)[None, :], np.array(py, np.int64)[None, :]
    jidx = np.arange(M, dtype=np.int64)[None, :]
    pen = np.array(list(c.pen_d2) + [c.pen_far], np.int64)               # the last entry stands for "above c2"
    c2 = len(c.pen_d2) - 1
    TX, TY, Hd = np.full(K, tx, np.int64), np.full(K, ty, np.int64), np.full(K, h, np.int64)
    alive = np.ones(K, bool)
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
        if not alive.any():
            break
        a = np.flatnonzero(alive)
        total[a] += pen[np.minimum(d2[a], c2 + 1)]
        dx, dy = (TX[a, None] - PX) >> 8, (TY[a, None] - PY) >> 8
        key = ((np.minimum(dx * dx + dy * dy, c.qcap) << 8) | jidx).min(axis=1)
        total[a] += ((key >> 8) * c.w_path) >> 16
        jm[a] = key & 0xFF
    n_hit = int(K - alive.sum())
    S = np.minimum(total + c.w_goal * (M - 1 - jm), S_CAP)
    s_min = int(S.min())
    k_best = int(np.argmin(S))                                            # the first among equals
    wt = np.array(c.wtab, np.int64)
    w = wt[np.minimum((S - s_min) >> c.w_shift, len(wt) - 1)]
    den = int(w.sum())
    Ua = np.array(U, np.int64).reshape(T, 3)
    num = (w[:, None, None] * (X - Ua[None])).sum(axis=0)                 # |.| < 2^59
    new = _clamp_u_v(m, Ua + (2 * num + den) // (2 * den))
    return [tuple(int(v) for v in r) for r in new], Record(s_min, k_best, int(S[0]), den, n_hit, step), S


# ---- the warm start, the host's ----
def shift(U):
    return list(U[1:]) + [U[-1]]


# ---- the closed-loop scene of DESIGN.md 4.12 ----
SCENE_W, SCENE_H, SCENE_REACH = 120, 90, 8
SCENE_VERTICES = ((10.0, 45.0), (50.0, 56.5), (70.0, 56.5), (110.0, 45.0))
SCENE_K, SCENE_T, SCENE_WINDOW = 1024, 32, 96


def scene_cls():
    """int8 [W, H]: the border, the wall of column 60 with its door at J 52 .. 61, the pillar."""
    from worldmap_ref import EMPTY, OCCUPIED
    c = np.full((SCENE_W, SCENE_H), EMPTY, np.int8)
    c[0, :] = c[-1, :] = OCCUPIED
    c[:, 0] = c[:, -1] = OCCUPIED
    c[60, :] = OCCUPIED
    c[60, 52:62] = EMPTY
    c[88:93, 43:48] = OCCUPIED
    return c


def polyline_points(vertices=SCENE_VERTICES):
    """floor(length) points a segment, evenly spaced from its first vertex, its last excluded; the final vertex appended.
    -> [(x, y)] in cells."""
    pts = []
    for (x0, y0), (x1, y1) in zip(vertices[:-1], vertices[1:]):
        n = int(math.floor(math.hypot(x1 - x0, y1 - y0)))
        for i in range(n):
            pts.append((x0 + (x1 - x0) * i / n, y0 + (y1 - y0) * i / n))
    pts.append(tuple(vertices[-1]))
    return pts


def quantise_points(pts):
    return [round(x * 65536.0) for x, _ in pts], [round(y * 65536.0) for _, y in pts]


def scene_model():
    return Model(0, 131072, 0, 1565, 0, (mref.noise_scale(0.5 * 65536.0), 0, mref.noise_scale(500.0)))


def scene_costs():
    pen = [round(60.0 * max(0.0, 1.0 - math.sqrt(d) / 7.0)) for d in range(50)]
    wtab = [round(65535.0 * math.exp(-4.0 * i / 64.0)) for i in range(256)]
    return Costs(9, pen, 0, 4000, 8, 400 << 16, 20, wtab, 2)


def window_from(px, py, tx, ty, n=SCENE_WINDOW):
    """n points from the index closest to (tx, ty), the lowest among equals."""
    best = min(range(len(px)), key=lambda j: ((tx - px[j]) ** 2 + (ty - py[j]) ** 2, j))
    return px[best:best + n], py[best:best + n]


def closed_loop(plane, seed, K=SCENE_K, T=SCENE_T, max_steps=200, stepper=None):
    """The scene's run -> (steps taken or None, smallest d2 of an occupied cell, the cells).  stepper: what makes a
    step, this statement's by default."""
    stepper = stepper or step
    m, c = scene_model(), scene_costs()
    px, py = quantise_points(polyline_points())
    tx, ty, h = px[0], py[0], 0
    U = [(0, 0, 0)] * T
    cells, d2_min = [], FAR
    for n in range(max_steps):
        wx, wy = window_from(px, py, tx, ty)
        new, _, _ = stepper(plane, K, seed, m, c, wx, wy, tx, ty, h, U, n)
        tx, ty, h = advance(tx, ty, h, *new[0])
        U = shift(new)
        I, J = cell(tx, ty)
        cells.append((I, J))
        d2_min = min(d2_min, int(plane[I, J]))
        if (tx - px[-1]) ** 2 + (ty - py[-1]) ** 2 <= (3 << 15) ** 2:     # within 1.5 cells of the last point
            return n + 1, d2_min, cells
    return None, d2_min, cells
