"""The world map's correlative match (DESIGN.md 4.11 rules 9 to 15, include/kompass_hip.h kc_worldmap_match_*) as a
literal numpy statement: int64 arithmetic, every candidate of the window against every point, map bounds tested per
landing cell, no scratch plane, no chunks.  Written from the rules, not from the kernels.
Planes are arrays m[I, J] of shape (W, H); a local grid is g[i, j] of shape (gh, gw), as in worldmap_ref.py."""
import math
from collections import namedtuple

import numpy as np

import worldmap_ref as ref

MAX_YAW, MAX_REACH, MAX_SIDE = 31, 31, 8192

Match = namedtuple("Match", "k u v score score_guess points pose")   # pose: the corrected (cq, sq, tx, ty)


def check_window(n_yaw, yaw_step, reach):
    """Rule 10's ranges; raises ValueError."""
    if not (0 <= int(n_yaw) <= MAX_YAW) or not (0 <= int(reach) <= MAX_REACH):
        raise ValueError("n_yaw and reach must be in 0 .. 31")
    if not (math.isfinite(yaw_step) and yaw_step >= 0.0):
        raise ValueError("yaw_step must be finite and >= 0")


def rotations(yaw, n_yaw, yaw_step):
    """Rule 10: [(Cq_k, Sq_k) for k = -K .. K]; round() is round-half-to-even, as lrint in the default mode."""
    out = []
    for k in range(-n_yaw, n_yaw + 1):
        yk = yaw + float(k) * yaw_step
        out.append((round(math.cos(yk) * 65536.0), round(math.sin(yk) * 65536.0)))
    return out


def points(local, c=None):
    """Rule 9: (a, b) int64 arrays of the cells that hold 100."""
    local = np.asarray(local)
    c0, c1 = ref.central(*local.shape) if c is None else c
    i, j = np.nonzero(local == ref.OCCUPIED)
    return i.astype(np.int64) - c0, j.astype(np.int64) - c1


def weights(cls):
    """Rule 12 over the map itself: uint8 [W, H]."""
    occ = np.asarray(cls) == ref.OCCUPIED
    W, H = occ.shape
    pad = np.zeros((W + 2, H + 2), bool)   # a cell outside the map is nobody's neighbour
    pad[1:-1, 1:-1] = occ
    at = lambda di, dj: pad[1 + di:1 + di + W, 1 + dj:1 + dj + H]   # noqa: E731
    orth = at(1, 0) | at(-1, 0) | at(0, 1) | at(0, -1)
    diag = at(1, 1) | at(1, -1) | at(-1, 1) | at(-1, -1)
    return np.where(occ, 3, np.where(orth, 2, np.where(diag, 1, 0))).astype(np.uint8)


def table(cls, local, qpose, rot, reach, c=None):
    """Rules 11 to 13: the scores, uint32 [2K+1, 2S+1, 2S+1] indexed [k + K, v + S, u + S]."""
    w = weights(cls).astype(np.int64)
    W, H = w.shape
    a, b = points(local, c)
    _, _, tx, ty = (int(x) for x in qpose)
    S = int(reach)
    T = 2 * S + 1
    out = np.zeros((len(rot), T, T), np.int64)
    u = np.arange(-S, S + 1, dtype=np.int64)[None, None, :]
    v = np.arange(-S, S + 1, dtype=np.int64)[None, :, None]
    step = max(1, (1 << 22) // (T * T))     # points at a time: memory only, sums of integers do not care
    for r, (cq, sq) in enumerate(rot):
        X = tx + int(cq) * a - int(sq) * b
        Y = ty + int(sq) * a + int(cq) * b
        I0 = (X + (1 << 15)) >> 16      # numpy's >> on int64 is arithmetic
        J0 = (Y + (1 << 15)) >> 16
        for lo in range(0, len(a), step):
            I = I0[lo:lo + step, None, None] + u          # [point, v + S, u + S]
            J = J0[lo:lo + step, None, None] + v
            ok = (I >= 0) & (I < W) & (J >= 0) & (J < H)
            out[r] += np.where(ok, w[np.where(ok, I, 0), np.where(ok, J, 0)], 0).sum(axis=0)
    assert out.max(initial=0) < (1 << 32)
    return out.astype(np.uint32)


def winner(scores):
    """Rule 14 on a table [2K+1, 2S+1, 2S+1]: (k, u, v) of the largest score, the smallest (u*u + v*v, |k|, k, v, u)
    among equals."""
    scores = np.asarray(scores)
    K, S = scores.shape[0] // 2, scores.shape[1] // 2
    best = None
    for k in range(-K, K + 1):
        for v in range(-S, S + 1):
            for u in range(-S, S + 1):
                key = (-int(scores[k + K, v + S, u + S]), u * u + v * v, abs(k), k, v, u)
                if best is None or key < best:
                    best = key
    return best[3], best[5], best[4]


def winner_fast(scores):
    """winner() without the Python loop, for the large tables: the same order through one integer key."""
    scores = np.asarray(scores).astype(np.int64)
    K, S = scores.shape[0] // 2, scores.shape[1] // 2
    k = np.arange(-K, K + 1, dtype=np.int64)[:, None, None]
    v = np.arange(-S, S + 1, dtype=np.int64)[None, :, None]
    u = np.arange(-S, S + 1, dtype=np.int64)[None, None, :]
    tie = ((((u * u + v * v) * 64 + np.abs(k)) * 128 + (k + 64)) * 128 + (v + 64)) * 128 + (u + 64)
    lim = int(tie.max()) + 1
    key = scores * lim + (lim - 1 - tie)
    r, vi, ui = np.unravel_index(int(np.argmax(key)), key.shape)
    return int(r) - K, int(ui) - S, int(vi) - S


def match(cls, local, qpose, rot, reach, c=None):
    """Rules 9 to 15 -> (Match, table)."""
    t = table(cls, local, qpose, rot, reach, c)
    K, S = len(rot) // 2, int(reach)
    k, u, v = winner_fast(t)
    _, _, tx, ty = (int(x) for x in qpose)
    cq, sq = rot[k + K]
    n = int(len(points(local, c)[0]))
    return Match(k, u, v, int(t[k + K, v + S, u + S]), int(t[K, S, S]), n,
                 (int(cq), int(sq), tx + (u << 16), ty + (v << 16))), t


def match_pose(world, local, pose, n_yaw, yaw_step, reach, c=None):
    """The same from a WorldMapRef and a guess (x, y, yaw) -> (Match, table, (x, y, yaw) corrected as rule 15 says)."""
    check_window(n_yaw, yaw_step, reach)
    x, y, yaw = (float(p) for p in pose)
    q = ref.quantise_pose(world.resolution, world.origin, x, y, yaw)
    m, t = match(world.cls, local, q, rotations(yaw, n_yaw, yaw_step), reach, c)
    R = world.resolution
    return m, t, (x + m.u * R, y + m.v * R, yaw + float(m.k) * yaw_step)


def gather(world, pose, gh, gw, c=None):
    """Rule 4's gather of the cls plane: the local grid a mapper at `pose` would hand out if it saw the map itself
    (cells that fall outside the map are -1)."""
    q = ref.quantise_pose(world.resolution, world.origin, *pose)
    c0, c1 = ref.central(gh, gw) if c is None else c
    local = np.full((gh, gw), -1, np.int32)
    idx = np.arange(gh * gw).reshape(gh, gw)
    obs, seen = world.observe(idx, q, (c0, c1))
    I, J = np.nonzero(seen)
    local.ravel()[obs[I, J]] = world.cls[I, J]
    return local


def recovery_world():
    """The scene of the recovery test (issue / DESIGN.md 4.11): 120 x 90 cells at 0.05 m, origin (0, 0)."""
    w = ref.WorldMapRef(120, 90, 0.05, (0.0, 0.0))
    g = np.zeros((120, 90), np.int8)
    g[:5, :] = -1
    g[111:, :] = -1
    g[5, 5:80] = 100
    g[110, 5:80] = 100
    g[5:111, 5] = 100
    g[5:111, 79] = 100
    g[30:40, 30:36] = 100
    g[70:74, 50:70] = 100
    g[50, 5:25] = 100
    w.set_prior(g)
    return w


def recovery_draws(n=12):
    """[(true pose, guess, (k0, u0, v0))], the draws in the order the issue gives, step = radians(1)."""
    rng = np.random.default_rng(1)
    R, step = float(np.float32(0.05)), math.radians(1.0)
    out = []
    for _ in range(n):
        px = rng.uniform(1.5, 4.5)
        py = rng.uniform(1.0, 3.0)
        yaw = rng.uniform(-math.pi, math.pi)
        k0 = int(rng.integers(-4, 5))
        u0 = int(rng.integers(-5, 6))
        v0 = int(rng.integers(-5, 6))
        out.append(((px, py, yaw), (px - u0 * R, py - v0 * R, yaw - k0 * step), (k0, u0, v0)))
    return out
