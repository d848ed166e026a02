"""Hand-made inputs for rules 64 to 69 with their answers worked out by hand, shared by the CPU test (statement against
the answers) and the GPU test (device against statement and answers).  A case is a dict: cls, reach, pose (quantised),
angles, zq, range_max, cfg, and `labels`, the expected labels, where they are known without the statement.

A beam is aimed at a cell's centre by its angle atan2(dj, di) and its range hypot(di, dj): the endpoint then lies
within 2^-10 cells of the centre, half a cell from every edge, so its cell is certain.  Where the endpoint itself must be
exact (rule 67's q), the pose's yaw is 0 and the beam's angle 0: dx = 2^30, dy = 0, EX = TX + 2^15 + zq to the unit."""
import math

import numpy as np

from worldmap_ref import EMPTY, OCCUPIED, UNEXPLORED

CELL = 65536
RES = 0.05
R32 = float(np.float32(RES))


def centre_pose(i, j, yaw=0.0):
    return round(math.cos(yaw) * 65536.0), round(math.sin(yaw) * 65536.0), round(i * CELL), round(j * CELL)


def aim(pose_cell, yaw, cell):
    """-> (angle in the scan frame, zq) of a beam from the centre of pose_cell to the centre of cell"""
    di, dj = cell[0] - pose_cell[0], cell[1] - pose_cell[1]
    return math.atan2(dj, di) - yaw, round(math.hypot(di, dj) * CELL)


def zmax_of(cells):
    return round(float(np.float32(R32 * cells)) / R32 * 65536.0)


# ---- rule 66 on a 24 x 16 map, reach 4, m2 = 4 ----
def rule66_case():
    W, H = 24, 16
    cls = np.full((W, H), EMPTY, np.int8)
    cls[12, 8] = OCCUPIED
    cls[6, 12] = UNEXPLORED
    start, yaw = (2, 8), 0.3
    rmax_cells = 30
    zmax = zmax_of(rmax_cells)
    targets = [((12, 8), False),     # an occupied cell
               ((6, 12), False),     # a never-observed one: new territory, not motion
               ((6, 4), True),       # empty, nothing within reach: FAR counts as above m2
               ((10, 8), False),     # empty at dist2 = 4 == m2
               ((10, 9), True),      # empty at dist2 = 5 == m2 + 1
               ((23, 15), True),     # the map's last column and row
               ((24, 15), False),    # one cell outside, along I
               ((23, 16), False),    # and along J
               ((-1, 8), False)]     # and below zero
    beams = [aim(start, yaw, c) for c, _ in targets]
    angles = [a for a, _ in beams] + [0.1, 0.2, 0.4]
    zq = [z for _, z in beams] + [-1, 0, zmax]      # says nothing; the start cell itself (empty, far); no return
    dyn = [d for _, d in targets] + [False, True, False]
    labels, n = [], 0
    for d in dyn:                                    # min_beams 1, gap 0, join_q 0: every dynamic beam is a cluster
        labels.append(n if d else -1)
        n += 1 if d else 0
    # (the dynamic beams here are never neighbours with equal endpoints, so join_q = 0 joins none of them)
    return dict(cls=cls, reach=4, pose=centre_pose(*start, yaw), angles=np.array(angles), zq=np.array(zq, np.int32),
                range_max=float(np.float32(R32 * rmax_cells)), cfg=dict(m2=4, gap=0, join_q=0, min_beams=1),
                labels=np.array(labels, np.int32))


# ---- rule 67 and 68 on an open 64 x 16 map: every endpoint along row 8 from cell (2, 8) is dynamic ----
def _open_row(zq, cfg, labels):
    cls = np.full((64, 16), EMPTY, np.int8)
    return dict(cls=cls, reach=3, pose=centre_pose(2, 8), angles=np.zeros(len(zq)), zq=np.array(zq, np.int32),
                range_max=float(np.float32(R32 * 60)), cfg=cfg, labels=np.array(labels, np.int32))


def rule67_cases():
    out = {}
    z0 = 10 * CELL
    gap = 2
    # an index gap of exactly gap + 1 continues the run; of gap + 2 starts another
    out["gap_plus_1"] = _open_row([z0, -1, -1, z0 + 100, z0 + 200], dict(m2=4, gap=gap, join_q=9 << 16, min_beams=1),
                                  [0, -1, -1, 0, 0])
    out["gap_plus_2"] = _open_row([z0, -1, -1, -1, z0 + 100, z0 + 200], dict(m2=4, gap=gap, join_q=9 << 16, min_beams=1),
                                  [0, -1, -1, -1, 1, 1])
    # q: the endpoints differ by 769 * 256 units along x and by nothing along y, q = 769^2; join_q at q and one below
    d = 769 * 256
    out["q_eq_join_q"] = _open_row([z0, z0 + d], dict(m2=4, gap=0, join_q=769 * 769, min_beams=1), [0, 0])
    out["q_eq_join_q_plus_1"] = _open_row([z0, z0 + d], dict(m2=4, gap=0, join_q=769 * 769 - 1, min_beams=1), [0, 1])
    # the shift is arithmetic: a step backwards of 769 * 256 - 255 units gives (-d + 255) >> 8 = -769 as well
    out["q_backwards"] = _open_row([z0 + d, z0 + 255], dict(m2=4, gap=0, join_q=769 * 769 - 1, min_beams=1), [0, 1])
    # a run of min_beams is kept, one of min_beams - 1 dropped (-2); kept clusters are numbered without the dropped
    out["min_beams"] = _open_row([z0, z0, -1, z0, z0, z0, -1, z0, z0, z0, z0], dict(m2=4, gap=0, join_q=0, min_beams=3),
                                 [-2, -2, -1, 0, 0, 0, -1, 1, 1, 1, 1])
    return out


# ---- patterns for the kernels' own edges: a 48 x 48 room, the sensor in its middle, reach 4 ----
def room_cls(side=48):
    c = np.full((side, side), EMPTY, np.int8)
    c[0, :] = c[-1, :] = c[:, 0] = c[:, -1] = OCCUPIED
    return c


def pattern_case(n_beams, seed, knock=0.25, jump=0.05, cfg=None, pose_cell=(24.0, 24.0), yaw=0.7):
    """n_beams over the full circle at 10 cells + 3 sin(5 a): neighbours lie close, so runs are long; `knock` of them say
    nothing (gaps of every length), `jump` of them stand 6 cells further out (rule 67's distance test splits there)."""
    rng = np.random.default_rng(seed)
    a = -math.pi + 0.013 + np.arange(n_beams) * (2 * math.pi / n_beams)
    r = 10.0 + 3.0 * np.sin(5.0 * a)
    r[rng.random(n_beams) < jump] += 6.0
    zq = np.rint(r * CELL).astype(np.int32)
    zq[rng.random(n_beams) < knock] = -1
    return dict(cls=room_cls(), reach=4, pose=centre_pose(*pose_cell, yaw), angles=a, zq=zq,
                range_max=float(np.float32(R32 * 40)), cfg=cfg or dict(m2=4, gap=2, join_q=9 << 16, min_beams=3), labels=None)


def alternating_case(n_beams=1024):
    """every other beam dynamic, gap 0, min_beams 1: n / 2 clusters of one beam each"""
    c = pattern_case(n_beams, 0, knock=0.0, jump=0.0, cfg=dict(m2=4, gap=0, join_q=9 << 16, min_beams=1))
    c["zq"][1::2] = -1
    lab = np.full(n_beams, -1, np.int32)
    lab[0::2] = np.arange((n_beams + 1) // 2)
    c["labels"] = lab
    return c
