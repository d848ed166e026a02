"""The world map's virtual laser scan (DESIGN.md 4.11 rules 20 to 27, include/kompass_hip.h kc_worldmap_scan) as a
literal statement in Python integers: a loop a beam, a step a turn of the loop, the box of rule 23 as the only end of a
walk, no rounds and no early exit.  A plane is an array m[I, J] of shape (W, H).  Python's >> on int is arithmetic and
its float is the IEEE double, so rule 24's one division and one product are what the operators give."""
import math

import numpy as np

from worldmap_ref import EMPTY, OCCUPIED, UNEXPLORED, quantise_pose  # noqa: F401

MAX_RADIUS = 2048
MAX_BEAMS = 65536
MAX_RAYS = 1 << 22
UNKNOWN_BLOCKS = 1


def scan_table(angles):
    """Rule 21 -> int [n, 2] of (ac_k, as_k).  round() is round-half-to-even, as lrint in the default mode."""
    out = np.zeros((len(angles), 2), np.int64)
    for k, a in enumerate(angles):
        a = float(a)
        if not math.isfinite(a):
            raise ValueError("beam angle not finite")
        out[k] = round(math.cos(a) * 1073741824.0), round(math.sin(a) * 1073741824.0)
    return out


def scan_check(resolution, n_poses, n_beams, range_max, flags=0):
    """The refusals of rules 20, 21 and 25, in the library's order -> Rc."""
    r = float(np.float32(resolution))
    m = float(np.float32(range_max))
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError("the resolution must be positive")
    if n_poses < 1 or n_beams < 1:
        raise ValueError("at least one pose and one beam")
    if n_beams > MAX_BEAMS or n_poses * n_beams > MAX_RAYS:
        raise IndexError("too many beams")
    if not (math.isfinite(m) and m > 0.0):
        raise ValueError("range_max must be a finite float > 0")
    if m / r > MAX_RADIUS:   # ceil(q) > 2048 iff q > 2048
        raise IndexError("range above 2048 cells")
    if flags & ~UNKNOWN_BLOCKS:
        raise ValueError("unknown flag bits")
    return math.ceil(m / r)


def merge(real, v):
    """Rule 27 for one beam."""
    return real if (math.isfinite(real) and real < v) else v


def scan_pose(cls, resolution, pose, table, range_max, flags=0, real=None):
    """One quantised pose (cq, sq, tx, ty) -> (ranges float64 [B], cells int32 [B])."""
    cls = np.asarray(cls)
    W, H = cls.shape
    B = len(table)
    r_res = float(np.float32(resolution))
    r_max = float(np.float32(range_max))
    Rc = scan_check(resolution, 1, B, range_max, flags)
    cq, sq, tx, ty = (int(v) for v in pose)
    X0, Y0 = tx + (1 << 15), ty + (1 << 15)
    I0, J0 = X0 >> 16, Y0 >> 16
    fx, fy = X0 & 0xFFFF, Y0 & 0xFFFF
    blocking = (OCCUPIED, UNEXPLORED) if flags & UNKNOWN_BLOCKS else (OCCUPIED,)

    def blocks(I, J):
        return 0 <= I < W and 0 <= J < H and int(cls[I, J]) in blocking

    ranges = np.empty(B, np.float64)
    cells = np.empty(B, np.int32)
    for k in range(B):
        ac, as_ = int(table[k][0]), int(table[k][1])
        dx = (cq * ac - sq * as_ + (1 << 15)) >> 16
        dy = (sq * ac + cq * as_ + (1 << 15)) >> 16
        sx, sy = (1 if dx > 0 else -1), (1 if dy > 0 else -1)
        ex = 65536 - fx if dx > 0 else fx
        ey = 65536 - fy if dy > 0 else fy
        I, J = I0, J0
        hit = None                       # (I, J, r)
        if blocks(I, J):
            hit = (I, J, 0.0)            # e = 0
        else:
            while True:
                if dy == 0:
                    along_x = True
                elif dx == 0:
                    along_x = False
                else:
                    along_x = ex * abs(dy) <= ey * abs(dx)
                if along_x:
                    e, a = ex, abs(dx)
                    I += sx
                    ex += 65536
                else:
                    e, a = ey, abs(dy)
                    J += sy
                    ey += 65536
                if abs(I - I0) > Rc + 1 or abs(J - J0) > Rc + 1:
                    break
                if blocks(I, J):
                    r = (float(e) * 16384.0 / float(a)) * r_res
                    if r <= r_max:
                        hit = (I, J, r)
                    break                # the first blocking cell decides
        v = hit[2] if hit else r_max
        if real is not None:
            v = merge(float(real[k]), v)
        ranges[k] = v
        cells[k] = hit[0] + hit[1] * W if hit else -1
    return ranges, cells


def scan(cls, resolution, origin, poses, angles, range_max, flags=0, real=None):
    """poses: a list of (x, y, yaw) -> (ranges [M, B], cells [M, B])."""
    table = scan_table(angles)
    scan_check(resolution, len(poses), len(table), range_max, flags)
    out = [scan_pose(cls, resolution, quantise_pose(resolution, origin, *p), table, range_max, flags, real) for p in poses]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
