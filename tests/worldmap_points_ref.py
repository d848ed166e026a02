"""The world map's obstacle list (DESIGN.md 4.11 rules 16 to 19, include/kompass_hip.h kc_worldmap_points) as a literal
numpy statement: int64 over ALL cells of the map, no window box.  A plane is an array m[I, J] of shape (W, H)."""
import math

import numpy as np

from worldmap_ref import OCCUPIED, quantise_pose

MAX_RADIUS = 2048


def window(resolution, origin, x, y, max_sensor_range):
    """Rule 16 -> (Ic, Jc, Rc).  ValueError / IndexError where the library gives KC_ERR_INVALID / KC_ERR_RANGE."""
    r = float(np.float32(resolution))
    m = float(np.float32(max_sensor_range))
    if not (math.isfinite(m) and m > 0.0):
        raise ValueError("max_sensor_range must be a finite float > 0")
    if not all(math.isfinite(v) for v in (origin[0], origin[1], x, y)) or not (math.isfinite(r) and r > 0.0):
        raise ValueError("the position, the origin and the resolution must be finite")
    _, _, tx, ty = quantise_pose(r, origin, x, y, 0.0)
    if m / r > MAX_RADIUS:   # ceil(q) > 2048 iff q > 2048
        raise IndexError("radius above 2048 cells")
    rc = math.ceil(m / r)
    return (tx + (1 << 15)) >> 16, (ty + (1 << 15)) >> 16, rc   # Python's >> on int is arithmetic: floor


def cell_points(resolution, origin, I, J):
    """Rule 18 for index arrays I, J -> float32 [n, 3]: product and sum each rounded once in double."""
    r = np.float64(np.float32(resolution))
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    pts = np.zeros((len(I), 3), np.float32)
    pts[:, 0] = (np.float64(origin[0]) + I.astype(np.float64) * r).astype(np.float32)
    pts[:, 1] = (np.float64(origin[1]) + J.astype(np.float64) * r).astype(np.float32)
    return pts


def worldmap_points_ref(cls, resolution, origin, x, y, max_sensor_range):
    """cls[I, J]: the map's class plane.  -> (xyz float32 [n, 3] sorted by (J, I), n, (i_min, i_max, j_min, j_max)),
    the bounds all -1 when n == 0."""
    cls = np.asarray(cls)
    W, H = cls.shape
    ic, jc, rc = window(resolution, origin, x, y, max_sensor_range)
    I = np.arange(W, dtype=np.int64)[:, None]
    J = np.arange(H, dtype=np.int64)[None, :]
    counts = (cls == OCCUPIED) & ((I - ic) ** 2 + (J - jc) ** 2 <= np.int64(rc) ** 2)
    jj, ii = np.nonzero(counts.T)   # row-major walk of the transpose: J ascending, then I
    n = len(ii)
    if n == 0:
        return np.zeros((0, 3), np.float32), 0, (-1, -1, -1, -1)
    return cell_points(resolution, origin, ii, jj), n, (int(ii.min()), int(ii.max()), int(jj.min()), int(jj.max()))


def sort_points(xyz, resolution, origin):
    """A list in any order -> the statement's order.  Rule 18 is monotone, not strictly: two cells could share a float,
    so the order is taken from the cell indices recovered from the coordinates, which the caller's comparison then
    checks bit for bit."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    r = float(np.float32(resolution))
    ii = np.rint((xyz[:, 0].astype(np.float64) - origin[0]) / r).astype(np.int64)
    jj = np.rint((xyz[:, 1].astype(np.float64) - origin[1]) / r).astype(np.int64)
    return xyz[np.lexsort((ii, jj))]
