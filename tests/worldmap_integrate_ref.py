"""The world map's scan integration (DESIGN.md 4.11 rules 52 to 56, include/kompass_hip.h kc_worldmap_integrate) as a
literal statement in Python integers: a loop a beam, a step a turn of the loop, rule 23's box as the only end of a walk,
q_s by its division.  Written from the rules, not from the kernel, which tests the product form and never the box.
A plane is an array m[I, J] of shape (W, H).  Rule 5 and rule 6 are worldmap_ref's."""
import math

import numpy as np

from worldmap_ref import EMPTY, OCCUPIED, WorldMapRef, quantise_pose
from worldmap_scan_ref import MAX_BEAMS, MAX_RADIUS, scan_table

CLEAR_NO_RETURN = 1
MISS, HIT = 1, 2  # the bits of a mark byte


def integrate_check(resolution, n_beams, range_max, flags=0, zq=None):
    """Rule 52's refusals in their order: counts, range_max, flags, zq -> (Rc, ZMAX)."""
    r = float(np.float32(resolution))
    m = float(np.float32(range_max))
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError("the resolution must be positive")
    if n_beams < 1:
        raise ValueError("at least one beam")
    if n_beams > MAX_BEAMS:
        raise IndexError("too many beams")
    if not (math.isfinite(m) and m > 0.0):
        raise ValueError("range_max must be a finite float > 0")
    if m / r > MAX_RADIUS:   # ceil(q) > 2048 iff q > 2048
        raise IndexError("range above 2048 cells")
    if flags & ~CLEAR_NO_RETURN:
        raise ValueError("unknown flag bits")
    zmax = round(m / r * 65536.0)
    if zq is not None:
        for z in zq:
            if not -1 <= int(z) <= zmax:
                raise ValueError("quantised range outside -1 .. ZMAX")
    return math.ceil(m / r), zmax


def quantise_ranges(ranges, resolution, range_max, range_min=0.0):
    """Rule 52 -> int32 [B].  round() is round-half-to-even, as llrint in the default mode."""
    r = float(np.float32(resolution))
    m = float(np.float32(range_max))
    lo = float(np.float32(range_min))
    _, zmax = integrate_check(resolution, len(ranges), range_max)
    out = []
    for z in ranges:
        z = float(z)
        if math.isnan(z) or z < 0.0 or z < lo:
            out.append(-1)
        elif z == math.inf or z >= m:
            out.append(zmax)
        else:
            out.append(round(z / r * 65536.0))
    return np.array(out, np.int32)


def walk(pose, t, Rc):
    """Rule 23 from the start cell -> [(I, J, q)]: the start cell with q = 0, then every step cell inside the box Rc + 1
    with q_s = floor(e_s 2^30 / a_s), and last the step that leaves the box, which the caller must not cross."""
    cq, sq, tx, ty = (int(v) for v in pose)
    ac, as_ = int(t[0]), int(t[1])
    X0, Y0 = tx + (1 << 15), ty + (1 << 15)
    I0, J0 = X0 >> 16, Y0 >> 16
    fx, fy = X0 & 0xFFFF, Y0 & 0xFFFF
    dx = (cq * ac - sq * as_ + (1 << 15)) >> 16
    dy = (sq * ac + cq * as_ + (1 << 15)) >> 16
    sx, sy = (1 if dx > 0 else -1), (1 if dy > 0 else -1)
    ex = 65536 - fx if dx > 0 else fx
    ey = 65536 - fy if dy > 0 else fy
    I, J = I0, J0
    out = [(I, J, 0)]
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
        out.append((I, J, (e << 30) // a))
        if abs(I - I0) > Rc + 1 or abs(J - J0) > Rc + 1:
            return out


def crossed(pose, t, Rc, z, zmax):
    """Rule 53: the cells a beam with limit z crosses, in the walk's order."""
    cells = walk(pose, t, Rc)
    qs = [q for _, _, q in cells]
    assert all(b >= a for a, b in zip(qs, qs[1:])), "q decreased along a walk"
    assert qs[-1] > zmax, "rule 23's box cut a crossing"
    return [(I, J) for I, J, q in cells[:-1] if q <= z]


def mark_plane(W, H, pose, table, zq, Rc, zmax, flags=0):
    """Rules 53 and 54 -> uint8 [W, H]."""
    marks = np.zeros((W, H), np.uint8)

    def mark(cell, bit):
        if 0 <= cell[0] < W and 0 <= cell[1] < H:
            marks[cell] |= bit

    for k in range(len(table)):
        z = int(zq[k])
        if z < 0 or (z == zmax and not flags & CLEAR_NO_RETURN):
            continue
        cells = crossed(pose, table[k], Rc, z, zmax)
        if z < zmax:
            mark(cells[-1], HIT)
            cells = cells[:-1]
        for c in cells:
            mark(c, MISS)
    return marks


class IntegrateRef(WorldMapRef):
    """A WorldMapRef that also integrates scans.  apply() hands update() rule 55's reading of a mark plane in the place of
    rule 4's observation, so rules 5 and 6 are worldmap_ref's, unchanged; an update of a local grid stays what it was."""
    _reading_marks = False

    def observe(self, local, qpose, c=None):
        if not self._reading_marks:
            return super().observe(local, qpose, c)
        m = np.asarray(local)
        obs = np.where(m & HIT, OCCUPIED, np.where(m & MISS, EMPTY, -1)).astype(np.int64)   # a hit beats a miss
        return obs, m != 0

    def apply(self, marks):
        """Rules 55, 5 and 6 for one mark plane -> (changed, (i_min, j_min, i_max, j_max))."""
        self._reading_marks = True
        try:
            return self.update(marks, (65536, 0, 0, 0))
        finally:
            self._reading_marks = False

    def marks(self, pose, angles, zq, range_max, flags=0):
        """pose: (x, y, yaw) or the quantised (cq, sq, tx, ty) -> (the mark plane, the quantised pose)"""
        q = pose if len(pose) == 4 else quantise_pose(self.resolution, self.origin, *pose)
        if len(zq) != len(angles):
            raise ValueError("one quantised range a beam")
        Rc, zmax = integrate_check(self.resolution, len(angles), range_max, flags, zq)
        return mark_plane(self.W, self.H, q, scan_table(angles), zq, Rc, zmax, flags), q

    def integrate(self, pose, angles, zq, range_max, flags=0):
        """-> (marks, changed, (i_min, j_min, i_max, j_max)); the planes are updated in place."""
        marks, _ = self.marks(pose, angles, zq, range_max, flags)
        changed, box = self.apply(marks)
        return marks, changed, box
