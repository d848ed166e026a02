"""The world map's distance plane (DESIGN.md 4.11 rules 42 and 43, include/kompass_hip.h kc_worldmap_*distance*) as a
brute-force statement: every cell against every offset of the square of side 2 reach + 1, no row pass, no column pass,
no tile.  Planes are arrays m[I, J] of shape (W, H), as worldmap_ref's."""
import numpy as np

from worldmap_ref import OCCUPIED, UNEXPLORED

FAR = 0xFFFF
UNKNOWN_BLOCKS = 1
MAX_REACH = 254


def check(reach, flags=0, off_allowed=True):
    """kc_worldmap_set_distance's refusals, in its order.  IndexError: KC_ERR_RANGE, ValueError: KC_ERR_INVALID."""
    if not (0 if off_allowed else 1) <= reach <= MAX_REACH:
        raise IndexError("reach outside 0 .. 254")
    if flags & ~UNKNOWN_BLOCKS or (reach == 0 and flags):
        raise ValueError("unknown flag bits")


def blocking(cls, flags=0):
    c = np.asarray(cls)
    return (c == OCCUPIED) | ((c == UNEXPLORED) if flags & UNKNOWN_BLOCKS else np.zeros(c.shape, bool))


def dist2_cell(cls, I, J, reach, flags=0):
    """Rule 42 for one cell, in Python ints: a loop over the square around it."""
    c = np.asarray(cls)
    W, H = c.shape
    b = blocking(c, flags)
    best = FAR
    for bI in range(I - reach, I + reach + 1):
        for bJ in range(J - reach, J + reach + 1):
            if 0 <= bI < W and 0 <= bJ < H and b[bI, bJ]:                 # cells outside the map never block
                d2 = (bI - I) ** 2 + (bJ - J) ** 2
                if d2 <= reach * reach and d2 < best:
                    best = d2
    return best


def dist2_plane(cls, reach, flags=0):
    """Rule 42 for every cell: a loop over the offsets (di, dj) of the disc, each a shifted comparison of whole planes.
    uint16 [W, H]."""
    check(reach, flags, off_allowed=False)
    c = np.asarray(cls)
    W, H = c.shape
    b = blocking(c, flags)
    out = np.full((W, H), FAR, np.int64)
    ri, rj = min(reach, W - 1), min(reach, H - 1)
    for di in range(-ri, ri + 1):
        for dj in range(-rj, rj + 1):
            d2 = di * di + dj * dj
            if d2 > reach * reach:
                continue
            i0, i1 = max(0, -di), min(W, W - di)                          # cells (I, J) with (I + di, J + dj) inside the map
            j0, j1 = max(0, -dj), min(H, H - dj)
            seen = b[i0 + di:i1 + di, j0 + dj:j1 + dj]
            view = out[i0:i1, j0:j1]
            np.minimum(view, np.where(seen, d2, FAR), out=view)
    return out.astype(np.uint16)


class DistRef:
    """Rule 43's bookkeeping over a plane cls[I][J] that the caller changes: mark what changed, refresh before reading."""

    def __init__(self, cls, reach, flags=0):
        check(reach, flags, off_allowed=False)
        self.cls = cls
        self.W, self.H = np.asarray(cls).shape
        self.reach, self.flags = int(reach), int(flags)
        self.plane = np.zeros((self.W, self.H), np.uint16)                # never read before the first refresh
        self.dirty = None
        self.last_box = (-1, -1, -1, -1)
        self.last_full = False
        self.mark_all()                                                   # enabling marks the whole map

    def mark_all(self):
        """kc_worldmap_set_prior_*, kc_worldmap_clear, kc_worldmap_set_model."""
        self.dirty = (0, 0, self.W - 1, self.H - 1)

    def mark(self, changed, box):
        """An update's result record."""
        if changed == 0:
            return
        if self.dirty is None:
            self.dirty = tuple(int(v) for v in box)
        else:
            d = self.dirty
            self.dirty = (min(d[0], box[0]), min(d[1], box[1]), max(d[2], box[2]), max(d[3], box[3]))

    def refresh(self):
        """-> the box recomputed, or None.  The box's cells are recomputed from the cls bytes of the box grown by reach
        once more and of nothing else: the slice below is all this reads."""
        self.last_box, self.last_full = (-1, -1, -1, -1), False
        if self.dirty is None:
            return None
        R, d = self.reach, self.dirty
        x0, y0 = max(d[0] - R, 0), max(d[1] - R, 0)
        x1, y1 = min(d[2] + R, self.W - 1), min(d[3] + R, self.H - 1)
        sx0, sy0 = max(x0 - R, 0), max(y0 - R, 0)
        sx1, sy1 = min(x1 + R, self.W - 1), min(y1 + R, self.H - 1)
        sub = dist2_plane(np.asarray(self.cls)[sx0:sx1 + 1, sy0:sy1 + 1], R, self.flags)
        self.plane[x0:x1 + 1, y0:y1 + 1] = sub[x0 - sx0:x1 - sx0 + 1, y0 - sy0:y1 - sy0 + 1]
        self.dirty = None
        self.last_box = (x0, y0, x1, y1)
        self.last_full = (x0, y0, x1, y1) == (0, 0, self.W - 1, self.H - 1)
        return self.last_box

    def field(self):
        self.refresh()
        return self.plane
