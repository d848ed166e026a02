"""The grid planner's any-angle rules (rules 9 to 12) as a plain CPU statement beside planner_ref.py
and planner_clearance_ref.py, which supply validity, clear2 and the walks.  Written from the rules, not from the
kernel: rule 9 is evaluated with numpy over the whole bounding box of a segment (the kernel visits the up to three
cells of a column), and the selection tests every candidate of a window, far end first, one after the other (the
kernel deals them to wavefronts in rounds of 16).

Arrays are [width, height] as in planner_ref; a walk is an (n, 2) array of cells."""
import math

import numpy as np

CLEAR_FAR = 0xFFFF
MAX_SPAN = 1024


# ---- rule 9: touched cells ----------------------------------------------------------------------------------------
def touched(a, b):
    """The cells the segment a - b touches: inside the bounding box of the two cells, and 2 |dx (j - ay) - dy (i -
    ax)| <= |dx| + |dy|.  (k, 2) int64 cells, i-major order."""
    ax, ay, bx, by = int(a[0]), int(a[1]), int(b[0]), int(b[1])
    dx, dy = bx - ax, by - ay
    i = np.arange(min(ax, bx), max(ax, bx) + 1, dtype=np.int64)[:, None]
    j = np.arange(min(ay, by), max(ay, by) + 1, dtype=np.int64)[None, :]
    hit = 2 * np.abs(dx * (j - ay) - dy * (i - ax)) <= abs(dx) + abs(dy)
    ii, jj = np.nonzero(hit)
    return np.stack([ii + min(ax, bx), jj + min(ay, by)], 1)


# ---- rule 10: clear segment ---------------------------------------------------------------------------------------
def segment_clear(valid, a, b, clear2=None, m=None):
    """Every touched cell valid, and with a clearance cost (clear2 and the walk's own smallest clear2, m) none of
    them below m."""
    t = touched(a, b)
    if not np.asarray(valid, bool)[t[:, 0], t[:, 1]].all():
        return False
    return clear2 is None or bool((np.asarray(clear2)[t[:, 0], t[:, 1]] >= m).all())


def walk_min_clear2(cells, clear2):
    c = np.asarray(cells, np.int64).reshape(-1, 2)
    return int(np.asarray(clear2)[c[:, 0], c[:, 1]].min())


# ---- rule 11: selection -------------------------------------------------------------------------------------------
def select(valid, cells, max_span, clear2=None):
    """The kept indices into the walk: from s, the largest t in (s, min(n - 1, s + max_span)] whose segment is clear,
    s + 1 without a test.  Ascending, first and last present."""
    assert 1 <= max_span <= MAX_SPAN
    p = np.asarray(cells, np.int64).reshape(-1, 2)
    n = len(p)
    assert n >= 1
    m = None if clear2 is None else walk_min_clear2(p, clear2)
    keep, s = [0], 0
    while s < n - 1:
        t = min(n - 1, s + max_span)
        while t > s + 1 and not segment_clear(valid, p[s], p[t], clear2, m):
            t -= 1
        keep.append(t)
        s = t
    return keep


def select_first_failure(valid, cells, max_span, clear2=None):
    """NOT the rule: the scan that stops at the first blocked line of sight.  Kept to show the two differ."""
    p = np.asarray(cells, np.int64).reshape(-1, 2)
    n = len(p)
    m = None if clear2 is None else walk_min_clear2(p, clear2)
    keep, s = [0], 0
    while s < n - 1:
        t = s + 1
        while t + 1 <= min(n - 1, s + max_span) and segment_clear(valid, p[s], p[t + 1], clear2, m):
            t += 1
        keep.append(t)
        s = t
    return keep


# ---- rule 12: outputs ---------------------------------------------------------------------------------------------
def length_cells(kept_cells):
    """sum sqrt(dx^2 + dy^2) over consecutive kept cells, in double, in path order."""
    c = np.asarray(kept_cells, np.int64).reshape(-1, 2)
    total = 0.0
    for k in range(1, len(c)):
        dx, dy = int(c[k, 0] - c[k - 1, 0]), int(c[k, 1] - c[k - 1, 1])
        total += math.sqrt(float(dx * dx + dy * dy))
    return total


def length_metres(kept_cells, resolution):
    """resolution (the float32 the class holds) times the sum, in double, then cast to float."""
    return np.float32(float(np.float32(resolution)) * length_cells(kept_cells))


def min_touched_clear2(cells, keep, clear2):
    """The smallest clear2 over the kept cells and the touched cells of the kept segments that were tested (span >=
    2); CLEAR_FAR without a clearance field."""
    if clear2 is None:
        return CLEAR_FAR
    p = np.asarray(cells, np.int64).reshape(-1, 2)
    c = np.asarray(clear2)
    best = min(int(c[p[k, 0], p[k, 1]]) for k in keep)
    for s, t in zip(keep[:-1], keep[1:]):
        if t - s >= 2:
            q = touched(p[s], p[t])
            best = min(best, int(c[q[:, 0], q[:, 1]].min()))
    return best


def shortcut(valid, cells, max_span, clear2=None):
    """The whole statement: dict(indices, cells, count, min_clear2, length) -- length in cells."""
    p = np.asarray(cells, np.int32).reshape(-1, 2)
    keep = select(valid, p, max_span, clear2)
    kept = p[keep]
    return dict(indices=np.array(keep, np.int32), cells=kept, count=len(keep),
                min_clear2=min_touched_clear2(p, keep, clear2), length=length_cells(kept))
