"""Finding moving obstacles in a laser scan and tracking them (DESIGN.md 4.11 rules 64 to 70 and the tracker,
include/kompass_hip.h kc_worldmap_movers) as a literal statement: Python ints for the detection, a loop a beam, no
compaction and no prefix count; Python floats (IEEE doubles) for the tracker.  Written from the rules, not from the
kernels.  Rule 21's table, rule 22's direction, rule 44's endpoint, rule 52's quantiser and refusals and rules 42 and
43's plane are imported, not restated.  A plane is an array m[I, J] of shape (W, H)."""
import math
from collections import namedtuple

import numpy as np

import worldmap_dist_ref as dref
from worldmap_integrate_ref import integrate_check, quantise_ranges  # noqa: F401  (the quantiser is the callers')
from worldmap_mcl_field_ref import beam_direction, endpoint
from worldmap_ref import EMPTY, quantise_pose
from worldmap_scan_ref import scan_table

MAX_CLUSTERS = 256
MAX_GAP, MAX_JOIN_Q, MAX_MIN_BEAMS = 64, 1 << 40, 65536
# the prototype's values: judgement, not measurement
M2, GAP, JOIN_Q, MIN_BEAMS = 4, 2, 9 << 16, 3

Cluster = namedtuple("Cluster", "k_first k_last n sx sy min_x max_x min_y max_y")      # rule 68
Record = namedtuple("Record", "n_dynamic n_runs n_kept n_returned")                   # rule 69


class StateError(RuntimeError):
    """KC_ERR_STATE"""


# ---- rule 70: kc_worldmap_movers_check, in the library's order.  ValueError: KC_ERR_INVALID, IndexError: KC_ERR_RANGE ----
def movers_check(resolution, n_beams, range_max, zq=None, m2=M2, gap=GAP, join_q=JOIN_Q, min_beams=MIN_BEAMS):
    """-> ZMAX"""
    _, zmax = integrate_check(resolution, n_beams, range_max, 0, zq)
    if m2 == 0:
        raise ValueError("m2 must be at least 1")
    if gap > MAX_GAP:
        raise IndexError("gap above 64")
    if join_q > MAX_JOIN_Q:
        raise IndexError("join_q above 2^40")
    if min_beams == 0:
        raise ValueError("min_beams must be at least 1")
    if min_beams > MAX_MIN_BEAMS:
        raise IndexError("min_beams above 65536")
    return zmax


# ---- rule 65 ----
def endpoint_q(pose, t, zq):
    """Rule 44's (EX, EY) themselves; worldmap_mcl_field_ref.endpoint gives their cells and is asserted equal."""
    cq, sq, tx, ty = (int(v) for v in pose)
    dx, dy = beam_direction(cq, sq, int(t[0]), int(t[1]))
    ex = tx + (1 << 15) + ((zq * dx + (1 << 29)) >> 30)
    ey = ty + (1 << 15) + ((zq * dy + (1 << 29)) >> 30)
    assert (ex >> 16, ey >> 16) == endpoint(tx, ty, dx, dy, zq)
    return ex, ey


# ---- rules 65 to 69 ----
def detect(cls, plane, reach, resolution, pose, angles, zq, range_max, m2=M2, gap=GAP, join_q=JOIN_Q, min_beams=MIN_BEAMS):
    """cls: int8 [W, H]; plane: the refreshed uint16 [W, H] distance plane, or None while it is off; reach: the plane's;
    pose: the quantised (cq, sq, tx, ty).  -> (labels int32 [B], Record, [Cluster], the first n_returned)."""
    if len(zq) != len(angles):
        raise ValueError("one quantised range a beam")
    zmax = movers_check(resolution, len(angles), range_max, zq, m2, gap, join_q, min_beams)
    table = scan_table(angles)
    if plane is None or reach == 0:
        raise StateError("the map's distance plane is off")
    if m2 > reach * reach:
        raise StateError("m2 above the plane's reach^2")
    cls = np.asarray(cls)
    W, H = cls.shape
    B = len(table)
    ends = [None] * B
    dynamic = []                                                          # rule 66, in scan order
    for k in range(B):
        z = int(zq[k])
        if not 0 <= z < zmax:
            continue
        ex, ey = endpoint_q(pose, table[k], z)
        ends[k] = (ex, ey)
        I, J = ex >> 16, ey >> 16
        if 0 <= I < W and 0 <= J < H and int(cls[I, J]) == EMPTY and int(plane[I, J]) > m2:
            dynamic.append(k)
    runs = []                                                             # rule 67: lists of beams
    for n, k in enumerate(dynamic):
        if n > 0:
            p = dynamic[n - 1]
            q = ((ends[k][0] - ends[p][0]) >> 8) ** 2 + ((ends[k][1] - ends[p][1]) >> 8) ** 2
            if k - p <= gap + 1 and q <= join_q:
                runs[-1].append(k)
                continue
        runs.append([k])
    labels = np.full(B, -1, np.int32)
    clusters = []
    for run in runs:                                                      # rule 68
        if len(run) < min_beams:
            labels[run] = -2
            continue
        labels[run] = len(clusters)
        xs, ys = [ends[k][0] for k in run], [ends[k][1] for k in run]
        clusters.append(Cluster(run[0], run[-1], len(run), sum(xs), sum(ys), min(xs), max(xs), min(ys), max(ys)))
    rec = Record(len(dynamic), len(runs), len(clusters), min(len(clusters), MAX_CLUSTERS))
    return labels, rec, clusters[:MAX_CLUSTERS]


class MoversRef:
    """detect() over a map statement: `world` has cls, resolution and origin (a worldmap_ref.WorldMapRef or an
    IntegrateRef), `dist` is a worldmap_dist_ref.DistRef over world.cls or None; the plane is refreshed first (rule 43)."""

    def __init__(self, world, dist):
        self.world, self.dist = world, dist

    def detect(self, pose, angles, zq, range_max, **cfg):
        q = pose if len(pose) == 4 else quantise_pose(self.world.resolution, self.world.origin, *pose)
        if self.dist is None:
            return detect(self.world.cls, None, 0, self.world.resolution, q, angles, zq, range_max, **cfg)
        movers_check(self.world.resolution, len(angles), range_max, zq if len(zq) == len(angles) else None, **cfg)
        if cfg.get("m2", M2) > self.dist.reach ** 2:
            raise StateError("m2 above the plane's reach^2")             # before the refresh: a refused call queues nothing
        return detect(self.world.cls, self.dist.field(), self.dist.reach, self.world.resolution, q, angles, zq, range_max, **cfg)


# ---- the front ends' geometry, in cells: 4.12 rule 1 puts cell I's centre at TX = I << 16, rule 65's EX at (I << 16) + 2^15 ----
def cluster_centre_q(c):
    """The cluster's centre in 4.12's Q16 coordinates, as doubles: (SX / n - 32768, SY / n - 32768)."""
    return c.sx / c.n - 32768.0, c.sy / c.n - 32768.0


def cluster_radius_q(c):
    """Half the longer side of the endpoints' box, in 2^-16 cells.  Points on a rim of radius r span at most 2 r along an
    axis, so this never passes r but by the endpoints' rounding; half the box's diagonal can, by up to sqrt(2)."""
    return max(c.max_x - c.min_x, c.max_y - c.min_y) / 2.0


def cluster_world(c, resolution, origin):
    """-> (x, y, radius) in metres: origin + ((SX / n) - 32768) / 65536 * res, radius as above."""
    r = float(np.float32(resolution))
    cx, cy = cluster_centre_q(c)
    return origin[0] + cx / 65536.0 * r, origin[1] + cy / 65536.0 * r, cluster_radius_q(c) / 65536.0 * r


def skip_mask(labels):
    """The member beams of every kept cluster."""
    return np.asarray(labels) >= 0


def apply_skip(zq, mask):
    """Rule 54's `says nothing` for the masked beams."""
    out = np.array(zq, np.int32)
    out[np.asarray(mask, bool)] = -1
    return out


# ---- the tracker: host only, in doubles ----
ALPHA, BETA, MAX_MISSES, GATE = 0.5, 0.3, 3, 6.0   # the prototype's values: judgement, not measurement


class Track:
    __slots__ = ("id", "x", "y", "vx", "vy", "radius", "hits", "misses")

    def __init__(self, id_, x, y, radius):
        self.id, self.x, self.y, self.vx, self.vy, self.radius, self.hits, self.misses = id_, x, y, 0.0, 0.0, radius, 1, 0


class MoverTracker:
    """Tracks in creation order with increasing ids.  update() takes [(x, y, radius)] in any one length unit and dt > 0;
    gate is in that unit."""

    def __init__(self, alpha=ALPHA, beta=BETA, max_misses=MAX_MISSES, gate=GATE):
        self.alpha, self.beta, self.max_misses, self.gate = float(alpha), float(beta), int(max_misses), float(gate)
        self.tracks = []
        self.next_id = 0

    def update(self, clusters, dt):
        dt = float(dt)
        if not dt > 0.0:
            raise ValueError("dt must be positive")
        used = [False] * len(clusters)
        kept = []
        for tr in self.tracks:
            px, py = tr.x + tr.vx * dt, tr.y + tr.vy * dt
            best, best_d = -1, 0.0
            for i, (zx, zy, _) in enumerate(clusters):
                if used[i]:
                    continue
                d = math.hypot(zx - px, zy - py)
                if d <= self.gate and (best < 0 or d < best_d):           # the lowest index among equals
                    best, best_d = i, d
            if best < 0:
                tr.x, tr.y = px, py                                       # coasts
                tr.misses += 1
                if tr.misses <= self.max_misses:
                    kept.append(tr)
                continue
            used[best] = True
            zx, zy, zr = clusters[best]
            if tr.hits == 1:                                              # the two-point start
                tr.vx, tr.vy = (zx - tr.x) / dt, (zy - tr.y) / dt
                tr.x, tr.y = zx, zy
            else:
                rx, ry = zx - px, zy - py
                tr.x, tr.y = px + self.alpha * rx, py + self.alpha * ry
                tr.vx, tr.vy = tr.vx + self.beta / dt * rx, tr.vy + self.beta / dt * ry
            tr.radius = max(tr.radius, zr)
            tr.hits += 1
            tr.misses = 0
            kept.append(tr)
        self.tracks = kept
        for i, (zx, zy, zr) in enumerate(clusters):                       # unmatched clusters, in cluster order
            if not used[i]:
                self.tracks.append(Track(self.next_id, float(zx), float(zy), float(zr)))
                self.next_id += 1

    def moving_obstacles(self):
        """[(x, y, vx, vy, radius)], a row a live track."""
        return [(t.x, t.y, t.vx, t.vy, t.radius) for t in self.tracks]


# ---- a simulated scan: the static scene's ranges shortened by discs ----
def shorten_by_discs(ranges, resolution, pose, angles, discs):
    """ranges: metres a beam (worldmap_scan_ref.scan_pose's); pose: the quantised (cq, sq, tx, ty); discs: [(OX, OY, r)] with
    the centre in 4.12's Q16 coordinates and r in cells.  A beam's range becomes the nearer of its own and the first
    crossing of a disc's rim along rule 22's direction u = (dx, dy) / 2^30, whose length is 1 only to about 2^-16: the
    crossing is the smaller root s of |s u - w|^2 = r^2, so that rule 44's endpoint lies on the rim up to its own
    rounding.  Doubles: this makes test input, it is not a rule."""
    r_res = float(np.float32(resolution))
    cq, sq, tx, ty = (int(v) for v in pose)
    out = np.array(ranges, np.float64)
    for k, t in enumerate(scan_table(angles)):
        dx, dy = beam_direction(cq, sq, int(t[0]), int(t[1]))
        ux, uy = dx / 1073741824.0, dy / 1073741824.0
        a = ux * ux + uy * uy
        for ox, oy, r in discs:
            wx, wy = (ox - tx) / 65536.0, (oy - ty) / 65536.0
            b = wx * ux + wy * uy
            disc = b * b - a * (wx * wx + wy * wy - r * r)
            if disc < 0.0:
                continue
            s = (b - math.sqrt(disc)) / a
            if s > 0.0 and s * r_res < out[k]:
                out[k] = s * r_res
    return out
