"""The rolling window's rules (DESIGN.md 4.11 rules 46 to 50, include/kompass_hip.h kc_worldmap_shift and its kin) as a
literal numpy statement.  It composes the statements of the map's other rules -- worldmap_ref (update), worldmap_dist_ref
(distance plane), worldmap_scan_ref (virtual scan), worldmap_points_ref (obstacle list), worldmap_mcl_ref (localiser) --
and edits none of them.  Planes are arrays m[I, J] of shape (W, H), as there."""
import numpy as np

import worldmap_dist_ref as dref
import worldmap_mcl_ref as mref
import worldmap_points_ref as pref
import worldmap_ref as wref
import worldmap_scan_ref as sref

MAX_SHIFT = 1 << 30  # rule 46's cap on |OI| and |OJ|


def origin_after(ox0, r, OI):
    """Rule 46 for one axis: the origin given at creation plus OI cells of the float32 resolution r widened to double;
    one product and one sum, never accumulated."""
    return float(ox0) + float(int(OI)) * float(np.float32(r))


def check_offset(OI, OJ, di, dj):
    """Rule 46's refusal: the offset a shift would leave."""
    if abs(int(OI) + int(di)) > MAX_SHIFT or abs(int(OJ) + int(dj)) > MAX_SHIFT:
        raise IndexError("offset above 2^30 cells")


def shift_plane(plane, di, dj, fill):
    """Rule 47 for one plane: P'[I, J] = P[I + di, J + dj] where that source cell lies inside the map, `fill` elsewhere."""
    p = np.asarray(plane)
    W, H = p.shape
    out = np.full_like(p, fill)
    for I in range(W):
        si = I + int(di)
        if not 0 <= si < W:
            continue
        for J in range(H):
            sj = J + int(dj)
            if 0 <= sj < H:
                out[I, J] = p[si, sj]
    return out


def shift_planes(evidence, cls, di, dj):
    """Rule 47 -> (evidence', cls'): cells without a source are never observed.  The slices are shift_plane's loop."""
    e, c = np.asarray(evidence), np.asarray(cls)
    W, H = e.shape
    di, dj = int(di), int(dj)
    eo = np.full_like(e, wref.NEVER)
    co = np.full_like(c, wref.UNEXPLORED)
    i0, i1 = max(0, -di), min(W, W - di)  # destination cells with a source inside the map
    j0, j1 = max(0, -dj), min(H, H - dj)
    if i0 < i1 and j0 < j1:
        eo[i0:i1, j0:j1] = e[i0 + di:i1 + di, j0 + dj:j1 + dj]
        co[i0:i1, j0:j1] = c[i0 + di:i1 + di, j0 + dj:j1 + dj]
    return eo, co


def trunc_div(a, b):
    """C's integer division: towards zero."""
    q = abs(int(a)) // abs(int(b))
    return q if (a >= 0) == (b > 0) else -q


def recentre_axis(S, c, margin, stride):
    if margin <= c <= S - 1 - margin:
        return 0
    return trunc_div(c - S // 2, stride) * stride


def recentre_plan(W, H, Ic, Jc, margin, stride):
    """Rule 49 -> (di, dj); ValueError for a policy it refuses."""
    if W <= 0 or H <= 0 or margin < 0 or stride < 1 or not 2 * margin < min(W, H):
        raise ValueError("margin >= 0, stride >= 1 and 2 margin < min(W, H)")
    return recentre_axis(W, int(Ic), margin, stride), recentre_axis(H, int(Jc), margin, stride)


def robot_cell(resolution, origin, x, y):
    """Rule 16's quantisation of the robot's position -> (Ic, Jc)."""
    _, _, tx, ty = wref.quantise_pose(resolution, origin, x, y, 0.0)
    return (tx + (1 << 15)) >> 16, (ty + (1 << 15)) >> 16


def shift_particles(tx, ty, di, dj):
    """Rule 50: TX' = clamp(TX - (di << 16)), TY alike -> (tx', ty') as lists of Python ints."""
    return ([mref.clamp(int(v) - (int(di) << 16)) for v in tx], [mref.clamp(int(v) - (int(dj) << 16)) for v in ty])


class RollingWorldMapRef:
    """A WorldMapRef whose window moves: the offset, the origin that follows it, and the consumers at that origin."""

    def __init__(self, width, height, resolution, origin=(0.0, 0.0), **model):
        self.origin0 = (float(origin[0]), float(origin[1]))
        self.OI = self.OJ = 0
        self.map = wref.WorldMapRef(width, height, resolution, self.origin0, **model)
        self.last = (0, (-1, -1, -1, -1))

    @property
    def W(self):
        return self.map.W

    @property
    def H(self):
        return self.map.H

    @property
    def resolution(self):
        return self.map.resolution

    @property
    def origin(self):
        r = self.map.resolution
        return origin_after(self.origin0[0], r, self.OI), origin_after(self.origin0[1], r, self.OJ)

    @property
    def offset(self):
        return self.OI, self.OJ

    @property
    def evidence(self):
        return self.map.evidence

    @property
    def cls(self):
        return self.map.cls

    def shift(self, di, dj):
        check_offset(self.OI, self.OJ, di, dj)
        if di or dj:
            self.map.evidence, self.map.cls = shift_planes(self.map.evidence, self.map.cls, di, dj)
        self.OI += int(di)
        self.OJ += int(dj)
        self.map.origin = self.origin
        self.last = (0, (-1, -1, -1, -1))  # rule 48

    def recentre(self, x, y, margin, stride):
        recentre_plan(self.W, self.H, 0, 0, margin, stride)  # the policy's refusals come first
        ic, jc = robot_cell(self.resolution, self.origin, x, y)
        di, dj = recentre_plan(self.W, self.H, ic, jc, margin, stride)
        self.shift(di, dj)
        return di, dj

    def update(self, local, pose, c=None, follow=None):
        if follow is not None:
            self.recentre(pose[0], pose[1], *follow)
        self.last = self.map.update(local, pose, c)
        return self.last

    def points(self, x, y, max_sensor_range):
        return pref.worldmap_points_ref(self.map.cls, self.resolution, self.origin, x, y, max_sensor_range)

    def scan(self, poses, angles, range_max, flags=0):
        return sref.scan(self.map.cls, self.resolution, self.origin, poses, angles, range_max, flags)

    def distance(self, reach, flags=0):
        return dref.dist2_plane(self.map.cls, reach, flags)
