"""Exact shape-against-voxel geometry (A4 contract) in Python integers and Fractions, and the case families
that test_collision_exact_cpu.py (oracle) and test_collision_exact_gpu.py (device) run.

The statement.  The octree frame F (rotation with float32 entries, float32 origin) is recomputed here in
float32 numpy from the mount quaternion, the mount position and the body pose; an occupied voxel with key k is
the closed cube [k res, (k + 1) res]^3 in F; the robot shape stands upright in the world with its centre at
(x, y, 0); both sets are closed, so touching counts.  Every input is converted exactly (float32 / double ->
Fraction) and no floating point takes part in a decision.

The formulations differ from the code under test on purpose:
  sphere, disc, cylinder   squared distance from the centre (taken into F with R^T) to its clamped point
  box / rectangle          both bodies as half-spaces; the intersection is a bounded polytope, non-empty exactly
                           when the meet of three bounding planes (two lines in the plane) satisfies them all
  tilted cylinder          cube cut by the slab |z| <= h / 2 (8 half-spaces), its vertices by the same plane-triple
                           routine, projected onto xy, exact monotone-chain hull, exact squared distance from the
                           origin to that polygon against r^2
  height gate (planar)     closed overlap of [kz res, (kz + 1) res] with [zc - h / 2, zc + h / 2]; the sphere takes
                           the z gap into its distance
  voxel keys               floor(fl(coord * fl(1 / res))) in Python floats (octomap's own double product);
                           |k| >= 32768 drops the point

classify() evaluates the predicate with the shape grown and shrunk by eps (radius and every half extent):
HIT if both hit, MISS if both miss, UNDECIDED otherwise.  The band is derived, not tuned: F's float32 entries are
an exact orthonormal frame rounded to float32, each within 2^-24 relative, so a point at distance L from F's
origin moves by at most about 3 * 2^-24 * L; eps = 2^-20 * L leaves a margin of about 5x, L being the shape's
circumscribed radius plus one voxel diagonal plus, where F's rotation is not the identity, the pose's distance
from F's origin.  Its only purpose is to keep F's non-orthonormality out of the verdict.  Imports nothing from the
oracle or the library."""
from __future__ import annotations

import functools
import itertools
import math
from fractions import Fraction as Fr

import numpy as np

CYLINDER, BOX, SPHERE = 0, 1, 2
HIT, MISS, UNDECIDED = 1, 0, -1
F32 = np.float32


def quat(axis, angle):
    ax = np.asarray(axis, float)
    ax = ax / np.linalg.norm(ax)
    s = math.sin(angle / 2)
    return (ax[0] * s, ax[1] * s, ax[2] * s, math.cos(angle / 2))


IDENT_ROT = (0.0, 0.0, 0.0, 1.0)
PLANAR_MOUNT = (quat((0, 0, 1), 0.7), (0.1, -0.05, 0.2))
TILT_MOUNTS = [(quat((0, 1, 0), 0.4), (0.1, -0.05, 0.2)), (quat((1, 1, 0.3), 0.8), (0.1, -0.05, 0.2))]
BODY = (0.3, -0.2)          # body pose of every sensor update (yaw 0: the body rotation is exactly the identity)

SHAPES = {"cylinder": (CYLINDER, [0.15, 0.4]), "box": (BOX, [0.4, 0.3, 0.5]), "longbox": (BOX, [1.5, 0.2, 0.5]),
          "sphere": (SPHERE, [0.2])}


# ---------------------------------------------------------------------------------------------------------------
# the frame, in float32
# ---------------------------------------------------------------------------------------------------------------
def quat_rot_f32(q_xyzw):
    """Rotation matrix of a float32 quaternion, every operation in float32 (Eigen's toRotationMatrix order)."""
    x, y, z, w = (F32(v) for v in q_xyzw)
    two, one = F32(2), F32(1)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[one - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, one - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, one - (txx + tyy)]]


def sensor_frame(srot, spos, body_xy):
    """F = body_tf * sensor_tf_body for a body at (x, y, yaw 0): the body rotation is exactly the identity, so the
    product keeps the mount's rotation and adds the float32 positions."""
    R = quat_rot_f32(srot)
    t = [F32(spos[0]) + F32(body_xy[0]), F32(spos[1]) + F32(body_xy[1]), F32(spos[2]) + F32(0)]
    return R, t


def identity_frame():
    o, z = F32(1), F32(0)
    return [[o, z, z], [z, o, z], [z, z, o]], [z, z, z]


def frame_is_planar(R):
    e = F32(1e-6)
    return bool(abs(R[0][2]) < e and abs(R[1][2]) < e and abs(R[2][0]) < e and abs(R[2][1]) < e and R[2][2] > 0)


def key_of(coord, res):
    """octomap coordToKey on one axis; None outside the 16-level tree."""
    f = math.floor(float(coord) * (1.0 / res))
    return f if abs(f) < 32768 else None


# ---------------------------------------------------------------------------------------------------------------
# a scene: one sensor update of one robot shape
# ---------------------------------------------------------------------------------------------------------------
class Scene:
    """feed: ("points", xyz float32 [n][3], global_frame) or ("scan", ranges, angles); state is (BODY, yaw 0)."""

    def __init__(self, shape, dims, res, feed, srot=IDENT_ROT, spos=(0.0, 0.0, 0.0), midvoxel=True, label=""):
        self.shape, self.dims, self.res, self.feed = shape, [float(F32(d)) for d in dims], float(res), feed
        self.srot, self.spos, self.label = tuple(float(v) for v in srot), tuple(float(v) for v in spos), label
        self.state = (BODY[0], BODY[1], 0.0, 0.0)
        if feed[0] == "points" and feed[2]:
            R, t = identity_frame()
        else:
            R, t = sensor_frame(self.srot, self.spos, BODY)
        self.identity = all(float(R[i][j]) == (1.0 if i == j else 0.0) for i in range(3) for j in range(3))
        self.planar = frame_is_planar(R)
        self.R = [[Fr(float(v)) for v in row] for row in R]
        self.t = [Fr(float(v)) for v in t]
        self.resq = Fr(self.res)
        if feed[0] == "points":
            pts = np.asarray(feed[1], F32).reshape(-1, 3)
        else:
            r, a = np.asarray(feed[1], float), np.asarray(feed[2], float)
            hz = F32(-float(F32(self.spos[2])) / 2.0)
            pts = np.array([[F32(r[i] * math.cos(a[i])), F32(r[i] * math.sin(a[i])), hz] for i in range(len(r))
                            if math.isfinite(r[i])], F32).reshape(-1, 3)
        assert self.planar or feed[0] == "scan"
        self.keys = set()
        for p in pts:
            k = tuple(key_of(c, self.res) for c in p)
            if None in k:
                continue
            if midvoxel:        # the key is not in question: >= res / 8 from every face (the scan's fixed height:
                for ax in range(3):     # off the face by more than any rounding of the product)
                    f = float(p[ax]) * (1.0 / self.res) - k[ax]
                    lim = 2.0 ** -30 if (feed[0] == "scan" and ax == 2) else 0.125
                    assert lim <= f <= 1.0 - lim, (label, p, ax, f)
            self.keys.add(k)
        self.keys = sorted(self.keys)
        d = [Fr(v) for v in self.dims]
        # rho3: circumscribed radius of the shape; rho: the bound the distance pre-filter uses (planar: in the plane)
        if shape == BOX:
            self.half = [d[0] / 2, d[1] / 2, d[2] / 2]
            self.rho3 = math.sqrt(sum(float(h) ** 2 for h in self.half))
            self.rho = self.rho3 if not self.planar else math.hypot(float(self.half[0]), float(self.half[1]))
        elif shape == CYLINDER:
            self.radius, self.hh = d[0], d[1] / 2
            self.rho3 = math.hypot(self.dims[0], self.dims[1] / 2)
            self.rho = self.rho3 if not self.planar else self.dims[0]
        else:
            self.radius = d[0]
            self.rho = self.rho3 = self.dims[0]

    # -- the band ---------------------------------------------------------------------------------------------
    def eps(self, x, y):
        L = self.rho3 + self.res * math.sqrt(3.0)
        if not self.identity:
            L += math.sqrt((x - float(self.t[0])) ** 2 + (y - float(self.t[1])) ** 2 + float(self.t[2]) ** 2)
        return Fr(L) / (1 << 20)

    # -- the predicate ----------------------------------------------------------------------------------------
    def hit(self, x, y, yaw, g=Fr(0)):
        """Does the shape, grown by g, at (x, y, yaw) meet an occupied voxel?  x, y: double or Fraction."""
        x, y = Fr(x), Fr(y)
        cw, sw = Fr(math.cos(yaw)), Fr(math.sin(yaw))
        return self._hit_planar(x, y, cw, sw, g) if self.planar else self._hit_tilted(x, y, cw, sw, g)

    def classify(self, x, y, yaw, eps=None):
        e = self.eps(float(x), float(y)) if eps is None else Fr(eps)
        if not self.hit(x, y, yaw, e):          # (shrinking never gains a hit: a miss of the grown shape is a MISS)
            return MISS
        return HIT if e == 0 or self.hit(x, y, yaw, -e) else UNDECIDED

    def _gap2(self, c, k):
        lo, hi = k * self.resq, (k + 1) * self.resq
        g = lo - c if c < lo else (c - hi if c > hi else 0)
        return g * g

    def _hit_planar(self, x, y, cw, sw, g):
        R, t, res = self.R, self.t, self.resq
        dx, dy = x - t[0], y - t[1]
        xf, yf = R[0][0] * dx + R[1][0] * dy, R[0][1] * dx + R[1][1] * dy
        zc = -t[2]
        if self.shape == SPHERE:
            r = self.radius + g
            return r >= 0 and any(self._gap2(xf, kx) + self._gap2(yf, ky) + self._gap2(zc, kz) <= r * r
                                  for kx, ky, kz in self.keys)
        hz = (self.hh if self.shape == CYLINDER else self.half[2]) + g
        if hz < 0:
            return False
        cols = {(kx, ky) for kx, ky, kz in self.keys if kz * res <= zc + hz and (kz + 1) * res >= zc - hz}
        if self.shape == CYLINDER:
            r = self.radius + g
            return r >= 0 and any(self._gap2(xf, kx) + self._gap2(yf, ky) <= r * r for kx, ky in cols)
        a, b = self.half[0] + g, self.half[1] + g
        if a < 0 or b < 0:
            return False
        ux, uy = R[0][0] * cw + R[1][0] * sw, R[0][1] * cw + R[1][1] * sw
        vx, vy = -uy, ux
        rect = [(ux, uy, ux * xf + uy * yf + a), (-ux, -uy, -(ux * xf + uy * yf) + a),
                (vx, vy, vx * xf + vy * yf + b), (-vx, -vy, -(vx * xf + vy * yf) + b)]
        out2 = (Fr(self.rho) * Fr(1001, 1000) + abs(g) + Fr(1, 1000)) ** 2
        for kx, ky in cols:
            if self._gap2(xf, kx) + self._gap2(yf, ky) > out2:
                continue
            sq = [(1, 0, (kx + 1) * res), (-1, 0, -kx * res), (0, 1, (ky + 1) * res), (0, -1, -ky * res)]
            if _feasible2([_ints(h) for h in rect + sq]):
                return True
        return False

    def _hit_tilted(self, x, y, cw, sw, g):
        R, t, res = self.R, self.t, self.resq
        d = (x - t[0], y - t[1], -t[2])
        cf = [R[0][i] * d[0] + R[1][i] * d[1] + R[2][i] * d[2] for i in range(3)]
        if self.shape == SPHERE:
            r = self.radius + g
            return r >= 0 and any(sum(self._gap2(cf[i], k[i]) for i in range(3)) <= r * r for k in self.keys)
        out2 = (Fr(self.rho) * Fr(1001, 1000) + abs(g) + Fr(1, 1000)) ** 2
        near = [k for k in self.keys if sum(self._gap2(cf[i], k[i]) for i in range(3)) <= out2]
        if self.shape == BOX:
            e = [h + g for h in self.half]
            if min(e) < 0:
                return False
            A = [[R[0][i] * cw + R[1][i] * sw for i in range(3)], [R[1][i] * cw - R[0][i] * sw for i in range(3)],
                 [R[2][i] for i in range(3)]]
            box = []
            for k in range(3):
                c0 = sum(A[k][i] * cf[i] for i in range(3))
                box += [(A[k][0], A[k][1], A[k][2], c0 + e[k]), (-A[k][0], -A[k][1], -A[k][2], -c0 + e[k])]
            box = [_ints(h) for h in box]
            for k in near:
                # (a point in both sets proves a hit: the box's centre, or a corner of the cube)
                if all(k[i] * res <= cf[i] <= (k[i] + 1) * res for i in range(3)):
                    return True
                corners = itertools.product(*[((k[i] * res), ((k[i] + 1) * res)) for i in range(3)])
                if any(all(q[0] * c[0] + q[1] * c[1] + q[2] * c[2] <= q[3] for q in box) for c in corners):
                    return True
                if next(_vertices3(box + _cube_planes(k, res)), None) is not None:
                    return True
            return False
        # cylinder, in world axes about the shape's centre w = p_w - (x, y, 0): the cube is
        # k_i res <= col_i(R) . (w + (x, y, 0) - t) <= (k_i + 1) res, the slab |w_z| <= h / 2
        r, hh = self.radius + g, self.hh + g
        if r < 0 or hh < 0:
            return False
        slab = [_ints((0, 0, 1, hh)), _ints((0, 0, -1, hh))]
        for k in near:
            planes = list(slab)
            for i in range(3):
                n = (R[0][i], R[1][i], R[2][i])
                off = n[0] * d[0] + n[1] * d[1] + n[2] * d[2]
                planes += [_ints((n[0], n[1], n[2], (k[i] + 1) * res - off)),
                           _ints((-n[0], -n[1], -n[2], -k[i] * res + off))]
            pts = {(Fr(P[0], D), Fr(P[1], D)) for P, D in _vertices3(planes)}
            if pts and _origin_poly_d2(_hull(sorted(pts))) <= r * r:
                return True
        return False

    # -- labelling help for the edge-edge family: which separating axes of the two boxes separate, exactly ----
    def sat_axes(self, x, y, yaw, k, g=Fr(0)):
        """For the tilted box against voxel k: the list of the 15 axes' verdicts (True: separates)."""
        x, y, cw, sw = Fr(x), Fr(y), Fr(math.cos(yaw)), Fr(math.sin(yaw))
        R, t, res = self.R, self.t, self.resq
        d = (x - t[0], y - t[1], -t[2])
        cf = [R[0][i] * d[0] + R[1][i] * d[1] + R[2][i] * d[2] for i in range(3)]
        A = [[R[0][i] * cw + R[1][i] * sw for i in range(3)], [R[1][i] * cw - R[0][i] * sw for i in range(3)],
             [R[2][i] for i in range(3)]]
        e = [h + g for h in self.half]
        h = res / 2
        T = [(k[i] + Fr(1, 2)) * res - cf[i] for i in range(3)]
        E = [[1, 0, 0], [0, 1, 0], [0, 0, 1]]

        def sep(L):
            lhs = abs(sum(T[i] * L[i] for i in range(3)))
            rhs = h * sum(abs(v) for v in L) + sum(e[j] * abs(sum(A[j][i] * L[i] for i in range(3))) for j in range(3))
            return lhs > rhs

        def cross(p, q):
            return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]
        return [sep(L) for L in E] + [sep(L) for L in A] + [sep(cross(E[i], A[j])) for j in range(3) for i in range(3)]


def _ints(h):
    """One inequality n . p <= d with Fraction coefficients, scaled by a positive number to integers."""
    m = 1
    for f in h:
        den = Fr(f).denominator
        m = m * den // math.gcd(m, den)
    return tuple(int(Fr(f) * m) for f in h)


def _cube_planes(k, res):
    out = []
    for i in range(3):
        n = [0, 0, 0]
        n[i] = 1
        out.append(_ints((n[0], n[1], n[2], (k[i] + 1) * res)))
        out.append(_ints((-n[0], -n[1], -n[2], -k[i] * res)))
    return out


def _feasible2(lines):
    """Is the bounded polygon {n . p <= d} non-empty?  Some meet of two bounding lines satisfies every inequality."""
    for a, b in itertools.combinations(lines, 2):
        D = a[0] * b[1] - a[1] * b[0]
        if D == 0:
            continue
        px, py = a[2] * b[1] - a[1] * b[2], a[0] * b[2] - a[2] * b[0]
        if D < 0:
            D, px, py = -D, -px, -py
        if all(q[0] * px + q[1] * py <= q[2] * D for q in lines):
            return True
    return False


def _vertices3(planes):
    """The vertices ((X, Y, Z), D), D > 0, point = (X, Y, Z) / D, of the bounded polytope {n . p <= d}: every meet
    of three bounding planes that satisfies all the inequalities (a vertex may come more than once)."""
    for a, b, c in itertools.combinations(planes, 3):
        bc = (b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0])
        D = a[0] * bc[0] + a[1] * bc[1] + a[2] * bc[2]
        if D == 0:
            continue
        ca = (c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0])
        ab = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
        P = [a[3] * bc[m] + b[3] * ca[m] + c[3] * ab[m] for m in range(3)]
        if D < 0:
            D, P = -D, [-v for v in P]
        if all(q[0] * P[0] + q[1] * P[1] + q[2] * P[2] <= q[3] * D for q in planes):
            yield P, D


def _hull(pts):
    """Monotone chain over sorted distinct points, counter-clockwise, collinear points dropped."""
    if len(pts) <= 2:
        return pts

    def half(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (p[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (p[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(p)
        return h
    lo, up = half(pts), half(pts[::-1])
    return lo[:-1] + up[:-1]


def _origin_poly_d2(poly):
    """Exact squared distance from the origin to a convex polygon (counter-clockwise hull, or 1 or 2 points)."""
    n = len(poly)
    if n == 1:
        return poly[0][0] ** 2 + poly[0][1] ** 2
    edges = [(poly[i], poly[(i + 1) % n]) for i in range(n if n > 2 else 1)]
    if n > 2 and all(a[0] * (b[1] - a[1]) - a[1] * (b[0] - a[0]) >= 0 for a, b in edges):
        return Fr(0)        # the origin lies left of (or on) every edge: inside
    best = None
    for a, b in edges:
        dx, dy = b[0] - a[0], b[1] - a[1]
        l2 = dx * dx + dy * dy
        ad = a[0] * dx + a[1] * dy
        if ad >= 0:
            d2 = a[0] ** 2 + a[1] ** 2
        elif -ad >= l2:
            d2 = b[0] ** 2 + b[1] ** 2
        else:
            d2 = a[0] ** 2 + a[1] ** 2 - ad * ad / l2
        best = d2 if best is None or d2 < best else best
    return best


# ---------------------------------------------------------------------------------------------------------------
# helpers of the generators
# ---------------------------------------------------------------------------------------------------------------
class Batch:
    """Poses of one scene with the exact verdict of each (HIT / MISS / UNDECIDED) and the band used."""

    def __init__(self, scene, poses, want, eps, name, options=None):
        self.scene, self.name, self.options = scene, name, dict(options or {})
        self.x = np.array([p[0] for p in poses], float)
        self.y = np.array([p[1] for p in poses], float)
        self.yaw = np.array([p[2] for p in poses], float)
        self.want = np.array(want, int)
        self.eps = float(eps)

    def take(self, idx, name):
        """The poses idx (repeats allowed) as a batch of their own: nothing is computed again."""
        poses = [(self.x[i], self.y[i], self.yaw[i]) for i in idx]
        return Batch(self.scene, poses, [self.want[i] for i in idx], self.eps, name, self.options)


def classify_batch(scene, poses, name, eps=None):
    want = [scene.classify(p[0], p[1], p[2], eps) for p in poses]
    e = eps if eps is not None else max(scene.eps(p[0], p[1]) for p in poses)
    return Batch(scene, poses, want, e, name)


def points_scene(shape, dims, res, keys, global_frame=True, srot=IDENT_ROT, spos=(0, 0, 0), label=""):
    """Mid-voxel points of the given (kx, ky, kz) keys."""
    pts = np.array([[(k + 0.5) * res for k in key] for key in keys], F32)
    sc = Scene(shape, dims, res, ("points", pts, global_frame), srot, spos, label=label)
    assert sc.keys == sorted(set(map(tuple, keys))), (label, sc.keys, keys)
    return sc


def scan_scene(shape, dims, res, cols, srot, spos, label=""):
    """A LaserScan whose returns fall mid-voxel into the given (kx, ky) columns of the sensor plane."""
    r = [math.hypot((kx + 0.5) * res, (ky + 0.5) * res) for kx, ky in cols]
    a = [math.atan2((ky + 0.5) * res, (kx + 0.5) * res) for kx, ky in cols]
    sc = Scene(shape, dims, res, ("scan", np.array(r), np.array(a)), srot, spos, label=label)
    assert sorted({k[:2] for k in sc.keys}) == sorted(set(map(tuple, cols))), (label, sc.keys, cols)
    return sc


def to_world(sc, pf):
    """A point of F in the world, in doubles (generators only: where to aim, never a verdict)."""
    R, t = sc.R, sc.t
    return [float(t[i]) + sum(float(R[i][j]) * pf[j] for j in range(3)) for i in range(3)]


def solve_contact(sc, p_out, p_in, yaw, g, lo=Fr(0), hi=Fr(1), tol=None):
    """Bisect, with the exact predicate of the shape grown by g, for the pose on the segment p_out -> p_in (a miss
    at lo, a hit at hi) at which the grown shape comes into contact, down to `tol` metres (default eps / 8).
    Returns the final bracket; pose_on() turns a parameter into the double pose."""
    g = Fr(g)
    ox, oy, ix, iy = Fr(p_out[0]), Fr(p_out[1]), Fr(p_in[0]), Fr(p_in[1])
    assert not sc.hit(ox + lo * (ix - ox), oy + lo * (iy - oy), yaw, g), (sc.label, p_out, p_in, yaw)
    assert sc.hit(ox + hi * (ix - ox), oy + hi * (iy - oy), yaw, g), (sc.label, p_out, p_in, yaw)
    length = Fr(math.hypot(p_in[0] - p_out[0], p_in[1] - p_out[1]))
    tol = sc.eps(p_in[0], p_in[1]) / 8 if tol is None else tol
    while (hi - lo) * length > tol:
        mid = (lo + hi) / 2
        if sc.hit(ox + mid * (ix - ox), oy + mid * (iy - oy), yaw, g):
            hi = mid
        else:
            lo = mid
    return lo, hi


def pose_on(p_out, p_in, s):
    return (float(Fr(p_out[0]) + s * (Fr(p_in[0]) - Fr(p_out[0]))), float(Fr(p_out[1]) + s * (Fr(p_in[1]) - Fr(p_out[1]))))


def near_contact_poses(sc, p_out, p_in, yaw, mults=(4, 64)):
    """Poses at signed clearance +-m eps from contact along p_out -> p_in: where the shape grown by m eps touches,
    the shape itself clears by m eps (a MISS); where the shape shrunk by m eps touches, it overlaps (a HIT).
    In the order (+m, -m) per m.  (The widest band is solved first; its bracket holds the others.)"""
    e = sc.eps(p_in[0], p_in[1])
    big = max(mults)
    _, hi_in = solve_contact(sc, p_out, p_in, yaw, -big * e)
    lo_out, _ = solve_contact(sc, p_out, p_in, yaw, big * e, hi=hi_in)
    out = []
    for m in mults:
        for sgn in (1, -1):
            lo, hi = solve_contact(sc, p_out, p_in, yaw, sgn * m * e, lo=lo_out, hi=hi_in)
            x, y = pose_on(p_out, p_in, (lo + hi) / 2)
            out.append((x, y, yaw))
    return out


# ---------------------------------------------------------------------------------------------------------------
# (a) dyadic exact contact, no band: F = I, t = 0, res = 1 / 8, dyadic poses, yaw 0
# ---------------------------------------------------------------------------------------------------------------
STEP = 2.0 ** -20


@functools.lru_cache(None)
def family_dyadic():
    """Each contact pose is a HIT at eps = 0 and the same pose one dyadic step 2^-20 m further off is a MISS."""
    assert (math.cos(0.0), math.sin(0.0)) == (1.0, 0.0)
    yaws = [0.0] + ([math.pi] if (math.cos(math.pi), math.sin(math.pi)) in ((-1.0, 0.0), (-1.0, -0.0)) else [])
    res, out = 0.125, []

    def pair(sc, contact, away, name):
        poses, want = [], []
        for (x, y), (ax, ay) in zip(contact, away):
            for yaw in (yaws if sc.shape == BOX else [0.0]):
                poses += [(x, y, yaw), (x + ax * STEP, y + ay * STEP, yaw)]
                want += [HIT, MISS]
        b = classify_batch(sc, poses, name, eps=0)
        assert list(b.want) == want, (name, list(b.want), want)
        out.append(b)

    for key in ((2, 1, 0), (-3, -2, 0), (0, -1, 0)):
        xlo, ylo = key[0] * res, key[1] * res
        xhi, yhi, xm, ym = xlo + res, ylo + res, xlo + res / 2, ylo + res / 2
        # disc r = 1/4 against each face
        sc = points_scene(CYLINDER, [0.25, 0.5], res, [key], label="disc face")
        pair(sc, [(xlo - 0.25, ym), (xhi + 0.25, ym), (xm, ylo - 0.25), (xm, yhi + 0.25)],
             [(-1, 0), (1, 0), (0, -1), (0, 1)], f"a/disc-face{key}")
        # disc r = 5/8 against each corner by 3-4-5
        sc = points_scene(CYLINDER, [0.625, 0.5], res, [key], label="disc corner")
        pair(sc, [(xlo - 0.375, ylo - 0.5), (xhi + 0.375, ylo - 0.5), (xlo - 0.5, yhi + 0.375), (xhi + 0.5, yhi + 0.375)],
             [(-1, 0), (1, 0), (0, 1), (0, 1)], f"a/disc-corner{key}")
        # sphere r = 7/8 by 2-3-6-7: offsets 1/4 and 3/8, z gap 3/4 (above and below the centre plane)
        for kz in (6, -7):
            sc = points_scene(SPHERE, [0.875], res, [(key[0], key[1], kz)], label="sphere 2367")
            pair(sc, [(xlo - 0.25, ylo - 0.375), (xhi + 0.375, yhi + 0.25), (xlo - 0.375, yhi + 0.25), (xhi + 0.25, ylo - 0.375)],
                 [(-1, 0), (0, 1), (-1, 0), (1, 0)], f"a/sphere{key}kz{kz}")
        # box 1/2 x 1/4: |q| = a + h on each face
        sc = points_scene(BOX, [0.5, 0.25, 0.5], res, [key], label="box face")
        pair(sc, [(xlo - 0.25, ym), (xhi + 0.25, ym), (xm, ylo - 0.125), (xm, yhi + 0.125)],
             [(-1, 0), (1, 0), (0, -1), (0, 1)], f"a/box-face{key}")
    # height gate: zlo = zc + h/2 (kz = 2) and zhi = zc - h/2 (kz = -3) exactly; the robot lower by 2^-19 is clear
    for shape, dims, hi in ((CYLINDER, [0.25, 0.5], 1), (BOX, [0.5, 0.25, 0.5], 2)):
        for kz in (2, -3):
            for h, want in ((0.5, HIT), (0.5 - 2.0 ** -19, MISS)):
                d = list(dims)
                d[hi] = h
                sc = points_scene(shape, d, res, [(1, 1, kz)], label="height gate")
                b = classify_batch(sc, [(0.1875, 0.1875, 0.0)], f"a/gate-shape{shape}kz{kz}h{h}", eps=0)
                assert list(b.want) == [want]
                out.append(b)
    out += _dyadic_upside_down()
    return out


UPSIDE_DOWN = ((1.0, 0.0, 0.0, 0.0), (0.25, -0.125, 0.375))     # a half turn about x: R = diag(1, -1, -1) exactly


def _dyadic_upside_down():
    """The 3-D tests without a band: a sensor mounted upside down gives a frame that is not planar and exact.
    The scan's layer kz = -2 lies at world z in [0.5, 0.625]; voxel column (3, 2).  A cylinder and a box 1 m tall
    touch it from below with their top face (2^-19 m shorter: clear); box and sphere touch it sideways, the
    sphere by 1-2-2-3: offsets 0.25 and 0.5, z gap 0.5, r = 0.75."""
    res, out = 0.125, []
    srot, spos = UPSIDE_DOWN

    def scene(shape, dims, label):
        sc = scan_scene(shape, dims, res, [(3, 2)], srot, spos, label=label)
        assert not sc.planar and sc.keys == [(3, 2, -2)]
        assert [[int(v) for v in row] for row in sc.R] == [[1, 0, 0], [0, -1, 0], [0, 0, -1]]
        return sc

    def world(sc, xf, yf):      # F -> world, exactly: both sums fit a double
        x, y = float(sc.t[0]) + xf, float(sc.t[1]) - yf
        assert Fr(x) == sc.t[0] + Fr(xf) and Fr(y) == sc.t[1] - Fr(yf)
        return x, y

    for shape, dims, hi in ((CYLINDER, [0.25, 1.0], 1), (BOX, [0.5, 0.25, 1.0], 2)):
        for h, want in ((1.0, HIT), (1.0 - 2.0 ** -19, MISS)):
            d = list(dims)
            d[hi] = h
            sc = scene(shape, d, "upside-down top")
            x, y = world(sc, 0.4375, 0.3125)
            b = classify_batch(sc, [(x, y, 0.0), (x + 0.0625, y - 0.03125, 0.0)], f"a/tilted-top-shape{shape}h{h}", eps=0)
            assert list(b.want) == [want, want], (b.name, list(b.want))
            out.append(b)
    # box 1/2 x 1/4 x 2 (tall enough to span the layer): |q| = a + h on the four faces, in F
    sc = scene(BOX, [0.5, 0.25, 2.0], "upside-down box face")
    poses, want = [], []
    for xf, yf, ax, ay in ((0.375 - 0.25, 0.3125, -1, 0), (0.5 + 0.25, 0.3125, 1, 0), (0.4375, 0.25 - 0.125, 0, -1),
                           (0.4375, 0.375 + 0.125, 0, 1)):
        poses += [world(sc, xf, yf) + (0.0,), world(sc, xf + ax * STEP, yf + ay * STEP) + (0.0,)]
        want += [HIT, MISS]
    b = classify_batch(sc, poses, "a/tilted-box-face", eps=0)
    assert list(b.want) == want, (b.name, list(b.want))
    out.append(b)
    # sphere r = 3/4: centre plane at z_F = 0.375, the layer's top at z_F = -0.125: gap 1/2
    sc = scene(SPHERE, [0.75], "upside-down sphere 1223")
    poses, want = [], []
    for xf, yf, ax, ay in ((0.375 - 0.25, 0.25 - 0.5, -1, 0), (0.5 + 0.5, 0.375 + 0.25, 1, 0), (0.375 - 0.5, 0.375 + 0.25, 0, 1),
                           (0.5 + 0.25, 0.25 - 0.5, 0, -1)):
        poses += [world(sc, xf, yf) + (0.0,), world(sc, xf + ax * STEP, yf + ay * STEP) + (0.0,)]
        want += [HIT, MISS]
    b = classify_batch(sc, poses, "a/tilted-sphere", eps=0)
    assert list(b.want) == want, (b.name, list(b.want))
    out.append(b)
    return out


# ---------------------------------------------------------------------------------------------------------------
# (b) near contact: +-4 eps and +-64 eps from contact, every shape, four frames, face / edge / vertex
# ---------------------------------------------------------------------------------------------------------------
BOX_YAWS = (0.0, 0.3, math.pi / 4, math.pi / 2, 2.0, -3.0)
FRAMES = ["identity", "planar", "tilt0", "tilt1"]


def _frame_scene(frame, shape, dims, res, cols, label):
    """The (kx, ky) columns as a scene of the named frame; the layer is the one the feed fixes."""
    if frame == "identity":
        return points_scene(shape, dims, res, [(kx, ky, 1) for kx, ky in cols], label=label)
    srot, spos = PLANAR_MOUNT if frame == "planar" else TILT_MOUNTS[int(frame[-1])]
    return scan_scene(shape, dims, res, cols, srot, spos, label=label)


def _tilt_columns(sc_probe, n_want, reach=0.12):
    """Columns of the sensor plane whose voxel centre lies within `reach` of the world plane z = 0."""
    kz = sc_probe.keys[0][2]
    res, out = sc_probe.res, []
    for kx in range(-30, 31):
        for ky in range(-30, 31):
            if max(abs(kx), abs(ky)) < 6:
                continue
            w = to_world(sc_probe, [(kx + 0.5) * res, (ky + 0.5) * res, (kz + 0.5) * res])
            if abs(w[2]) < reach:
                out.append((abs(w[2]), kx, ky))
    out.sort()
    return [(kx, ky) for _, kx, ky in out[:n_want]]


@functools.lru_cache(None)
def frame_columns(frame):
    """A few well-separated voxel columns per frame that the upright shapes can reach."""
    if frame in ("identity", "planar"):
        return [(12, 7), (-15, -9), (-1, 22)]
    srot, spos = TILT_MOUNTS[int(frame[-1])]
    probe = scan_scene(CYLINDER, [0.15, 0.4], 0.05, [(10, 10)], srot, spos)
    cand = _tilt_columns(probe, 400)
    picked = []
    for c in cand:      # keep them >= 45 columns apart, so that one pose meets one voxel
        if all(max(abs(c[0] - p[0]), abs(c[1] - p[1])) >= 14 for p in picked):
            picked.append(c)
        if len(picked) == 3:
            break
    return picked


def _features(sc, key):
    """Aim points of voxel `key` in F: (name, point, outward direction), planar: face and corner; 3-D: also vertex."""
    res = sc.res
    c = [(k + 0.5) * res for k in key]
    h = res / 2
    if sc.planar:
        return [("face", [c[0] + h, c[1] + 0.2 * h, c[2]], [1, 0, 0]), ("face-", [c[0] - 0.3 * h, c[1] - h, c[2]], [0, -1, 0]),
                ("edge", [c[0] - h, c[1] + h, c[2]], [-1, 1, 0])]
    return [("face", [c[0] + h, c[1], c[2]], [1, 0, 0]), ("face-", [c[0], c[1] - h, c[2]], [0, -1, 0]),
            ("edge", [c[0] - h, c[1] + h, c[2]], [-1, 1, 0]), ("vertex", [c[0] + h, c[1] + h, c[2] + h], [1, 1, 1]),
            ("vertex-", [c[0] - h, c[1] - h, c[2] - h], [-1, -1, -1])]


def approach(sc, key, feat):
    """(p_out, p_in) in the world for the approach to one feature: p_in above the voxel's centre (a hit if the
    voxel is within the shape's height at all), p_out 1.2 circumscribed radii + 4 voxels out along the feature's
    outward direction, seen from above."""
    _, pf, nf = feat
    c = to_world(sc, [(k + 0.5) * sc.res for k in key])
    a = to_world(sc, pf)
    b = to_world(sc, [pf[i] + nf[i] for i in range(3)])
    d = (b[0] - a[0], b[1] - a[1])
    n = math.hypot(*d)
    far = 1.2 * sc.rho + 4 * sc.res
    # aim through the feature: the line from p_out passes over the feature point, then on to the centre
    return (a[0] + d[0] / n * far, a[1] + d[1] / n * far), (a[0], a[1]), (c[0], c[1])


@functools.lru_cache(None)
def family_near(frame, shape_name):
    shape, dims = SHAPES[shape_name]
    cols = frame_columns(frame)
    sc = _frame_scene(frame, shape, dims, 0.05, cols, f"b/{frame}/{shape_name}")
    yaws = BOX_YAWS if shape == BOX else (0.0,)
    poses, want = [], []
    for ik, key in enumerate(sc.keys):
        for ifeat, feat in enumerate(_features(sc, key)):
            for iyaw, yaw in enumerate(yaws):
                if shape == BOX and not sc.planar and (ik + ifeat + iyaw) % 3:     # (trimmed: a third of them in 3-D,
                    continue                                                       # every feature at two yaws per voxel)
                p_out, p_feat, p_ctr = approach(sc, key, feat)
                p_in = p_feat if sc.hit(p_feat[0], p_feat[1], yaw, -64 * sc.eps(*p_feat)) else p_ctr
                if not sc.hit(p_in[0], p_in[1], yaw, -64 * sc.eps(*p_in)):
                    continue        # the voxel lies outside the shape's height here: nothing to approach
                if sc.hit(p_out[0], p_out[1], yaw, 64 * sc.eps(*p_out)):
                    continue
                poses += near_contact_poses(sc, p_out, p_in, yaw)
                want += [MISS, HIT, MISS, HIT]
    b = classify_batch(sc, poses, f"b/{frame}/{shape_name}")
    assert len(poses) >= 8, (frame, shape_name, len(poses))
    assert list(b.want) == want, (b.name, list(b.want), want)      # all decided, by construction
    return b


@functools.lru_cache(None)
def family_near_points(shape_name):
    """(b) once more for the planar tests through a point list in the sensor's frame (layers kz = -1 and -6 lie
    within every shape's height about zc = -0.2), the boxes at yaw 0.3."""
    shape, dims = SHAPES[shape_name]
    srot, spos = PLANAR_MOUNT
    sc = points_scene(shape, dims, 0.05, [(12, 7, -1), (-15, -9, -6)], False, srot, spos, f"b/points/{shape_name}")
    poses = []
    for key in sc.keys:
        for feat in _features(sc, key):
            p_out, p_in, _ = approach(sc, key, feat)
            poses += near_contact_poses(sc, p_out, p_in, 0.3)
    b = classify_batch(sc, poses, sc.label)
    assert list(b.want) == [MISS, HIT] * (len(poses) // 2), (b.name, list(b.want))
    return b


# ---------------------------------------------------------------------------------------------------------------
# (c) edge against edge for the tilted box: only a cross-product axis separates
# ---------------------------------------------------------------------------------------------------------------
# axis 3 j + i = (cube axis i) x (box axis j): (mount, shape, column, yaw, approach direction), found by a seeded
# search over yaws and directions for contacts at which no face normal separates.  Box axis 2 is vertical (voxels
# near z = 0 meet the box's upright edges); axes 0 and 1 are the rims of its top and bottom faces (voxels near
# |z| = 0.25).  The two mounts reach all nine pairs.
EDGE_CASES = {0: (0, "longbox", (18, 8), -2.978, -1.939), 1: (1, "box", (-26, -36), -0.265, -1.375),
              2: (0, "longbox", (18, -2), 0.371, 2.63), 3: (0, "box", (-10, -22), -1.921, -1.6),
              4: (1, "box", (-10, -22), -0.437, -0.139), 5: (0, "box", (17, -2), -1.525, 1.6),
              6: (1, "box", (-26, -26), -2.868, -0.411), 7: (0, "box", (4, -16), 0.688, -0.039),
              8: (1, "box", (11, 5), 0.988, -2.69)}


@functools.lru_cache(None)
def family_edge_edge():
    out = []
    for axis, (fi, shn, col, yaw, phi) in sorted(EDGE_CASES.items()):
        shape, dims = SHAPES[shn]
        srot, spos = TILT_MOUNTS[fi]
        sc = scan_scene(shape, dims, 0.05, [col], srot, spos, label=f"c/axis{axis}")
        key = sc.keys[0]
        c = to_world(sc, [(k + 0.5) * sc.res for k in key])
        far = 1.2 * sc.rho + 0.2
        p_in, p_out = (c[0], c[1]), (c[0] + far * math.cos(phi), c[1] + far * math.sin(phi))
        poses = near_contact_poses(sc, p_out, p_in, yaw, mults=(4,))
        b = classify_batch(sc, poses, f"c/axis{axis}")
        assert list(b.want) == [MISS, HIT], (b.name, list(b.want))
        sep = sc.sat_axes(poses[0][0], poses[0][1], yaw, key)
        assert not any(sep[:6]), (axis, sep)        # every face normal of the cube and of the box overlaps ...
        assert sep[6 + axis], (axis, sep)           # ... and this cross product separates
        b.only_axes = [i for i in range(9) if sep[6 + i]]
        out.append(b)
    return out


# ---------------------------------------------------------------------------------------------------------------
# (d) keys and masks: negative and positive keys across 0, every bit of a window word, the crop, pose counts
# ---------------------------------------------------------------------------------------------------------------
def _without(sc, key):
    import copy
    o = copy.copy(sc)
    o.keys = [k for k in sc.keys if k != key]
    return o


@functools.lru_cache(None)
def family_masks(frame, shape_name, along):
    """A row (along = 0) or column (along = 1) of 40 adjacent voxels, keys -20 .. 19: 40 consecutive cells of the
    window hold every bit 0 .. 31 of a word and at least one word boundary (bit 31 beside bit 32), wherever the
    window's origin falls.  Per voxel a pose that reaches it alone by 4 eps (a disc from the side, its centre over
    the middle of the voxel; a box corner first, its diagonal along the approach) and the pose 4 eps short.  Without the voxel aimed
    at, the hit pose is clear by more than 64 eps: its neighbours at +-1 cell are out of reach."""
    shape, dims = SHAPES[shape_name]
    cols = [((k, 5) if along == 0 else (-7, k)) for k in range(-20, 20)]
    sc = _frame_scene(frame, shape, dims, 0.05, cols, f"d/{frame}/{shape_name}/{along}")
    yaw = 0.0
    if shape == BOX:        # a corner of the rectangle points along the approach, in F
        fyaw = math.atan2(float(sc.R[1][0]), float(sc.R[0][0]))
        diag = math.atan2(float(sc.half[1]), float(sc.half[0]))
        yaw = fyaw + (math.pi / 2 if along == 0 else 0.0) - diag
    poses, want = [], []
    h = sc.res / 2
    for key in sc.keys:
        c = [(k + 0.5) * sc.res for k in key]
        face = [c[0], c[1] - h, c[2]] if along == 0 else [c[0] - h, c[1], c[2]]
        feat = ("face", face, [0, -1, 0] if along == 0 else [-1, 0, 0])
        p_out, p_in, _ = approach(sc, key, feat)
        pp = near_contact_poses(sc, p_out, p_in, yaw, mults=(4,))
        e = sc.eps(*pp[1][:2])
        assert not _without(sc, key).hit(pp[1][0], pp[1][1], yaw, 64 * e), (sc.label, key)
        poses += pp
        want += [MISS, HIT]
    b = classify_batch(sc, poses, sc.label)
    assert list(b.want) == want, (b.name, list(b.want), want)
    return b


@functools.lru_cache(None)
def family_counts():
    """Pose batches of 1, 255, 256 and 257 poses (one block of the pose kernel, and one pose more), from the row."""
    base = family_masks("identity", "cylinder", 0)
    n = len(base.x)
    return [base.take([(3 * i + 1) % n for i in range(cnt)], f"d/count{cnt}") for cnt in (1, 255, 256, 257)]


@functools.lru_cache(None)
def family_crop(frame, shape_name):
    """Pose 0 far away, so that the window of the batch is built about a distant point; later poses touch voxel A
    from the near side and from the far side (the far one is the pose furthest from pose 0: A lies just inside the
    crop), and voxel C lies beyond the reach of every pose (outside the crop, or just inside: never a hit)."""
    shape, dims = SHAPES[shape_name]
    A, C = (10, 5), (10 + int(math.ceil(SHAPES[shape_name][1][0] / 0.05)) + 8, 5)
    sc = _frame_scene(frame, shape, dims, 0.05, [A, C, (-40, 30)], f"d/crop/{frame}/{shape_name}")
    key = [k for k in sc.keys if k[:2] == A][0]
    c = [(k + 0.5) * sc.res for k in key]
    h = sc.res / 2
    far = to_world(sc, [c[0] - 60 * sc.res, c[1], c[2]])
    poses, want = [(far[0], far[1], 0.0)], [MISS]
    for feat in (("near", [c[0] - h, c[1], c[2]], [-1, 0, 0]), ("far", [c[0] + h, c[1], c[2]], [1, 0, 0])):
        p_out, p_in, _ = approach(sc, key, feat)
        n = math.hypot(p_out[0] - p_in[0], p_out[1] - p_in[1])      # (start between A and C, clear of both)
        p_out = pose_on(p_in, p_out, Fr((sc.rho + sc.res) / n))
        poses += near_contact_poses(sc, p_out, p_in, 0.0, mults=(4,))
        want += [MISS, HIT]
    b = classify_batch(sc, poses, sc.label)
    assert list(b.want) == want, (b.name, list(b.want), want)
    return b


# ---------------------------------------------------------------------------------------------------------------
# (e) the height gate, through the sensor builds: point lists, F = I
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def family_height():
    """The voxel layer kz = 4 begins at the robot's nominal top (0.2 m), kz = -5 ends at its bottom; the robot's
    height (the sphere's radius) is set +-4 eps and +-64 eps about that, in float32, which is 3e-8 m fine here."""
    out = []
    res = 0.05
    for name, (shape, dims) in SHAPES.items():
        if name == "longbox":
            continue
        nominal = points_scene(shape, dims, res, [(3, -2, 4)])
        e = float(nominal.eps(0.175, -0.075))
        for kz in (4, -5):
            for m in (4, 64):
                for sgn, want in ((1, HIT), (-1, MISS)):
                    d = list(dims)
                    if shape == SPHERE:
                        d[0] = 0.2 + sgn * m * e
                    else:
                        d[-1] = 2 * (0.2 + sgn * m * e)
                    sc = points_scene(shape, d, res, [(3, -2, kz), (-30, 12, 0)], label=f"e/{name}/kz{kz}/{sgn * m}eps")
                    b = classify_batch(sc, [(0.175, -0.075, 0.4), (0.19, -0.06, -1.0)], sc.label)
                    assert list(b.want) == [want, want], (b.name, list(b.want), want)
                    out.append(b)
    return out


# ---------------------------------------------------------------------------------------------------------------
# (f) key formation: points one float32 ulp either side of k res
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def family_keys():
    """One point per scene, on the x, y or z axis at fl32(k res) and one ulp either side (and -0.0), a needle of a
    cylinder (r = 1 cm) over the centres of the cells k - 1, k, k + 1: which cell holds the voxel, if any.
    b.columns is the number of voxel columns the update keeps (the key inside the tree and inside the height)."""
    res, out = 0.05, []
    mid = [0.125, -0.075, 0.025]            # keys (2, -2, 0)
    for axis in range(3):
        for k in (-32768, -32767, -1, 0, 1, 32767):
            c0 = F32(k * res)
            vals = [np.nextafter(c0, F32(-np.inf)), c0, np.nextafter(c0, F32(np.inf))] + ([F32(-0.0)] if k == 0 else [])
            for v in vals:
                p = [F32(m) for m in mid]
                p[axis] = F32(v)
                sc = Scene(CYLINDER, [0.01, 0.4], res, ("points", np.array([p], F32), True), midvoxel=False,
                           label=f"f/axis{axis}/k{k}/{float(v)!r}")
                poses = []
                for kk in (k - 1, k, k + 1):
                    q = list(mid)
                    if axis < 2:
                        q[axis] = (kk + 0.5) * res
                    poses.append((q[0], q[1], 0.0))
                b = classify_batch(sc, poses[:1] if axis == 2 else poses, sc.label)
                assert UNDECIDED not in b.want
                gated = {kk[:2] for kk in sc.keys if kk[2] * sc.resq <= sc.hh and (kk[2] + 1) * sc.resq >= -sc.hh}
                b.columns = len(gated)
                out.append(b)
    return out


# ---------------------------------------------------------------------------------------------------------------
# (g) fuzz
# ---------------------------------------------------------------------------------------------------------------
FUZZ_SEED = 20
FUZZ_POSES = 300
FUZZ_HOLES = {(1, 1), (3, 1), (2, 2), (0, 3), (3, 3), (4, 4), (1, 4)}


@functools.lru_cache(None)
def family_fuzz(frame, shape_name):
    """300 poses within (circumscribed radius + 2 res) of a 5 x 5 voxel patch with holes; yaw uniform."""
    shape, dims = SHAPES[shape_name]
    k0 = frame_columns(frame)[0]
    cols = [(k0[0] + i, k0[1] + j) for i in range(5) for j in range(5) if (i, j) not in FUZZ_HOLES]
    sc = _frame_scene(frame, shape, dims, 0.05, cols, f"g/{frame}/{shape_name}")
    kz = sc.keys[0][2]
    rng = np.random.default_rng([FUZZ_SEED, FRAMES.index(frame), list(SHAPES).index(shape_name)])
    ctr = to_world(sc, [(k0[0] + 2.5) * sc.res, (k0[1] + 2.5) * sc.res, (kz + 0.5) * sc.res])
    reach = 2.5 * sc.res * math.sqrt(2.0) + sc.rho3 + 2 * sc.res
    poses = []
    while len(poses) < FUZZ_POSES:
        dx, dy = rng.uniform(-reach, reach, 2)
        if math.hypot(dx, dy) <= reach:
            poses.append((ctr[0] + dx, ctr[1] + dy, rng.uniform(-math.pi, math.pi)))
    return classify_batch(sc, poses, sc.label)


def all_batches():
    """Every batch of every family (the mutation check of the oracle walks this)."""
    out = list(family_dyadic())
    out += [family_near(f, s) for f in FRAMES for s in SHAPES] + [family_near_points(s) for s in SHAPES]
    out += family_edge_edge()
    out += [family_masks(f, s, a) for f in ("identity", "planar") for s in ("cylinder", "box") for a in (0, 1)]
    out += family_counts()
    out += [family_crop(f, s) for f in ("identity", "planar") for s in ("cylinder", "box", "sphere")]
    out += family_height() + family_keys()
    out += [family_fuzz(f, s) for f in FRAMES for s in SHAPES]
    return out


# ---------------------------------------------------------------------------------------------------------------
# the comparison both tests make
# ---------------------------------------------------------------------------------------------------------------
def assert_batch(b, got, who):
    """Every decided pose of the batch: `got` (booleans of the code under test) equals the exact verdict."""
    got = np.asarray(got).astype(int)
    decided = b.want != UNDECIDED
    bad = np.flatnonzero(decided & (got != b.want))
    assert bad.size == 0, (
        f"{who} disagrees with the exact geometry in {b.name} (eps {b.eps:.3e} m, {int((~decided).sum())} of "
        f"{len(got)} undecided): " + "; ".join(
            f"pose ({b.x[i]!r}, {b.y[i]!r}, yaw {b.yaw[i]!r}) exact {'HIT' if b.want[i] else 'MISS'} "
            f"got {'HIT' if got[i] else 'MISS'}" for i in bad[:4]))


def assert_fuzz_conditions(b):
    """Conditions on the fuzz batch itself, not measurements: <= 1 % undecided, each outcome >= 10 % of the rest."""
    n, und = len(b.want), int((b.want == UNDECIDED).sum())
    hits, miss = int((b.want == HIT).sum()), int((b.want == MISS).sum())
    assert und <= 0.01 * n, f"{b.name}: {und} of {n} undecided at eps {b.eps:.3e} m"
    assert hits >= 0.1 * (n - und) and miss >= 0.1 * (n - und), f"{b.name}: {hits} hits, {miss} misses"
