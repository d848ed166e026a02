"""Independent Python restatement of the reference DepthDetector (vision/depth_detector.cpp:84-178) and of
Bbox2D(PointsOfInterest) (datatypes/tracking.h), for the tests.  Not collected by pytest.

Float32 scalar arithmetic throughout (every constant wrapped), np.sort medians, the band tests in double (the
literal 1.5 is a double), and the Eigen isometry chain of utils/transformation.h with libm sinf / cosf through
ctypes (Eigen's AngleAxisf calls the float functions).  The rules this build adds where the reference reads out
of bounds: pixels outside the frame are skipped and the box limits are exact integers."""
from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _fn in ("sinf", "cosf"):
    getattr(_libm, _fn).restype = ctypes.c_float
    getattr(_libm, _fn).argtypes = [ctypes.c_float]

F = np.float32


def sinf(x) -> np.float32:
    return F(_libm.sinf(F(x)))


def cosf(x) -> np.float32:
    return F(_libm.cosf(F(x)))


def add3(a, b, c):
    """Eigen's fixed-size 3-term sum: a + (b + c)."""
    return F(a) + (F(b) + F(c))


# ---------------------------------------------------------------- isometries (Eigen::Isometry3f)
def rotation_of(w, x, y, z):
    """QuaternionBase::toRotationMatrix (not normalised)."""
    w, x, y, z = F(w), F(x), F(y), F(z)
    two = F(2)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = F(1)
    return [[one - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, one - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, one - (txx + tyy)]]


def quat_of(R):
    """Quaternionf(Matrix3f) -> (w, x, y, z)."""
    half = F(0.5)
    t = add3(R[0][0], R[1][1], R[2][2])
    if t > F(0):
        t = F(np.sqrt(t + F(1)))
        w = half * t
        t = half / t
        return w, (R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    v = [F(0)] * 3
    t = F(np.sqrt(R[i][i] - R[j][j] - R[k][k] + F(1)))
    v[i] = half * t
    t = half / t
    w = (R[k][j] - R[j][k]) * t
    v[j] = (R[j][i] + R[i][j]) * t
    v[k] = (R[k][i] + R[i][k]) * t
    return w, v[0], v[1], v[2]


class Iso:
    def __init__(self, R, t):
        self.R = [[F(v) for v in row] for row in R]
        self.t = [F(v) for v in t]

    @staticmethod
    def identity():
        return Iso([[1, 0, 0], [0, 1, 0], [0, 0, 1]], [0, 0, 0])

    @staticmethod
    def from_quat_xyzw(q, t):
        """getTransformation(Quaternionf(Vector4f xyzw), translation)."""
        return Iso(rotation_of(q[3], q[0], q[1], q[2]), t)

    @staticmethod
    def from_state(x, y, yaw):
        """getTransformation(Path::State): eulerToRotationMatrix(0, 0, yaw) -> Quaternionf -> matrix."""
        ha = F(0.5) * F(yaw)
        Rz = rotation_of(cosf(ha), F(0), F(0), sinf(ha))
        return Iso(rotation_of(*quat_of(Rz)), [F(x), F(y), F(0)])

    def __mul__(self, B):
        R = [[add3(self.R[i][0] * B.R[0][j], self.R[i][1] * B.R[1][j], self.R[i][2] * B.R[2][j]) for j in range(3)]
             for i in range(3)]
        t = [add3(self.R[i][0] * B.t[0], self.R[i][1] * B.t[1], self.R[i][2] * B.t[2]) + self.t[i] for i in range(3)]
        return Iso(R, t)

    def apply(self, p):
        p = [F(v) for v in p]
        return [self.t[i] + add3(self.R[i][0] * p[0], self.R[i][1] * p[1], self.R[i][2] * p[2]) for i in range(3)]


# ---------------------------------------------------------------- the detector
def median(v):
    """getMedian: sorted, v[n/2] or 0.5f * (v[n/2-1] + v[n/2])."""
    s = np.sort(v)
    n = len(s)
    if n % 2 == 0:
        return F(0.5) * (s[n // 2 - 1] + s[n // 2])
    return s[n // 2]


def box_stats(img, box, factor, min_depth, max_depth):
    """(count, median, mad, min_d, max_d) of one box; zeros after the count when it is dropped (count <= 1)."""
    tx, ty, sx, sy = (int(v) for v in box)
    h, w = img.shape
    y0, y1 = max(ty, 0), min(ty + sy, h - 1)
    x0, x1 = max(tx, 0), min(tx + sx, w - 1)
    if y0 > y1 or x0 > x1:
        return 0, F(0), F(0), F(0), F(0)
    depth = img[y0:y1 + 1, x0:x1 + 1].astype(np.float32) * F(factor)
    vals = depth[(depth <= F(max_depth)) & (depth >= F(min_depth))]
    n = len(vals)
    if n <= 1:
        return n, F(0), F(0), F(0), F(0)
    med = median(vals)
    mad = median(np.abs(vals - med))
    lo = float(med) - 1.5 * float(mad)
    hi = float(med) + 1.5 * float(mad)
    mn, mx = F(max_depth), F(min_depth)
    v64 = vals.astype(np.float64)
    low = vals[v64 >= lo]
    if len(low) and low.min() < mn:
        mn = low.min()
    high = vals[v64 <= hi]
    if len(high) and high.max() > mx:
        mx = high.max()
    return n, F(med), F(mad), F(mn), F(mx)


class Detector:
    def __init__(self, depth_range, translation, rotation_xyzw, focal, principal, factor=1e-3):
        factor = F(factor)
        with np.errstate(over="ignore", invalid="ignore"):
            ok = np.isfinite(factor) and factor > 0 and np.isfinite(F(65535) * factor)
        if not ok:
            raise ValueError("depth conversion factor")
        self.min_depth, self.max_depth = F(depth_range[0]), F(depth_range[1])
        self.factor = factor
        self.fx, self.fy = F(focal[0]), F(focal[1])
        self.cx, self.cy = F(principal[0]), F(principal[1])
        self.camera_in_body = Iso.from_quat_xyzw([F(v) for v in rotation_xyzw], translation)
        self.body_in_world = Iso.identity()

    def stats(self, img, boxes):
        return [box_stats(img, b, self.factor, self.min_depth, self.max_depth) for b in boxes]

    def boxes(self, img, boxes, state=None):
        """(centres [m, 3], sizes [m, 3], kept indices [m]) as float32 / int32 arrays."""
        if state is not None:
            self.body_in_world = Iso.from_state(*state)
        cam = self.body_in_world * self.camera_in_body
        cs, ss, idx = [], [], []
        for i, b in enumerate(boxes):
            n, med, _, mn, mx = box_stats(img, b, self.factor, self.min_depth, self.max_depth)
            if n <= 1:
                continue
            tx, ty, sx, sy = (F(int(v)) for v in b)
            half = F(0.5)
            x_opt = (tx + half * sx - self.cx) * med / self.fx
            y_opt = (ty + half * sy - self.cy) * med / self.fy
            size_cam = [mx - mn, sx * med / self.fx, sy * med / self.fy]
            cs.append(cam.apply([med, -x_opt, -y_opt]))
            ss.append([add3(abs(cam.R[r][0]) * size_cam[0], abs(cam.R[r][1]) * size_cam[1],
                            abs(cam.R[r][2]) * size_cam[2]) for r in range(3)])
            idx.append(i)
        return (np.array(cs, np.float32).reshape(-1, 3), np.array(ss, np.float32).reshape(-1, 3),
                np.array(idx, np.int32))


# ---------------------------------------------------------------- Bbox2D(PointsOfInterest, mad_scale = 2)
def box_from_pois(points, img_size, mad_scale=2.0):
    """(top.x, top.y, size.x, size.y) of Bbox2D(const PointsOfInterest &, mad_scale)."""
    if len(points) == 0:
        raise ValueError("PointsOfInterest has no points")
    xs = sorted(int(p[0]) for p in points)
    ys = sorted(int(p[1]) for p in points)
    n = len(xs)
    mx, my = xs[n // 2], ys[n // 2]
    dx = sorted(abs(x - mx) for x in xs)
    dy = sorted(abs(y - my) for y in ys)
    hw = max(int(F(mad_scale) * F(dx[n // 2])), 5)
    hh = max(int(F(mad_scale) * F(dy[n // 2])), 5)
    x0, y0 = max(0, mx - hw), max(0, my - hh)
    x1, y1 = min(int(img_size[0]) - 1, mx + hw), min(int(img_size[1]) - 1, my + hh)
    return x0, y0, x1 - x0, y1 - y0
