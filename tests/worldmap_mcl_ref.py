"""The world map's Monte-Carlo localiser (DESIGN.md 4.11 rules 28 to 41, include/kompass_hip.h kc_mcl_*) as a literal
statement in Python integers: a loop a particle, a loop a beam, a step a turn of the walk's loop; no rounds, no early
exit, no numpy in the arithmetic.  Python's >> on int is arithmetic, its int has no width (every `& M64` below is
where the library's uint64 wraps), its float is the IEEE double and round() rounds half to even, as lrint does."""
import math

import numpy as np

from worldmap_ref import EMPTY, MAX_OFFSET, OCCUPIED, UNEXPLORED
from worldmap_scan_ref import MAX_RADIUS, UNKNOWN_BLOCKS, scan_table

M64 = (1 << 64) - 1
SKIP_NO_RETURN = 2
MAX_PARTICLES = 65536
MAX_BEAMS = 1024
MAX_RAYS = 1 << 22
MAX_TABLE = 4096
ACC_CAP = 1 << 30
MAX_INCREMENT = MAX_OFFSET
NOISE_STD = math.sqrt((65536.0 * 65536.0 - 1.0) / 3.0)   # of g: four uniform 16-bit fields


class StateError(RuntimeError):
    """KC_ERR_STATE"""


# ---- rule 29: the heading table ----
def heading(h):
    if not 0 <= h <= 65535:
        raise IndexError("heading outside 0 .. 65535")
    a = 2.0 * math.pi * float(h) / 65536.0
    return round(math.cos(a) * 65536.0), round(math.sin(a) * 65536.0)


_HEADINGS = None


def headings():
    global _HEADINGS
    if _HEADINGS is None:
        _HEADINGS = [heading(h) for h in range(65536)]
    return _HEADINGS


# ---- rule 30: random numbers ----
def mix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, step, p, c):
    return mix64(mix64((seed ^ (step << 32)) & M64) ^ ((p << 8) | c))


def noise(v, s):
    g = (v & 0xFFFF) + ((v >> 16) & 0xFFFF) + ((v >> 32) & 0xFFFF) + ((v >> 48) & 0xFFFF) - 131070
    return (g * s + (1 << 15)) >> 16


def noise_scale(sigma_units):
    """The front ends' s for a sigma in the quantity's own units (2^-16 cells, or 2^-16 turns)."""
    s = round(float(sigma_units) * 65536.0 / NOISE_STD)
    if not 0 <= s <= 0x7FFFFFFF:
        raise ValueError("sigma out of range")
    return s


def clamp(v):
    return max(-MAX_OFFSET, min(MAX_OFFSET, v))


# ---- rule 38: the refusals, in the library's order ----
def check(resolution, n_particles, n_beams, range_max, pen=None, err_shift=0, wtab=None, w_shift=0, flags=0):
    """-> (Rc, ZMAX).  ValueError: KC_ERR_INVALID, IndexError: KC_ERR_RANGE."""
    r = float(np.float32(resolution))
    m = float(np.float32(range_max))
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError("the resolution must be positive")
    if n_particles < 1 or n_beams < 1:
        raise ValueError("at least one particle and one beam")
    if n_particles > MAX_PARTICLES:
        raise IndexError("too many particles")
    if n_beams > MAX_BEAMS:
        raise IndexError("too many beams")
    if n_particles * n_beams > MAX_RAYS:
        raise IndexError("too many rays")
    if not (math.isfinite(m) and m > 0.0):
        raise ValueError("range_max must be a finite float > 0")
    if m / r > MAX_RADIUS:
        raise IndexError("range above 2048 cells")
    if pen is not None:
        if len(pen) < 1:
            raise ValueError("empty penalty table")
        if len(pen) > MAX_TABLE:
            raise IndexError("penalty table too long")
        if not 0 <= err_shift <= 30:
            raise ValueError("err_shift outside 0 .. 30")
    if wtab is not None:
        if len(wtab) < 1:
            raise ValueError("empty weight table")
        if len(wtab) > MAX_TABLE:
            raise IndexError("weight table too long")
        if not 0 <= w_shift <= 30:
            raise ValueError("w_shift outside 0 .. 30")
        if not 1 <= int(wtab[0]) <= (1 << 20):
            raise ValueError("wtab[0] outside 1 .. 2^20")
        for i in range(1, len(wtab)):
            if int(wtab[i]) > int(wtab[i - 1]):
                raise ValueError("the weight table increases")
    if flags & ~(UNKNOWN_BLOCKS | SKIP_NO_RETURN):
        raise ValueError("unknown flag bits")
    return math.ceil(m / r), round(m / r * 65536.0)


# ---- rule 33: the measured ranges ----
def quantise_ranges(ranges, resolution, range_max, flags=0):
    r = float(np.float32(resolution))
    m = float(np.float32(range_max))
    zmax = round(m / r * 65536.0)
    out = []
    for z in ranges:
        z = float(z)
        if math.isfinite(z) and 0.0 <= z < m:
            out.append(round(z / r * 65536.0))
        else:
            out.append(-1 if flags & SKIP_NO_RETURN else zmax)
    return out


# ---- rule 32: the expected range of one beam, the walk of worldmap_scan_ref.scan_pose with an integer range ----
def expected_range(cls, W, H, pose, ac, as_, Rc, zmax, flags):
    cq, sq, tx, ty = pose
    X0, Y0 = tx + (1 << 15), ty + (1 << 15)
    I0, J0 = X0 >> 16, Y0 >> 16
    fx, fy = X0 & 0xFFFF, Y0 & 0xFFFF
    blocking = (OCCUPIED, UNEXPLORED) if flags & UNKNOWN_BLOCKS else (OCCUPIED,)

    def blocks(I, J):
        return 0 <= I < W and 0 <= J < H and int(cls[I][J]) in blocking

    dx = (cq * ac - sq * as_ + (1 << 15)) >> 16
    dy = (sq * ac + cq * as_ + (1 << 15)) >> 16
    sx, sy = (1 if dx > 0 else -1), (1 if dy > 0 else -1)
    ex = 65536 - fx if dx > 0 else fx
    ey = 65536 - fy if dy > 0 else fy
    I, J = I0, J0
    if blocks(I, J):
        return 0
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
            return zmax
        if blocks(I, J):
            q = (e << 30) // a
            return zmax if q > zmax else q


class Record:
    """Rule 37."""
    FIELDS = ("w1", "w2", "sx", "sy", "sc", "ss", "amin", "best", "best_tx", "best_ty", "best_h", "step")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw[f])

    def as_tuple(self):
        return tuple(getattr(self, f) for f in self.FIELDS)

    def __repr__(self):
        return "Record(" + ", ".join(f"{f}={getattr(self, f)}" for f in self.FIELDS) + ")"


def estimate(rec, resolution, origin):
    """Rule 39 -> dict(x, y, yaw, n_eff, txe, tye)."""
    r = float(np.float32(resolution))
    txe = rec.best_tx + rec.sx // rec.w1
    tye = rec.best_ty + rec.sy // rec.w1
    return dict(txe=txe, tye=tye, x=origin[0] + float(txe) / 65536.0 * r, y=origin[1] + float(tye) / 65536.0 * r,
                yaw=math.atan2(float(rec.ss), float(rec.sc)), n_eff=float(rec.w1) * float(rec.w1) / float(rec.w2))


def spread(tx, ty, w, est, resolution):
    """The front ends' weighted std of position in metres: doubles in index order, about the estimate."""
    r = float(np.float32(resolution))
    s = 0.0
    for p in range(len(tx)):
        dx, dy = float(tx[p] - est["txe"]), float(ty[p] - est["tye"])
        s += float(w[p]) * (dx * dx + dy * dy)
    return math.sqrt(s / float(sum(w))) / 65536.0 * r


def should_resample(rec, n, r_num=1, r_den=2):
    """Rule 40's decision: n_eff < N r_num / r_den, exactly."""
    return rec.w1 * rec.w1 * r_den < r_num * n * rec.w2


def record_of(tx, ty, h, acc, wtab, w_shift, step):
    """Rules 35 to 37 from the states and the accumulated penalties -> (Record, weights)."""
    n = len(tx)
    amin = min(acc)
    best = acc.index(amin)
    ew = len(wtab)
    w = [int(wtab[min((acc[p] - amin) >> w_shift, ew - 1)]) for p in range(n)]
    H = headings()
    rec = Record(w1=sum(w), w2=sum(v * v for v in w), sx=sum(w[p] * (tx[p] - tx[best]) for p in range(n)),
                 sy=sum(w[p] * (ty[p] - ty[best]) for p in range(n)), sc=sum(w[p] * H[h[p]][0] for p in range(n)),
                 ss=sum(w[p] * H[h[p]][1] for p in range(n)), amin=amin, best=best, best_tx=tx[best], best_ty=ty[best],
                 best_h=h[best], step=step)
    return rec, w


def systematic(w, u0):
    """Rule 40's selection: for each slot j the smallest i with N cum_i > u0 + j W1."""
    n = len(w)
    w1 = sum(w)
    cum, c = [], 0
    for v in w:
        c += v
        cum.append(c)
    src = []
    for j in range(n):
        t = u0 + j * w1
        i = 0
        while not n * cum[i] > t:
            i += 1
        src.append(i)
    return src


class MclRef:
    """The localiser over a plane cls[I][J] of shape (W, H).  The plane is read at every step, so a caller may change it
    between steps (the closed loop)."""

    def __init__(self, cls, resolution, n_particles, angles, range_max, seed=0):
        self.cls = cls
        self.W, self.H = np.asarray(cls).shape
        self.resolution = float(np.float32(resolution))
        self.range_max = float(np.float32(range_max))
        self.n = int(n_particles)
        self.table = [(int(a), int(b)) for a, b in scan_table(angles)]
        self.Rc, self.zmax = check(resolution, self.n, len(self.table), range_max)
        self.seed = int(seed) & M64
        self.model = None
        self.tx = self.ty = self.h = self.acc = None
        self.step_count = 0
        self.min_prev = 0
        self.w = None
        self.rec = None

    def set_model(self, pen, err_shift, wtab, w_shift):
        check(self.resolution, self.n, len(self.table), self.range_max, pen, err_shift, wtab, w_shift)
        self.model = ([int(v) for v in pen], int(err_shift), [int(v) for v in wtab], int(w_shift))
        self.w = None                                                     # weights of another table: a resample needs a new step

    def _start(self):
        self.acc = [0] * self.n
        self.step_count = 0
        self.min_prev = 0
        self.w = None

    def init_pose(self, tx0, ty0, h0, s_xy, s_h):
        if abs(tx0) > MAX_OFFSET or abs(ty0) > MAX_OFFSET:
            raise IndexError("pose more than 2^20 cells from the origin")
        if not 0 <= h0 <= 65535:
            raise IndexError("heading outside 0 .. 65535")
        if s_xy < 0 or s_h < 0:
            raise ValueError("negative scale")
        self.tx, self.ty, self.h = [], [], []
        for p in range(self.n):
            self.tx.append(clamp(tx0 + noise(draw(self.seed, 0, p, 0), s_xy)))
            self.ty.append(clamp(ty0 + noise(draw(self.seed, 0, p, 1), s_xy)))
            self.h.append((h0 + noise(draw(self.seed, 0, p, 2), s_h)) & 0xFFFF)
        self._start()

    def init_global(self):
        cls = np.asarray(self.cls)
        free = [(I, J) for J in range(self.H) for I in range(self.W) if int(cls[I][J]) == EMPTY]  # order of I + J * W
        if not free:
            raise StateError("no free cell")
        self.tx, self.ty, self.h = [], [], []
        for p in range(self.n):
            I, J = free[draw(self.seed, 0, p, 0) % len(free)]
            v = draw(self.seed, 0, p, 1)
            self.tx.append((I << 16) + (v & 0xFFFF) - (1 << 15))
            self.ty.append((J << 16) + ((v >> 16) & 0xFFFF) - (1 << 15))
            self.h.append((v >> 32) & 0xFFFF)
        self._start()
        return len(free)

    def step(self, d_f, d_l, d_h, s_f, s_l, s_h, zq, flags=0):
        if self.model is None or self.tx is None:
            raise StateError("a step needs a model and an init")
        if abs(d_f) > MAX_INCREMENT or abs(d_l) > MAX_INCREMENT:
            raise IndexError("increment too large")
        if s_f < 0 or s_l < 0 or s_h < 0:
            raise ValueError("negative scale")
        if flags & ~(UNKNOWN_BLOCKS | SKIP_NO_RETURN):
            raise ValueError("unknown flag bits")
        if len(zq) != len(self.table):
            raise ValueError("one range a beam")
        for z in zq:
            if not (0 <= z <= self.zmax or (z == -1 and flags & SKIP_NO_RETURN)):
                raise ValueError("quantised range outside 0 .. ZMAX")
        pen, err_shift, wtab, w_shift = self.model
        E = len(pen)
        self.step_count += 1
        step, seed = self.step_count, self.seed
        cls = np.asarray(self.cls)
        H = headings()
        for p in range(self.n):
            C, S = H[self.h[p]]
            F = d_f + noise(draw(seed, step, p, 0), s_f)
            L = d_l + noise(draw(seed, step, p, 1), s_l)
            self.tx[p] = clamp(self.tx[p] + ((C * F - S * L + (1 << 15)) >> 16))
            self.ty[p] = clamp(self.ty[p] + ((S * F + C * L + (1 << 15)) >> 16))
            self.h[p] = (self.h[p] + d_h + noise(draw(seed, step, p, 2), s_h)) & 0xFFFF
            C, S = H[self.h[p]]
            pose = (C, S, self.tx[p], self.ty[p])
            cost = 0
            for k, (ac, as_) in enumerate(self.table):
                if zq[k] < 0:
                    continue
                q = expected_range(cls, self.W, self.H, pose, ac, as_, self.Rc, self.zmax, flags)
                cost += pen[min(abs(q - zq[k]) >> err_shift, E - 1)]
            self.acc[p] = min(self.acc[p] - self.min_prev + cost, ACC_CAP)
        self.rec, self.w = record_of(self.tx, self.ty, self.h, self.acc, wtab, w_shift, step)
        self.min_prev = self.rec.amin
        return self.rec

    def resample(self):
        if self.w is None:
            raise StateError("a resample needs a step's weights")
        u0 = draw(self.seed, self.step_count, self.n, 15) % self.rec.w1
        src = systematic(self.w, u0)
        self.tx = [self.tx[i] for i in src]
        self.ty = [self.ty[i] for i in src]
        self.h = [self.h[i] for i in src]
        self.acc = [0] * self.n
        self.min_prev = 0
        self.w = None
        return src

    def particles(self):
        return (np.array(self.tx, np.int64), np.array(self.ty, np.int64), np.array(self.h, np.uint32),
                np.array(self.acc, np.uint32))


# ---- the front ends' judgement (rule 34 and 36's tables from a sensor model; DESIGN.md says which part is judgement) ----
def quantise_heading(yaw):
    return round(float(yaw) / (2.0 * math.pi) * 65536.0) & 0xFFFF


def odometry_increment(resolution, a, b):
    """(x, y, yaw) a -> b as (d_f, d_l, d_h): the displacement in a's frame in 2^-16 cells, the turn in heading units."""
    r = float(np.float32(resolution))
    dx, dy = float(b[0]) - float(a[0]), float(b[1]) - float(a[1])
    c, s = math.cos(float(a[2])), math.sin(float(a[2]))
    d_f = round((c * dx + s * dy) / r * 65536.0)
    d_l = round((-s * dx + c * dy) / r * 65536.0)
    d_h = round((float(b[2]) - float(a[2])) / (2.0 * math.pi) * 65536.0)
    return d_f, d_l, d_h


def sensor_tables(resolution, sigma_hit, err_shift=12, n_pen=256, floor=0.05, pen_scale=64.0, w_shift=4, n_w=1024,
                  wtab0=1 << 16, temperature=256.0):
    """pen[i] = lrint(pen_scale * -log(floor + (1 - floor) exp(-d^2 / 2 sigma^2))) for the bin's lower edge d = i 2^err_shift
    (2^-16 cells) and sigma = sigma_hit metres; wtab[i] = lrint(wtab0 exp(-i 2^w_shift / temperature))."""
    r = float(np.float32(resolution))
    sig = float(sigma_hit) / r * 65536.0
    pen = []
    for i in range(n_pen):
        d = float(i << err_shift)
        pen.append(min(65535, round(pen_scale * -math.log(floor + (1.0 - floor) * math.exp(-d * d / (2.0 * sig * sig))))))
    wtab = [round(wtab0 * math.exp(-float(i << w_shift) / temperature)) for i in range(n_w)]
    return pen, err_shift, wtab, w_shift
