"""The localiser's likelihood-field model (DESIGN.md 4.11 rules 44 and 45, include/kompass_hip.h kc_mcl_set_field_model)
in two forms.

MclFieldRef is the loop statement: worldmap_mcl_ref.MclRef with rule 32 to 34's penalty loop replaced by rules 44 and
45, in Python ints, a loop a particle and a loop a beam.

MclFieldVec states init, predict, endpoint and penalty over all particles at once in numpy int64 / uint64 (whose
arithmetic wraps as the library's does and whose >> on int64 is arithmetic); the record still comes from
worldmap_mcl_ref.record_of in Python ints.  It may serve as a reference only where it has been shown equal to the loop
statement, which tests/test_worldmap_mcl_field_cpu.py does on a small case."""
import math

import numpy as np

import worldmap_dist_ref as dref
import worldmap_mcl_ref as mref
from worldmap_ref import EMPTY, MAX_OFFSET

FAR = dref.FAR
MAX_C2 = mref.MAX_TABLE - 1


# ---- kc_mcl_field_check, in the library's order ----
def field_check(resolution, n_particles, n_beams, range_max, pen_d2=None, reach=0, wtab=None, w_shift=0, flags=0):
    """-> (Rc, ZMAX).  ValueError: KC_ERR_INVALID, IndexError: KC_ERR_RANGE."""
    out = mref.check(resolution, n_particles, n_beams, range_max)
    if pen_d2 is not None:
        if len(pen_d2) < 2:
            raise ValueError("a field penalty table needs c2 + 1 >= 2 entries")
        if len(pen_d2) > mref.MAX_TABLE:
            raise IndexError("penalty table too long")
        if reach != 0:
            if not 1 <= reach <= dref.MAX_REACH:
                raise IndexError("reach outside 1 .. 254")
            if len(pen_d2) - 1 > reach * reach:
                raise ValueError("c2 above reach^2")
    mref.check(resolution, n_particles, n_beams, range_max, None, 0, wtab, w_shift)
    if flags & ~mref.SKIP_NO_RETURN:
        raise ValueError("a field step takes SKIP_NO_RETURN alone")
    return out


# ---- the front ends' judgement ----
def field_tables(resolution, sigma_hit, reach=0, floor=0.05, pen_scale=64.0, w_shift=4, n_w=1024, wtab0=1 << 16,
                 temperature=256.0):
    """-> (pen_d2, pen_far, reach, wtab, w_shift).  pen_d2[d] = lrint(pen_scale * -log(floor + (1 - floor) exp(-d / (2
    sigma_cells^2)))) for d = 0 .. reach^2, pen_far = lrint(pen_scale * -log(floor)); reach 0: ceil(3 sigma_cells) within
    1 .. 63."""
    r = float(np.float32(resolution))
    sig = float(sigma_hit) / r
    if reach == 0:
        reach = max(1, min(63, math.ceil(3.0 * sig)))
    pen = [min(65535, round(pen_scale * -math.log(floor + (1.0 - floor) * math.exp(-float(d) / (2.0 * sig * sig)))))
           for d in range(reach * reach + 1)]
    far = min(65535, round(pen_scale * -math.log(floor)))
    wtab = mref.sensor_tables(resolution, sigma_hit, n_pen=1, w_shift=w_shift, n_w=n_w, wtab0=wtab0, temperature=temperature)[2]
    return pen, far, reach, wtab, w_shift


def beam_direction(C, S, ac, as_):
    """Rule 22."""
    return (C * ac - S * as_ + (1 << 15)) >> 16, (S * ac + C * as_ + (1 << 15)) >> 16


def endpoint(tx, ty, dx, dy, zq):
    """Rule 44 -> (I, J).  Python's >> floors: a negative EX gives a negative I."""
    ex = tx + (1 << 15) + ((zq * dx + (1 << 29)) >> 30)
    ey = ty + (1 << 15) + ((zq * dy + (1 << 29)) >> 30)
    return ex >> 16, ey >> 16


class MclFieldRef(mref.MclRef):
    """The loop statement.  `dist` is a worldmap_dist_ref.DistRef over the same cls plane: the step refreshes it."""

    def __init__(self, cls, resolution, n_particles, angles, range_max, seed=0, dist=None):
        super().__init__(cls, resolution, n_particles, angles, range_max, seed)
        self.dist = dist
        self.field = None

    def set_model(self, pen, err_shift, wtab, w_shift):
        super().set_model(pen, err_shift, wtab, w_shift)
        self.field = None                                                 # back to the beam model

    def set_field_model(self, pen_d2, pen_far, wtab, w_shift):
        field_check(self.resolution, self.n, len(self.table), self.range_max, pen_d2, 0, wtab, w_shift)
        if not 0 <= pen_far <= 0xFFFF:
            raise ValueError("pen_far is a uint16")
        self.field = ([int(v) for v in pen_d2], int(pen_far), [int(v) for v in wtab], int(w_shift))
        self.w = None

    def step(self, d_f, d_l, d_h, s_f, s_l, s_h, zq, flags=0):
        if self.field is None:
            return super().step(d_f, d_l, d_h, s_f, s_l, s_h, zq, flags)
        if self.tx is None:
            raise mref.StateError("a step needs an init")
        if abs(d_f) > mref.MAX_INCREMENT or abs(d_l) > mref.MAX_INCREMENT:
            raise IndexError("increment too large")
        if s_f < 0 or s_l < 0 or s_h < 0:
            raise ValueError("negative scale")
        if flags & ~(mref.UNKNOWN_BLOCKS | mref.SKIP_NO_RETURN):
            raise ValueError("unknown flag bits")
        if flags & mref.UNKNOWN_BLOCKS:
            raise ValueError("the plane's own flag decides what blocks")
        if len(zq) != len(self.table):
            raise ValueError("one range a beam")
        for z in zq:
            if not (0 <= z <= self.zmax or (z == -1 and flags & mref.SKIP_NO_RETURN)):
                raise ValueError("quantised range outside 0 .. ZMAX")
        pen_d2, pen_far, wtab, w_shift = self.field
        c2 = len(pen_d2) - 1
        if self.dist is None:
            raise mref.StateError("the map's distance plane is off")
        if c2 > self.dist.reach * self.dist.reach:
            raise mref.StateError("c2 above the plane's reach^2")
        plane = self.dist.field()                                         # refreshed
        self.step_count += 1
        step, seed = self.step_count, self.seed
        H = mref.headings()
        for p in range(self.n):
            C, S = H[self.h[p]]
            F = d_f + mref.noise(mref.draw(seed, step, p, 0), s_f)
            L = d_l + mref.noise(mref.draw(seed, step, p, 1), s_l)
            self.tx[p] = mref.clamp(self.tx[p] + ((C * F - S * L + (1 << 15)) >> 16))
            self.ty[p] = mref.clamp(self.ty[p] + ((S * F + C * L + (1 << 15)) >> 16))
            self.h[p] = (self.h[p] + d_h + mref.noise(mref.draw(seed, step, p, 2), s_h)) & 0xFFFF
            C, S = H[self.h[p]]
            cost = 0
            for k, (ac, as_) in enumerate(self.table):
                if not 0 <= zq[k] < self.zmax:                            # rule 45: no return, or skipped
                    continue
                dx, dy = beam_direction(C, S, ac, as_)
                I, J = endpoint(self.tx[p], self.ty[p], dx, dy, zq[k])
                d2 = int(plane[I][J]) if 0 <= I < self.W and 0 <= J < self.H else FAR
                cost += pen_d2[d2] if d2 <= c2 else pen_far
            self.acc[p] = min(self.acc[p] - self.min_prev + cost, mref.ACC_CAP)
        self.rec, self.w = mref.record_of(self.tx, self.ty, self.h, self.acc, wtab, w_shift, step)
        self.min_prev = self.rec.amin
        return self.rec


# ---- the vectorised form ----
_U = np.uint64


def mix64_v(x):
    with np.errstate(over="ignore"):
        z = x + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def draw_v(seed, step, p, c):
    key = _U(mref.mix64((seed ^ (step << 32)) & mref.M64))
    return mix64_v(key ^ ((p.astype(_U) << _U(8)) | _U(c)))


def noise_v(v, s):
    g = ((v & _U(0xFFFF)) + ((v >> _U(16)) & _U(0xFFFF)) + ((v >> _U(32)) & _U(0xFFFF)) + (v >> _U(48))).astype(np.int64) - 131070
    return (g * np.int64(s) + (1 << 15)) >> 16


class MclFieldVec:
    """The same localiser over int64 arrays; field model only.  `plane`: a callable that returns the refreshed uint16
    [W, H] plane (a DistRef's field), read at every step."""

    def __init__(self, cls, resolution, n_particles, angles, range_max, seed, plane):
        self.cls = cls
        self.W, self.H = np.asarray(cls).shape
        self.resolution = float(np.float32(resolution))
        self.n = int(n_particles)
        self.table = np.array(mref.scan_table(angles), np.int64).reshape(-1, 2)
        self.Rc, self.zmax = mref.check(resolution, self.n, len(self.table), range_max)
        self.seed = int(seed) & mref.M64
        self.plane = plane
        self.heads = np.array(mref.headings(), np.int64)
        self.p = np.arange(self.n, dtype=np.int64)
        self.step_count = 0
        self.min_prev = 0
        self.w = self.rec = None

    def set_field_model(self, pen_d2, pen_far, wtab, w_shift):
        self.pen_d2 = np.array(list(pen_d2) + [int(pen_far)], np.int64)   # the last entry stands for "above c2"
        self.c2 = len(pen_d2) - 1
        self.wtab, self.w_shift = [int(v) for v in wtab], int(w_shift)

    def _start(self):
        self.acc = np.zeros(self.n, np.int64)
        self.step_count = 0
        self.min_prev = 0
        self.w = None

    def init_pose(self, tx0, ty0, h0, s_xy, s_h):
        self.tx = np.clip(tx0 + noise_v(draw_v(self.seed, 0, self.p, 0), s_xy), -MAX_OFFSET, MAX_OFFSET)
        self.ty = np.clip(ty0 + noise_v(draw_v(self.seed, 0, self.p, 1), s_xy), -MAX_OFFSET, MAX_OFFSET)
        self.h = (h0 + noise_v(draw_v(self.seed, 0, self.p, 2), s_h)) & 0xFFFF
        self._start()

    def init_global(self):
        free = np.flatnonzero(np.asarray(self.cls).T.reshape(-1) == EMPTY)   # the order of I + J * W
        if free.size == 0:
            raise mref.StateError("no free cell")
        cell = free[(draw_v(self.seed, 0, self.p, 0) % _U(free.size)).astype(np.int64)]
        v = draw_v(self.seed, 0, self.p, 1)
        self.tx = ((cell % self.W) << 16) + (v & _U(0xFFFF)).astype(np.int64) - (1 << 15)
        self.ty = ((cell // self.W) << 16) + ((v >> _U(16)) & _U(0xFFFF)).astype(np.int64) - (1 << 15)
        self.h = ((v >> _U(32)) & _U(0xFFFF)).astype(np.int64)
        self._start()
        return int(free.size)

    def step(self, d_f, d_l, d_h, s_f, s_l, s_h, zq, flags=0):
        self.step_count += 1
        step = self.step_count
        C, S = self.heads[self.h, 0], self.heads[self.h, 1]
        F = d_f + noise_v(draw_v(self.seed, step, self.p, 0), s_f)
        L = d_l + noise_v(draw_v(self.seed, step, self.p, 1), s_l)
        self.tx = np.clip(self.tx + ((C * F - S * L + (1 << 15)) >> 16), -MAX_OFFSET, MAX_OFFSET)
        self.ty = np.clip(self.ty + ((S * F + C * L + (1 << 15)) >> 16), -MAX_OFFSET, MAX_OFFSET)
        self.h = (self.h + d_h + noise_v(draw_v(self.seed, step, self.p, 2), s_h)) & 0xFFFF
        C, S = self.heads[self.h, 0][:, None], self.heads[self.h, 1][:, None]
        z = np.array(zq, np.int64)
        use = (z >= 0) & (z < self.zmax)
        z, ac, as_ = z[use][None, :], self.table[use, 0][None, :], self.table[use, 1][None, :]
        dx = (C * ac - S * as_ + (1 << 15)) >> 16
        dy = (S * ac + C * as_ + (1 << 15)) >> 16
        I = (self.tx[:, None] + (1 << 15) + ((z * dx + (1 << 29)) >> 30)) >> 16
        J = (self.ty[:, None] + (1 << 15) + ((z * dy + (1 << 29)) >> 30)) >> 16
        inside = (I >= 0) & (I < self.W) & (J >= 0) & (J < self.H)
        plane = np.asarray(self.plane())
        d2 = np.where(inside, plane[np.where(inside, I, 0), np.where(inside, J, 0)].astype(np.int64), FAR)
        cost = self.pen_d2[np.minimum(d2, self.c2 + 1)].sum(axis=1)
        self.acc = np.minimum(self.acc - self.min_prev + cost, mref.ACC_CAP)
        self.rec, self.w = mref.record_of(self.tx.tolist(), self.ty.tolist(), self.h.tolist(), self.acc.tolist(), self.wtab,
                                          self.w_shift, step)
        self.min_prev = self.rec.amin
        return self.rec

    def resample(self):
        """Rule 40 by a search in the prefix sums: N cum_i and u0 + j W1 stay below 2^53, exact in int64."""
        u0 = mref.draw(self.seed, self.step_count, self.n, 15) % self.rec.w1
        cum = np.cumsum(np.array(self.w, np.int64)) * self.n
        src = np.searchsorted(cum, u0 + np.arange(self.n, dtype=np.int64) * self.rec.w1, side="right")
        self.tx, self.ty, self.h = self.tx[src], self.ty[src], self.h[src]
        self.acc = np.zeros(self.n, np.int64)
        self.min_prev = 0
        self.w = None
        return src.tolist()

    def particles(self):
        return (self.tx.astype(np.int64), self.ty.astype(np.int64), self.h.astype(np.uint32), self.acc.astype(np.uint32))
