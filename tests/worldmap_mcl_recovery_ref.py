"""The localiser's fit record and its recovery by injected free-cell particles (DESIGN.md 4.11 rules 59 to 63,
include/kompass_hip.h kc_mcl_last_fit, kc_mcl_recovery_update, kc_mcl_resample_inject) as a statement in Python ints, on
top of worldmap_mcl_ref.MclRef / worldmap_mcl_field_ref.MclFieldRef.

FitRef is the loop statement: after the parent's step it forms every particle's step cost again from the new states, a
loop a particle and a loop a beam, and the fit from those; its resample_inject is rule 40's copy followed by rule 62's
draws, a loop an injected slot over the list of free cells.

FitVec gives worldmap_mcl_field_ref.MclFieldVec the same two over numpy int64 / uint64.  As every vectorised form here it
may serve as a reference only where it has been shown equal to the loop form, which
tests/test_worldmap_mcl_recovery_cpu.py does on a small case.

Filter is the host classes' policy around either form: the fit, rule 61's two averages, the decision to resample."""
import numpy as np

import worldmap_mcl_field_ref as fref
import worldmap_mcl_ref as mref
from worldmap_ref import EMPTY, MAX_OFFSET

MAX_PENALTY = 0xFFFF
MAX_FIT = MAX_PENALTY * 256
DEFAULT_POLICY = (4, 1, 1, 4)                                    # a_slow, a_fast, max_num / max_den: judgement, not measurement


class Fit:
    """Rule 59: kc_mcl_fit."""
    FIELDS = ("cost_sum", "cost_min", "cost_best", "step")

    def __init__(self, cost, best, step):
        self.cost_sum, self.cost_min, self.cost_best, self.step = sum(cost), min(cost), cost[best], step

    def as_tuple(self):
        return tuple(getattr(self, f) for f in self.FIELDS)

    def __repr__(self):
        return "Fit(" + ", ".join(f"{f}={getattr(self, f)}" for f in self.FIELDS) + ")"


# ---- rule 60: the beams of a step that contributed ----
def beams_used(zq, zmax, field):
    if field:
        return sum(1 for z in zq if 0 <= z < zmax)               # rule 45
    return sum(1 for z in zq if z != -1)                         # rule 33


# ---- rule 61: kc_mcl_recovery_update, in the library's order ----
def recovery_update(cost_sum, n, b_used, state, a_slow=4, a_fast=1, max_num=1, max_den=4):
    """state: (slow, fast, primed) -> (state, m or -1, n_inject).  ValueError: KC_ERR_INVALID, IndexError: KC_ERR_RANGE."""
    slow, fast, primed = state
    if not 0 <= a_slow <= 30:
        raise ValueError("a_slow outside 0 .. 30")
    if not 0 <= a_fast <= 30:
        raise ValueError("a_fast outside 0 .. 30")
    if max_den == 0:
        raise ValueError("max_den is 0")
    if max_num > max_den:
        raise ValueError("max_num above max_den")
    if not 1 <= n <= mref.MAX_PARTICLES:
        raise IndexError("particles outside 1 .. 65536")
    if b_used > mref.MAX_BEAMS:
        raise IndexError("more beams than a step has")
    if cost_sum > n * b_used * MAX_PENALTY:
        raise IndexError("cost_sum above N B_used 65535")
    if primed and not (0 <= slow <= MAX_FIT and 0 <= fast <= MAX_FIT):
        raise IndexError("an average outside 0 .. 65535 * 256")
    if b_used == 0:
        return (slow, fast, primed), -1, 0
    m = cost_sum * 256 // (n * b_used)
    if not primed:
        return (m, m, True), m, 0
    slow += (m - slow) >> a_slow                                 # Python's >> floors, as an arithmetic shift does
    fast += (m - fast) >> a_fast
    if fast <= slow:
        return (slow, fast, True), m, 0
    return (slow, fast, True), m, min(n * max_num // max_den, n * (fast - slow) // fast)


# ---- rule 62: the injected slots ----
def injected_slots(n_particles, n):
    return [j for j in range(n_particles) if (j + 1) * n // n_particles > j * n // n_particles]


def free_cells(cls):
    """The KC_EMPTY cells in the order of I + J * width."""
    c = np.asarray(cls)
    W, H = c.shape
    return [(I, J) for J in range(H) for I in range(W) if int(c[I][J]) == EMPTY]


def _checked(m, n):
    if not 0 <= n <= m.n:
        raise IndexError("more injected slots than particles")
    if m.w is None:
        raise mref.StateError("a resample needs a step's weights")


class FitRef(fref.MclFieldRef):
    """The loop statement, either sensor model."""
    fit = None

    def set_model(self, *a):
        super().set_model(*a)
        self.fit = None

    def set_field_model(self, *a):
        super().set_field_model(*a)
        self.fit = None

    def init_pose(self, *a):
        super().init_pose(*a)                                             # a refused init leaves the fit with the particles
        self.fit = None

    def init_global(self):
        n = super().init_global()
        self.fit = None
        return n

    def step_costs(self, zq, flags):
        """cost_p of rule 34 or rules 44 and 45 for the states as the step left them."""
        Hd = mref.headings()
        cls = np.asarray(self.cls)
        plane = self.dist.field() if self.field is not None else None
        out = []
        for p in range(self.n):
            C, S = Hd[self.h[p]]
            cost = 0
            for k, (ac, as_) in enumerate(self.table):
                if self.field is None:
                    pen, err_shift = self.model[0], self.model[1]
                    if zq[k] < 0:
                        continue
                    q = mref.expected_range(cls, self.W, self.H, (C, S, self.tx[p], self.ty[p]), ac, as_, self.Rc, self.zmax, flags)
                    cost += pen[min(abs(q - zq[k]) >> err_shift, len(pen) - 1)]
                else:
                    pen_d2, pen_far = self.field[0], self.field[1]
                    if not 0 <= zq[k] < self.zmax:
                        continue
                    I, J = fref.endpoint(self.tx[p], self.ty[p], *fref.beam_direction(C, S, ac, as_), zq[k])
                    d2 = int(plane[I][J]) if 0 <= I < self.W and 0 <= J < self.H else fref.FAR
                    cost += pen_d2[d2] if d2 <= len(pen_d2) - 1 else pen_far
            out.append(cost)
        return out

    def step(self, d_f, d_l, d_h, s_f, s_l, s_h, zq, flags=0):
        before = [a - self.min_prev for a in self.acc] if self.acc is not None else None
        rec = super().step(d_f, d_l, d_h, s_f, s_l, s_h, zq, flags)      # a refused step leaves the fit as it was
        cost = self.step_costs(zq, flags)
        assert self.acc == [min(b + c, mref.ACC_CAP) for b, c in zip(before, cost)]      # rule 35 over the same costs
        self.fit = Fit(cost, rec.best, rec.step)
        return rec

    def resample_inject(self, n):
        """Rule 62 -> the source of every slot, -1 for an injected one."""
        _checked(self, n)
        step = self.step_count
        src = self.resample()
        free = free_cells(self.cls) if n else []
        if not free:
            return src
        for j in injected_slots(self.n, n):
            I, J = free[mref.draw(self.seed, step, j, 16) % len(free)]
            v = mref.draw(self.seed, step, j, 17)
            self.tx[j] = (I << 16) + (v & 0xFFFF) - (1 << 15)
            self.ty[j] = (J << 16) + ((v >> 16) & 0xFFFF) - (1 << 15)
            self.h[j] = (v >> 32) & 0xFFFF
            src[j] = -1
        return src


_U = np.uint64


class FitVec(fref.MclFieldVec):
    """MclFieldVec with the step's costs kept for the fit, and rule 62."""
    fit = None

    def init_pose(self, *a):
        super().init_pose(*a)
        self.fit = None

    def init_global(self):
        n = super().init_global()
        self.fit = None
        return n

    def step(self, d_f, d_l, d_h, s_f, s_l, s_h, zq, flags=0):
        """MclFieldVec.step, the cost kept."""
        self.step_count += 1
        step = self.step_count
        C, S = self.heads[self.h, 0], self.heads[self.h, 1]
        F = d_f + fref.noise_v(fref.draw_v(self.seed, step, self.p, 0), s_f)
        L = d_l + fref.noise_v(fref.draw_v(self.seed, step, self.p, 1), s_l)
        self.tx = np.clip(self.tx + ((C * F - S * L + (1 << 15)) >> 16), -MAX_OFFSET, MAX_OFFSET)
        self.ty = np.clip(self.ty + ((S * F + C * L + (1 << 15)) >> 16), -MAX_OFFSET, MAX_OFFSET)
        self.h = (self.h + d_h + fref.noise_v(fref.draw_v(self.seed, step, self.p, 2), s_h)) & 0xFFFF
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
        d2 = np.where(inside, plane[np.where(inside, I, 0), np.where(inside, J, 0)].astype(np.int64), fref.FAR)
        cost = self.pen_d2[np.minimum(d2, self.c2 + 1)].sum(axis=1)
        self.acc = np.minimum(self.acc - self.min_prev + cost, mref.ACC_CAP)
        self.rec, self.w = mref.record_of(self.tx.tolist(), self.ty.tolist(), self.h.tolist(), self.acc.tolist(), self.wtab,
                                          self.w_shift, step)
        self.min_prev = self.rec.amin
        self.fit = Fit(cost.tolist(), self.rec.best, step)
        return self.rec

    def resample_inject(self, n):
        _checked(self, n)
        step = self.step_count
        src = self.resample()
        free = np.flatnonzero(np.asarray(self.cls).T.reshape(-1) == EMPTY) if n else np.zeros(0, np.int64)
        if free.size == 0:
            return src
        j = np.arange(self.n, dtype=np.int64)
        j = j[(j + 1) * n // self.n > j * n // self.n]
        cell = free[(fref.draw_v(self.seed, step, j, 16) % _U(free.size)).astype(np.int64)]
        v = fref.draw_v(self.seed, step, j, 17)
        self.tx[j] = ((cell % self.W) << 16) + (v & _U(0xFFFF)).astype(np.int64) - (1 << 15)
        self.ty[j] = ((cell // self.W) << 16) + ((v >> _U(16)) & _U(0xFFFF)).astype(np.int64) - (1 << 15)
        self.h[j] = ((v >> _U(32)) & _U(0xFFFF)).astype(np.int64)
        src = np.array(src)
        src[j] = -1
        return src.tolist()


class Filter:
    """What the host classes do around a step (rule 63): the fit m, rule 61's averages, which always run, and the resample:
    when rule 40 asks for one or, with a policy, when n_inject > 0.  policy: None (recovery off) or (a_slow, a_fast,
    max_num, max_den)."""

    def __init__(self, m, policy=None, r_num=1, r_den=2):
        self.m, self.policy, self.ratio = m, policy, (r_num, r_den)
        self.state = (0, 0, False)

    def reset(self):
        """After either init."""
        self.state = (0, 0, False)

    def step(self, d_f, d_l, d_h, s_f, s_l, s_h, zq, flags=0):
        m = self.m
        rec = m.step(d_f, d_l, d_h, s_f, s_l, s_h, zq, flags)
        used = beams_used(zq, m.zmax, getattr(m, "field", True) is not None)
        self.state, fit, n = recovery_update(m.fit.cost_sum, m.n, used, self.state, *(self.policy or DEFAULT_POLICY))
        if self.policy is None:
            n = 0
        resampled = mref.should_resample(rec, m.n, *self.ratio) or n > 0
        out = dict(rec=rec, fit=fit, fit_slow=self.state[0], fit_fast=self.state[1], injected=n, resampled=resampled,
                   cost_min=m.fit.cost_min, cost_best=m.fit.cost_best, beams_used=used, fit_record=m.fit)
        if resampled:
            m.resample_inject(n)
        return out
