"""One model of a world map and the contexts attached to it, and the seeded operation walks over it (DESIGN.md 4.11 and
4.12; tests/test_worldmap_walk_cpu.py and tests/test_worldmap_walk_gpu.py).

WalkModel holds what a kh.WorldMapContext, one kh.MclContext and one kh.MppiContext over it hold between calls, and
answers every operation of a walk by calling the statements that exist.  It states no rule of 4.11 or 4.12 (the few state
checks no statement has are listed at the end):

  planes, model parameters   worldmap_integrate_ref.IntegrateRef, whose update, set_prior, clear and set_model are
                             worldmap_ref.WorldMapRef's.  (worldmap_shift_ref.RollingWorldMapRef.update says the same through
                             the same WorldMapRef; the one used here is WorldMapRef.update.)
  offset, origin, shifts     worldmap_shift_ref.check_offset, shift_planes, origin_after, recentre_plan, robot_cell
  distance plane             worldmap_dist_ref.DistRef (mark, mark_all, refresh) for the lazy state and for what
                             distance_info() reports; worldmap_dist_ref.dist2_plane of the whole map for the plane every
                             consumer reads.  Both are formed at every read and kept in `last_planes` for the CPU test, which
                             asserts them equal; a model with read_lazy set hands its consumers the lazy one.
  read-only calls            worldmap_points_ref, worldmap_scan_ref.scan, worldmap_match_ref.match_pose, worldmap_movers_ref
  the localiser              worldmap_mcl_recovery_ref.FitRef; worldmap_shift_ref.shift_particles for rule 50, the shifts since
                             the last entry kept as one sum and applied when the next entry runs
  the controller             mppi_movers_ref.step (mppi_ref.step's roll-out with rule 16; equal to it without movers)

A refused operation leaves the model exactly as it was: the statements' own checks and StateErrors come before any change,
and the one thing this module changes ahead of a statement, the pending shift of the particles, it puts back.

An operation is a tuple of Python literals, (kind, arguments...), so that a list of them printed by repr() is accepted by
WalkModel.replay.  What a call is handed beyond the literals (a local grid, the quantised ranges of a scan) is formed by
WalkModel.args(op) from the literals and the model's present state, for the model and the device alike.

walk_ops(seed, n) draws a list while it drives a WalkModel: the list is a function of the seed and of the model's own
state, and can be produced, and its coverage asserted, without a device.  With three calls a kind, 78 of the 80 operations
of a default walk are spoken for, and most of them by the sequences the coverage conditions name: such a walk is a shuffle
of those sequences with drawn arguments.  A longer walk (n > 80) goes on, once the quotas are met, with any kind that is
ready and with the unhinted draws: shifts up to +-6 cells, (0, 0) and past the cap, any reach with either flag.

Checks that are the model's own, because no statement has them (the host's wording is read once, here): the plane's copy
and refresh while the plane is off; an MPPI step while it is off or with c2 above reach^2, and before costs and a path;
a path point beyond 2^20 cells; a team other than 1, 4 or 8 lanes; particles, a resample before an init."""
import copy
import math
from collections import namedtuple

import numpy as np

import mppi_movers_ref as mm
import mppi_ref as mp
import worldmap_dist_ref as dref
import worldmap_integrate_ref as iref
import worldmap_match_ref as mtref
import worldmap_mcl_field_ref as fref
import worldmap_mcl_recovery_ref as rref
import worldmap_mcl_ref as mref
import worldmap_movers_ref as wm
import worldmap_points_ref as pref
import worldmap_ref as wref
import worldmap_scan_ref as sref
import worldmap_shift_ref as shref

W, H, RES, ORIGIN0 = 45, 38, 0.05, (-0.4, 0.3)
RANGE_MAX = 1.5                                                           # 30 cells: the scans', the integrations', the localiser's
MCL_BEAMS, MPPI_T, MPPI_M = 24, 8, 17
MCL_ANGLES = [(-math.pi + 2.0 * math.pi * k / MCL_BEAMS) for k in range(MCL_BEAMS)]
DEFAULT_SEEDS = (11, 12, 13, 14, 15, 16)
DEFAULT_OPS = 80

MUTATING = ("update", "integrate", "shift", "recentre", "set_prior", "clear", "set_model", "set_distance")
CLASS_READERS = ("points", "scan", "match")
PLANE_READERS = ("distance", "distance_refresh", "movers")                # and a field step, and an MPPI step
MCL_KINDS = ("mcl_model", "mcl_init_pose", "mcl_init_global", "mcl_step", "mcl_resample", "mcl_resample_inject", "mcl_particles")
MPPI_KINDS = ("mppi_set_costs", "mppi_set_path", "mppi_set_movers", "mppi_set_team", "mppi_step")
KINDS = MUTATING + CLASS_READERS + PLANE_READERS + MCL_KINDS + MPPI_KINDS
MCL_ENTRIES = ("mcl_step", "mcl_resample", "mcl_resample_inject", "mcl_particles")


Refused = namedtuple("Refused", "error")                                  # a refused operation's result


class StateError(RuntimeError):
    """KC_ERR_STATE where no statement has the check: particles before an init, the plane's copy while it is off."""


STATE_ERRORS = (StateError, mref.StateError, mp.StateError, wm.StateError)


def refusal_of(exc):
    """The name a refusal goes by in a result: the binding maps KC_ERR_INVALID to ValueError, KC_ERR_RANGE to IndexError
    and KC_ERR_STATE to KompassHipError."""
    if isinstance(exc, STATE_ERRORS):
        return "StateError"
    if isinstance(exc, IndexError):
        return "IndexError"
    if isinstance(exc, ValueError):
        return "ValueError"
    raise exc


def walk_config(seed):
    """What a seed's contexts are created with: N and K on both sides of their kernels' edges over the default seeds."""
    return dict(N=(65, 300)[seed % 2], K=(65, 257)[(seed // 2) % 2], mcl_seed=1000 + seed, mppi_seed=2000 + seed)


# ---- the inputs a literal stands for ----
def prior_grid(k):
    """A room outline, unexplored outside it, with scattered occupied cells and one block inside: int8 [W, H]."""
    rng = np.random.default_rng(7000 + int(k))
    g = np.full((W, H), wref.UNEXPLORED, np.int8)
    i0, j0, i1, j1 = 2 + int(k) % 3, 3, W - 4, H - 3 - int(k) % 2
    g[i0:i1 + 1, j0:j1 + 1] = wref.EMPTY
    g[i0, j0:j1 + 1] = g[i1, j0:j1 + 1] = wref.OCCUPIED
    g[i0:i1 + 1, j0] = g[i0:i1 + 1, j1] = wref.OCCUPIED
    for _ in range(10):
        g[int(rng.integers(i0 + 2, i1 - 1)), int(rng.integers(j0 + 2, j1 - 1))] = wref.OCCUPIED
    bi, bj = int(rng.integers(i0 + 4, i1 - 7)), int(rng.integers(j0 + 4, j1 - 6))
    g[bi:bi + 3, bj:bj + 2] = wref.OCCUPIED
    return g


def local_grid(gseed, gh, gw):
    """A mapper's grid: int32 [gh, gw], mostly empty, some occupied, some unknown."""
    rng = np.random.default_rng(8000 + int(gseed))
    return rng.choice(np.array([0, 0, 0, 0, 100, 100, -1], np.int32), size=(int(gh), int(gw))).astype(np.int32)


def beam_angles(n):
    return [(-math.pi + 2.0 * math.pi * k / n) for k in range(int(n))]


def mppi_model():
    return mp.Model(0, 65536, 0, 1500, 0, (mref.noise_scale(0.4 * 65536.0), 0, mref.noise_scale(400.0)))


def mppi_costs(c2):
    pen = [round(60.0 * max(0.0, 1.0 - math.sqrt(d) / math.sqrt(c2))) for d in range(int(c2) + 1)]
    wtab = [round(65535.0 * math.exp(-4.0 * i / 64.0)) for i in range(256)]
    return mp.Costs(1, pen, 0, 4000, 8, 400 << 16, 20, wtab, 2)


def mppi_path(a, b):
    """MPPI_M points from cell a to cell b in 4.12's Q16 coordinates."""
    px = [round((a[0] + (b[0] - a[0]) * j / (MPPI_M - 1)) * 65536.0) for j in range(MPPI_M)]
    py = [round((a[1] + (b[1] - a[1]) * j / (MPPI_M - 1)) * 65536.0) for j in range(MPPI_M)]
    return px, py


def mcl_beam_tables():
    return mref.sensor_tables(RES, 0.1)


def mcl_field_tables(reach):
    pen, far, _, wtab, w_shift = fref.field_tables(RES, 0.1, reach=int(reach))
    return pen, far, wtab, w_shift


MCL_STEP = (3000, 0, 50, mref.noise_scale(2000.0), 0, mref.noise_scale(30.0))   # d_f, d_l, d_h, s_f, s_l, s_h


def freeze(x):
    """A result as nested tuples of Python values: arrays by dtype, shape and bytes, so that == is bit for bit."""
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        return ("array", a.dtype.str, a.shape, a.tobytes())
    if isinstance(x, dict):
        return tuple((k, freeze(v)) for k, v in sorted(x.items()))
    if isinstance(x, (tuple, list)):
        return tuple(freeze(v) for v in x)
    if isinstance(x, (np.integer, np.bool_)):
        return int(x)
    if isinstance(x, np.floating):
        return float(x)
    return x


class _PlaneView:
    """What FitRef and MoversRef take for a DistRef: the reach, and field() as the model's read of the plane."""

    def __init__(self, model):
        self.model = model

    @property
    def reach(self):
        return self.model.dist.reach

    def field(self):
        return self.model.read_plane()


class WalkModel:
    read_lazy = False

    def __init__(self, config):
        self.config = dict(config)
        self.map = iref.IntegrateRef(W, H, RES, ORIGIN0)
        self.OI = self.OJ = 0
        self.dist = None
        self.view = _PlaneView(self)
        self.last_planes = None
        self.labels = None                                                # of the last `movers` that was not refused
        self.mcl = rref.FitRef(self.map.cls, RES, config["N"], MCL_ANGLES, RANGE_MAX, config["mcl_seed"])
        self.pending = (0, 0)
        self.m_model = mppi_model()
        self.m_costs = self.m_path = None
        self.m_movers = mm.NONE
        self.team = 8
        self.log = []                                                     # a dict an operation: what the coverage conditions read
        self._full = (None, None)

    # ---- what the device reports between calls ----
    @property
    def origin(self):
        return (shref.origin_after(ORIGIN0[0], RES, self.OI), shref.origin_after(ORIGIN0[1], RES, self.OJ))

    def info(self):
        return W, H, float(np.float32(RES)), self.origin

    def offset(self):
        return self.OI, self.OJ

    def planes(self):
        return self.map.cls, self.map.evidence

    def distance_info(self):
        if self.dist is None:
            return 0, 0, (-1, -1, -1, -1), False
        return self.dist.reach, self.dist.flags, tuple(self.dist.last_box), bool(self.dist.last_full)

    def full_plane(self):
        """dist2_plane of the whole map at the plane's reach and flags."""
        key = (self.map.cls.tobytes(), self.dist.reach, self.dist.flags)
        if self._full[0] != key:
            self._full = (key, dref.dist2_plane(self.map.cls, self.dist.reach, self.dist.flags))
        return self._full[1]

    # ---- the lazy state: the places a wrong host would differ in ----
    def _new_dist(self, reach, flags):
        return dref.DistRef(self.map.cls, reach, flags) if reach else None

    def _mark(self, changed, box):
        if self.dist is not None:
            self.dist.mark(changed, box)

    def _mark_all(self):
        if self.dist is not None:
            self.dist.mark_all()

    def _mark_shift(self, di, dj):
        self._mark_all()

    def _refresh(self):
        self.dist.cls = self.map.cls
        return self.dist.refresh()

    def _pend(self, di, dj):
        self.pending = (self.pending[0] + di, self.pending[1] + dj)

    def _refused_integrate(self, a):
        pass

    def _marks(self, marks):
        return marks

    def read_plane(self):
        """Rule 43's refresh, then the plane a consumer reads; an operation refreshes once, however often its statement asks
        (FitRef reads the plane for the step and again for the fit)."""
        if self._note.get("plane_read"):
            return self.dist.plane if self.read_lazy else self.full_plane()
        box = self._refresh()
        lazy, full = self.dist.plane, self.full_plane()
        self.last_planes = (lazy.copy(), full)
        self._note["plane_read"] = True
        self._note["refreshed"] = box
        return lazy if self.read_lazy else full

    def read_again(self):
        """The last reading call made once more, as the device test does with an MPPI step for every team: a refresh with
        nothing to do, after which the last box is all -1."""
        self._refresh()

    def _need_plane(self, c2, what):
        if self.dist is None:
            raise StateError("the map's distance plane is off")
        if c2 > self.dist.reach ** 2:
            raise StateError(f"{what} above the plane's reach^2")

    # ---- the arguments a call is handed ----
    def world_pose(self, cell_pose):
        """(cell I, cell J, yaw) in the map's present offset -> (x, y, yaw) in the world."""
        ox, oy = self.origin
        r = float(np.float32(RES))
        return ox + cell_pose[0] * r, oy + cell_pose[1] * r, float(cell_pose[2])

    def _ranges_from(self, cell_pose, angles):
        """The map's own scan from a pose, metres a beam; all range_max where the pose cannot be quantised."""
        try:
            return sref.scan(self.map.cls, RES, self.origin, [self.world_pose(cell_pose)], angles, RANGE_MAX)[0][0]
        except IndexError:
            return np.full(len(angles), RANGE_MAX)

    def args(self, op, labels=None):
        """The concrete arguments of an operation, as a dict; a function of the literals and the present state.  labels: the
        device's own of its last `movers`, for the skip mask of an integration that takes one."""
        kind, a = op[0], op[1:]
        labels = self.labels if labels is None else labels
        if kind == "update":
            return dict(grid=local_grid(a[0], a[1], a[2]), pose=self.world_pose(a[3]))
        if kind == "integrate":
            cell_pose, n, zseed, flags, skip = a
            angles = beam_angles(n)
            rng = np.random.default_rng(9000 + zseed)
            r = np.array(self._ranges_from(cell_pose, angles), np.float64)
            r = np.where(rng.random(n) < 0.3, r * rng.uniform(0.3, 0.9, n), r)       # something new in front of the map's own
            r[rng.random(n) < 0.1] = math.inf
            r[rng.random(n) < 0.05] = math.nan
            zq = iref.quantise_ranges(r, RES, RANGE_MAX)
            masked = 0
            if skip and labels is not None and len(labels) == n:
                mask = wm.skip_mask(labels)
                zq, masked = wm.apply_skip(zq, mask), int(mask.sum())
            return dict(pose=self.world_pose(cell_pose), angles=angles, zq=zq, range_max=RANGE_MAX, flags=flags, masked=masked)
        if kind == "recentre":
            x, y, _ = self.world_pose((a[0], a[1], 0.0))
            return dict(x=x, y=y, margin=a[2], stride=a[3])
        if kind == "set_prior":
            return dict(grid=prior_grid(a[0]))
        if kind == "points":
            x, y, _ = self.world_pose((a[0], a[1], 0.0))
            return dict(x=x, y=y, max_sensor_range=a[2], count_only=bool(a[3]))
        if kind == "scan":
            return dict(poses=[self.world_pose(p) for p in a[0]], angles=beam_angles(a[1]), range_max=RANGE_MAX, flags=a[2])
        if kind == "match":
            true_pose, (gh, gw), (k0, u0, v0), n_yaw, yaw_step, reach = a
            x, y, yaw = self.world_pose(true_pose)
            r = float(np.float32(RES))
            try:
                grid = mtref.gather(self.map, (x, y, yaw), gh, gw)
            except IndexError:
                grid = np.zeros((gh, gw), np.int32)
            return dict(grid=grid, pose=(x - u0 * r, y - v0 * r, yaw - k0 * yaw_step), n_yaw=n_yaw, yaw_step=yaw_step, reach=reach)
        if kind == "movers":
            cell_pose, n, discs, m2 = a
            angles = beam_angles(n)
            r = self._ranges_from(cell_pose, angles)
            pose = self.world_pose(cell_pose)
            try:
                q = wref.quantise_pose(RES, self.origin, *pose)
                r = wm.shorten_by_discs(r, RES, q, angles, [(int(d[0] * 65536), int(d[1] * 65536), d[2]) for d in discs])
            except IndexError:
                pass
            return dict(pose=pose, angles=angles, zq=iref.quantise_ranges(r, RES, RANGE_MAX), range_max=RANGE_MAX, m2=m2)
        if kind == "mcl_step":
            r = self._ranges_from(a[0], MCL_ANGLES)
            return dict(zq=mref.quantise_ranges(r, RES, RANGE_MAX, a[1]), flags=a[1])
        if kind == "mppi_step":
            (tx, ty, h), (F, Hh), step = a
            return dict(tx=tx, ty=ty, h=h, U=[(F, 0, Hh)] * MPPI_T, step=step)
        return {}

    # ---- the operations ----
    def apply(self, op):
        """-> the expected result; Refused(name) for a refusal."""
        kind = op[0]
        self._note = dict(kind=kind, refused=False, plane_read=False)
        try:
            out = getattr(self, "_op_" + kind)(self.args(op), *op[1:])
        except (ValueError, IndexError, RuntimeError) as e:
            out = Refused(refusal_of(e))
            self._note.update(refused=True, plane_read=False, why=str(e))
        self.log.append(self._note)
        return out

    @classmethod
    def replay(cls, ops, config):
        """A list from a fresh model -> (the model, the results)."""
        m = cls(config)
        return m, [m.apply(op) for op in ops]

    def _changed(self, res):
        self._mark(*res)
        self._note["changed"], self._note["box"] = res
        return res

    def _op_update(self, a, *_):
        return self._changed(self.map.update(a["grid"], a["pose"]))

    def _op_integrate(self, a, *_):
        try:
            marks, _ = self.map.marks(a["pose"], a["angles"], a["zq"], a["range_max"], a["flags"])
        except (ValueError, IndexError):
            self._refused_integrate(a)
            raise
        self._note["masked"] = a["masked"]
        return self._changed(self.map.apply(self._marks(marks)))

    def _shift(self, di, dj):
        shref.check_offset(self.OI, self.OJ, di, dj)
        if di or dj:
            self.map.evidence, self.map.cls = shref.shift_planes(self.map.evidence, self.map.cls, di, dj)
            self._mark_shift(di, dj)
            self._pend(di, dj)
        self.OI += di
        self.OJ += dj
        self.map.origin = self.origin
        self._note["shift"] = (di, dj)

    def _op_shift(self, a, di, dj):
        self._shift(di, dj)

    def _op_recentre(self, a, *_):
        shref.recentre_plan(W, H, 0, 0, a["margin"], a["stride"])         # the policy's refusals come first
        ic, jc = shref.robot_cell(RES, self.origin, a["x"], a["y"])
        di, dj = shref.recentre_plan(W, H, ic, jc, a["margin"], a["stride"])
        self._shift(di, dj)
        return di, dj

    def _op_set_prior(self, a, *_):
        self.map.set_prior(a["grid"])
        self._mark_all()

    def _op_clear(self, a):
        self.map.clear()
        self._mark_all()

    def _op_set_model(self, a, occ_thr):
        self.map.set_model(occ_thr=occ_thr)
        self._mark_all()

    def _op_set_distance(self, a, reach, flags):
        dref.check(reach, flags)
        self._note.update(reach=reach, reach_before=self.dist.reach if self.dist is not None else 0,
                          dirty_before=self.dist is not None and self.dist.dirty is not None)
        self.dist = self._new_dist(reach, flags)

    def _op_points(self, a, *_):
        xyz, n, bounds = pref.worldmap_points_ref(self.map.cls, RES, self.origin, a["x"], a["y"], a["max_sensor_range"])
        self._note["trivial"] = n == 0
        return (n, bounds) if a["count_only"] else (xyz, bounds)

    def _op_scan(self, a, *_):
        ranges, cells = sref.scan(self.map.cls, RES, self.origin, a["poses"], a["angles"], a["range_max"], a["flags"])
        self._note["trivial"] = bool((ranges == float(np.float32(a["range_max"]))).all())
        return ranges, cells

    def _op_match(self, a, *_):
        m, _, _ = mtref.match_pose(self.map, a["grid"], a["pose"], a["n_yaw"], a["yaw_step"], a["reach"])
        return m._asdict()

    def _op_distance(self, a):
        self._need_plane(0, "")
        return self.read_plane().copy()

    def _op_distance_refresh(self, a):
        self._need_plane(0, "")
        self.read_plane()

    def _op_movers(self, a, *_):
        labels, rec, clusters = wm.MoversRef(self.map, self.view if self.dist is not None else None).detect(
            a["pose"], a["angles"], a["zq"], a["range_max"], m2=a["m2"])
        self.labels = labels
        self._note["trivial"] = rec.n_dynamic == 0
        return labels, tuple(rec), [tuple(c) for c in clusters]

    # the localiser
    def _mcl(self, entry, call):
        """One call of the localiser: its view of the map, rule 50 ahead of an entry, and everything back on a refusal."""
        m = self.mcl
        m.cls, m.dist = self.map.cls, (self.view if self.dist is not None else None)
        keep = (m.tx, m.ty, self.pending)
        if entry and m.tx is None and entry != "mcl_step":
            raise StateError("no particles before an init")
        if entry and m.tx is not None:
            self._note["followed"] = self.pending
            m.tx, m.ty = shref.shift_particles(m.tx, m.ty, *self.pending)
            self.pending = (0, 0)
        try:
            return call(m)
        except (ValueError, IndexError, RuntimeError):
            m.tx, m.ty, self.pending = keep
            raise

    def _op_mcl_model(self, a, kind, reach):
        if kind == "beam":
            self._mcl(False, lambda m: m.set_model(*mcl_beam_tables()))
        else:
            self._mcl(False, lambda m: m.set_field_model(*mcl_field_tables(reach)))

    def _started(self, out):
        self.pending = (0, 0)
        self._note["pending_dropped"] = True
        return out

    def _op_mcl_init_pose(self, a, tx, ty, h, s_xy, s_h):
        self._started(self._mcl(False, lambda m: m.init_pose(tx, ty, h, s_xy, s_h)))

    def _op_mcl_init_global(self, a):
        return self._started(self._mcl(False, lambda m: m.init_global()))

    def _op_mcl_step(self, a, *_):
        self._note["field"] = self.mcl.field is not None
        rec = self._mcl("mcl_step", lambda m: m.step(*MCL_STEP, a["zq"], a["flags"]))
        self._note["trivial"] = all(v == mref.ACC_CAP for v in self.mcl.acc)
        return rec.as_tuple(), self.mcl.fit.as_tuple()

    def _op_mcl_resample(self, a):
        self._mcl(True, lambda m: m.resample())

    def _op_mcl_resample_inject(self, a, n):
        self._mcl(True, lambda m: m.resample_inject(n))

    def _op_mcl_particles(self, a):
        return self._mcl(True, lambda m: m.particles())

    # the controller
    def _op_mppi_set_costs(self, a, c2):
        c = mppi_costs(c2)
        mp.check(self.config["K"], MPPI_T, 1, None, c)
        self.m_costs = c

    def _op_mppi_set_path(self, a, p0, p1):
        px, py = mppi_path(p0, p1)
        mp.check(self.config["K"], MPPI_T, len(px))
        if any(abs(v) > wref.MAX_OFFSET for v in px + py):
            raise IndexError("a path point lies more than 2^20 cells from the origin")
        self.m_path = (px, py)

    def _op_mppi_set_movers(self, a, rows, pen):
        mv = mm.movers(rows, pen)
        mm.check_movers(mv)
        self.m_movers = mv if rows else mm.NONE

    def _op_mppi_set_team(self, a, lanes):
        if lanes not in (1, 4, 8):
            raise ValueError("a sample takes 1, 4 or 8 lanes")
        self.team = lanes

    def _op_mppi_step(self, a, *_):
        if self.m_costs is None or self.m_path is None:
            raise StateError("a step needs costs and a path")
        K = self.config["K"]
        mp.check_step(K, MPPI_T, a["tx"], a["ty"], a["h"], a["U"], a["step"])
        self._need_plane(len(self.m_costs.pen_d2) - 1, "c2")
        U, rec, S = mm.step(self.read_plane(), K, self.config["mppi_seed"], self.m_model, self.m_costs, *self.m_path, a["tx"], a["ty"],
                            a["h"], a["U"], a["step"], self.m_movers)
        self._note["trivial"] = rec.n_hit == K
        return U, tuple(rec), np.asarray(S).astype(np.uint32)


# ---- the generator ----
class _Walk:
    """Draws operations while it drives a model.  Every kind has a quota of three; sequences the coverage conditions name
    are queued as wishes, a kind a step, and drawn like any other operation when their turn comes."""

    def __init__(self, seed, n):
        self.rng = np.random.default_rng(seed)
        self.n = n
        self.model = WalkModel(walk_config(seed))
        self.ops = []
        self.count = {k: 0 for k in KINDS}
        self.wishes = []
        self.step_no = 0
        self.last_update = None
        self.wiped = False
        self.free_run = False                                             # every quota is met: the rest of a longer walk is drawn freely

    # small draws
    def ri(self, lo, hi):
        return int(self.rng.integers(lo, hi + 1))

    def pick(self, seq):
        return seq[int(self.rng.integers(0, len(seq)))]

    def chance(self, p):
        return bool(self.rng.random() < p)

    def cells(self, value):
        return np.argwhere(self.model.map.cls == value)

    def free_cell(self, clear2=0):
        """A free cell, at more than clear2 (squared cells) from anything occupied where there is one."""
        m = self.model
        free = m.map.cls == wref.EMPTY
        if clear2:
            far = free & (dref.dist2_plane(m.map.cls, 6) > clear2)
            free = far if far.any() else free
        c = np.argwhere(free)
        if len(c) == 0:
            return self.ri(5, W - 6), self.ri(5, H - 6)
        i, j = c[int(self.rng.integers(0, len(c)))]
        return int(i), int(j)

    def cell_pose(self, inside=None):
        """(I, J, yaw) in cells: mostly inside the map, sometimes outside it, rarely beyond rule 3's 2^20 cells."""
        u = self.rng.random()
        yaw = round(float(self.rng.uniform(-3.1, 3.1)), 3)
        if inside is None and u < 0.03:
            return float((1 << 20) + 10), 5.0, yaw
        if inside is None and u < 0.15:
            return float(self.pick((-4, W + 3))), float(self.ri(-4, H + 3)), yaw
        i, j = self.free_cell() if inside == "free" else (self.ri(2, W - 3), self.ri(2, H - 3))
        return i + round(float(self.rng.uniform(-0.4, 0.4)), 2), j + round(float(self.rng.uniform(-0.4, 0.4)), 2), yaw

    # one draw a kind
    def draw(self, kind, hint=None):
        m, d = self.model, self
        if kind == "update":
            if hint == "saturate" and self.last_update is not None:
                return self.last_update
            gh, gw = self.pick((9, 12, 15)), self.pick((9, 12, 15))
            pose = self.cell_pose("in" if hint else None)
            if hint == "corner":
                pose = (W - 5.0, H - 6.0, pose[2])
                gh = gw = 9
            self.last_update = ("update", self.ri(0, 999), gh, gw, pose)
            return self.last_update
        if kind == "integrate":
            if hint == "skip" and m.labels is not None:
                return ("integrate", self.movers_pose, len(m.labels), self.ri(0, 999), 1, True)
            pose = self.cell_pose("free" if hint else None)
            unknown = self.cells(wref.UNEXPLORED)
            if hint in ("unknown", "refused") and len(unknown):           # where a ray changes a class whatever the evidence
                i, j = unknown[int(self.rng.integers(0, len(unknown)))]
                pose = (float(i), float(j), pose[2])
            if hint == "corner":                                          # far from the update's corner
                near = unknown[unknown[:, 0] <= 12] if len(unknown) else unknown
                i, j = near[int(self.rng.integers(0, len(near)))] if len(near) else (2, 3)
                pose = (float(i), float(j), pose[2])
            flags = 2 if hint == "refused" or self.chance(0.05) else self.ri(0, 1)     # 2: no flag of rule 52's
            return ("integrate", pose, self.pick((24, 24, 64, 96) if hint != "corner" else (24,)), self.ri(0, 999), flags, False)
        if kind == "shift":
            if hint == "clearing":
                if self.chance(0.5):
                    return ("shift", self.pick((W, -W - 3)), self.ri(-2, 2))
                return ("shift", self.ri(-2, 2), self.pick((H, -H - 1)))
            if hint == "moves":                                           # within +-6 cells, not (0, 0)
                di, dj = self.ri(-6, 6), self.ri(-6, 6)
                return ("shift", di or self.pick((-1, 1)), dj)
            if hint == "still":
                return ("shift", 0, 0)
            u = self.rng.random()
            if u < 0.08:
                return ("shift", 0, 0)
            if u < 0.14:
                return ("shift", (1 << 30) + 3, 0)                        # past rule 46's cap
            return ("shift", self.ri(-6, 6), self.ri(-6, 6))
        if kind == "recentre":
            i, j = (self.ri(0, W - 1), self.ri(0, H - 1)) if self.chance(0.7) else (self.ri(-6, W + 5), self.ri(-6, H + 5))
            return ("recentre", float(i), float(j), self.pick((4, 8, 12)), self.pick((1, 2, 4)))
        if kind == "set_prior":
            return ("set_prior", self.ri(0, 9))
        if kind == "clear":
            return ("clear",)
        if kind == "set_model":
            return ("set_model", self.pick((1, 2, 3)))
        if kind == "set_distance":
            if hint is not None:                                          # (reach, flags) of a sequence
                return ("set_distance",) + tuple(hint)
            reach = self.pick((4, 9, 9, 70, 0))
            return ("set_distance", reach, self.ri(0, 1) if reach else 0)
        if kind == "points":
            occ = self.cells(wref.OCCUPIED)
            i, j = occ[int(self.rng.integers(0, len(occ)))] if len(occ) else (self.ri(0, W), self.ri(0, H))
            return ("points", float(int(i) + self.ri(-3, 3)), float(int(j) + self.ri(-3, 3)), self.pick((0.3, 0.6, 1.5)), self.ri(0, 1))
        if kind == "scan":
            poses = [self.cell_pose("free" if self.chance(0.8) else None) for _ in range(self.ri(1, 3))]
            return ("scan", poses, self.pick((1, 7, 24, 64, 65)), self.ri(0, 1))
        if kind == "match":
            return ("match", self.cell_pose("free" if self.chance(0.85) else None), (self.pick((12, 15)), self.pick((12, 15))),
                    (self.ri(-1, 1), self.ri(-2, 2), self.ri(-2, 2)), 1, 0.02, 2)
        if kind in ("distance", "distance_refresh"):
            return (kind,)
        if kind == "movers":
            i, j = self.free_cell(16)
            pose = (float(i), float(j), round(float(self.rng.uniform(-3.1, 3.1)), 3))
            discs = []
            for _ in range(self.ri(1, 2)):
                ci, cj = self.free_cell(25)
                discs.append((ci + 0.5, cj + 0.5, self.pick((1.0, 1.5))))
            if self.chance(0.04):
                pose = self.cell_pose()
            self.movers_pose = pose
            return ("movers", pose, self.pick((64, 96, 96)), discs, 25 if hint == "m2" else self.pick((4, 4, 4, 9, 25)))
        if kind == "mcl_model":
            if hint is not None:
                return ("mcl_model", "beam", 0) if hint == "beam" else ("mcl_model", "field", hint)
            if m.mcl.field is not None and self.chance(0.3):
                return ("mcl_model", "beam", 0)
            return ("mcl_model", "field", self.pick((3, 3, 8)))          # back from the beam model, mostly
        if kind == "mcl_init_pose":
            i, j = self.free_cell(4)
            tx = (1 << 36) + 1 if hint is None and self.chance(0.05) else (i << 16)     # a sequence's init is not the refused one
            return ("mcl_init_pose", tx, j << 16, self.ri(0, 65535), mref.noise_scale(0.5 * 65536), mref.noise_scale(300.0))
        if kind == "mcl_init_global":
            return ("mcl_init_global",)
        if kind == "mcl_step":
            return ("mcl_step", self.cell_pose("free"), self.pick((0, 0, 2)))
        if kind == "mcl_resample":
            return ("mcl_resample",)
        if kind == "mcl_resample_inject":
            return ("mcl_resample_inject", self.pick((0, 1, m.config["N"] // 4, m.config["N"])))
        if kind == "mcl_particles":
            return ("mcl_particles",)
        if kind == "mppi_set_costs":
            return ("mppi_set_costs", hint if hint is not None else self.pick((16, 16, 81)))
        if kind == "mppi_set_path":
            return ("mppi_set_path", self.free_cell(4), self.free_cell(4))
        if kind == "mppi_set_movers":
            if self.chance(0.35):
                return ("mppi_set_movers", [], 0)
            rows = []
            for _ in range(self.ri(1, 3)):
                i, j = self.free_cell()
                rows.append((i << 16, j << 16, self.ri(-20000, 20000), self.ri(-20000, 20000), 4 << 16, 25 << 16, (200 * 65536) // 21))
            return ("mppi_set_movers", rows, 4000)
        if kind == "mppi_set_team":
            return ("mppi_set_team", self.pick((1, 4, 8)))
        if kind == "mppi_step":
            i, j = self.free_cell(9)
            tx = (1 << 36) + 1 if self.chance(0.04) else (i << 16) + self.ri(-20000, 20000)
            self.step_no += 1
            return ("mppi_step", (tx, (j << 16) + self.ri(-20000, 20000), self.ri(0, 65535)), (self.pick((20000, 40000)), self.ri(-300, 300)),
                    self.step_no)
        raise KeyError(kind)

    # what may come next
    def ready(self, kind, strict=False):
        """False for a kind whose answer now would be a refusal by state or trivial by the map, where another kind can
        come first."""
        m = self.model
        occ = int((m.map.cls == wref.OCCUPIED).sum())
        free = int((m.map.cls == wref.EMPTY).sum())
        on = m.dist is not None
        mc = m.mcl
        chance = (lambda p: False) if strict else self.chance
        if kind in ("clear", "set_model"):
            return self.free_run and chance(0.3)                          # else in the walk's one stretch of wipes alone
        if kind == "set_prior":
            return self.wiped
        if kind in ("points", "scan", "match"):
            return occ >= 12
        if kind == "movers":
            return (on or chance(0.05)) and free >= 150 and occ >= 12
        if kind in ("distance", "distance_refresh"):
            return on or chance(0.05)
        if kind == "mcl_init_global":
            return free > 0 or chance(0.04)
        if kind == "mcl_init_pose":
            return free > 0
        if kind == "mcl_step":
            has_model = mc.field is not None or mc.model is not None
            field_ok = mc.field is None or (on and len(mc.field[0]) - 1 <= m.dist.reach ** 2)
            return mc.tx is not None and has_model and (field_ok or chance(0.05)) and occ >= 12
        if kind in ("mcl_resample", "mcl_resample_inject"):
            return mc.w is not None or chance(0.04)
        if kind == "mcl_particles":
            return mc.tx is not None or chance(0.04)
        if kind == "mppi_step":
            ok = m.m_costs is not None and m.m_path is not None and on and len(m.m_costs.pen_d2) - 1 <= m.dist.reach ** 2
            return (ok and free >= 150) or (m.m_costs is not None and m.m_path is not None and chance(0.04))
        if kind in ("mppi_set_path", "mppi_set_movers"):
            return free > 0
        return True

    def need(self, kind):
        return max(0, 3 - self.count[kind])

    def draw_good(self, kind, hint=None):
        """draw(), for a reading kind up to eight times: the first whose answer on a copy of the model is neither trivial
        nor refused, now and then a refused one."""
        if kind in ("update", "integrate") and hint in ("in", "corner", "unknown", "free"):
            for _ in range(8):                                            # a sequence's change has to change a class
                op = self.draw(kind, hint)
                probe = copy.deepcopy(self.model)
                probe.apply(op)
                if probe.log[-1].get("changed", 0) > 0:
                    break
            return op
        if kind not in ("points", "scan", "movers", "mppi_step") or hint == "m2":
            return self.draw(kind, hint)
        for _ in range(8):
            op = self.draw(kind, hint)
            probe = copy.deepcopy(self.model)
            probe.apply(op)
            note = probe.log[-1]
            if (note["refused"] and self.chance(0.2)) or not (note["refused"] or note.get("trivial")):
                break
        return op

    def emit(self, op):
        self.ops.append(op)
        self.count[op[0]] += 1
        return self.model.apply(op)

    def reader(self):
        """A plane reader's kind: one that is still wanted, where one is ready."""
        m = self.model
        cand = [k for k in ("distance_refresh", "movers", "mppi_step", "mcl_step", "distance") if self.ready(k, strict=True)]
        if "mcl_step" in cand and m.mcl.field is None:
            cand.remove("mcl_step")
        cand = cand or ["distance_refresh"]
        wanted = [k for k in cand if self.need(k) and k != "distance"]     # the plane's copy is kept for where it decides
        return self.pick(wanted or cand[:1])

    SCRIPTS = {
        "a": [("reader", None), ("update", "in"), ("shift", "moves"), ("distance", None)],
        "b": [("reader", None), ("integrate", "corner"), ("update", "corner"), ("distance", None)],
        # with flags 1 unknown cells block, so that every change of class shows in the plane; the planes of flags 0 are (d)'s
        # second and (i)'s first, and the first of a walk that carries (c)
        "c": [("reader", None), ("set_distance", (0, 0)), ("update", "in"), ("set_distance", (70, 1)), ("distance", None)],
        "d": [("set_distance", (9, 1)), ("reader", None), ("update", "in"), ("set_distance", (70, 0)), ("reader", None),
              ("integrate", "unknown"), ("set_distance", (4, 1)), ("reader", None), ("movers", "m2")],
        # (e): the plane is read after the clearing shift with nothing else that marks it in between, then the map comes back
        "e": [("reader", None), ("shift", "clearing"), ("distance", None), ("set_prior", None)],
        "f": [("reader", None), ("reader", None)],
        "g1": [("mcl_init_pose", "inside"), ("mcl_step", None), ("shift", "moves"), ("shift", "moves"), ("mcl_resample", None)],
        "g2": [("mcl_init_pose", "inside"), ("mcl_step", None), ("shift", "moves"), ("shift", "moves"), ("mcl_resample_inject", None)],
        "g3": [("mcl_init_global", None), ("shift", "moves"), ("shift", "moves"), ("mcl_particles", None)],
        "g4": [("mcl_init_pose", "inside"), ("shift", "moves"), ("shift", "moves"), ("mcl_step", None)],
        # every wipe of a walk in one stretch, since a walk has three set_prior to bring the map back with; it holds (h)
        "w": [("mcl_init_pose", "inside"), ("clear", None), ("any", None), ("set_model", None), ("any", None), ("clear", None), ("any", None),
              ("set_model", None), ("any", None), ("clear", None), ("set_model", None), ("set_prior", "wiped"), ("mcl_model", "beam"), ("mcl_step", None),
              ("mcl_model", 3)],
        "i": [("set_distance", (9, 0)), ("reader", None), ("mppi_set_costs", 81), ("mcl_model", 8), ("mcl_init_pose", "inside"), ("set_distance", (4, 1)),
              ("mppi_step", None), ("mcl_step", None), ("set_distance", (70, 1)), ("mppi_step", None), ("mcl_step", None)],
        "j": [("movers", None), ("integrate", "skip")],
        "k": [("integrate", "refused"), ("integrate", "unknown")],
        "sat": [("update", "in"), ("update", "saturate")],
    }
    # Which sequences a seed carries, by seed % 6: with three calls a kind in 80 operations a walk has three shifts, three
    # set_distance and three steps to spend, so the sequences are dealt out so that each fits its walk's quotas and every
    # one of them, and the input of every wrong variant of the CPU test, comes up in two walks or more of any six
    # consecutive seeds.
    PLANS = {
        0: ("d", "g1", "a", "k", "w", "f"),
        1: ("i", "g2", "e", "b", "sat", "w", "f"),
        2: ("c", "g3", "a", "k", "j", "w", "f"),
        3: ("d", "g4", "e", "b", "w", "f"),
        4: ("i", "g1", "a", "k", "sat", "w", "f"),
        5: ("c", "g2", "e", "b", "j", "w", "f"),
    }

    def run(self, seed):
        plan = list(self.PLANS[seed % 6])
        first = [("set_prior", self.ri(0, 9)), ("mppi_set_costs", 16)]
        if "i" not in plan:                                               # (i) comes first and brings its own
            first.append(("mcl_model", "field", 3))
        far = float((1 << 20) + 10)
        if "c" in plan:
            first.append(("set_distance", 9, 0))                         # (d) and (i) spend all three themselves
            first.append(("scan", [(far, 5.0, 0.5)], 7, 0))               # a pose beyond rule 3's 2^20 cells
            # past rule 46's cap, or the shift that moves nothing: it launches nothing, marks nothing, and no particle follows it
            first.append(("shift", (1 << 30) + 3, 0) if "g3" in plan else ("shift", 0, 0))
        elif "d" in plan:
            first.append(("distance_refresh",))                           # the plane is off
            first.append(("mcl_step", (20.0, 20.0, 0.0), 0))              # a step before an init
            first.append(("scan", [(8.0, 20.0, 0.0)], 1, 0))              # one beam, at -pi: onto the room's wall
        for op in first:
            self.emit(op)
        self.emit(self.draw("mppi_set_path"))
        self.rng.shuffle(plan)
        plan.sort(key=lambda name: name in ("d", "i"))                     # the last is popped first: the plane comes on
        while len(self.ops) < self.n:
            left = self.n - len(self.ops)
            owed = sum(self.need(k) for k in KINDS)
            if not self.wishes and plan and self.chance(0.6):
                self.wishes = list(self.SCRIPTS[plan.pop()])
            if self.wishes:
                kind, hint = self.wishes.pop(0)
                if kind == "any":                                         # something wanted that an empty map can answer
                    pool = [k for k in KINDS if self.need(k) and self.ready(k, strict=True) and k not in MCL_KINDS
                            and k not in ("set_prior", "set_distance", "shift", "distance", "update", "integrate")]
                    if not pool:
                        continue
                    kind = self.pick(pool)
                self.wiped = self.wiped or hint == "wiped"              # the stretch of wipes is over: set_prior is the filler's again
                kind = self.reader() if kind == "reader" else kind
                self.emit(self.draw_good(kind, hint))
                continue
            self.free_run = owed == 0 and not plan
            if self.free_run:                                             # a walk longer than its quotas: any kind that is ready
                pool = [k for k in KINDS if self.ready(k)]
                self.emit(self.draw_good(self.pick(pool)))
                continue
            booked = [k for name in plan for k, _ in self.SCRIPTS[name]]    # what the sequences still to come will spend
            wanted = [k for k in KINDS if self.need(k) > booked.count(k)]
            fresh = [k for k in ("mcl_resample", "mcl_resample_inject") if self.need(k) and self.model.mcl.w is not None]
            if fresh:                                                     # a step's weights are there: the resample that is owed
                self.emit(self.draw(self.pick(fresh)))
                continue
            pool = [k for k in wanted if self.ready(k)]
            if not pool:                                                  # nothing wanted is ready: bring back what it waits for
                m = self.model
                needs_map = any(k in wanted for k in CLASS_READERS + ("movers", "mppi_step", "mcl_step", "mcl_init_pose"))
                if needs_map and ((m.map.cls == wref.OCCUPIED).sum() < 12 or (m.map.cls == wref.EMPTY).sum() < 150):
                    kind = "set_prior"
                elif m.dist is None:
                    kind = "set_distance"
                elif m.mcl.tx is None:
                    kind = "mcl_init_pose"
                else:
                    kind = self.pick(wanted or list(KINDS))
                self.emit(self.draw(kind, (9, 1) if kind == "set_distance" else None))
                continue
            weights = np.array([1.0 + self.need(k) for k in pool])
            kind = pool[int(self.rng.choice(len(pool), p=weights / weights.sum()))]
            self.emit(self.draw_good(kind))
        return self.ops


def walk_ops(seed, n=DEFAULT_OPS):
    """-> n operation tuples: a function of the seed and of the model's own state alone."""
    return _Walk(seed, n).run(seed)
