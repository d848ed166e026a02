"""Seeded random walks over one kh.WorldMapContext with one kh.MclContext and one kh.MppiContext attached, against
tests/worldmap_walk_model.py's WalkModel after every call.  The kernels are pinned elsewhere; what a
walk is after lies between them, on the host: the distance plane's dirty box, the shifts a localiser has still to follow, the
state a refused call must leave alone.

For every operation the device's return value equals the model's bit for bit, a refusal raises the type the binding maps
the model's refusal to, and distance_info() equals the model's; after every mutating operation and every refusal so do
planes(), offset() and info(); at the end everything once more, and distance() against dist2_plane of the whole map.  The
distance plane is read only where the walk reads it: a read more would refresh it, and hide the lazy path a walk is for.
Each MPPI step runs with the walk's present team; the first three of a walk that are not refused run with 1, 4 and 8 lanes.

KC_WALK_SEEDS="21,22,..." adds seeds for a longer campaign, as KC_FUZZ_SEEDS does in test_gpu_fuzz.py.  An added seed walks
KC_WALK_OPS operations (240 unless set): past the quotas of the first 80 a walk is drawn freely, which is where a campaign
finds what the named sequences do not hold.

tests/test_worldmap_walk_cpu.py shows without a device that these walks meet their coverage conditions and would tell six
kinds of faulty host apart.  The model alone takes 0.63, 0.15, 0.80, 0.43, 0.40 and 0.57 s for the default seeds 11 to 16
(80 operations each, one CPU core; most of it the beam model's step at N = 300 and the planes of reach 70); a walk's test,
model and device together, 0.3 to 1.2 s on an MI355X.

FIXED holds fixed lists for findings, as named tests beside the seeds."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402

import mppi_movers_ref as mm  # noqa: E402
import worldmap_dist_ref as dref  # noqa: E402
import worldmap_points_ref as pref  # noqa: E402
import worldmap_walk_model as wk  # noqa: E402
from worldmap_walk_model import Refused, WalkModel, freeze, walk_config, walk_ops  # noqa: E402

_SEEDS = list(wk.DEFAULT_SEEDS) + [int(s) for s in os.environ.get("KC_WALK_SEEDS", "").split(",") if s.strip()]
LONG_OPS = int(os.environ.get("KC_WALK_OPS", "240"))
TEAMS = (1, 4, 8)


class Device:
    """The three contexts of a walk, and each operation as the call it stands for, its result in the model's form."""

    def __init__(self, config):
        self.config = config
        self.ctx = kh.WorldMapContext(wk.W, wk.H, wk.RES, wk.ORIGIN0)
        self.mcl = kh.MclContext(self.ctx, config["N"], wk.MCL_ANGLES, wk.RANGE_MAX, seed=config["mcl_seed"])
        self.mppi = kh.MppiContext(self.ctx, config["K"], wk.MPPI_T, seed=config["mppi_seed"])
        m = wk.mppi_model()
        self.mppi.set_model(m.f_lo, m.f_hi, m.l_hi, m.h_hi, m.kq, m.s)
        self.labels = None
        self.team = 8
        self.mppi.set_team(self.team)
        self.all_teams = 0                                                # MPPI steps run with every team so far
        self.info, self.repeated = None, False

    def close(self):
        for c in (self.mppi, self.mcl, self.ctx):
            c.close()

    def call(self, op, a):
        """-> the result, or Refused(name)."""
        self.info, self.repeated = None, False
        try:
            return getattr(self, "_" + op[0])(a, *op[1:])
        except ValueError:
            return Refused("ValueError")
        except IndexError:
            return Refused("IndexError")
        except kh.KompassHipError as e:
            if "[kc -5]" not in str(e):                                   # KC_ERR_STATE alone is a refusal by state
                raise
            return Refused("StateError")

    def _update(self, a, *_):
        return self.ctx.update(a["grid"], a["pose"])

    def _integrate(self, a, *_):
        return self.ctx.integrate(a["pose"], a["angles"], a["zq"], a["range_max"], a["flags"])

    def _shift(self, a, di, dj):
        self.ctx.shift(di, dj)

    def _recentre(self, a, *_):
        return self.ctx.recentre(a["x"], a["y"], a["margin"], a["stride"])

    def _set_prior(self, a, *_):
        self.ctx.set_prior(a["grid"])

    def _clear(self, a):
        self.ctx.clear()

    def _set_model(self, a, occ_thr):
        self.ctx.set_model(occ_thr=occ_thr)

    def _set_distance(self, a, reach, flags):
        self.ctx.set_distance(reach, flags=flags)

    def _points(self, a, *_):
        if a["count_only"]:
            return self.ctx.points(a["x"], a["y"], a["max_sensor_range"], count_only=True)
        xyz, bounds = self.ctx.points(a["x"], a["y"], a["max_sensor_range"])
        return pref.sort_points(xyz, wk.RES, self.ctx.info()[3]), bounds

    def _scan(self, a, *_):
        return self.ctx.scan(a["poses"], a["angles"], a["range_max"], return_cells=True, flags=a["flags"])

    def _match(self, a, *_):
        return self.ctx.match(a["grid"], a["pose"], n_yaw=a["n_yaw"], yaw_step=a["yaw_step"], reach=a["reach"])

    def _distance(self, a):
        return self.ctx.distance()

    def _distance_refresh(self, a):
        self.ctx.distance_refresh()

    def _movers(self, a, *_):
        labels, rec, clusters = self.ctx.movers(a["pose"], a["angles"], a["zq"], a["range_max"], m2=a["m2"])
        self.labels = labels.copy()
        return labels, rec, clusters

    def _mcl_model(self, a, kind, reach):
        if kind == "beam":
            self.mcl.set_model(*wk.mcl_beam_tables())
        else:
            self.mcl.set_field_model(*wk.mcl_field_tables(reach))

    def _mcl_init_pose(self, a, tx, ty, h, s_xy, s_h):
        self.mcl.init_pose(tx, ty, h, s_xy, s_h)

    def _mcl_init_global(self, a):
        return self.mcl.init_global()

    def _mcl_step(self, a, *_):
        rec = self.mcl.step(*wk.MCL_STEP, a["zq"], a["flags"])
        return rec.as_tuple(), self.mcl.last_fit().as_tuple()

    def _mcl_resample(self, a):
        self.mcl.resample()

    def _mcl_resample_inject(self, a, n):
        self.mcl.resample_inject(n)

    def _mcl_particles(self, a):
        return self.mcl.particles()

    def _mppi_set_costs(self, a, c2):
        c = wk.mppi_costs(c2)
        self.mppi.set_costs(c.r2, c.pen_d2, c.pen_far, c.pen_hit, c.w_path, c.qcap, c.w_goal, c.wtab, c.w_shift)

    def _mppi_set_path(self, a, p0, p1):
        self.mppi.set_path(*wk.mppi_path(p0, p1))

    def _mppi_set_movers(self, a, rows, pen):
        mv = mm.movers(rows, pen)
        self.mppi.set_movers(*mv[:7], pen_hit_mv=mv.pen_hit)

    def _mppi_set_team(self, a, lanes):
        self.mppi.set_team(lanes)
        self.team = lanes

    def _one_step(self, a):
        U, rec = self.mppi.step(a["tx"], a["ty"], a["h"], a["U"], a["step"])
        return [tuple(int(v) for v in r) for r in U], rec.as_tuple() + (int(rec.n_hit_moving),), self.mppi.costs()

    def _mppi_step(self, a, *_):
        out = self._one_step(a)                                           # a refusal leaves here
        self.info = self.ctx.distance_info()                              # of the walk's own step, not of the repeats below
        self.repeated = self.all_teams < 3
        if self.repeated:
            self.all_teams += 1
            for lanes in TEAMS:
                self.mppi.set_team(lanes)
                again = self._one_step(a)
                assert freeze(again) == freeze(out), f"{lanes} lanes a sample give another step than {self.team}"
            self.mppi.set_team(self.team)
        return out

    # what the device reports between calls
    def state(self):
        cls, ev = self.ctx.planes()
        return dict(cls=cls, evidence=ev, offset=self.ctx.offset(), info=self.ctx.info())


def model_state(model):
    cls, ev = model.planes()
    return dict(cls=cls, evidence=ev, offset=model.offset(), info=model.info())


def differs(got, want):
    """'' when equal bit for bit, else where not."""
    g, w = freeze(got), freeze(want)
    if g == w:
        return ""
    if isinstance(want, dict):
        return "; ".join(f"{k}: {differs(got[k], want[k])}" for k in want if freeze(got[k]) != freeze(want[k]))
    if isinstance(want, np.ndarray) and isinstance(got, np.ndarray) and got.shape == want.shape:
        at = np.argwhere(np.asarray(got) != np.asarray(want))
        return f"{len(at)} elements differ, the first at {at[0].tolist()}: {got[tuple(at[0])]!r} for {want[tuple(at[0])]!r}"
    if isinstance(want, (tuple, list)) and isinstance(got, (tuple, list)) and len(got) == len(want):
        return "; ".join(f"[{i}] {differs(a, b)}" for i, (a, b) in enumerate(zip(got, want)) if freeze(a) != freeze(b))
    return f"{got!r} for {want!r}"[:600]


def run_walk(ops, config, label):
    """The walk on the device and on the model side by side."""
    model, dev = WalkModel(config), Device(config)

    def fail(i, what):
        pytest.fail(f"{label}, operation {i} {ops[i]!r}: {what}\nreplay with WalkModel.replay(ops, {config!r}), ops =\n{ops[:i + 1]!r}",
                    pytrace=False)

    try:
        for i, op in enumerate(ops):
            a = model.args(op, dev.labels)
            try:
                got = dev.call(op, a)
            except AssertionError as e:
                fail(i, str(e))
            want = model.apply(op)
            if isinstance(want, Refused) or isinstance(got, Refused):
                if not (isinstance(got, Refused) and isinstance(want, Refused) and got == want):
                    fail(i, f"the device answers {str(got)[:200]}, the model {str(want)[:200]}")
            elif differs(got, want):
                fail(i, "the result: " + differs(got, want))
            if op[0] in wk.MUTATING or isinstance(want, Refused):
                d = differs(dev.state(), model_state(model))
                if d:
                    fail(i, "the map afterwards: " + d)
            if dev.info is not None and dev.info != model.distance_info():
                fail(i, f"distance_info() after the step is {dev.info!r}, the model's {model.distance_info()!r}")
            if dev.repeated:
                model.read_again()
            if dev.ctx.distance_info() != model.distance_info():
                fail(i, f"distance_info() is {dev.ctx.distance_info()!r}, the model's {model.distance_info()!r}")
        last = len(ops) - 1
        d = differs(dev.state(), model_state(model))
        if d:
            fail(last, "the map at the end: " + d)
        if model.dist is not None:
            d = differs(dev.ctx.distance(), dref.dist2_plane(model.map.cls, model.dist.reach, model.dist.flags))
            if d:
                fail(last, "the distance plane at the end: " + d)
        if model.mcl.tx is not None:
            model._note = {}
            d = differs(dev.mcl.particles(), model._op_mcl_particles({}))
            if d:
                fail(last, "the particles at the end: " + d)
    finally:
        dev.close()
    return model


@pytest.mark.parametrize("seed", _SEEDS)
def test_walk(seed):
    n = wk.DEFAULT_OPS if seed in wk.DEFAULT_SEEDS else LONG_OPS
    ops = walk_ops(seed, n)
    model = run_walk(ops, walk_config(seed), f"seed {seed}")
    assert len(model.log) == len(ops) == n


FIXED = {
    # kc_mcl_init_global dropped the particles of an earlier init before it found that the map had no free cell, so the
    # refused call left a localiser that answered nothing until the next init.  No seeded walk reaches this with particles
    # in hand, so the list is not reduced from one.  Here the particles stay, follow the shift, and step on.
    "refused_init_global_keeps_the_particles": [
        ("set_prior", 3), ("mcl_model", "field", 3), ("set_distance", 4, 0), ("mcl_init_pose", 20 << 16, 18 << 16, 1000, 56756, 520),
        ("mcl_step", (20.0, 18.0, 0.3), 0), ("clear",), ("mcl_init_global",), ("shift", 2, -1), ("mcl_particles",),
        ("set_prior", 4), ("mcl_step", (18.0, 19.0, 0.3), 0), ("mcl_resample",), ("mcl_particles",)],
    # Seed 26 at 240 operations, reduced: a step, kc_mcl_set_model, a resample.  The library refuses the resample, as its
    # header says (the weights of the last step are another table's); worldmap_mcl_ref.MclRef.set_model kept them, where
    # MclFieldRef.set_field_model already dropped them.  The statement was wrong and is mended; the library is unchanged.
    "set_model_drops_the_weights": [
        ("set_prior", 3), ("mcl_model", "field", 3), ("set_distance", 4, 0), ("mcl_init_pose", 20 << 16, 18 << 16, 1000, 56756, 520),
        ("mcl_step", (20.0, 18.0, 0.3), 0), ("mcl_model", "beam", 0), ("mcl_resample_inject", 16), ("mcl_step", (20.0, 18.0, 0.3), 0),
        ("mcl_resample_inject", 16), ("mcl_particles",)],
}


@pytest.mark.parametrize("name", sorted(FIXED))
def test_fixed_walk(name):
    config = dict(N=65, K=65, mcl_seed=5, mppi_seed=6)
    model = run_walk(FIXED[name], config, name)
    assert [n["refused"] for n in model.log].count(True) == 1 and model.log[6]["refused"]
