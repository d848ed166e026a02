"""The localiser's likelihood-field model on the device (kc_mcl_set_field_model; DESIGN.md 4.11 rules 44 and 45) against
the statement tests/worldmap_mcl_field_ref.py: states, acc, record and resampled states bit for bit against the loop
form, and the global run at 16384 particles against the vectorised form (which tests/test_worldmap_mcl_field_cpu.py
shows equal to the loop form).  One context a test.

The map is test_worldmap_mcl_gpu's: 97 x 61 with occupied, empty and never-observed cells."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import worldmap_dist_ref as dref  # noqa: E402
import worldmap_mcl_field_ref as fref  # noqa: E402
import worldmap_mcl_ref as mref  # noqa: E402
import worldmap_ref as ref  # noqa: E402

RES, ORIGIN = 0.05, (-0.33, 1.7)
W, H = 97, 61
OCC, UNK, EMP = ref.OCCUPIED, ref.UNEXPLORED, ref.EMPTY
RANGE = float(np.float32(float(np.float32(RES)) * 5.5))
REACH = 4
PEN_D2 = [min(65535, 5 * d + (d % 3)) for d in range(REACH * REACH + 1)]     # not monotonic: a wrong index shows
PEN_FAR = 97
PEN = [min(65535, 3 * i * i + i) for i in range(64)]                         # the beam model's, for the switch
ERR_SHIFT = 13
WTAB = [round(65536 * math.exp(-i / 8.0)) for i in range(128)]
W_SHIFT = 5
SKIP = mref.SKIP_NO_RETURN


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


@pytest.fixture(scope="module")
def cls():
    rng = np.random.default_rng(5)
    c = rng.choice(np.int8([OCC, UNK, EMP]), size=(W, H), p=[0.06, 0.15, 0.79]).astype(np.int8)
    c[0, :] = c[-1, :] = OCC
    c[:, 0] = c[:, -1] = OCC
    return c


def beams(n, start=-math.pi + 0.013):
    return start + np.arange(n) * (2 * math.pi / n)


class Pair:
    """A device localiser and the loop statement over one map and one distance plane, driven together."""

    def __init__(self, cls, n, b, seed=3, reach=REACH, flags=0, field=True):
        self.wref = ref.WorldMapRef(W, H, RES, ORIGIN)
        self.wref.set_prior(cls)
        self.map = kh.WorldMapContext(W, H, RES, ORIGIN)
        self.map.set_prior(cls)
        self.dist = None
        if reach:
            self.map.set_distance(reach, flags=flags)
            self.dist = dref.DistRef(self.wref.cls, reach, flags)
        ang = beams(b)
        self.dev = kh.MclContext(self.map, n, ang, RANGE, seed)
        self.ref = fref.MclFieldRef(self.wref.cls, RES, n, ang, RANGE, seed, dist=self.dist)
        assert self.dev.model_kind() == kh.MCL_MODEL_NONE
        if field:
            self.field()

    def field(self, pen_d2=PEN_D2):
        self.dev.set_field_model(pen_d2, PEN_FAR, WTAB, W_SHIFT)
        self.ref.set_field_model(pen_d2, PEN_FAR, WTAB, W_SHIFT)
        assert self.dev.model_kind() == kh.MCL_MODEL_FIELD

    def beam(self):
        self.dev.set_model(PEN, ERR_SHIFT, WTAB, W_SHIFT)
        self.ref.set_model(PEN, ERR_SHIFT, WTAB, W_SHIFT)
        assert self.dev.model_kind() == kh.MCL_MODEL_BEAM

    def update(self, grid, pose):
        got = self.map.update(grid, pose)
        assert got == self.wref.update(grid, pose)
        self.ref.cls = self.wref.cls                             # the statement's update makes a new plane
        if self.dist is not None:
            self.dist.cls = self.wref.cls
            self.dist.mark(*got)
        return got

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.dev.close()
        self.map.close()

    def same_particles(self, what=""):
        got, want = self.dev.particles(), self.ref.particles()
        for name, g, w in zip(("tx", "ty", "h", "acc"), got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5].ravel(), g[:4], w[:4])

    def init_pose(self, *a):
        self.dev.init_pose(*a)
        self.ref.init_pose(*a)
        self.same_particles("init")

    def step(self, *a, **kw):
        got = self.dev.step(*a, **kw)
        want = self.ref.step(*a, **kw)
        assert got.as_tuple() == want.as_tuple(), (got.as_tuple(), want.as_tuple())
        self.same_particles(f"step {want.step}")
        assert self.dev.step_count() == want.step
        return want

    def resample(self):
        self.dev.resample()
        src = self.ref.resample()
        self.same_particles("resample")
        return src


def scan(b, zmax, rng, plain=False):
    """b quantised ranges up to the range; unless plain, every fifth beam has no return and every seventh is skipped."""
    z = [int(v) for v in rng.integers(0, zmax, b)]
    if not plain:
        for k in range(b):
            if k % 5 == 3:
                z[k] = zmax
            if k % 7 == 5:
                z[k] = -1
    return z


def outside(p, zq):
    """How many endpoints of the statement's particles fall off the map on each side: (I < 0, I >= W, J < 0, J >= H)."""
    n = [0, 0, 0, 0]
    Hd = mref.headings()
    for i in range(p.n):
        C, S = Hd[p.h[i]]
        for k, (ac, as_) in enumerate(p.table):
            if 0 <= zq[k] < p.zmax:
                I, J = fref.endpoint(p.tx[i], p.ty[i], *fref.beam_direction(C, S, ac, as_), zq[k])
                for s, off in enumerate((I < 0, I >= W, J < 0, J >= H)):
                    n[s] += off
    return n


@pytest.mark.parametrize("b", [1, 24, 70])                      # above 64 a particle spans wavefronts; 70 does not divide 256
@pytest.mark.parametrize("n", [1, 3, 65, 300])
def test_field_steps_equal_the_statement(cls, n, b):
    """Three steps and a resample; the particles spread over the whole map and beyond its border."""
    rng = np.random.default_rng(n * 100 + b)
    with Pair(cls, n, b) as p:
        p.init_pose(round(W / 2 * 65536), round(H / 2 * 65536), 12345, 25 * 65536 if n > 3 else 65536, 20000)
        zmax = p.ref.zmax
        for k in range(3):
            rec = p.step(30000 * k, -7000, 900, 6000, 3000, 500, scan(b, zmax, rng, plain=b == 1), SKIP)
            if k == 1:
                p.resample()
        assert rec.step == 3 and (n == 1 or len(set(p.ref.acc)) > 1)


@pytest.mark.parametrize("side,pose", [(0, (1.0, 30.0)), (1, (95.5, 30.0)), (2, (48.0, 0.8)), (3, (48.0, 60.0))])
def test_endpoints_leave_the_map_on_every_side(cls, side, pose):
    with Pair(cls, 65, 24) as p:
        p.init_pose(round(pose[0] * 65536), round(pose[1] * 65536), 50000, 2 * 65536, 30000)
        zq = [int(5.4 * 65536)] * 24
        for _ in range(2):
            p.step(0, 0, 0, 3000, 3000, 300, zq)
            assert outside(p.ref, zq)[side] > 20
        # a plane where everything blocks: the border's FAR comes from the bounds test alone
        p.map.set_distance(REACH, flags=1)
        p.ref.dist = p.dist = dref.DistRef(p.wref.cls, REACH, 1)
        p.step(0, 0, 0, 3000, 3000, 300, zq)


def test_switching_models_keeps_the_particles(cls):
    rng = np.random.default_rng(9)
    with Pair(cls, 65, 24, field=False) as p:
        p.beam()
        p.init_pose(round(40 * 65536), round(30 * 65536), 1000, 3 * 65536, 3000)
        zmax = p.ref.zmax
        p.step(20000, 0, 100, 3000, 3000, 300, scan(24, zmax, rng), SKIP)
        p.field()
        p.same_particles("beam -> field")
        with pytest.raises(kh.KompassHipError, match=r"\[kc -5\]"):
            p.dev.resample()                                     # the weights were another table's
        p.step(20000, 0, 100, 3000, 3000, 300, scan(24, zmax, rng), SKIP)
        p.resample()
        p.step(20000, 0, 100, 3000, 3000, 300, scan(24, zmax, rng), SKIP)
        p.beam()
        p.same_particles("field -> beam")
        rec = p.step(20000, 0, 100, 3000, 3000, 300, scan(24, zmax, rng), SKIP | mref.UNKNOWN_BLOCKS)
        assert rec.step == 4


def test_a_step_right_after_an_update_sees_the_new_plane(cls):
    rng = np.random.default_rng(11)
    with Pair(cls, 65, 24) as p:
        p.init_pose(round(40 * 65536), round(30 * 65536), 1000, 3 * 65536, 3000)
        zmax = p.ref.zmax
        p.step(0, 0, 0, 3000, 3000, 300, scan(24, zmax, rng), SKIP)
        assert p.map.distance_info()[3]                          # the first step made the full refresh
        before = p.ref.dist.plane.copy()
        g = rng.choice(np.int32([100, 0]), size=(15, 15)).astype(np.int32)
        changed = sum(p.update(g, (ORIGIN[0] + 40 * RES, ORIGIN[1] + 30 * RES, 0.4))[0] for _ in range(4))   # evidence enough to turn
        assert changed > 0                                                                                   # classes both ways
        p.step(0, 0, 0, 3000, 3000, 300, scan(24, zmax, rng), SKIP)
        info = p.map.distance_info()
        assert info[2] == p.ref.dist.last_box and not info[3] and info[2][0] > 0       # a partial refresh, the statement's box
        assert (p.ref.dist.plane != before).any()
        p.step(0, 0, 0, 3000, 3000, 300, scan(24, zmax, rng), SKIP)
        assert p.map.distance_info()[2] == (-1, -1, -1, -1)      # nothing was dirty: no refresh launch


def test_refusals_queue_nothing(cls):
    with Pair(cls, 3, 4, reach=0, field=False) as p:
        p.dev.set_field_model(PEN_D2, PEN_FAR, WTAB, W_SHIFT)
        p.ref.set_field_model(PEN_D2, PEN_FAR, WTAB, W_SHIFT)
        p.init_pose(round(40 * 65536), round(30 * 65536), 1000, 65536, 3000)
        zq = [65536, 2 * 65536, -1, 70000]

        def refused(exc, match, *a):
            with pytest.raises(exc, match=match):
                p.dev.step(*a)
            assert p.dev.step_count() == 0
            p.same_particles("refused")

        refused(kh.KompassHipError, r"\[kc -5\]", 0, 0, 0, 0, 0, 0, zq, SKIP)                   # the plane is off
        p.map.set_distance(3)
        refused(kh.KompassHipError, r"\[kc -5\]", 0, 0, 0, 0, 0, 0, zq, SKIP)                   # c2 = 16 > 9
        assert p.map.distance_info()[2] == (-1, -1, -1, -1)                                    # ... and no refresh was queued
        p.map.set_distance(REACH)
        refused(ValueError, r"\[kc -1\]", 0, 0, 0, 0, 0, 0, zq, SKIP | mref.UNKNOWN_BLOCKS)     # the plane's own flag decides
        refused(ValueError, r"\[kc -1\]", 0, 0, 0, 0, 0, 0, zq, 0)                              # a -1 without the flag
        assert p.map.distance_info()[2] == (-1, -1, -1, -1)
        p.ref.dist = dref.DistRef(p.wref.cls, REACH)
        p.step(0, 0, 0, 0, 0, 0, zq, SKIP)
        for bad in ([7], [1] * 4097):
            with pytest.raises((ValueError, IndexError)):
                p.dev.set_field_model(bad, PEN_FAR, WTAB, W_SHIFT)
        assert p.dev.model_kind() == kh.MCL_MODEL_FIELD


# ---- the global run ----
def test_global_run_equals_the_vectorised_statement():
    """16384 x 24 over test_worldmap_mcl_field_cpu's room, drive, scans and noise: record and best particle at each of
    the 12 steps, the estimate within the CPU test's bounds."""
    import test_worldmap_mcl_field_cpu as cpu

    base = cpu.base
    c = base.room()
    path = base.drive()
    table = mref.scan_table(cpu.ROOM_BEAMS)
    scans = [base.sref.scan_pose(c, cpu.ROOM_RES, ref.quantise_pose(cpu.ROOM_RES, (0.0, 0.0), *q), table, cpu.ROOM_RANGE)[0] for q in path]
    seed = 3                                                     # the statement's worst yaw of the six
    pen, far, reach, wtab, ws = fref.field_tables(cpu.ROOM_RES, 0.1)
    dist = dref.DistRef(c, reach)
    vec = fref.MclFieldVec(c, cpu.ROOM_RES, cpu.GLOBAL_N, cpu.ROOM_BEAMS, cpu.ROOM_RANGE, seed, dist.field)
    vec.set_field_model(pen, far, wtab, ws)
    cells = 65536.0 / float(np.float32(cpu.ROOM_RES))
    s = (mref.noise_scale(base.NOISE[0] * cells), mref.noise_scale(base.NOISE[1] * cells),
         mref.noise_scale(base.NOISE[2] / (2 * math.pi) * 65536.0))
    with kh.WorldMapContext(base.ROOM_W, base.ROOM_H, cpu.ROOM_RES) as m:
        m.set_prior(c)
        m.set_distance(reach)
        with kh.MclContext(m, cpu.GLOBAL_N, cpu.ROOM_BEAMS, cpu.ROOM_RANGE, seed) as dev:
            dev.set_field_model(pen, far, wtab, ws)
            assert dev.init_global() == vec.init_global() == 10196
            for k in range(1, 13):
                d = mref.odometry_increment(cpu.ROOM_RES, path[k - 1], path[k])
                zq = mref.quantise_ranges(scans[k], cpu.ROOM_RES, cpu.ROOM_RANGE, SKIP)
                got, want = dev.step(*d, *s, zq, SKIP), vec.step(*d, *s, zq, SKIP)
                assert got.as_tuple() == want.as_tuple(), (k, got.as_tuple(), want.as_tuple())
                if mref.should_resample(want, vec.n):
                    dev.resample()
                    vec.resample()
            for g, w in zip(dev.particles(), vec.particles()):
                assert np.array_equal(g, w)
            rec = mref.Record(**dict(zip(mref.Record.FIELDS, got.as_tuple())))
            pos, yaw = base.errors(mref.estimate(rec, cpu.ROOM_RES, (0.0, 0.0)), path[-1])
            assert pos < cpu.GLOBAL_POS_BOUND and yaw < cpu.GLOBAL_YAW_BOUND


# ---- the front ends ----
def test_front_ends(cls):
    import kompass_cpp
    from kompass_core.mapping import MCL, WorldMap

    angles = beams(24)
    wm = WorldMap(W, H, RES, ORIGIN)
    wm.set_prior(cls)
    loc = MCL(wm, 65, angles, RANGE, sigma_hit=0.1, seed=4, model="field", skip_no_return=True, resample_ratio=(0, 1))
    assert loc.model == "field" and wm._map.distance_reach == 6               # ceil(3 * 0.1 / 0.05): enabled by the localiser
    pen, far, reach, wtab, ws = fref.field_tables(RES, 0.1)
    stmt = fref.MclFieldRef(cls, RES, 65, angles, RANGE, 4, dist=dref.DistRef(cls, reach))
    stmt.set_field_model(pen, far, wtab, ws)
    x0, y0 = ORIGIN[0] + 40 * RES, ORIGIN[1] + 30 * RES
    loc.init((x0, y0, 0.3), 0.1, 0.05)
    q = ref.quantise_pose(RES, ORIGIN, x0, y0, 0.0)
    stmt.init_pose(q[2], q[3], mref.quantise_heading(0.3), mref.noise_scale(0.1 * 65536.0 / float(np.float32(RES))),
                   mref.noise_scale(0.05 / (2 * math.pi) * 65536.0))
    ranges = np.linspace(0.02, 0.3, 24)
    ranges[5] = float("inf")
    a, b = (0.0, 0.0, 0.0), (0.03, 0.01, 0.02)
    est = loc.step(a, b, ranges)
    cell = 65536.0 / float(np.float32(RES))
    s = (mref.noise_scale(0.02 * cell), mref.noise_scale(0.01 * cell), mref.noise_scale(0.01 / (2 * math.pi) * 65536.0))
    want = stmt.step(*mref.odometry_increment(RES, a, b), *s, mref.quantise_ranges(ranges, RES, RANGE, SKIP), SKIP)
    assert tuple(est.record) == want.as_tuple()
    e = mref.estimate(want, RES, ORIGIN)
    assert (est.x, est.y, est.yaw) == (e["x"], e["y"], e["yaw"])
    with pytest.raises(ValueError):
        MCL(wm, 65, angles, RANGE, model="walk")
    assert MCL(wm, 8, angles, RANGE).model == "beam"
    # the class itself: tables by hand, a plane that is already long enough is left alone
    cm = kompass_cpp.mapping.MCL(wm._map, 65, list(angles), RANGE, 4)
    assert not cm.field_model
    cm.set_field_tables(pen[:10], far, 3, wtab, ws)
    assert cm.field_model and wm._map.distance_reach == 6
    cm.set_model()
    assert not cm.field_model
