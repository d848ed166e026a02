"""The localiser's fit record and its injecting resample on the device (kc_mcl_last_fit, kc_mcl_resample_inject;
DESIGN.md 4.11 rules 59 to 63) against the statement tests/worldmap_mcl_recovery_ref.py, bit for bit: the loop form on
small cases, the vectorised form (which tests/test_worldmap_mcl_recovery_cpu.py shows equal to it) on the two large ones.
One context a test."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import worldmap_dist_ref as dref  # noqa: E402
import worldmap_mcl_field_ref as fref  # noqa: E402
import worldmap_mcl_recovery_ref as rref  # noqa: E402
import worldmap_mcl_ref as mref  # noqa: E402
import worldmap_ref as ref  # noqa: E402
import worldmap_shift_ref as sref  # noqa: E402

RES, ORIGIN = 0.05, (-0.33, 1.7)
W, H = 97, 61
OCC, UNK, EMP = ref.OCCUPIED, ref.UNEXPLORED, ref.EMPTY
RANGE = float(np.float32(float(np.float32(RES)) * 5.5))
REACH = 4
PEN_D2 = [min(65535, 5 * d + (d % 3)) for d in range(REACH * REACH + 1)]     # not monotonic: a wrong index shows
PEN_FAR = 97
PEN = [min(65535, 3 * i * i + i) for i in range(64)]
ERR_SHIFT = 13
WTAB = [round(65536 * math.exp(-i / 8.0)) for i in range(128)]
W_SHIFT = 5
SKIP = mref.SKIP_NO_RETURN


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def random_plane(w, h, seed=5, p=(0.06, 0.15, 0.79)):
    rng = np.random.default_rng(seed)
    return rng.choice(np.int8([OCC, UNK, EMP]), size=(w, h), p=list(p)).astype(np.int8)


@pytest.fixture(scope="module")
def cls():
    c = random_plane(W, H)
    c[0, :] = c[-1, :] = OCC
    c[:, 0] = c[:, -1] = OCC
    return c


def beams(n, start=-math.pi + 0.013):
    return start + np.arange(n) * (2 * math.pi / n)


class Pair:
    """A device localiser and the loop statement over one map, driven together."""

    def __init__(self, cls, n, b, field, seed=3):
        w, h = cls.shape
        self.wref = ref.WorldMapRef(w, h, RES, ORIGIN)
        self.wref.set_prior(cls)
        self.map = kh.WorldMapContext(w, h, RES, ORIGIN)
        self.map.set_prior(cls)
        self.dist = None
        if field:
            self.map.set_distance(REACH)
            self.dist = dref.DistRef(self.wref.cls, REACH, 0)
        ang = beams(b)
        self.dev = kh.MclContext(self.map, n, ang, RANGE, seed)
        self.ref = rref.FitRef(self.wref.cls, RES, n, ang, RANGE, seed, dist=self.dist)
        for m in (self.dev, self.ref):
            if field:
                m.set_field_model(PEN_D2, PEN_FAR, WTAB, W_SHIFT)
            else:
                m.set_model(PEN, ERR_SHIFT, WTAB, W_SHIFT)

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

    def step(self, *a):
        got = self.dev.step(*a)
        want = self.ref.step(*a)
        assert got.as_tuple() == want.as_tuple(), (got.as_tuple(), want.as_tuple())
        fit = self.dev.last_fit().as_tuple()
        assert fit == self.ref.fit.as_tuple(), (fit, self.ref.fit)
        self.same_particles(f"step {want.step}")
        return want

    def resample_inject(self, n):
        self.dev.resample_inject(n)
        src = self.ref.resample_inject(n)
        self.same_particles(f"inject {n}")
        assert self.dev.last_fit().as_tuple() == self.ref.fit.as_tuple()         # a resample leaves the fit
        return src

    def update(self, grid, pose):
        got = self.map.update(grid, pose)
        assert got == self.wref.update(grid, pose)
        self.ref.cls = self.wref.cls                             # the statement's update makes a new plane
        return got


def scan(b, zmax, rng, skip):
    """b quantised ranges up to the range; every fifth beam has no return, with SKIP every seventh is skipped."""
    z = [int(v) for v in rng.integers(0, zmax, b)]
    for k in range(b):
        if k % 5 == 3:
            z[k] = zmax
        if skip and k % 7 == 5:
            z[k] = -1
    return z


def no_fit(dev):
    with pytest.raises(kh.KompassHipError, match=r"\[kc -5\]"):
        dev.last_fit()


# ---- rule 59: the fit ----
@pytest.mark.parametrize("skip", [0, SKIP])
@pytest.mark.parametrize("b", [1, 5, 24])
@pytest.mark.parametrize("n", [1, 65, 300, 1025])                # below a wavefront, above one, above one pass of the weigh kernel
@pytest.mark.parametrize("field", [False, True])
def test_fit_equals_the_statement(cls, field, n, b, skip):
    """Two steps: the record and the particles are worldmap_mcl_ref's (today's), the fit the new statement's.  The second
    step's acc carries the first's and min_prev, its costs do not."""
    rng = np.random.default_rng(n * 100 + b)
    with Pair(cls, n, b, field) as p:
        no_fit(p.dev)
        p.init_pose(round(W / 2 * 65536), round(H / 2 * 65536), 12345, 25 * 65536 if n > 3 else 65536, 20000)
        no_fit(p.dev)
        zmax = p.ref.zmax
        for k in range(2):
            zq = scan(b, zmax, rng, skip)
            rec = p.step(30000 * k, -7000, 900, 6000, 3000, 500, zq, skip)
            used = rref.beams_used(zq, zmax, field)
            assert p.ref.fit.cost_sum <= n * used * 65535 and p.ref.fit.cost_min <= p.ref.fit.cost_best
            assert p.ref.fit.step == rec.step == k + 1
        if field:
            p.dev.set_field_model(PEN_D2, PEN_FAR, WTAB, W_SHIFT)
        else:
            p.dev.set_model(PEN, ERR_SHIFT, WTAB, W_SHIFT)
        no_fit(p.dev)                                            # a fit in another table's penalties


def test_cost_sum_beyond_32_bits():
    """4096 x 1024 rays of 65535: a field table whose pen_far is 65535 over a map without an occupied cell, so that every
    endpoint is FAR.  cost_sum = 2^22 * 65535; a particle's cost 1024 * 65535 < 2^30.  Against the vectorised statement
    and the closed form."""
    n, b = 4096, 1024
    c = np.full((W, H), EMP, np.int8)
    ang = beams(b)
    pen_d2 = [7] * (REACH * REACH + 1)
    with kh.WorldMapContext(W, H, RES, ORIGIN) as m:
        m.set_prior(c)
        m.set_distance(REACH)
        with kh.MclContext(m, n, ang, RANGE, 8) as dev:
            vec = rref.FitVec(c, RES, n, ang, RANGE, 8, dref.DistRef(c, REACH).field)
            for x in (dev, vec):
                x.set_field_model(pen_d2, 65535, WTAB, W_SHIFT)
                x.init_pose(round(W / 2 * 65536), round(H / 2 * 65536), 777, 20 * 65536, 20000)
            zq = [int(v) for v in np.random.default_rng(1).integers(0, dev.zmax, b)]
            got, want = dev.step(0, 0, 0, 6000, 3000, 500, zq), vec.step(0, 0, 0, 6000, 3000, 500, zq)
            assert got.as_tuple() == want.as_tuple()
            fit = dev.last_fit().as_tuple()
            assert fit == vec.fit.as_tuple() == (n * b * 65535, b * 65535, b * 65535, 1) and fit[0] > 1 << 37
            for g, w in zip(dev.particles(), vec.particles()):
                assert np.array_equal(g, w)
            assert kh.mcl_recovery_update(fit[0], n, b, (0, 0, False))[1] == 65535 * 256


# ---- rule 62: the injecting resample ----
def counts(n):
    return sorted({0, 1, n // 4, n - 1, n})


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300, 1025])
def test_inject_equals_the_statement(cls, n):
    """Every count of {0, 1, N / 4, N - 1, N} in turn on one context, a step before each."""
    rng = np.random.default_rng(n)
    with Pair(cls, n, 5, False) as p:
        p.init_pose(round(W / 2 * 65536), round(H / 2 * 65536), 12345, 25 * 65536, 20000)
        for k, count in enumerate(counts(n)):
            p.step(30000, -7000, 900, 6000, 3000, 500, scan(5, p.ref.zmax, rng, SKIP), SKIP)
            src = p.resample_inject(count)
            assert src.count(-1) == count and [j for j, s in enumerate(src) if s == -1] == rref.injected_slots(n, count)
            i, j = (np.array(p.ref.tx) + 32768) >> 16, (np.array(p.ref.ty) + 32768) >> 16
            inj = np.array(src) == -1
            assert (cls[i[inj], j[inj]] == EMP).all() and (p.dev.particles()[3] == 0).all()
        with pytest.raises(IndexError, match=r"\[kc -2\]"):
            p.dev.resample_inject(n + 1)                         # the range before the state
        with pytest.raises(kh.KompassHipError, match=r"\[kc -5\]"):
            p.dev.resample_inject(1)                             # no step since the resample
        p.same_particles("refused")


@pytest.mark.parametrize("h", [1, 2, 1030])                      # 1030: above one pass of the row prefix's workgroup
@pytest.mark.parametrize("w", [63, 64, 65, 130])                 # around one and two ballots a row
def test_inject_over_map_shapes(w, h):
    """The last column holds a free cell, and the draws reach it."""
    c = random_plane(w, h, seed=w * 7 + h, p=(0.3, 0.4, 0.3))
    c[w - 1, h - 1] = EMP
    c[w - 1, 0] = EMP
    n = 300
    with Pair(c, n, 3, False) as p:
        p.init_pose(round(w / 2 * 65536), round(h / 2 * 65536), 500, 9 * 65536, 20000)
        hit = set()
        for seed_step in range(3):
            p.step(0, 0, 0, 6000, 3000, 500, [65536, 2 * 65536, p.ref.zmax], 0)
            src = p.resample_inject(n)
            assert src == [-1] * n
            hit |= set(zip(((np.array(p.ref.tx) + 32768) >> 16).tolist(), ((np.array(p.ref.ty) + 32768) >> 16).tolist()))
        free = set(rref.free_cells(c))
        assert hit <= free
        if len(free) < 200:
            assert {(w - 1, h - 1), (w - 1, 0)} <= hit           # 900 draws over fewer than 200 cells


@pytest.mark.parametrize("plane", ["one", "last_row", "none"])
def test_inject_over_sparse_planes(plane):
    w, h = 130, 7
    c = np.full((w, h), OCC, np.int8)
    c[:, 2] = UNK
    if plane == "one":
        c[w - 1, h - 1] = EMP
    elif plane == "last_row":
        c[3::5, h - 1] = EMP
    n = 65
    with Pair(c, n, 3, False) as p:
        p.init_pose(round(w / 2 * 65536), round(h / 2 * 65536), 500, 9 * 65536, 20000)
        for count in (16, n):
            p.step(0, 0, 0, 6000, 3000, 500, [65536, 2 * 65536, p.ref.zmax], 0)
            before = [list(p.ref.tx), list(p.ref.ty)]
            src = p.resample_inject(count)
            cells = set(zip(((np.array(p.ref.tx) + 32768) >> 16).tolist(), ((np.array(p.ref.ty) + 32768) >> 16).tolist()))
            if plane == "none":
                assert -1 not in src and p.ref.tx == [before[0][s] for s in src]     # rule 40's state everywhere, no error
            elif count == n:
                assert cells == ({(w - 1, h - 1)} if plane == "one" else cells & {(i, h - 1) for i in range(3, w, 5)})
                assert plane == "one" or len(cells) > 15


def test_no_injection_is_the_plain_resample(cls):
    """kc_mcl_resample_inject(0) on one context, kc_mcl_resample on a second: the same states, acc and next step."""
    rng = np.random.default_rng(4)
    with kh.WorldMapContext(W, H, RES, ORIGIN) as m:
        m.set_prior(cls)
        with kh.MclContext(m, 300, beams(5), RANGE, 6) as a, kh.MclContext(m, 300, beams(5), RANGE, 6) as b:
            for x in (a, b):
                x.set_model(PEN, ERR_SHIFT, WTAB, W_SHIFT)
                x.init_pose(round(W / 2 * 65536), round(H / 2 * 65536), 12345, 25 * 65536, 20000)
            for k in range(2):
                zq = scan(5, a.zmax, rng, SKIP)
                ra, rb = a.step(30000, -7000, 900, 6000, 3000, 500, zq, SKIP), b.step(30000, -7000, 900, 6000, 3000, 500, zq, SKIP)
                assert ra.as_tuple() == rb.as_tuple() and a.last_fit().as_tuple() == b.last_fit().as_tuple()
                a.resample_inject(0)
                b.resample()
                for g, w in zip(a.particles(), b.particles()):
                    assert np.array_equal(g, w)


def test_inject_follows_a_changed_map():
    """Three free cells; the map's own update turns one of them occupied between two injecting resamples, and the second
    draws from the two that are left."""
    c = np.full((W, H), OCC, np.int8)
    spots = [(20, 30), (50, 31), (90, 7)]
    for s in spots:
        c[s] = EMP
    n = 300
    with Pair(c, n, 3, False) as p:
        p.init_pose(round(W / 2 * 65536), round(H / 2 * 65536), 500, 9 * 65536, 20000)

        def cells():
            return set(zip(((np.array(p.ref.tx) + 32768) >> 16).tolist(), ((np.array(p.ref.ty) + 32768) >> 16).tolist()))

        p.step(0, 0, 0, 6000, 3000, 500, [65536, 2 * 65536, p.ref.zmax], 0)
        p.resample_inject(n)
        assert cells() == set(spots)
        g = np.full((5, 5), 100, np.int32)
        changed = sum(p.update(g, (ORIGIN[0] + 50 * RES, ORIGIN[1] + 31 * RES, 0.0))[0] for _ in range(3))   # -8 + 3 * 3 = 1: occupied
        assert changed == 1 and p.wref.cls[50, 31] == OCC
        p.step(0, 0, 0, 6000, 3000, 500, [65536, 2 * 65536, p.ref.zmax], 0)
        p.resample_inject(n)                                     # right behind the update: ordered by the event
        assert cells() == {spots[0], spots[2]}


def test_a_map_written_right_behind_the_resample():
    """The map's writers wait for no reader, so kc_mcl_resample_inject returns only when its reads of the plane are over:
    the very next calls overwrite the whole 130 x 1030 plane (a prior without a free cell, then a shift), with nothing
    read back in between, and the injected particles are still those of the plane as it was at the resample.  This can
    catch a race when the timing falls that way; it cannot prove there is none."""
    w, h, n = 130, 1030, 1025
    c = random_plane(w, h, seed=77, p=(0.3, 0.4, 0.3))
    with Pair(c, n, 3, False) as p:
        p.init_pose(round(w / 2 * 65536), round(h / 2 * 65536), 500, 9 * 65536, 20000)
        for k in range(3):
            p.step(0, 0, 0, 6000, 3000, 500, [65536, 2 * 65536, p.ref.zmax], 0)
            p.dev.resample_inject(n)
            p.map.set_prior(np.full((w, h), OCC, np.int8))       # no host wait between the resample and these two
            p.map.shift(7, -300)
            src = p.ref.resample_inject(n)                       # the statement, on the plane as it was
            p.ref.tx, p.ref.ty = sref.shift_particles(p.ref.tx, p.ref.ty, 7, -300)   # rule 50: the read-back follows the shift
            assert src == [-1] * n
            p.same_particles(f"round {k}")
            p.map.shift(-7, 300)
            p.map.set_prior(c)
            p.ref.tx, p.ref.ty = sref.shift_particles(p.ref.tx, p.ref.ty, -7, 300)
            p.same_particles(f"back {k}")


def test_inject_after_a_shift(cls):
    """The resample is the first entry after WorldMap's shift: the particles move by rule 50 and the draw reads the shifted
    plane."""
    rng = np.random.default_rng(12)
    n = 300
    with Pair(cls, n, 5, False) as p:
        p.init_pose(round(W / 2 * 65536), round(H / 2 * 65536), 12345, 25 * 65536, 20000)
        p.step(30000, -7000, 900, 6000, 3000, 500, scan(5, p.ref.zmax, rng, SKIP), SKIP)
        p.map.shift(30, -20)
        p.wref.evidence, p.wref.cls = sref.shift_planes(p.wref.evidence, p.wref.cls, 30, -20)
        p.ref.cls = p.wref.cls
        p.ref.tx, p.ref.ty = sref.shift_particles(p.ref.tx, p.ref.ty, 30, -20)
        src = p.resample_inject(n // 4)
        i, j = (np.array(p.ref.tx) + 32768) >> 16, (np.array(p.ref.ty) + 32768) >> 16
        inj = np.array(src) == -1
        assert inj.sum() == n // 4 and (p.wref.cls[i[inj], j[inj]] == EMP).all()
        assert (i[inj] < W - 30).all() and (j[inj] >= 20).all()  # what entered the window is never observed: not free
        p.step(30000, -7000, 900, 6000, 3000, 500, scan(5, p.ref.zmax, rng, SKIP), SKIP)


# ---- rule 63: the recovery run through the front end ----
@pytest.fixture(scope="module")
def cpu():
    import test_worldmap_mcl_recovery_cpu as t

    return t


def front_end(cpu, recovery):
    from kompass_core.mapping import MCL, WorldMap

    c, truth = cpu.kidnap_scene()[:2]
    wm = WorldMap(c.shape[0], c.shape[1], cpu.ROOM_RES)
    wm.set_prior(c)
    loc = MCL(wm, cpu.RECOVERY_N, cpu.ROOM_BEAMS, cpu.ROOM_RANGE, sigma_hit=0.1, seed=0, model="field", skip_no_return=True,
              motion_noise=cpu.base.NOISE, spread=False, recovery=recovery)
    loc.init(truth[0], *cpu.INIT_SIGMA)
    return loc


def same_states(loc, vec, k):
    for name, g, w in zip(("tx", "ty", "h", "acc"), loc._mcl.particles(), vec.particles()):
        assert np.array_equal(g, w), (k, name)


def test_recovery_run_equals_the_statement(cpu):
    """Seed 0 of the CPU scenario, 16384 particles, 36 steps through kompass_core.mapping.MCL(recovery=True): every step's
    record, fit, averages, n_inject and particle states equal the vectorised statement's; the final errors are inside the
    CPU test's bounds."""
    _, truth, odom, scans = cpu.kidnap_scene()
    loc = front_end(cpu, True)
    f = rref.Filter(cpu.statement(0), rref.DEFAULT_POLICY)
    same_states(loc, f.m, 0)
    injected = []
    for k in range(1, cpu.STEPS + 1):
        est, want = loc.step(*odom[k], scans[k]), f.step(*cpu.step_args(k))
        assert tuple(est.record) == want["rec"].as_tuple(), k
        assert (est.fit, est.fit_slow, est.fit_fast, est.injected, est.resampled) == (want["fit"], want["fit_slow"], want["fit_fast"], want["injected"], want["resampled"]), k
        assert (est.cost_min, est.cost_best, est.beams_used) == (want["cost_min"], want["cost_best"], want["beams_used"]), k
        same_states(loc, f.m, k)
        injected.append(est.injected)
    assert injected[:12] == [0] * 12 and injected[12] == cpu.RECOVERY_N // 4 and sum(injected[30:]) == 0
    e = mref.estimate(want["rec"], cpu.ROOM_RES, (0.0, 0.0))
    assert (est.x, est.y, est.yaw) == (e["x"], e["y"], e["yaw"])
    pos, yaw = cpu.base.errors(e, truth[-1])
    assert pos < cpu.RECOVERY_POS_BOUND and yaw < 2 * cpu.RECOVERY_YAW_WORST


def test_run_without_recovery_equals_todays_statement(cpu):
    """The same run with recovery=None against worldmap_mcl_field_ref.MclFieldVec and rule 40's decision alone, as before
    this feature; the fit is still reported, nothing is injected, and the filter stays lost."""
    _, truth, odom, scans = cpu.kidnap_scene()
    loc = front_end(cpu, None)
    old = cpu.statement(0, form=fref.MclFieldVec)
    for k in range(1, cpu.STEPS + 1):
        args = cpu.step_args(k)
        est, want = loc.step(*odom[k], scans[k]), old.step(*args)
        assert tuple(est.record) == want.as_tuple(), k
        resample = mref.should_resample(want, old.n)
        assert est.injected == 0 and est.resampled == resample
        if resample:
            old.resample()
        same_states(loc, old, k)
        assert est.fit >= 0 and est.beams_used == rref.beams_used(args[6], old.zmax, True)
    pos, _ = cpu.base.errors(mref.estimate(want, cpu.ROOM_RES, (0.0, 0.0)), truth[-1])
    assert pos > cpu.LOST_POS_BOUND


# ---- the front ends ----
def test_front_ends(cls):
    import kompass_cpp
    from kompass_core.mapping import MCL, WorldMap

    angles = beams(24)
    wm = WorldMap(W, H, RES, ORIGIN)
    wm.set_prior(cls)
    # the beam model, a policy that injects at the second step whatever it says: a_slow 30 holds slow at the first m
    loc = MCL(wm, 65, angles, RANGE, sigma_hit=0.1, seed=4, skip_no_return=True, resample_ratio=(0, 1), spread=False,
              recovery=(30, 0, (1, 2)))
    stmt = rref.FitRef(cls, RES, 65, angles, RANGE, 4)
    stmt.set_model(*mref.sensor_tables(RES, 0.1))
    f = rref.Filter(stmt, (30, 0, 1, 2), 0, 1)
    x0, y0 = ORIGIN[0] + 40 * RES, ORIGIN[1] + 30 * RES
    loc.init((x0, y0, 0.3), 0.1, 0.05)
    q = ref.quantise_pose(RES, ORIGIN, x0, y0, 0.0)
    stmt.init_pose(q[2], q[3], mref.quantise_heading(0.3), mref.noise_scale(0.1 * 65536.0 / float(np.float32(RES))),
                   mref.noise_scale(0.05 / (2 * math.pi) * 65536.0))
    cell = 65536.0 / float(np.float32(RES))
    s = (mref.noise_scale(0.02 * cell), mref.noise_scale(0.01 * cell), mref.noise_scale(0.01 / (2 * math.pi) * 65536.0))
    a, b = (0.0, 0.0, 0.0), (0.03, 0.01, 0.02)
    injected = []
    for ranges in (np.linspace(0.2, 0.27, 24), np.linspace(0.02, 0.1, 24), np.full(24, np.inf)):
        ranges[5] = float("inf")
        est = loc.step(a, b, ranges)
        want = f.step(*mref.odometry_increment(RES, a, b), *s, mref.quantise_ranges(ranges, RES, RANGE, SKIP), SKIP)
        assert tuple(est.record) == want["rec"].as_tuple()
        assert (est.fit, est.fit_slow, est.fit_fast, est.injected, est.resampled, est.beams_used) == \
            (want["fit"], want["fit_slow"], want["fit_fast"], want["injected"], want["resampled"], want["beams_used"])
        for g, w in zip(loc._mcl.particles(), stmt.particles()):
            assert np.array_equal(g, w)
        injected.append(est.injected)
    assert injected[0] == 0 and injected[1] > 0                  # by the statement the second scan fits worse: an injection is run
    assert (est.fit, est.beams_used, est.injected) == (-1, 0, 0) and est.fit_fast == want["fit_fast"] > 0     # no beam: nothing said
    loc.set_recovery(None)
    assert not loc._mcl.recovery
    loc.init((x0, y0, 0.3), 0.1, 0.05)
    est = loc.step(a, b, np.linspace(0.02, 0.1, 24))
    assert est.fit == est.fit_slow == est.fit_fast >= 0 and est.injected == 0         # either init un-primes the averages
    # the class itself: setRecovery's refusals are kc_mcl_recovery_update's, and a refusal leaves the policy as it was
    cm = kompass_cpp.mapping.MCL(wm._map, 65, list(angles), RANGE, 4)
    assert not cm.recovery
    for bad in (dict(a_slow=31), dict(a_slow=-1), dict(a_fast=31), dict(max_den=0), dict(max_num=5, max_den=4)):
        with pytest.raises(ValueError):
            cm.set_recovery(**bad)
        assert not cm.recovery
    cm.set_recovery()
    assert cm.recovery
    cm.clear_recovery()
    assert not cm.recovery
