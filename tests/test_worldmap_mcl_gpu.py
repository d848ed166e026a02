"""The Monte-Carlo localiser on the device (kc_mcl_*; DESIGN.md 4.11 rules 28 to 41) against the Python statement
tests/worldmap_mcl_ref.py: states, acc, record and resampled states bit for bit, after each init, each step and a forced
resample.  One context a test.

The map is 97 x 61 (the width no multiple of 4) with occupied, empty and never-observed cells.  The range is 5.5 cells
(Rc = 6) so that the statement's loop a ray stays short: a walk still crosses the first round of 8 steps and leaves the
box, and the particles are spread so that some start in occupied and never-observed cells."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import worldmap_mcl_ref as mref  # noqa: E402
import worldmap_ref as ref  # noqa: E402

RES, ORIGIN = 0.05, (-0.33, 1.7)
W, H = 97, 61
OCC, UNK, EMP = ref.OCCUPIED, ref.UNEXPLORED, ref.EMPTY
RANGE = float(np.float32(float(np.float32(RES)) * 5.5))          # a float32, as the library takes it
PEN = [min(65535, 3 * i * i + i) for i in range(64)]
ERR_SHIFT = 13
WTAB = [round(65536 * math.exp(-i / 8.0)) for i in range(128)]      # the tail is 0
W_SHIFT = 5


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def seeded_map(seed=5, p_occ=0.06, p_unknown=0.15):
    rng = np.random.default_rng(seed)
    cls = rng.choice(np.int8([OCC, UNK, EMP]), size=(W, H), p=[p_occ, p_unknown, 1.0 - p_occ - p_unknown]).astype(np.int8)
    cls[0, :] = cls[-1, :] = OCC
    cls[:, 0] = cls[:, -1] = OCC
    return cls


@pytest.fixture(scope="module")
def cls():
    c = seeded_map()
    assert {OCC, UNK, EMP} == set(np.unique(c).tolist())
    return c


def beams(n, start=-math.pi + 0.013):
    return start + np.arange(n) * (2 * math.pi / n)


class Pair:
    """A device localiser and the statement over one map, driven together."""

    def __init__(self, cls, n, b, seed=3, range_max=RANGE, pen=PEN, err_shift=ERR_SHIFT, wtab=WTAB, w_shift=W_SHIFT, angles=None):
        self.cls = cls
        self.map = kh.WorldMapContext(cls.shape[0], cls.shape[1], RES, ORIGIN)
        self.map.set_prior(cls)
        ang = beams(b) if angles is None else angles
        self.dev = kh.MclContext(self.map, n, ang, range_max, seed)
        self.ref = mref.MclRef(cls, RES, n, ang, range_max, seed)
        assert (self.dev.rc, self.dev.zmax) == (self.ref.Rc, self.ref.zmax)
        if pen is not None:
            self.dev.set_model(pen, err_shift, wtab, w_shift)
            self.ref.set_model(pen, err_shift, wtab, w_shift)

    def close(self):
        self.dev.close()
        self.map.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def same_particles(self, what=""):
        got, want = self.dev.particles(), self.ref.particles()
        for name, g, w in zip(("tx", "ty", "h", "acc"), got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5].ravel(), g[:4], w[:4])

    def init_pose(self, *a):
        self.dev.init_pose(*a)
        self.ref.init_pose(*a)
        self.same_particles("init")

    def init_global(self):
        assert self.dev.init_global() == self.ref.init_global()
        self.same_particles("global init")

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


def middle(di=0.0, dj=0.0):
    return round((W / 2 + di) * 65536), round((H / 2 + dj) * 65536)


def some_ranges(zmax, b, seed):
    """Quantised ranges all over 0 .. ZMAX, both ends among them."""
    z = np.random.default_rng(seed).integers(0, zmax + 1, size=b)
    z[0] = zmax
    z[-1] = 0
    return [int(v) for v in z]


SPREAD = mref.noise_scale(9 * 65536)        # nine cells: particles in walls, in unknown cells and near the border
TURN = mref.noise_scale(65536 / 7)
DRIVE = [(40000, -9000, 700), (-25000, 30000, -1500), (65536 * 2, 0, 65000), (1234, 5678, -9)]
SHAPES = [(n, b) for n in (1, 63, 64, 65, 257, 1000) for b in (1, 63, 64, 65, 257)] + [(4097, 8)]


@pytest.mark.parametrize("n,b", SHAPES)
def test_shapes(cls, n, b):
    """Partial wavefronts, a particle's beams across wavefronts and workgroups, B no divisor of 64; 4097: the prefix sum's
    chunks are uneven.  Init, three steps, a forced resample; the small shapes take a fourth step on the resampled set."""
    short = float(np.float32(RES)) * 2.5       # Rc = 3 for the three largest shapes: the statement's loop a ray again
    with Pair(cls, n, b, seed=n * 1000 + b, range_max=RANGE if n * b <= 50000 else short) as t:
        t.init_pose(*middle(), 11111, SPREAD, TURN)
        for s, (d_f, d_l, d_h) in enumerate(DRIVE[:3]):
            t.step(d_f, d_l, d_h, mref.noise_scale(20000), mref.noise_scale(9000), mref.noise_scale(300),
                   some_ranges(t.ref.zmax, b, s), flags=kh.SCAN_UNKNOWN_BLOCKS if s == 1 else 0)
        t.resample()
        if n * b <= 20000:
            t.step(*DRIVE[3], 0, 0, 0, some_ranges(t.ref.zmax, b, 9))


def test_outside_and_occupied_starts(cls):
    """A particle outside the map: every beam gives ZMAX, cells outside never block (also with unknown_blocks); one that
    starts in an occupied cell: q = 0 for every beam."""
    occ_i, occ_j = (int(v) for v in np.argwhere(cls[1:-1, 1:-1] == OCC)[0] + 1)
    for tx0, ty0, want_q in [(-40 << 16, 20 << 16, None), (occ_i << 16, occ_j << 16, 0)]:
        for flags in (0, kh.SCAN_UNKNOWN_BLOCKS):
            with Pair(cls, 3, 33) as t:
                t.init_pose(tx0, ty0, 500, 0, 0)
                zq = some_ranges(t.ref.zmax, 33, 1)
                rec = t.step(0, 0, 0, 0, 0, 0, zq, flags=flags)
                q = t.ref.zmax if want_q is None else want_q
                assert rec.amin == sum(PEN[min(abs(q - z) >> ERR_SHIFT, len(PEN) - 1)] for z in zq)
                assert rec.best == 0


def test_heading_wraps(cls):
    with Pair(cls, 70, 9) as t:
        t.init_pose(*middle(2.3, -1.1), 65535, 0, 0)
        assert set(t.ref.h) == {65535}
        t.step(1000, 0, 1, 0, 0, 0, some_ranges(t.ref.zmax, 9, 2))
        assert set(t.ref.h) == {0}
        t.step(1000, 0, -3, 0, 0, 0, some_ranges(t.ref.zmax, 9, 3))
        assert set(t.ref.h) == {65533}
        t.step(0, 0, 3, 0, 0, mref.noise_scale(4), some_ranges(t.ref.zmax, 9, 4))    # noise on both sides of the wrap
        assert min(t.ref.h) < 100 and max(t.ref.h) > 65000


@pytest.mark.parametrize("skip", [False, True])
def test_beams_without_a_return(cls, skip):
    """NaN, inf and >= range_max measured beams: ZMAX, or nothing at all with KC_MCL_SKIP_NO_RETURN."""
    flags = kh.MCL_SKIP_NO_RETURN if skip else 0
    ranges = [0.1, float("nan"), float("inf"), RANGE, 2 * RANGE, -0.1, 0.0, np.nextafter(np.float32(RANGE), np.float32(0)), 0.2]
    zq_ref = mref.quantise_ranges(ranges, RES, RANGE, flags)
    zq = kh.mcl_quantise_ranges(ranges, RES, RANGE, flags)
    assert zq.tolist() == zq_ref
    none = -1 if skip else round(RANGE / float(np.float32(RES)) * 65536.0)
    assert zq_ref[1:6] == [none] * 5 and zq_ref[6] == 0 and 0 < zq_ref[7] <= mref.check(RES, 1, 1, RANGE)[1]
    with Pair(cls, 130, len(ranges)) as t:
        t.init_pose(*middle(), 0, SPREAD, TURN)
        t.step(3000, 0, 0, 0, 0, 0, zq_ref, flags=flags)
        t.step(3000, 0, 0, 0, 0, 0, zq_ref, flags=flags | kh.SCAN_UNKNOWN_BLOCKS)
        if skip:                                                     # -1 without the flag is refused and queues nothing
            with pytest.raises(ValueError):
                t.dev.step(0, 0, 0, 0, 0, 0, zq_ref, flags=0)
            t.same_particles("after a refusal")
            assert t.dev.step_count() == 2


def test_acc_reaches_the_cap():
    """A map of walls, particles spread far around it: one inside pays 1024 * 65535 a step against beams without a
    return, one outside whose beams miss the map pays nothing; 16 steps stay below 2^30, the 17th is cut."""
    walls = np.full((W, H), OCC, np.int8)
    with Pair(walls, 6, 1024, pen=[0] + [65535] * 7, err_shift=10, wtab=[5, 5, 1, 0], w_shift=29, seed=8) as t:
        t.init_pose(*middle(), 0, mref.noise_scale(60 * 65536), 0)
        zq = [t.ref.zmax] * 1024
        for s in range(17):
            t.step(0, 0, 0, 0, 0, 0, zq)
            assert (max(t.ref.acc) == mref.ACC_CAP) == (s == 16), (s, max(t.ref.acc))
        assert min(t.ref.acc) == 0


def test_equal_costs_best_is_zero_and_resample_is_identity(cls):
    with Pair(cls, 200, 16) as t:
        t.init_pose(-500 << 16, -500 << 16, 100, mref.noise_scale(65536), TURN)   # all far outside: every q is ZMAX
        rec = t.step(500, 0, 3, 0, 0, 0, some_ranges(t.ref.zmax, 16, 4))
        assert rec.best == 0 and rec.w1 == 200 * WTAB[0] and len(set(t.ref.acc)) == 1
        before = t.ref.particles()
        assert t.resample() == list(range(200))
        after = t.dev.particles()
        assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3]))


def test_zero_tail_weights_get_no_copy(cls):
    with Pair(cls, 300, 12, wtab=[1 << 20, 7, 0], w_shift=8) as t:
        t.init_pose(*middle(), 0, SPREAD, TURN)
        t.step(0, 0, 0, 0, 0, 0, some_ranges(t.ref.zmax, 12, 6))
        w = list(t.ref.w)
        assert 0 in w and (1 << 20) in w
        src = t.resample()
        assert all(w[i] > 0 for i in src)


def test_clamped_tx(cls):
    with Pair(cls, 65, 5) as t:
        t.init_pose(ref.MAX_OFFSET - 5, -ref.MAX_OFFSET + 5, 0, mref.noise_scale(4096), 0)
        assert ref.MAX_OFFSET in t.ref.tx and -ref.MAX_OFFSET in t.ref.ty
        t.step(1 << 20, 0, 0, 0, 0, 0, some_ranges(t.ref.zmax, 5, 7))
        assert set(t.ref.tx) == {ref.MAX_OFFSET}
        t.step(-(1 << 36), 0, 32768, 0, 0, 0, some_ranges(t.ref.zmax, 5, 7))
        assert set(t.ref.tx) == {0}


def test_global_init(cls):
    with Pair(cls, 777, 7) as t:
        t.init_global()
        i, j = (np.array(t.ref.tx) + 32768) >> 16, (np.array(t.ref.ty) + 32768) >> 16
        assert (cls[i, j] == EMP).all() and len(set(zip(i.tolist(), j.tolist()))) > 500
        t.step(*DRIVE[0], 0, 0, 0, some_ranges(t.ref.zmax, 7, 8))
        t.resample()
        t.step(*DRIVE[1], 0, 0, 0, some_ranges(t.ref.zmax, 7, 9))


def test_global_init_single_and_no_free_cell():
    one = np.full((W, H), OCC, np.int8)
    one[:, ::2] = UNK
    one[70, 33] = EMP
    with Pair(one, 100, 4) as t:
        t.init_global()
        assert set((np.array(t.ref.tx) + 32768) >> 16) == {70} and set((np.array(t.ref.ty) + 32768) >> 16) == {33}
        t.step(0, 0, 0, 0, 0, 0, some_ranges(t.ref.zmax, 4, 1))
    one[70, 33] = OCC
    with Pair(one, 100, 4) as t:
        with pytest.raises(mref.StateError):
            t.ref.init_global()
        with pytest.raises(kh.KompassHipError, match=r"\[kc -5\]"):
            t.dev.init_global()
        with pytest.raises(kh.KompassHipError, match=r"\[kc -5\]"):
            t.dev.particles()


def test_step_before_init_and_before_model(cls):
    with Pair(cls, 10, 4) as t:
        with pytest.raises(kh.KompassHipError, match=r"\[kc -5\]"):
            t.dev.step(0, 0, 0, 0, 0, 0, [0, 0, 0, 0])
        with pytest.raises(mref.StateError):
            t.ref.step(0, 0, 0, 0, 0, 0, [0, 0, 0, 0])
        with pytest.raises(kh.KompassHipError, match=r"\[kc -5\]"):
            t.dev.resample()
        t.init_pose(*middle(), 0, 0, 0)
        with pytest.raises(kh.KompassHipError, match=r"\[kc -5\]"):
            t.dev.resample()                                         # no step's weights yet
    with Pair(cls, 10, 4, pen=None) as t:
        t.dev.init_pose(*middle(), 0, 0, 0)
        with pytest.raises(kh.KompassHipError, match=r"\[kc -5\]"):
            t.dev.step(0, 0, 0, 0, 0, 0, [0, 0, 0, 0])


def test_map_is_untouched_and_read_in_place(cls):
    with Pair(cls, 500, 40) as t:
        before = [p.copy() for p in t.map.planes()]
        t.init_pose(*middle(), 0, SPREAD, TURN)
        t.step(*DRIVE[0], 0, 0, 0, some_ranges(t.ref.zmax, 40, 1))
        t.resample()
        after = t.map.planes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        # the next step sees a changed map: the walk reads the map's own plane
        changed = cls.copy()
        changed[20:60, 25:35] = OCC
        t.map.set_prior(changed)
        t.ref.cls = changed
        t.step(*DRIVE[1], 0, 0, 0, some_ranges(t.ref.zmax, 40, 2))


def test_sums_beyond_64_bits(cls):
    """Headings all round the circle, then one step of 2^20 cells forward: the particles stand on a circle of that radius,
    far outside the map (equal costs, best 0), at the largest weight: SX and SY pass 2^64."""
    with Pair(cls, 1000, 6, wtab=[1 << 20], w_shift=0) as t:
        t.init_pose(0, 0, 0, 0, mref.noise_scale(65536 / 3))
        rec = t.step(1 << 36, 0, 0, 0, 0, 0, some_ranges(t.ref.zmax, 6, 3))
        assert rec.w1 == 1000 << 20 and rec.best == 0 and min(abs(rec.sx), abs(rec.sy)) > 1 << 64
        assert min(t.ref.tx) < -(1 << 35) and max(t.ref.tx) > 1 << 35
