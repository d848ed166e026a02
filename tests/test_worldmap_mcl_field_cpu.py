"""The localiser's likelihood-field model without a device (DESIGN.md 4.11 rules 44 and 45): the host-only check of the
library against the statement's, the front ends' tables, the two forms of the statement tests/worldmap_mcl_field_ref.py
against each other, rule 44 at its extremes, and whether the statement localises: from an offset as the beam model's
test asks, and from a global init, which the beam statement could not be run far enough to show.

The convergence tests run the statement alone; DESIGN.md 4.11 has their measured errors."""
import math

import numpy as np
import pytest

import kompass_cpp
import kompass_hip as kh
import test_worldmap_mcl_cpu as base
import worldmap_dist_ref as dref
import worldmap_mcl_field_ref as fref
import worldmap_mcl_ref as mref
import worldmap_ref as ref

CPP = kompass_cpp.mapping.MCL
ROOM_RES, ROOM_RANGE, ROOM_BEAMS = base.ROOM_RES, base.ROOM_RANGE, base.ROOM_BEAMS

# ---- kc_mcl_field_check ----
GOOD = dict(resolution=0.05, n_particles=100, n_beams=64, range_max=10.0, pen_d2=[0, 1, 2, 3, 4], reach=2, wtab=[9, 9, 4, 0],
            w_shift=2, flags=2)
# one refusal each, in the documented order; every case also carries all the LATER faults, so the first must win
FAULTS = [("resolution", float("nan"), ValueError), ("n_particles", 0, ValueError), ("n_particles", 65537, IndexError),
          ("n_beams", 1025, IndexError), ("range_max", float("inf"), ValueError), ("range_max", 0.05 * 2048.5, IndexError),
          ("pen_d2", [7], ValueError), ("pen_d2", [1] * 4097, IndexError), ("reach", 255, IndexError), ("reach", 1, ValueError),
          ("wtab", [], ValueError), ("wtab", [1] * 4097, IndexError), ("w_shift", -1, ValueError),
          ("wtab", [(1 << 20) + 1], ValueError), ("wtab", [5, 6], ValueError), ("flags", 1, ValueError), ("flags", 4, ValueError)]


def both_checks(**kw):
    out = []
    for fn in (fref.field_check, kh.mcl_field_check):
        try:
            out.append(fn(**kw))
        except (ValueError, IndexError) as e:
            out.append(type(e))
    return out


def test_field_check_accepts_and_reports():
    assert both_checks(**GOOD) == [(200, 13107200)] * 2
    assert both_checks(**dict(GOOD, pen_d2=[1] * 4096, reach=64)) == [(200, 13107200)] * 2       # c2 = 4095 <= 64^2
    assert both_checks(**dict(GOOD, pen_d2=[1] * 4096, reach=0)) == [(200, 13107200)] * 2        # the reach is not tested
    assert both_checks(**dict(GOOD, pen_d2=[1] * 4096, reach=63)) == [ValueError] * 2            # 4095 > 3969
    assert both_checks(**dict(GOOD, pen_d2=[3, 4], reach=254)) == [(200, 13107200)] * 2
    assert both_checks(**dict(GOOD, pen_d2=None, wtab=None, reach=999, w_shift=99, flags=0)) == [(200, 13107200)] * 2


@pytest.mark.parametrize("first", range(len(FAULTS)))
def test_field_check_refuses_in_order(first):
    kw, faulty = dict(GOOD), set()
    for name, value, _ in FAULTS[first:]:                       # the fault under test, and one later fault per other argument
        if name not in faulty:
            kw[name] = value
            faulty.add(name)
    want = FAULTS[first][2]
    assert both_checks(**kw) == [want, want], (FAULTS[first], sorted(faulty))


def test_front_end_tables_agree():
    for res, sigma, kw in ((0.05, 0.1, {}), (0.05, 0.1, dict(reach=6)), (0.1, 0.03, {}), (0.02, 1.0, {}), (0.05, 0.2, dict(floor=0.2, pen_scale=10.0))):
        pen, far, reach, wtab, ws = CPP.field_tables(res, sigma, **kw)
        assert (list(pen), far, reach, list(wtab), ws) == fref.field_tables(res, sigma, **kw)
        assert len(pen) == reach * reach + 1 and fref.field_check(res, 1, 1, 10.0, pen, reach, wtab, ws)
    pen, far, reach, wtab, _ = fref.field_tables(0.05, 0.1)
    assert reach == 6 and pen[0] == 0 and far == round(64.0 * -math.log(0.05)) == 192 and pen == sorted(pen) and pen[-1] <= far
    assert wtab == mref.sensor_tables(0.05, 0.1)[2]
    assert fref.field_tables(0.1, 0.03)[2] == 1 and fref.field_tables(0.02, 1.0)[2] == 63       # the clip at both ends


# ---- rule 44 ----
def test_endpoint_at_the_extremes():
    zmax = round(2048.0 * 65536.0)                               # the largest ZMAX rule 38 lets through
    big = (1 << 30) + (1 << 15)                                  # rule 44's bound on |dx|
    assert fref.beam_direction(65536, 0, 1 << 30, 0) == (1 << 30, 0) and fref.beam_direction(0, 65536, 1 << 30, 0) == (0, 1 << 30)
    assert fref.beam_direction(-65536, 0, 0, 1 << 30) == (0, -(1 << 30))
    for dx in (big, -big):
        prod = (zmax - 1) * dx
        assert abs(prod) < (1 << 27) * big < 1 << 58
        I, J = fref.endpoint(0, 0, dx, -dx, zmax - 1)
        assert I == ((1 << 15) + ((prod + (1 << 29)) >> 30)) >> 16 and J == ((1 << 15) + ((-prod + (1 << 29)) >> 30)) >> 16
        assert abs(I) in (2048, 2049) and I * J < 0
        # the vectorised form's int64 holds the product and floors alike
        assert int(np.int64(prod)) == prod and int((np.int64(prod) + np.int64(1 << 29)) >> np.int64(30)) == (prod + (1 << 29)) >> 30
    # a negative EX floors: EX = -1 is cell -1, not cell 0
    assert fref.endpoint(-(1 << 15) - 1, -(1 << 15), 0, 0, 5) == (-1, 0)
    assert fref.endpoint(0, 0, -(1 << 30), 0, 1 << 15) == (0, 0)           # EX = 0: the left edge of cell 0
    assert fref.endpoint(0, 0, -(1 << 30), 0, (1 << 15) + 1) == (-1, 0)
    assert int((np.int64(-1)) >> np.int64(16)) == -1 == (-1) >> 16
    # (zq dx + 2^29) >> 30 rounds to nearest, a half upwards, for either sign
    edge = (1 << 16) - (1 << 15) - 1                             # X0 = 2^16 - 1: one unit below cell 1
    assert fref.endpoint(edge, 0, 1 << 29, 0, 1)[0] == 1 and fref.endpoint(edge, 0, (1 << 29) - 1, 0, 1)[0] == 0
    assert fref.endpoint(-(1 << 15), 0, -(1 << 29), 0, 1)[0] == 0 and fref.endpoint(-(1 << 15), 0, -(1 << 29) - 1, 0, 1)[0] == -1


# ---- the two forms ----
def small_world():
    rng = np.random.default_rng(23)
    c = rng.choice(np.array([ref.EMPTY] * 10 + [ref.UNEXPLORED, ref.OCCUPIED], np.int8), (37, 29))
    c[0, :] = c[-1, :] = ref.OCCUPIED
    return c


def pair(c, n, angles, range_max, seed, reach, flags=0, tables=None):
    dist = dref.DistRef(c, reach, flags)
    loop = fref.MclFieldRef(c, 0.1, n, angles, range_max, seed, dist=dist)
    vec = fref.MclFieldVec(c, 0.1, n, angles, range_max, seed, dist.field)
    t = tables or fref.field_tables(0.1, 0.15, reach=reach, w_shift=2, temperature=64.0)
    loop.set_field_model(t[0], t[1], t[3], t[4])
    vec.set_field_model(t[0], t[1], t[3], t[4])
    return loop, vec


def same(loop, vec):
    a, b = loop.particles(), vec.particles()
    return all((x == y).all() for x, y in zip(a, b))


def test_loop_form_equals_vectorised_form():
    """N 64, B 7, three steps, a resample forced after the second; poses near the border so that endpoints leave the
    map; a -1 beam and a ZMAX beam."""
    c = small_world()
    angles = [0.0, 0.9, 1.8, 2.7, 3.6, 4.5, 5.4]
    for seed, start in ((0, "pose"), (1, "global")):
        loop, vec = pair(c, 64, angles, 1.5, seed, 3)
        if start == "pose":
            loop.init_pose(3 << 16, 26 << 16, 9000, 150000, 9000)
            vec.init_pose(3 << 16, 26 << 16, 9000, 150000, 9000)
        else:
            assert loop.init_global() == vec.init_global()
        assert same(loop, vec)
        zmax = loop.zmax
        scans = [[zmax - 1, 3 << 16, -1, zmax, 0, 7 << 16, 5 << 15], [1 << 16, 2 << 16, 3 << 16, 4 << 16, 5 << 16, 6 << 16, 7 << 16],
                 [zmax, zmax, -1, 9 << 15, 1, 2, 3]]
        for k, zq in enumerate(scans):
            args = (70000, -20000, 700, 9000, 4000, 300, zq, mref.SKIP_NO_RETURN)
            ra, rb = loop.step(*args), vec.step(*args)
            assert ra.as_tuple() == rb.as_tuple() and loop.w == vec.w and same(loop, vec), (seed, k)
            if k == 1:
                assert loop.resample() == vec.resample() and same(loop, vec)
        assert len(set(loop.acc)) > 8                                # the penalties tell the particles apart


def test_field_step_refusals_of_the_statement():
    c = small_world()
    loop, _ = pair(c, 4, [0.0, 1.0], 1.5, 0, 3)
    loop.init_pose(5 << 16, 5 << 16, 0, 100, 100)
    with pytest.raises(ValueError):
        loop.step(0, 0, 0, 0, 0, 0, [5, 5], mref.UNKNOWN_BLOCKS)
    loop.dist = None
    with pytest.raises(mref.StateError):
        loop.step(0, 0, 0, 0, 0, 0, [5, 5])
    loop.dist = dref.DistRef(c, 1)                               # the reach was lowered: c2 = 9 > 1
    with pytest.raises(mref.StateError):
        loop.step(0, 0, 0, 0, 0, 0, [5, 5])
    assert loop.step_count == 0
    loop.set_model(*mref.sensor_tables(0.1, 0.1))                # back to the beam model, the particles stay
    tx = list(loop.tx)
    assert loop.step(0, 0, 0, 0, 0, 0, [5, 5]).step == 1 and loop.tx == tx


# ---- does the statement localise?  (no device: the statement alone) ----
@pytest.fixture(scope="module")
def scene():
    c = base.room()
    path = base.drive()
    table = mref.scan_table(ROOM_BEAMS)
    scans = [base.sref.scan_pose(c, ROOM_RES, ref.quantise_pose(ROOM_RES, (0.0, 0.0), *p), table, ROOM_RANGE)[0] for p in path]
    return c, path, scans


def localise(scene, m, steps=12, flags=0):
    """base.localise with the step's flags: the statement along the drive -> [(estimate, record)] a step."""
    c, path, scans = scene
    cells = 65536.0 / float(np.float32(ROOM_RES))
    s = (mref.noise_scale(base.NOISE[0] * cells), mref.noise_scale(base.NOISE[1] * cells),
         mref.noise_scale(base.NOISE[2] / (2 * math.pi) * 65536.0))
    out = []
    for k in range(1, steps + 1):
        d = mref.odometry_increment(ROOM_RES, path[k - 1], path[k])
        rec = m.step(*d, *s, mref.quantise_ranges(scans[k], ROOM_RES, ROOM_RANGE, flags), flags)
        out.append((mref.estimate(rec, ROOM_RES, (0.0, 0.0)), rec))
        if mref.should_resample(rec, m.n):
            m.resample()
    return out


@pytest.mark.parametrize("seed", range(6))
def test_field_statement_converges_from_an_offset(scene, seed):
    """The beam model's test with the field model in its place: 128 particles, 24 beams, 12 steps, the init 3 cells and 3
    degrees off; the final errors below 1.5 cells and 1.5 degrees, the spread shrinking.  DESIGN.md 4.11 has the six
    measured pairs."""
    c, path, scans = scene
    pen, far, reach, wtab, ws = fref.field_tables(ROOM_RES, 0.1)
    m = fref.MclFieldRef(c, ROOM_RES, 128, ROOM_BEAMS, ROOM_RANGE, seed, dist=dref.DistRef(c, reach))
    m.set_field_model(pen, far, wtab, ws)
    x0, y0, yaw0 = path[0]
    off = 3 * ROOM_RES
    cells = 65536.0 / float(np.float32(ROOM_RES))
    m.init_pose(round((x0 + off * 0.8) / ROOM_RES * 65536.0), round((y0 - off * 0.6) / ROOM_RES * 65536.0),
                mref.quantise_heading(yaw0 + math.radians(3.0)), mref.noise_scale(0.1 * cells),
                mref.noise_scale(math.radians(3.0) / (2 * math.pi) * 65536.0))
    spreads = []

    class Spy:                                                   # the spread needs the weights of the step, before a resample
        def __getattr__(self, name):
            return getattr(m, name)

        def step(self, *a):
            rec = m.step(*a)
            spreads.append(mref.spread(m.tx, m.ty, m.w, mref.estimate(rec, ROOM_RES, (0.0, 0.0)), ROOM_RES))
            return rec

    run = localise(scene, Spy())
    pos, yaw = base.errors(run[-1][0], path[-1])
    print(f"seed {seed}: position error {pos:.3f} cells, yaw error {yaw:.3f} degrees, spread {spreads[0]:.4f} -> {spreads[-1]:.4f} m")
    assert pos < 1.5 and yaw < 1.5
    assert spreads[-1] < spreads[0]


GLOBAL_N = 16384
GLOBAL_POS_BOUND = 3.0          # cells: twice the worst of the float sketch the feature was argued from (1.5)
# degrees: twice the statement's own worst over the six seeds, 2.256 at seed 3.  The six (cells, degrees) after step 12:
# (0.800, 1.768), (1.068, 0.598), (1.003, 1.493), (0.541, 2.256), (0.834, 0.437), (1.427, 0.279); DESIGN.md 4.11 has the table
GLOBAL_YAW_BOUND = 2 * 2.256


def global_run(scene, seed):
    """16384 particles over the free cells, the default field tables, beams without a return skipped -> [(estimate,
    record)] a step, from the vectorised statement."""
    c = scene[0]
    pen, far, reach, wtab, ws = fref.field_tables(ROOM_RES, 0.1)
    dist = dref.DistRef(c, reach)
    m = fref.MclFieldVec(c, ROOM_RES, GLOBAL_N, ROOM_BEAMS, ROOM_RANGE, seed, dist.field)
    m.set_field_model(pen, far, wtab, ws)
    assert m.init_global() == 10196
    return localise(scene, m, flags=mref.SKIP_NO_RETURN)


@pytest.mark.parametrize("seed", range(6))
def test_field_statement_localises_from_a_global_init(scene, seed):
    run = global_run(scene, seed)
    pos, yaw = base.errors(run[-1][0], scene[1][-1])
    print(f"seed {seed}: position error {pos:.3f} cells, yaw error {yaw:.3f} degrees, n_eff {run[-1][0]['n_eff']:.1f}")
    assert pos < GLOBAL_POS_BOUND
    assert yaw < GLOBAL_YAW_BOUND
