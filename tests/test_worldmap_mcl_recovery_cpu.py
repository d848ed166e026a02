"""The localiser's fit record and recovery without a device (DESIGN.md 4.11 rules 59 to 63): the library's host-only
kc_mcl_recovery_update against the statement tests/worldmap_mcl_recovery_ref.py, rule 62's slots, the two forms of the
statement against each other, and whether the policy does what it is for: the statement alone is kidnapped into another
room and must find its way back, and must not without the injection.

DESIGN.md 4.11 has the measured errors of the recovery runs."""
import functools
import math

import numpy as np
import pytest

import kompass_hip as kh
import test_worldmap_mcl_cpu as base
import test_worldmap_mcl_field_cpu as fcpu
import worldmap_dist_ref as dref
import worldmap_mcl_field_ref as fref
import worldmap_mcl_recovery_ref as rref
import worldmap_mcl_ref as mref
import worldmap_ref as ref

ROOM_RES, ROOM_RANGE, ROOM_BEAMS = base.ROOM_RES, base.ROOM_RANGE, base.ROOM_BEAMS
SKIP = mref.SKIP_NO_RETURN


# ---- rule 61: kc_mcl_recovery_update ----
def both_updates(*a, **kw):
    out = []
    for fn in (rref.recovery_update, kh.mcl_recovery_update):
        try:
            out.append(fn(*a, **kw))
        except (ValueError, IndexError) as e:
            out.append(type(e))
    return out


def test_update_primes_then_filters():
    fresh = (0, 0, False)
    # m = floor(5000 * 256 / (100 * 10)) = 1280
    assert both_updates(5000, 100, 10, fresh) == [((1280, 1280, True), 1280, 0)] * 2
    assert both_updates(5000, 100, 10, (77, -3, False)) == [((1280, 1280, True), 1280, 0)] * 2      # an unprimed state is not read
    # a worse step: slow += (2560 - 1280) >> 4 = 80, fast += 1280 >> 1 = 640; n = min(25, floor(100 * 560 / 1920) = 29)
    assert both_updates(10000, 100, 10, (1280, 1280, True)) == [((1360, 1920, True), 2560, 25)] * 2
    assert both_updates(10000, 100, 10, (1280, 1280, True), 4, 1, 1, 2) == [((1360, 1920, True), 2560, 29)] * 2
    assert both_updates(10000, 100, 10, (1280, 1280, True), 4, 1, 0, 1) == [((1360, 1920, True), 2560, 0)] * 2     # max 0: never
    assert both_updates(10000, 100, 10, (1280, 1280, True), 4, 1, 7, 7) == [((1360, 1920, True), 2560, 29)] * 2    # max 1
    # floor(1 * 560 / 1920) = 0 and floor(1 / 4) = 0
    assert both_updates(100, 1, 10, (1280, 1280, True))[0][2] == 0
    # shifts 0 follow m at once, 30 not at all
    assert both_updates(10000, 100, 10, (1280, 1280, True), 0, 0) == [((2560, 2560, True), 2560, 0)] * 2
    assert both_updates(10000, 100, 10, (1280, 1280, True), 30, 0, 1, 1) == [((1280, 2560, True), 2560, 50)] * 2


def test_update_without_a_beam_changes_nothing():
    for state in ((0, 0, False), (9, 9, False), (1360, 1920, True)):
        assert both_updates(0, 100, 0, state) == [(state, -1, 0)] * 2
    assert both_updates(1, 100, 0, (1, 2, True)) == [IndexError] * 2                    # a cost without a beam


def test_update_fast_below_slow_injects_nothing():
    # a better step: the differences are negative, the arithmetic shift floors them
    # slow += (1000 - 1361) >> 4 = -23 (not -22), fast += (1000 - 1921) >> 1 = -461 (not -460)
    got = both_updates(390625, 1000, 100, (1361, 1921, True))
    assert got == [((1338, 1460, True), 1000, 83)] * 2 and (1000 - 1361) >> 4 == -23 and (1000 - 1921) >> 1 == -461
    got = both_updates(390625, 1000, 100, (1500, 1001, True))
    assert got == [((1468, 1000, True), 1000, 0)] * 2                                   # fast <= slow
    assert both_updates(390625, 1000, 100, (1000, 1000, True)) == [((1000, 1000, True), 1000, 0)] * 2       # equal: none
    assert both_updates(0, 1000, 100, (1, 1, True)) == [((0, 0, True), 0, 0)] * 2       # -1 >> 4 = -1: down to 0, never below


def test_update_beyond_32_bits():
    # cost_sum near 2^38, its product with 256 near 2^46: N B = 2^22 rays of 65535
    n, b = 4096, 1024
    top = n * b * 65535
    assert top * 256 > 1 << 45 and top > 1 << 37
    assert both_updates(top, n, b, (0, 0, False)) == [((rref.MAX_FIT, rref.MAX_FIT, True), rref.MAX_FIT, 0)] * 2
    assert both_updates(top - 1, n, b, (0, 0, False))[1][1] == rref.MAX_FIT - 1
    assert both_updates(top + 1, n, b, (0, 0, False)) == [IndexError] * 2
    got = both_updates(top, n, b, (0, 0, True), 4, 1, 1, 1)
    assert got == [((rref.MAX_FIT >> 4, rref.MAX_FIT >> 1, True), rref.MAX_FIT, n * ((rref.MAX_FIT >> 1) - (rref.MAX_FIT >> 4)) // (rref.MAX_FIT >> 1))] * 2
    # N max_num beyond 32 bits
    assert both_updates(top, 65536, 64, (0, 0, True), 4, 0, 0xFFFFFFFF, 0xFFFFFFFF)[1][2] == 65536 * (rref.MAX_FIT - (rref.MAX_FIT >> 4)) // rref.MAX_FIT


def test_update_against_the_statement_on_a_random_walk():
    rng = np.random.default_rng(61)
    state = [(0, 0, False)] * 2
    for k in range(400):
        n, b = int(rng.integers(1, 65537)), int(rng.integers(0, 1025))
        cost = int(rng.integers(0, n * b * (65535 if k % 7 == 0 else 300) + 1))
        a = (int(rng.integers(0, 31)), int(rng.integers(0, 31)), int(rng.integers(0, 9)), 8)
        got = [rref.recovery_update(cost, n, b, state[0], *a), kh.mcl_recovery_update(cost, n, b, state[1], *a)]
        assert got[0] == got[1], (k, n, b, cost, a)
        state = [got[0][0], got[1][0]]


GOOD = dict(cost_sum=1000, n=100, b_used=10, state=(5, 5, True), a_slow=4, a_fast=1, max_num=1, max_den=4)
# one refusal each, in the documented order; every case also carries all the LATER faults, so the first must win
FAULTS = [("a_slow", 31, ValueError), ("a_slow", -1, ValueError), ("a_fast", 31, ValueError), ("max_den", 0, ValueError),
          ("max_num", 5, ValueError), ("n", 0, IndexError), ("n", 65537, IndexError), ("b_used", 1025, IndexError),
          ("cost_sum", 1 << 40, IndexError), ("state", (-1, 5, True), IndexError), ("state", (5, rref.MAX_FIT + 1, True), IndexError)]


@pytest.mark.parametrize("first", range(len(FAULTS)))
def test_update_refuses_in_order(first):
    kw, faulty = dict(GOOD), set()
    for name, value, _ in FAULTS[first:]:                       # the fault under test, and one later fault per other argument
        if name not in faulty:
            kw[name] = value
            faulty.add(name)
    want = FAULTS[first][2]
    assert both_updates(**kw) == [want, want], (FAULTS[first], sorted(faulty))
    assert both_updates(**GOOD) == [((20, 130, True), 256, 25)] * 2


# ---- rule 62: the slots ----
@pytest.mark.parametrize("n_particles", [1, 7, 64, 300])
def test_exactly_n_slots_spread_evenly(n_particles):
    for n in range(n_particles + 1):
        slots = rref.injected_slots(n_particles, n)
        assert len(slots) == n and slots == sorted(set(slots))
        # the i-th injected slot, as the device finds it: ceil((i + 1) N / n) - 1
        assert slots == [((i + 1) * n_particles + n - 1) // n - 1 for i in range(n)]
        if n > 1:
            gaps = [b - a for a, b in zip(slots, slots[1:])]
            assert max(gaps) - min(gaps) <= 1
    assert rref.injected_slots(n_particles, n_particles) == list(range(n_particles))
    if n_particles > 1:
        assert rref.injected_slots(n_particles, 1) == [n_particles - 1]


# ---- the two forms ----
def pair(c, n, angles, range_max, seed, reach):
    dist = dref.DistRef(c, reach)
    loop = rref.FitRef(c, 0.1, n, angles, range_max, seed, dist=dist)
    vec = rref.FitVec(c, 0.1, n, angles, range_max, seed, dist.field)
    t = fref.field_tables(0.1, 0.15, reach=reach, w_shift=2, temperature=64.0)
    loop.set_field_model(t[0], t[1], t[3], t[4])
    vec.set_field_model(t[0], t[1], t[3], t[4])
    return loop, vec


def test_loop_form_equals_vectorised_form():
    """fcpu's small case (N 64, B 7) with a fit at every step and an injecting resample after each: n = 0, N / 4, N."""
    c = fcpu.small_world()
    angles = [0.0, 0.9, 1.8, 2.7, 3.6, 4.5, 5.4]
    for seed in (0, 1):
        loop, vec = pair(c, 64, angles, 1.5, seed, 3)
        loop.init_pose(3 << 16, 26 << 16, 9000, 150000, 9000)
        vec.init_pose(3 << 16, 26 << 16, 9000, 150000, 9000)
        assert loop.fit is None and vec.fit is None
        zmax = loop.zmax
        scans = [[zmax - 1, 3 << 16, -1, zmax, 0, 7 << 16, 5 << 15], [1 << 16, 2 << 16, 3 << 16, 4 << 16, 5 << 16, 6 << 16, 7 << 16],
                 [zmax, zmax, -1, 9 << 15, 1, 2, 3]]
        for k, (zq, n) in enumerate(zip(scans, (0, 16, 64))):
            args = (70000, -20000, 700, 9000, 4000, 300, zq, SKIP)
            ra, rb = loop.step(*args), vec.step(*args)
            assert ra.as_tuple() == rb.as_tuple() and loop.fit.as_tuple() == vec.fit.as_tuple(), (seed, k)
            assert loop.fit.cost_min <= loop.fit.cost_best and loop.fit.cost_sum >= 64 * loop.fit.cost_min
            sa, sb = loop.resample_inject(n), vec.resample_inject(n)
            assert sa == sb and sa.count(-1) == n and fcpu.same(loop, vec), (seed, k)
            i, j = (np.array(loop.tx) + 32768) >> 16, (np.array(loop.ty) + 32768) >> 16
            inj = [s == -1 for s in sa]
            assert (c[i[inj], j[inj]] == ref.EMPTY).all()                        # an injected particle lies in a free cell
    # a plane without a free cell: the injected slots keep rule 40's state
    full = np.full((37, 29), ref.OCCUPIED, np.int8)
    loop, vec = pair(full, 64, angles, 1.5, 0, 3)
    for m in (loop, vec):
        m.init_pose(3 << 16, 26 << 16, 9000, 150000, 9000)
        m.step(0, 0, 0, 9000, 4000, 300, scans[1], SKIP)
    assert loop.resample_inject(64) == vec.resample_inject(64) and fcpu.same(loop, vec)
    with pytest.raises(IndexError):
        loop.resample_inject(65)
    with pytest.raises(mref.StateError):
        loop.resample_inject(3)                                                  # no step since the resample


def test_fitvec_step_is_the_parent_statements_step():
    """FitVec.step restates MclFieldVec.step with the cost kept (the parent statement hands no cost out): the two must not
    drift apart.  The small case again, both inits, a -1 beam and a ZMAX beam, a resample after the second step: equal
    records, weights and states at every step."""
    c = fcpu.small_world()
    angles = [0.0, 0.9, 1.8, 2.7, 3.6, 4.5, 5.4]
    t = fref.field_tables(0.1, 0.15, reach=3, w_shift=2, temperature=64.0)
    for seed, start in ((0, "pose"), (1, "global")):
        dist = dref.DistRef(c, 3)
        new = rref.FitVec(c, 0.1, 64, angles, 1.5, seed, dist.field)
        old = fref.MclFieldVec(c, 0.1, 64, angles, 1.5, seed, dist.field)
        for m in (new, old):
            m.set_field_model(t[0], t[1], t[3], t[4])
            if start == "pose":
                m.init_pose(3 << 16, 26 << 16, 9000, 150000, 9000)
            else:
                assert m.init_global() > 0
        zmax = new.zmax
        scans = [[zmax - 1, 3 << 16, -1, zmax, 0, 7 << 16, 5 << 15], [1 << 16, 2 << 16, 3 << 16, 4 << 16, 5 << 16, 6 << 16, 7 << 16],
                 [zmax, zmax, -1, 9 << 15, 1, 2, 3]]
        for k, zq in enumerate(scans):
            args = (70000, -20000, 700, 9000, 4000, 300, zq, SKIP)
            ra, rb = new.step(*args), old.step(*args)
            assert ra.as_tuple() == rb.as_tuple() and new.w == old.w and fcpu.same(new, old), (seed, k)
            assert (new.step_count, new.min_prev) == (old.step_count, old.min_prev)
            if k == 1:
                assert new.resample_inject(0) == old.resample() and fcpu.same(new, old)


def test_the_loop_form_states_the_beam_model_too():
    c = fcpu.small_world()
    m = rref.FitRef(c, 0.1, 16, [0.0, 1.3, 2.6, 3.9], 1.5, 2)
    m.set_model(*mref.sensor_tables(0.1, 0.1))
    m.init_pose(9 << 16, 9 << 16, 100, 90000, 9000)
    zq = [3 << 16, -1, m.zmax, 1 << 15]
    m.step(1000, 0, 10, 900, 400, 30, zq, SKIP)
    assert m.fit.step == 1 and m.fit.cost_sum == sum(m.acc) and rref.beams_used(zq, m.zmax, False) == 3
    assert rref.beams_used(zq, m.zmax, True) == 2


# ---- does the policy recover?  (no device: the statement alone) ----
RECOVERY_N = 16384
KIDNAP_STEP = 13
STEPS = 36
RECOVERY_POS_BOUND = fcpu.GLOBAL_POS_BOUND                       # 3.0 cells
# degrees: the bound is twice the statement's own worst over the six seeds, 1.795 at seed 2.  The six (cells, degrees) after
# step 36: (0.093, 0.222), (0.237, 1.088), (0.628, 1.795), (1.566, 0.289), (0.116, 0.466), (0.329, 0.954); DESIGN.md 4.11 has
# the table
RECOVERY_YAW_WORST = 1.795
LOST_POS_BOUND = 40.0                                            # cells: a filter that stays lost


def kidnap_drive(steps=23):
    """The drive after the teleport, in the room left of the first wall: 24 poses from cell (30, 10), 2 cells and 2 degrees
    a step."""
    x, y, yaw = 30 * ROOM_RES, 10 * ROOM_RES, 1.6
    out = [(x, y, yaw)]
    for _ in range(steps):
        x, y, yaw = x + 2 * ROOM_RES * math.cos(yaw), y + 2 * ROOM_RES * math.sin(yaw), yaw + math.radians(2.0)
        out.append((x, y, yaw))
    return out


@functools.lru_cache(maxsize=None)
def kidnap_scene():
    """-> (room, truth, odometry, scans), index k for step k (index 0: the init).  Steps 1 to 12 are base.drive(); step 13
    is the teleport: its odometry says (0, 0, 0) and its scan is taken at the second drive's first pose, cell (30, 10);
    steps 14 to 36 follow that drive with its true odometry."""
    c = base.room()
    first, second = base.drive(), kidnap_drive()
    truth = first + second
    assert len(truth) == STEPS + 1
    odom = [None] + [(truth[k - 1], truth[k]) for k in range(1, STEPS + 1)]
    odom[KIDNAP_STEP] = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    table = mref.scan_table(ROOM_BEAMS)
    scans = [base.sref.scan_pose(c, ROOM_RES, ref.quantise_pose(ROOM_RES, (0.0, 0.0), *p), table, ROOM_RANGE)[0] for p in truth]
    return c, truth, odom, scans


def motion_scales():
    cells = 65536.0 / float(np.float32(ROOM_RES))
    return (mref.noise_scale(base.NOISE[0] * cells), mref.noise_scale(base.NOISE[1] * cells),
            mref.noise_scale(base.NOISE[2] / (2 * math.pi) * 65536.0))


INIT_SIGMA = (0.1, math.radians(3.0))                            # metres, radians: the init at the truth


def statement(seed, n=RECOVERY_N, form=rref.FitVec):
    """The vectorised statement over the room, the default field tables, initialised at the truth.  form:
    fref.MclFieldVec for the statement as it was before the fit."""
    c, truth = kidnap_scene()[:2]
    pen, far, reach, wtab, ws = fref.field_tables(ROOM_RES, 0.1)
    m = form(c, ROOM_RES, n, ROOM_BEAMS, ROOM_RANGE, seed, dref.DistRef(c, reach).field)
    m.set_field_model(pen, far, wtab, ws)
    x0, y0, yaw0 = truth[0]
    q = ref.quantise_pose(ROOM_RES, (0.0, 0.0), x0, y0, 0.0)
    m.init_pose(q[2], q[3], mref.quantise_heading(yaw0), mref.noise_scale(INIT_SIGMA[0] * 65536.0 / float(np.float32(ROOM_RES))),
                mref.noise_scale(INIT_SIGMA[1] / (2 * math.pi) * 65536.0))
    return m


def step_args(k):
    """Step k's arguments in the ABI's integers."""
    _, _, odom, scans = kidnap_scene()
    return (*mref.odometry_increment(ROOM_RES, *odom[k]), *motion_scales(), mref.quantise_ranges(scans[k], ROOM_RES, ROOM_RANGE, SKIP), SKIP)


@functools.lru_cache(maxsize=None)
def recovery_run(seed, recover):
    """-> a list, index k - 1 for step k, of (Filter.step's dict, position error in cells, yaw error in degrees)."""
    truth = kidnap_scene()[1]
    f = rref.Filter(statement(seed), rref.DEFAULT_POLICY if recover else None)
    out = []
    for k in range(1, STEPS + 1):
        s = f.step(*step_args(k))
        out.append((s, *base.errors(mref.estimate(s["rec"], ROOM_RES, (0.0, 0.0)), truth[k])))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_statement_recovers_from_a_kidnap(seed):
    run = recovery_run(seed, True)
    print(f"seed {seed}: after step {STEPS} position error {run[-1][1]:.3f} cells, yaw error {run[-1][2]:.3f} degrees; injected "
          f"{[s['injected'] for s, _, _ in run]}; fit {[s['fit'] for s, _, _ in run]}")
    assert run[-1][1] < RECOVERY_POS_BOUND
    assert run[-1][2] < 2 * RECOVERY_YAW_WORST
    assert [s["injected"] for s, _, _ in run[1:12]] == [0] * 11  # steps 2 to 12: localised, nothing injected
    assert run[KIDNAP_STEP - 1][0]["injected"] > 0


@pytest.mark.parametrize("seed", range(6))
def test_statement_stays_lost_without_the_injection(seed):
    """The control: the same runs with recovery off.  The averages still run, nothing is injected."""
    run = recovery_run(seed, False)
    print(f"seed {seed}: position errors after the kidnap {[round(p, 1) for _, p, _ in run[KIDNAP_STEP - 1:]]}")
    assert all(p > LOST_POS_BOUND for _, p, _ in run[KIDNAP_STEP - 1:])
    assert all(s["injected"] == 0 for s, _, _ in run)
    on = recovery_run(seed, True)
    assert [s["rec"].as_tuple() for s, _, _ in run[:12]] == [s["rec"].as_tuple() for s, _, _ in on[:12]]     # equal up to the kidnap
    assert [(s["fit"], s["fit_slow"], s["fit_fast"]) for s, _, _ in run[:13]] == [(s["fit"], s["fit_slow"], s["fit_fast"]) for s, _, _ in on[:13]]


@pytest.mark.parametrize("seed", range(6))
def test_fit_separates_lost_from_localised(seed):
    run = recovery_run(seed, True)
    localised = max(s["fit"] for s, _, _ in run[3:12])           # steps 4 to 12
    lost = min(s["fit"] for s, _, _ in run[12:15])               # steps 13 to 15
    print(f"seed {seed}: fit at most {localised} while localised, at least {lost} right after the kidnap")
    assert 0 <= localised and 2 * localised < lost
