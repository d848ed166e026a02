"""The Monte-Carlo localiser without a device (DESIGN.md 4.11 rules 28 to 41): the host-only entries of the library
(kc_mcl_check, kc_mcl_heading), the host classes' arithmetic (kompass_cpp.mapping.MCL's statics) and the Python
statement tests/worldmap_mcl_ref.py itself: its random numbers, its resampling, its sums, and whether it localises.

The convergence tests run the statement alone; DESIGN.md 4.11 has their measured errors."""
import math

import numpy as np
import pytest

import kompass_cpp
import kompass_hip as kh
import worldmap_mcl_ref as mref
import worldmap_ref as ref
import worldmap_scan_ref as sref

CPP = kompass_cpp.mapping.MCL
M64 = (1 << 64) - 1


# ---- rule 30 ----
def test_mix64_known_answer():
    assert mref.mix64(0) == 0xE220A8397B1DCDAF
    assert mref.draw(0, 0, 0, 0) == mref.mix64(mref.mix64(0))
    assert mref.draw(5, 3, 7, 2) == mref.mix64(mref.mix64(5 ^ (3 << 32)) ^ ((7 << 8) | 2))
    assert all(0 <= mref.draw(2 ** 64 - 1, 2 ** 32 - 1, 65535, c) <= M64 for c in (0, 15, 255))


def test_noise_bounds_and_symmetry():
    rng = np.random.default_rng(1)
    vs = [0, M64, 0xFFFF, 0xFFFF0000FFFF0000] + [int(v) for v in rng.integers(0, 2 ** 63, 400)]
    for s in (0, 1, 37, 65536, 2 ** 20 + 3, 2 ** 31 - 1):
        bound = (131070 * s + (1 << 15)) >> 16
        for v in vs:
            n = mref.noise(v, s)
            assert abs(n) <= bound
            mirror = v ^ M64                                   # every field a -> 65535 - a: g -> -g
            x = ((v & 0xFFFF) + ((v >> 16) & 0xFFFF) + ((v >> 32) & 0xFFFF) + (v >> 48) - 131070) * s
            # the two roundings to nearest differ only where x lies on a half: both go up there
            assert n + mref.noise(mirror, s) == (1 if (x & 0xFFFF) == 0x8000 else 0)
    assert mref.noise(M64, 65536) == 131070 and mref.noise(0, 65536) == -131070
    assert mref.noise_scale(mref.NOISE_STD) == 65536 and CPP.noise_scale(mref.NOISE_STD) == 65536
    for sigma in (0.0, 1.0, 12345.6, 9 * 65536.0):
        assert CPP.noise_scale(sigma) == mref.noise_scale(sigma) == kh.mcl_noise_scale(sigma)


def test_noise_has_the_stated_deviation():
    g = [mref.noise(mref.draw(11, 1, p, 0), 65536) for p in range(20000)]
    assert abs(np.mean(g)) < 3 * mref.NOISE_STD / math.sqrt(len(g))
    assert abs(np.std(g) / mref.NOISE_STD - 1.0) < 0.03


# ---- rule 29 ----
def test_heading_table_at_every_heading():
    want = mref.headings()
    for h in range(65536):
        assert kh.mcl_heading(h) == want[h], h
    assert want[0] == (65536, 0) and want[16384] == (0, 65536) and want[32768] == (-65536, 0)
    with pytest.raises(IndexError):
        kh.mcl_heading(65536)
    with pytest.raises(IndexError):
        mref.heading(65536)


# ---- rule 38 ----
GOOD = dict(resolution=0.05, n_particles=100, n_beams=64, range_max=10.0, pen=[0, 1, 2], err_shift=3, wtab=[9, 9, 4, 0],
            w_shift=2, flags=3)
# one refusal each, in the documented order; every case also carries all the LATER faults, so the first must win
FAULTS = [("resolution", float("nan"), ValueError), ("n_particles", 0, ValueError), ("n_particles", 65537, IndexError),
          ("n_beams", 1025, IndexError), ("n_beams", 1024, IndexError),      # 4097 x 1024 rays, below
          ("range_max", float("inf"), ValueError), ("range_max", 0.05 * 2048.5, IndexError),
          ("pen", [], ValueError), ("pen", [1] * 4097, IndexError), ("err_shift", 31, ValueError),
          ("wtab", [], ValueError), ("wtab", [1] * 4097, IndexError), ("w_shift", -1, ValueError),
          ("wtab", [(1 << 20) + 1], ValueError), ("wtab", [5, 6], ValueError), ("flags", 4, ValueError)]


def both_checks(**kw):
    out = []
    for fn in (mref.check, kh.mcl_check):
        try:
            out.append(fn(**kw))
        except (ValueError, IndexError) as e:
            out.append(type(e))
    return out


def test_check_accepts_and_reports():
    assert both_checks(**GOOD) == [(200, 13107200)] * 2
    assert both_checks(**dict(GOOD, n_particles=65536, n_beams=64)) == [(200, 13107200)] * 2    # 2^22 rays exactly
    assert both_checks(**dict(GOOD, n_particles=4096, n_beams=1024)) == [(200, 13107200)] * 2
    assert both_checks(**dict(GOOD, range_max=0.05 * 2047.5))[0][0] == 2048
    assert both_checks(**dict(GOOD, pen=None, wtab=None, err_shift=99, w_shift=99)) == [(200, 13107200)] * 2
    assert both_checks(**dict(GOOD, wtab=[1 << 20] * 4096, pen=[65535] * 4096, err_shift=30, w_shift=30)) == [(200, 13107200)] * 2


@pytest.mark.parametrize("first", range(len(FAULTS)))
def test_check_refuses_in_order(first):
    kw, faulty = dict(GOOD), set()
    for name, value, _ in FAULTS[first:]:                       # the fault under test, and one later fault per other argument
        if name not in faulty:
            kw[name] = value
            faulty.add(name)
    if FAULTS[first][:2] == ("n_beams", 1024):
        kw["n_particles"] = 4097                               # the ray cap: neither count is above its own
    want = FAULTS[first][2]
    assert both_checks(**kw) == [want, want], (FAULTS[first], sorted(faulty))


# ---- rule 40 ----
def test_systematic_copies_are_floor_or_ceil():
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 64, 301):
        for trial in range(6):
            w = [int(v) for v in rng.integers(0, 1 << 20, n)]
            w[int(rng.integers(0, n))] = 1 << 20
            if n > 2:
                w[int(rng.integers(0, n))] = 0
            w1 = sum(w)
            for u0 in (0, w1 - 1, int(rng.integers(0, w1))):
                src = mref.systematic(w, u0)
                assert src == sorted(src) and len(src) == n
                for i in range(n):
                    copies = src.count(i)
                    assert copies in (n * w[i] // w1, -(-n * w[i] // w1)), (n, i, copies)
                    assert w[i] > 0 or copies == 0


def test_systematic_equal_weights_and_one_heavy():
    for n in (1, 5, 64, 1000):
        for u0 in (0, 3, 7 * n - 1):
            assert mref.systematic([7] * n, u0 % (7 * n)) == list(range(n))
        for heavy in (0, n // 2, n - 1):
            w = [0] * n
            w[heavy] = 12345
            assert mref.systematic(w, 12344) == [heavy] * n == mref.systematic(w, 0)


def test_resample_decision_is_exact():
    n = 1000
    # n_eff = w1^2 / w2 against n / 2: w1^2 * 2 < n * w2
    w2 = 2 * 10 ** 12 + 1
    for w1 in (10 ** 9, 10 ** 9 + 1, 31622776, 31622777):      # 10^18 * 2 < 1000 * w2 = 2 10^15 + 1000 ... and sqrt(10^15)
        rec = mref.Record(w1=w1, w2=w2, sx=0, sy=0, sc=1, ss=0, amin=0, best=0, best_tx=0, best_ty=0, best_h=0, step=1)
        assert mref.should_resample(rec, n) == (w1 * w1 * 2 < n * w2) == CPP.should_resample(w1, w2, n)
    # just on either side of the threshold, where a double's 53 bits cannot tell: w1^2 * 2 = n * w2 -+ 1
    w1 = (1 << 30) + 1234567
    for n, w2, want in [(2, w1 * w1, False), (2, w1 * w1 + 1, True), (2, w1 * w1 - 1, False)]:
        rec = mref.Record(w1=w1, w2=w2, sx=0, sy=0, sc=1, ss=0, amin=0, best=0, best_tx=0, best_ty=0, best_h=0, step=1)
        assert mref.should_resample(rec, n) is want and CPP.should_resample(w1, w2, n) is want
        assert float(w1) * float(w1) * 2.0 == float(n) * float(w2)      # the doubles see a tie every time
    assert CPP.should_resample(5, 25, 7, 0, 1) is False                 # num = 0: never


# ---- rules 37 and 39 ----
def test_record_sums_beyond_64_bits():
    n = 300
    tx = [-(1 << 36)] + [1 << 36] * (n - 1)
    ty = [1 << 36] + [-(1 << 36)] * (n - 1)
    h = [(37 * p) & 0xFFFF for p in range(n)]
    rec, w = mref.record_of(tx, ty, h, [0] * n, [1 << 20], 0, 4)
    assert w == [1 << 20] * n and rec.best == 0
    assert rec.sx == (n - 1) * (1 << 20) * (1 << 37) > (1 << 64) and rec.sy == -rec.sx
    H = mref.headings()
    assert rec.sc == sum((1 << 20) * H[v][0] for v in h) and rec.w2 == n << 40
    # the record's (lo, hi) halves as the library hands them out, joined by the ctypes structure
    r = kh.MclRecord(w1=rec.w1, w2=rec.w2, sx_lo=rec.sx & M64, sx_hi=rec.sx >> 64, sy_lo=rec.sy & M64, sy_hi=rec.sy >> 64)
    assert (r.sx, r.sy) == (rec.sx, rec.sy) and r.sy_hi < 0
    est = mref.estimate(rec, 0.05, (1.0, -2.0))
    assert est["txe"] == -(1 << 36) + rec.sx // rec.w1 and est["tye"] == (1 << 36) + rec.sy // rec.w1
    e = CPP.estimate_of(rec.w1, rec.w2, rec.sx & M64, rec.sx >> 64, rec.sy & M64, rec.sy >> 64, rec.sc, rec.ss, rec.best_tx,
                        rec.best_ty, 0.05, 1.0, -2.0)
    assert (e.txe, e.tye, e.x, e.y, e.yaw, e.n_eff) == (est["txe"], est["tye"], est["x"], est["y"], est["yaw"], est["n_eff"])


def test_estimate_floors_negative_sums():
    for sx, w1, want in [(-1, 3, -1), (-3, 3, -1), (-4, 3, -2), (4, 3, 1), (0, 3, 0), (-(1 << 70) - 1, 1 << 20, -(1 << 50) - 1)]:
        rec = mref.Record(w1=w1, w2=w1, sx=sx, sy=-sx, sc=-5, ss=-5, amin=0, best=0, best_tx=100, best_ty=-100, best_h=0, step=1)
        est = mref.estimate(rec, 0.25, (0.5, 0.25))
        assert est["txe"] == 100 + want and est["tye"] == -100 + (-sx) // w1
        e = CPP.estimate_of(w1, w1, sx & M64, sx >> 64, (-sx) & M64, (-sx) >> 64, -5, -5, 100, -100, 0.25, 0.5, 0.25)
        assert (e.txe, e.tye) == (est["txe"], est["tye"])
        assert (e.x, e.y, e.yaw) == (est["x"], est["y"], est["yaw"]) and e.yaw == math.atan2(-5.0, -5.0)


def test_host_quantisers_agree():
    ranges = [0.1, float("nan"), float("inf"), 10.0, 20.0, -0.1, 0.0, 9.999999, 0.2, 3.14159]
    for flags in (0, mref.SKIP_NO_RETURN):
        want = mref.quantise_ranges(ranges, 0.05, 10.0, flags)
        assert list(CPP.quantise_ranges(ranges, 0.05, 10.0, flags)) == want == kh.mcl_quantise_ranges(ranges, 0.05, 10.0, flags).tolist()
    for yaw in (0.0, -0.3, math.pi, -math.pi, 7.0, 1e-6):
        assert CPP.quantise_heading(yaw) == mref.quantise_heading(yaw)
    a, b = (0.3, -1.2, 0.7), (0.41, -1.0, 0.9)
    assert tuple(CPP.odometry_increment(0.05, a, b)) == mref.odometry_increment(0.05, a, b)
    pen, es, wtab, ws = CPP.sensor_tables(0.05, 0.1)
    assert (list(pen), es, list(wtab), ws) == mref.sensor_tables(0.05, 0.1)
    assert mref.check(0.05, 1, 1, 10.0, pen, es, wtab, ws)


# ---- does the statement localise?  (no device: the statement alone) ----
ROOM_W, ROOM_H, ROOM_RES = 120, 90, 0.05
ROOM_RANGE = 2.5                                                # 50 cells
ROOM_BEAMS = [k * (2 * math.pi / 24) for k in range(24)]


def room():
    """Walls all round, three interior walls with doors and a few seeded pillars: no symmetry."""
    c = np.full((ROOM_W, ROOM_H), ref.EMPTY, np.int8)
    c[0, :] = c[-1, :] = ref.OCCUPIED
    c[:, 0] = c[:, -1] = ref.OCCUPIED
    c[40, 0:55] = ref.OCCUPIED
    c[40, 20:28] = ref.EMPTY
    c[40:95, 60] = ref.OCCUPIED
    c[62:70, 60] = ref.EMPTY
    c[85, 15:60] = ref.OCCUPIED
    c[85, 40:46] = ref.EMPTY
    rng = np.random.default_rng(17)
    for i, j in zip(rng.integers(5, ROOM_W - 5, 14), rng.integers(5, ROOM_H - 5, 14)):
        c[i:i + 2, j:j + 2] = ref.OCCUPIED
    return c


def drive(steps=12):
    """A curved drive through the middle room: 2 cells and 5 degrees a step."""
    x, y, yaw = 55 * ROOM_RES, 22 * ROOM_RES, 0.3
    out = [(x, y, yaw)]
    for _ in range(steps):
        x, y, yaw = x + 2 * ROOM_RES * math.cos(yaw), y + 2 * ROOM_RES * math.sin(yaw), yaw + math.radians(5.0)
        out.append((x, y, yaw))
    return out


@pytest.fixture(scope="module")
def scene():
    c = room()
    path = drive()
    table = sref.scan_table(ROOM_BEAMS)
    scans = [sref.scan_pose(c, ROOM_RES, ref.quantise_pose(ROOM_RES, (0.0, 0.0), *p), table, ROOM_RANGE)[0] for p in path]
    return c, path, scans


MODEL = dict(sigma_hit=0.1)                                     # the front ends' default tables
NOISE = (0.01, 0.005, 0.005)                                    # metres forward and lateral, radians, a step


def localise(scene, m, steps=12):
    """Run the statement along the drive -> [(estimate, spread)] a step; the odometry is the true increment."""
    c, path, scans = scene
    cells = 65536.0 / float(np.float32(ROOM_RES))
    s = (mref.noise_scale(NOISE[0] * cells), mref.noise_scale(NOISE[1] * cells), mref.noise_scale(NOISE[2] / (2 * math.pi) * 65536.0))
    out = []
    for k in range(1, steps + 1):
        d = mref.odometry_increment(ROOM_RES, path[k - 1], path[k])
        rec = m.step(*d, *s, mref.quantise_ranges(scans[k], ROOM_RES, ROOM_RANGE))
        est = mref.estimate(rec, ROOM_RES, (0.0, 0.0))
        out.append((est, mref.spread(m.tx, m.ty, m.w, est, ROOM_RES)))
        if mref.should_resample(rec, m.n):
            m.resample()
    return out


def errors(est, truth):
    dyaw = (est["yaw"] - truth[2] + math.pi) % (2 * math.pi) - math.pi
    return math.hypot(est["x"] - truth[0], est["y"] - truth[1]) / ROOM_RES, abs(math.degrees(dyaw))


@pytest.mark.parametrize("seed", range(6))
def test_statement_converges_from_an_offset(scene, seed):
    """128 particles, 24 beams, 12 steps; the init is 3 cells and 3 degrees off the truth.  The final errors must be below
    half of that: 1.5 cells and 1.5 degrees.  DESIGN.md 4.11 has the six measured pairs."""
    c, path, scans = scene
    m = mref.MclRef(c, ROOM_RES, 128, ROOM_BEAMS, ROOM_RANGE, seed)
    m.set_model(*mref.sensor_tables(ROOM_RES, **MODEL))
    x0, y0, yaw0 = path[0]
    off = 3 * ROOM_RES
    tx0 = round((x0 + off * 0.8) / ROOM_RES * 65536.0)
    ty0 = round((y0 - off * 0.6) / ROOM_RES * 65536.0)
    cells = 65536.0 / float(np.float32(ROOM_RES))
    m.init_pose(tx0, ty0, mref.quantise_heading(yaw0 + math.radians(3.0)), mref.noise_scale(0.1 * cells),
                mref.noise_scale(math.radians(3.0) / (2 * math.pi) * 65536.0))
    run = localise(scene, m)
    pos, yaw = errors(run[-1][0], path[-1])
    print(f"seed {seed}: position error {pos:.3f} cells, yaw error {yaw:.3f} degrees, spread {run[0][1]:.4f} -> {run[-1][1]:.4f} m")
    assert pos < 1.5 and yaw < 1.5
    assert run[-1][1] < run[0][1]


def test_statement_global_init_covers_the_free_cells(scene):
    """512 particles over the room's free cells.  Whether the filter then finds the robot is NOT asserted: on this room,
    with seed 0, 512 particles and the 12 steps above, the statement settles on a wrong mode (the best particle 38 cells
    from the truth after step 12): 512 hypotheses over 10196 cells x 65536 headings are too few."""
    c = scene[0]
    m = mref.MclRef(c, ROOM_RES, 512, ROOM_BEAMS, ROOM_RANGE, 0)
    n_free = m.init_global()
    assert n_free == int((c == ref.EMPTY).sum()) == 10196
    i, j = (np.array(m.tx) + 32768) >> 16, (np.array(m.ty) + 32768) >> 16
    assert (c[i, j] == ref.EMPTY).all() and m.acc == [0] * 512 and m.step_count == 0
    assert len(set(zip(i.tolist(), j.tolist()))) > 480 and len(set(v >> 13 for v in m.h)) == 8      # spread over cells and octants
