"""CPU: the oracle's mapper (ko.scan_to_grid, ko.BayesMapper) against tests/mapper_ref.py, a literal restatement
of LocalMapper and bresenhamEnhanced that walks every step from the start cell, grid for grid and bit for bit.

The oracle and the kernels share one derivation of the clipped walk (a step range and a closed-form state before
its first step); these tests pin that derivation to the reference's loop at the edges where it can slip: sensors
on and outside every border, slopes 0, 1, 1/2 and 2/3, lines that leave through a side or a corner or end one
cell outside, 1 x N and N x 1 grids, and (with the native walker, tests/native/bresenham_literal.cpp) lines of up
to 2^29 steps and sensors up to just below 2^30 cells away.  Each line is also compared on its own, so that a
cell one beam misses cannot hide under another beam's."""
import json
from pathlib import Path

import numpy as np
import pytest

import mapper_ref as mr
from oracle import ko

GOLD = Path(__file__).parent / "golden"
BAYES = dict(p_prior=0.6, p_occupied=0.9, p_empty=0.1, range_sure=0.1, range_max=20.0, wall_size=0.2)
# the range of a beam enters a cell's probability only through distance < range - wall_size: a wide wall makes
# the last cells of every beam depend on which beam wrote them last
WALL = dict(BAYES, wall_size=2.5)
RES = 0.5   # a power of two: sensor cells are exact


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _per_beam_grids(H, W, pos, ang, rng, walker=None):
    """The restatement's grid of every beam on its own: [n, H, W]."""
    s, b, i, j, ends = mr.emissions(H, W, RES, pos, 0.0, ang, rng, walker)
    g = np.full((len(ang), H, W), mr.UNEXPLORED, np.int32)
    at_end = (i == ends[b, 0]) & (j == ends[b, 1])
    np.maximum.at(g, (b[~at_end], i[~at_end], j[~at_end]), mr.EMPTY)
    g[b[at_end], i[at_end], j[at_end]] = mr.OCCUPIED
    return g


def _check_each_line(H, W, sensor, targets):
    pos = mr.sensor_pos(H, W, RES, sensor)
    ang, rng, ends = mr.aim(H, W, RES, pos, targets)
    np.testing.assert_array_equal(ends, np.asarray(targets))
    want = _per_beam_grids(H, W, pos, ang, rng)
    for k in range(len(ang)):
        got = ko.scan_to_grid(H, W, RES, pos, 0.0, ang[k:k + 1], rng[k:k + 1])
        if not np.array_equal(got, want[k]):
            raise AssertionError(f"{H}x{W} sensor {sensor} -> {tuple(targets[k])}: "
                                 f"{int((got != want[k]).sum())} cells differ")
    # and all of them as one scan
    np.testing.assert_array_equal(ko.scan_to_grid(H, W, RES, pos, 0.0, ang, rng),
                                  mr.scan_to_grid(H, W, RES, pos, 0.0, ang, rng))
    return len(ang)


# ---------------------------------------------------------------------------
# every short line, one at a time
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(12, 9), (7, 7), (1, 13), (13, 1)])
def test_every_short_line_from_border_and_outside_cells(H, W):
    """From the border cells and from 1, 2 and 3 cells outside every side and corner, every end cell within 7 cells
    (slopes 0, 1, 1/2, 2/3 and all the rest; zero-length lines; ends inside, on the border, one cell out and
    beyond, leaving through a side or a corner)."""
    sensors = mr.border_and_outside_cells(H, W, dists=(1, 2, 3))
    offs = [(a, b) for a in range(-7, 8) for b in range(-7, 8)]
    n = 0
    for s in sensors:
        n += _check_each_line(H, W, s, [(s[0] + a, s[1] + b) for a, b in offs])
    assert n == len(sensors) * 225


def test_slopes_that_hit_the_on_the_line_stamp():
    """|slope| 0, 1, 1/2, 2/3 (and 1/3, 3/4) at lengths up to 60 steps in every direction, from inside and from
    outside, in a grid they cross: the double stamp of error + errorprev == ddx and e = 0 (mod ddmaj)."""
    H, W = 23, 31
    dirs = [(1, 0), (0, 1), (1, 1), (2, 1), (1, 2), (3, 2), (2, 3), (3, 1), (4, 3)]
    for s in [(11, 15), (0, 0), (-5, 15), (11, -9), (30, 40)]:
        targets = []
        for a, b in dirs:
            for sa in (1, -1):
                for sb in (1, -1):
                    for m in (1, 2, 5, 13, 20):
                        targets.append((s[0] + sa * a * m, s[1] + sb * b * m))
        _check_each_line(H, W, s, targets)


# ---------------------------------------------------------------------------
# random scenes, whole scans
# ---------------------------------------------------------------------------
def _random_scene(r):
    H, W = int(r.integers(1, 40)), int(r.integers(1, 40))
    s = (int(r.integers(-20, H + 20)), int(r.integers(-20, W + 20)))
    pos = mr.sensor_pos(H, W, RES, s)
    n = int(r.integers(1, 40))
    ang = r.uniform(-4, 4, n)                               # unsorted, beyond +-pi
    rng = r.uniform(-5, 30, n) * RES                        # negative ranges point backwards
    rng[r.random(n) < 0.1] = 0.0                            # zero-length beams
    return H, W, pos, ang, rng


def test_random_scenes_each_line():
    """300 random scenes (grids 1..39 on a side, sensors up to 20 cells outside, unsorted angles, negative and zero
    ranges), every beam on its own and the scan as a whole."""
    r = np.random.default_rng(11)
    for _ in range(300):
        H, W, pos, ang, rng = _random_scene(r)
        want = _per_beam_grids(H, W, pos, ang, rng)
        for k in range(len(ang)):
            np.testing.assert_array_equal(ko.scan_to_grid(H, W, RES, pos, 0.0, ang[k:k + 1], rng[k:k + 1]),
                                          want[k])
        np.testing.assert_array_equal(ko.scan_to_grid(H, W, RES, pos, 0.0, ang, rng),
                                      want.max(axis=0) if len(ang) else np.full((H, W), -1))


def test_cfg4_scan_and_fixture():
    """The benchmark's cfg4 scan (4096 beams into 1000 x 1000 at 0.05 m) and the reference's fixture scan."""
    import synthetic as syn
    ang, rng = syn.dense_scan(4096, 4.0)
    np.testing.assert_array_equal(ko.scan_to_grid(1000, 1000, 0.05, (0, 0, 0), 0.0, ang, rng),
                                  mr.scan_to_grid(1000, 1000, 0.05, (0, 0, 0), 0.0, ang, rng))
    d = json.loads((GOLD / "laserscan_data.json").read_text())
    r = np.array(d["ranges"], np.float64)
    a = d["angle_min"] + np.arange(len(r)) * d["angle_increment"]
    for H, W, res, pos, orient in [(200, 200, 0.1, (0, 0, 0), 0.0), (151, 97, 0.05, (0.3, -0.45, 0), 0.7)]:
        want = mr.scan_to_grid(H, W, res, pos, orient, a, r)
        np.testing.assert_array_equal(ko.scan_to_grid(H, W, res, pos, orient, a, r), want)
        assert (want == 100).sum() > 0


# ---------------------------------------------------------------------------
# Bayesian scans: the last write in (beam, point) order wins
# ---------------------------------------------------------------------------
def _bayes_both(H, W, res, pos, orient, ang, rng, prev, walker=None, params=WALL):
    o = ko.BayesMapper(H, W, res, pos, orient, **params)
    o.set_previous(prev)
    got_g, got_p = o.scan_to_grid_baysian(ang, rng)
    want_g, want_p = mr.scan_to_grid_baysian(H, W, res, pos, orient, ang, rng, prev, params, walker)
    np.testing.assert_array_equal(got_g, want_g)
    np.testing.assert_array_equal(_bits(got_p), _bits(want_p))
    return want_g, want_p


def test_bayes_shared_and_recrossed_cells():
    """Beams along the same direction with different ranges (each later one re-crosses the cells of the earlier
    ones and ends in a cell they crossed), several beams ending in one cell, and a random previous grid: the
    probability of a cell is the one of the LAST beam that reaches it."""
    H, W = 41, 37
    r = np.random.default_rng(3)
    prev = r.uniform(0.05, 0.95, (H, W)).astype(np.float32)
    pos = mr.sensor_pos(H, W, RES, (20, 18))
    ang = np.array([0.3, 0.3, 0.3, 0.3, 1.2, 1.2 + 1e-4, 1.2 - 1e-4, -2.0, 0.3])
    rng = np.array([9.0, 4.0, 7.5, 2.0, 6.0, 6.0, 6.0, 30.0, 5.0])
    g, p = _bayes_both(H, W, RES, pos, 0.0, ang, rng, prev)
    # the order decides: the reversed scan gives different probabilities on the shared cells
    _, p_rev = mr.scan_to_grid_baysian(H, W, RES, pos, 0.0, ang[::-1], rng[::-1], prev, WALL)
    assert (_bits(p_rev) != _bits(p)).sum() > 3
    _bayes_both(H, W, RES, pos, 0.0, ang[::-1], rng[::-1], prev)


def test_bayes_random_scenes_and_cfg4():
    r = np.random.default_rng(5)
    for _ in range(120):
        H, W, pos, ang, rng = _random_scene(r)
        prev = r.uniform(0.05, 0.95, (H, W)).astype(np.float32)
        _bayes_both(H, W, RES, pos, 0.0, ang, rng, prev)
    import synthetic as syn
    ang, rng = syn.dense_scan(4096, 4.0)
    prev = r.uniform(0.2, 0.8, (1000, 1000)).astype(np.float32)
    _bayes_both(1000, 1000, 0.05, (0, 0, 0), 0.0, ang, rng, prev, params=BAYES)


def test_warp_restatement_matches_the_oracle():
    """The per-cell part of getPreviousGridInCurrentPose on the oracle's inverted matrix."""
    r = np.random.default_rng(9)
    for H, W, res, pose in [(200, 200, 0.05, ((0.03, -0.01), 0.004)), (151, 97, 0.1, ((-0.7, 0.2), -0.9))]:
        prev = r.uniform(0.05, 0.95, (H, W)).astype(np.float32)
        o = ko.BayesMapper(H, W, res, (0, 0, 0), 0.0, **BAYES)
        o.set_previous(prev)
        inv = o.warp_matrix(*pose)
        np.testing.assert_array_equal(_bits(o.get_previous_grid_in_current_pose(*pose)),
                                      _bits(mr.warp_previous(prev, inv, BAYES["p_prior"])))


# ---------------------------------------------------------------------------
# sensors far from the grid
# ---------------------------------------------------------------------------
native = pytest.mark.skipif(not mr.have_gxx(), reason="needs g++")


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    return mr.native_walker(mr.build_native(tmp_path_factory.mktemp("bresenham_literal")))


def _far_scans(H, W, dist):
    """Beams from sensors dist cells outside each side and corner into, to and across the grid."""
    for s in mr.border_and_outside_cells(H, W, dists=(dist,))[9:]:
        pos = mr.sensor_pos(H, W, RES, s)
        c = np.array([H / 2, W / 2]) - s
        base = np.arctan2(c[1], c[0])
        d = float(np.hypot(*c))
        ang = base + np.array([0.0, 3.0, -5.0, 11.0, -17.0, 0.5, 1.5, -0.7, 8.0]) / d
        rng = np.array([0.99, 1.01, 2.0, 0.99, 1.01, 2.0, 0.8, 1.2, 1.0]) * d * RES
        yield s, pos, ang, rng


def _check_far(dist, walker=None):
    H, W = 61, 47
    r = np.random.default_rng(dist)
    for s, pos, ang, rng in _far_scans(H, W, dist):
        want = _per_beam_grids(H, W, pos, ang, rng, walker)
        assert (want.max(axis=0) >= 0).sum() > 10, s     # the beams do cross the grid
        for k in range(len(ang)):
            np.testing.assert_array_equal(ko.scan_to_grid(H, W, RES, pos, 0.0, ang[k:k + 1], rng[k:k + 1]),
                                          want[k])
        np.testing.assert_array_equal(ko.scan_to_grid(H, W, RES, pos, 0.0, ang, rng), want.max(axis=0))
        _bayes_both(H, W, RES, pos, 0.0, ang, rng, r.uniform(0.05, 0.95, (H, W)).astype(np.float32), walker)


def test_sensors_64_cells_outside():
    """Sensors 64 cells outside each side and corner of an odd grid: the oracle starts the walk in closed form
    there, the restatement walks every step."""
    _check_far(64)


@native
def test_sensors_10_4_cells_outside(walker):
    _check_far(10_000, walker)


@native
def test_native_walker_equals_the_python_walk(walker):
    r = np.random.default_rng(2)
    for _ in range(40):
        H, W, pos, ang, rng = _random_scene(r)
        a = mr.emissions(H, W, RES, pos, 0.0, ang, rng)
        b = mr.emissions(H, W, RES, pos, 0.0, ang, rng, walker)
        for u, v in zip(a, b):
            np.testing.assert_array_equal(np.asarray(u), np.asarray(v))


@native
def test_lines_of_2_29_steps(walker):
    """One-beam scans from inside the grid to end cells 2^28 and 2^29 cells out and just below the 2^30 offset
    (beams of 10^6 m and more at slopes 0, 1/2, 1, 2/3 and an irrational one), each against the walk of every
    step."""
    H, W, res = 37, 29, 1.0
    pos = (0.25, -0.25, 0.0)
    far = 2.0 ** 28
    beams = [(np.pi, far), (np.arctan2(1, 2), far * np.sqrt(1.25)), (np.arctan2(-2, -3), far * np.sqrt(13 / 9)),
             (-np.pi / 4, far * np.sqrt(2)), (2.0, 1e6), (np.pi / 2, 2.0 ** 29), (0.0, 2.0 ** 30 - 64)]
    for a, rg in beams:
        t = mr.end_cell(H, W, res, pos, 0.0, a, rg)
        assert t is not None and max(abs(t[0]), abs(t[1])) > 5e5
        want = mr.scan_to_grid(H, W, res, pos, 0.0, [a], [rg], walker)
        np.testing.assert_array_equal(ko.scan_to_grid(H, W, res, pos, 0.0, [a], [rg]), want)
        assert (want == 0).sum() > 0


FAR = [46_340, 46_341, 2_000_000, 2 ** 25, 2 ** 30 - 1024]


def _crosses(H, W, s, t):
    """Whether the segment s -> t passes through the grid box (a margin of one cell)."""
    s, t = np.asarray(s, np.float64), np.asarray(t, np.float64)
    lo, hi = np.array([-1.0, -1.0]), np.array([H + 1.0, W + 1.0])
    d = t - s
    t0, t1 = 0.0, 1.0
    for k in range(2):
        if d[k] == 0:
            if not lo[k] <= s[k] <= hi[k]:
                return False
            continue
        a, b = sorted(((lo[k] - s[k]) / d[k], (hi[k] - s[k]) / d[k]))
        t0, t1 = max(t0, a), min(t1, b)
    return t0 <= t1


def far_scene(dist, side, H, W, res=1.0):
    """A sensor dist cells out on one side (or corner) and beams at the float32 angles around the direction of the
    grid's centre, with ranges short of, at and past the grid; four of the beams whose line crosses the grid are kept."""
    s = (H // 2 + side[0] * dist, W // 2 + side[1] * dist)
    pos = mr.sensor_pos(H, W, res, s)
    c = np.array([H / 2, W / 2]) - s
    base = np.float32(np.arctan2(c[1], c[0]))
    d = float(np.hypot(*c)) * res
    ang, rng = [], []
    for k in range(-6, 7):
        a = float(np.nextafter(base, np.float32(np.inf * np.sign(k))) if k else base)
        for _ in range(abs(k) - 1):
            a = float(np.nextafter(np.float32(a), np.float32(np.inf * np.sign(k))))
        for f in (1.1, 1.0, 2.0):
            t = mr.end_cell(H, W, res, pos, 0.0, a, d * f)
            if t is not None and _crosses(H, W, mr.start_cell(H, W, res, pos), t):
                ang.append(a)
                rng.append(d * f)
    keep = np.unique(np.linspace(0, len(ang) - 1, min(len(ang), 4)).round().astype(int))   # four, spread out
    return pos, np.array(ang)[keep], np.array(rng)[keep]


@native
@pytest.mark.parametrize("dist", FAR)
def test_far_sensor_plain_and_bayes(dist, walker):
    """Sensors 46 340 / 46 341 cells from the grid centre, 2 * 10^6 (where a double quotient for
    the closed-form state stops being exact), 2^25, and just below 2^30 (the largest sensor offset accepted):
    beams into and across the grid, plain and Bayesian, against the walk of every step."""
    H, W = (33, 45) if dist < 2 ** 25 else (301, 299)   # (a float32 angle step moves a line 2^30 out by ~100 cells)
    sides = ((-1, 0), (0, 1), (1, 1)) if dist < 2 ** 30 - 1024 else ((-1, 0),)
    for side in sides:
        pos, ang, rng = far_scene(dist, side, H, W)
        assert len(ang) >= 3
        prev = np.random.default_rng(dist).uniform(0.05, 0.95, (H, W)).astype(np.float32)
        want_g, _ = _bayes_both(H, W, 1.0, pos, 0.0, ang, rng, prev, walker)
        assert (want_g >= 0).sum() > 10
        np.testing.assert_array_equal(ko.scan_to_grid(H, W, 1.0, pos, 0.0, ang, rng), want_g)


def slope_half_scene():
    """A sensor 2^27 cells out whose beam lands on a line of |slope| exactly 1/2 (dx = 2 dy, found by a search over
    float32 angles, ranges and sensor positions) and crosses a 301 x 299 grid, plus two beams beside it.  On such a
    line e - 1 = n (i + 1) - 1: a double quotient (e - 1) / ddmaj rounds up to an integer on every other step once
    n i > 2^53, so the closed-form start needs the exact remainder test there (kc_mapper.hip, minor_after)."""
    H, W, pos = 301, 299, (-134217728.0, -67108864.0, 0.0)
    a, r = 0.46364760398864746, 150059952.0
    ang = np.array([a, a, float(np.nextafter(np.float32(a), np.float32(1)))])
    rng = np.array([r, float(np.nextafter(np.float32(r), np.float32(0))), r])
    return H, W, pos, ang, rng


def bayes_edge_scene(span):
    """A sensor whose farthest grid cell lies `span` cells away on both axes, beams into and across the grid: at
    span 2^15 - 1 the int square of the reference is exact (the kernel's narrow cell pass), at 2^15 the squared
    distance of the far corner is 2^31 and overflows an int (the wide pass)."""
    H, W = 33, 45
    s = (H - 1 - span, W - 1 - span)
    pos = mr.sensor_pos(H, W, 1.0, s)
    targets = [(H - 1, W - 1), (H - 1, 0), (0, W - 1), (H // 2, W // 2), (H + 3, W + 3), (H + 9, W - 5)]
    ang, rng, _ = mr.aim(H, W, 1.0, pos, targets)
    return H, W, pos, ang, rng


@native
def test_far_sensor_slope_half_line(walker):
    H, W, pos, ang, rng = slope_half_scene()
    s = mr.start_cell(H, W, 1.0, pos)
    t = mr.end_cell(H, W, 1.0, pos, 0.0, ang[0], rng[0])
    n, dmin = t[0] - s[0], t[1] - s[1]
    assert n == 2 * dmin and n > 2 ** 27 - 64
    # the steps that reach the grid: a double quotient is wrong on about half of them
    steps = range(-s[0] - 2, H - s[0] + 1)
    wrong = sum(1 for i in steps if np.floor(float(n * (i + 1) - 1) / float(2 * n)) != (n * (i + 1) - 1) // (2 * n))
    assert wrong > 50
    prev = np.random.default_rng(7).uniform(0.05, 0.95, (H, W)).astype(np.float32)
    want_g, _ = _bayes_both(H, W, 1.0, pos, 0.0, ang, rng, prev, walker)
    assert (want_g >= 0).sum() > 100
    np.testing.assert_array_equal(ko.scan_to_grid(H, W, 1.0, pos, 0.0, ang, rng), want_g)


@native
@pytest.mark.parametrize("span", [2 ** 15 - 1, 2 ** 15])
def test_bayes_distance_at_the_int_square_edge(span, walker):
    H, W, pos, ang, rng = bayes_edge_scene(span)
    prev = np.random.default_rng(span).uniform(0.05, 0.95, (H, W)).astype(np.float32)
    want_g, _ = _bayes_both(H, W, 1.0, pos, 0.0, ang, rng, prev, walker)
    assert want_g[H - 1, W - 1] >= 0          # the far corner is reached


def test_sensor_at_2_30_cells_is_refused():
    """A sensor whose offset position / resolution is not below 2^30 (the end cells' rule) is refused."""
    for p in [(2.0 ** 30, 0.0, 0.0), (0.0, -(2.0 ** 30), 0.0), (np.inf, 0, 0), (np.nan, 0, 0)]:
        with pytest.raises(ValueError):
            ko.scan_to_grid(10, 10, 1.0, p, 0.0, [0.0], [1.0])
        with pytest.raises(ValueError):
            ko.BayesMapper(10, 10, 1.0, p, 0.0, **BAYES)
        with pytest.raises(ValueError):
            mr.start_cell(10, 10, 1.0, p)
    below = (2.0 ** 30 - 128, 0.0, 0.0)
    assert ko.scan_to_grid(10, 10, 1.0, below, 0.0, [np.pi], [1.0]).min() == -1
