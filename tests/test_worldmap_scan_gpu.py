"""The world map's virtual laser scan on the device (kc_worldmap_scan, kc_dvz_deform_worldmap, kc_zone_check_worldmap;
DESIGN.md 4.11 rules 20 to 27) against the Python statement tests/worldmap_scan_ref.py: ranges and cells bit for bit.

The kernel walks in rounds of S = 8 steps (kWmScanS, kc_worldmap.hip): the rooms below put first hits on every step
index of the first rounds.  The main world is 37 x 29, neither side a multiple of 4 or 64."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import worldmap_ref as ref  # noqa: E402
import worldmap_scan_ref as sref  # noqa: E402

S = 8  # kWmScanS
RES, ORIGIN = 0.05, (-0.33, 1.7)
OCC, UNK, EMP = ref.OCCUPIED, ref.UNEXPLORED, ref.EMPTY


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def seeded_prior(w, h, seed, p_occ=0.08, p_unknown=0.2):
    rng = np.random.default_rng(seed)
    return rng.choice(np.int8([OCC, UNK, EMP]), size=(w, h), p=[p_occ, p_unknown, 1.0 - p_occ - p_unknown]).astype(np.int8)


def world(cls, res=RES, origin=ORIGIN):
    ctx = kh.WorldMapContext(cls.shape[0], cls.shape[1], res, origin)
    ctx.set_prior(cls)
    return ctx


def xy_of(cell_i, cell_j, res=RES, origin=ORIGIN):
    r = float(np.float32(res))
    return origin[0] + cell_i * r, origin[1] + cell_j * r


def range_of(rc, res=RES):
    """A range of rc - 1/2 cells: Rc = rc by rule 20's ceil."""
    return float(np.float32(res)) * (rc - 0.5)


def beams(n, start=-math.pi + 0.013):
    return start + np.arange(n) * (2 * math.pi / n)


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def check(ctx, cls, poses, angles, range_max, flags=0, res=RES, origin=ORIGIN):
    """poses: a list of (x, y, yaw); one pose goes the single way and the batch way"""
    want_r, want_c = sref.scan(cls, res, origin, poses, angles, range_max, flags)
    got_r, got_c = ctx.scan(poses, angles, range_max, flags=flags, return_cells=True)
    assert same(got_r, want_r), (poses, range_max, flags, np.argwhere(got_r != want_r)[:5])
    assert same(got_c, want_c), (poses, range_max, flags, np.argwhere(got_c != want_c)[:5])
    assert same(ctx.scan(poses, angles, range_max, flags=flags), want_r)     # without the cells
    if len(poses) == 1:
        r1, c1 = ctx.scan(poses[0], angles, range_max, flags=flags, return_cells=True)
        assert same(r1, want_r[0]) and same(c1, want_c[0])
    return want_r, want_c


@pytest.fixture(scope="module")
def small():
    cls = seeded_prior(37, 29, 11)
    assert {OCC, UNK, EMP} == set(np.unique(cls).tolist())
    with world(cls) as ctx:
        yield ctx, cls


ORIGINS = [(18, 14),                                                          # the middle
           (0, 14), (36, 14), (18, 0), (18, 28),                              # the four edges
           (0, 0), (36, 0), (0, 28), (36, 28),                                # the four corners
           (-1, 14), (37, 14), (18, -1), (18, 29),                            # one cell outside each edge
           (12.37, 9.81), (36.49, 28.49), (17.5, 13.5),                       # fractions of a cell, a cell corner
           (-200, 14), (18, 400), (5000, -5000)]                              # far outside


@pytest.mark.parametrize("rc", [1, 5, 64])
@pytest.mark.parametrize("flags", [0, kh.SCAN_UNKNOWN_BLOCKS])
def test_small_world(small, rc, flags):
    ctx, cls = small
    ang = beams(40)
    hits = 0
    for k, cell in enumerate(ORIGINS):
        x, y = xy_of(*cell)
        assert sref.scan_check(RES, 1, len(ang), range_of(rc), flags) == rc
        _, c = check(ctx, cls, [(x, y, 0.37 * k)], ang, range_of(rc), flags)
        hits += int((c >= 0).sum())
    assert hits > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_beam_counts(small, n):
    ctx, cls = small
    check(ctx, cls, [(*xy_of(12.37, 9.81), 0.4)], beams(n), range_of(9))


@pytest.mark.parametrize("m", [1, 2, 5])
def test_batches_of_poses(small, m):
    ctx, cls = small
    empty = np.argwhere(cls == EMP)[::97][:m]                              # starts inside empty cells, apart
    poses = [(*xy_of(i + 0.2, j - 0.3), -2.0 + 1.1 * p) for p, (i, j) in enumerate(empty)]
    want, _ = check(ctx, cls, poses, beams(70), range_of(12), kh.SCAN_UNKNOWN_BLOCKS)
    if m > 1:
        assert not same(want[0], want[1]), "the poses must be told apart"


def test_rooms_put_first_hits_on_every_step_of_the_rounds():
    """A square room of half-side h around the origin: an axis-aligned beam's first hit is its step h, a diagonal one's
    its step 2 h - 1 or 2 h; h = 1 .. 20 covers every step index of rounds 0 to 2 and more."""
    ang = np.concatenate([beams(56), [0.0, math.pi / 2, math.pi, -math.pi / 2, math.pi / 4, -3 * math.pi / 4]])
    seen = set()
    cls = np.full((45, 45), EMP, np.int8)
    with world(cls) as ctx:
        for h in range(1, 21):
            cls[:] = EMP
            cls[22 - h:22 + h + 1, [22 - h, 22 + h]] = OCC
            cls[[22 - h, 22 + h], 22 - h:22 + h + 1] = OCC
            ctx.set_prior(cls)
            for pose in [(*xy_of(22, 22), 0.0), (*xy_of(22.3, 21.8), 0.21)]:
                r, c = check(ctx, cls, [pose], ang, range_of(40))
                assert (c >= 0).all()
                if pose[2] == 0.0:                                         # the beam along +x ends on its step h
                    assert c[0, 56] == (22 + h) + 22 * 45
            seen.add(h - 1)                                                # that step's 0-based index
    assert set(range(2 * S)) <= seen


def test_empty_map_gives_range_max_everywhere():
    cls = np.full((37, 29), EMP, np.int8)
    with world(cls) as ctx:
        r, c = check(ctx, cls, [(*xy_of(18, 14), 0.3)], beams(100), 1.3)
        assert (r == float(np.float32(1.3))).all() and (c == -1).all()
        # a never-observed map blocks at once under the flag, and nowhere without it
        ctx.clear()
        unknown = np.full((37, 29), UNK, np.int8)
        r, c = check(ctx, unknown, [(*xy_of(18, 14), 0.3)], beams(100), 1.3, kh.SCAN_UNKNOWN_BLOCKS)
        assert (r == 0.0).all() and (c == 18 + 14 * 37).all()
        r, c = check(ctx, unknown, [(*xy_of(18, 14), 0.3)], beams(100), 1.3)
        assert (c == -1).all()


def test_long_walks_over_a_large_sparse_world():
    rng = np.random.default_rng(4)
    cls = np.full((1500, 1100), EMP, np.int8)
    cls[rng.integers(0, 1500, 300), rng.integers(0, 1100, 300)] = OCC
    cls[rng.integers(0, 1500, 300), rng.integers(0, 1100, 300)] = UNK
    cls[740:760, 540:560] = EMP
    with world(cls) as ctx:
        assert sref.scan_check(RES, 1, 360, range_of(700), 0) == 700
        r, c = check(ctx, cls, [(*xy_of(750.2, 549.7), 1.0)], beams(360), range_of(700))
        steps = np.abs(c[c >= 0] % 1500 - 750) + np.abs(c[c >= 0] // 1500 - 550)
        assert (c >= 0).sum() > 20 and (c < 0).sum() > 20 and steps.max() > 40 * S


def test_a_scan_after_an_update_sees_the_new_wall():
    W = H = 60
    origin = (-(W // 2 - 1) * float(np.float32(RES)),) * 2
    want = ref.WorldMapRef(W, H, RES, origin)
    grid = np.full((W, H), EMP, np.int32)
    with kh.WorldMapContext(W, H, RES, origin) as ctx:
        ang = beams(90)
        assert ctx.update(grid, (0.0, 0.0, 0.0)) == want.update(grid, (0.0, 0.0, 0.0))
        before, _ = check(ctx, want.cls, [(0.0, 0.0, 0.2)], ang, 1.2, origin=origin)
        assert (before == float(np.float32(1.2))).all()
        grid[40, 10:50] = OCC                                              # a wall 11 cells ahead
        assert ctx.update(grid, (0.0, 0.0, 0.0)) == want.update(grid, (0.0, 0.0, 0.0))
        after, c = check(ctx, want.cls, [(0.0, 0.0, 0.2)], ang, 1.2, origin=origin)
        assert (c >= 0).sum() > 10 and (c[c >= 0] % W == 40).all()


def test_the_angle_table_is_kept_and_replaced(small):
    ctx, cls = small
    ang = beams(130)
    pose = [(*xy_of(18.4, 14.2), 0.9)]
    first, _ = check(ctx, cls, pose, ang, range_of(20))
    again, _ = check(ctx, cls, pose, ang.copy(), range_of(20))             # the same bytes at another address
    assert same(first, again)
    ang2 = ang.copy()
    ang2[77] += 0.5
    changed, _ = check(ctx, cls, pose, ang2, range_of(20))
    assert not same(changed, first) and same(np.delete(changed, 77, 1), np.delete(first, 77, 1))
    check(ctx, cls, pose, ang2[:64], range_of(20))                         # a prefix: another length
    check(ctx, cls, pose, ang, range_of(20))


def test_every_refusal_is_followed_by_a_right_call(small):
    ctx, cls = small
    ang = beams(33)
    pose = (*xy_of(18, 14), 0.0)

    def ok():
        check(ctx, cls, [pose], ang, range_of(9))

    ok()
    bad_calls = [
        (ValueError, lambda: ctx.scan(pose, ang, 0.0)),
        (ValueError, lambda: ctx.scan(pose, ang, float("nan"))),
        (ValueError, lambda: ctx.scan(pose, ang, float("inf"))),
        (IndexError, lambda: ctx.scan(pose, ang, 103.0)),
        (ValueError, lambda: ctx.scan(pose, ang, 1.0, flags=2)),
        (ValueError, lambda: ctx.scan(pose, [], 1.0)),
        (ValueError, lambda: ctx.scan([], ang, 1.0)),
        (IndexError, lambda: ctx.scan(pose, np.zeros(65537), 1.0)),
        (IndexError, lambda: ctx.scan([pose] * 65, np.zeros(65536), 1.0)),
        (ValueError, lambda: ctx.scan(pose, [0.0, float("nan")], 1.0)),
        (ValueError, lambda: ctx.scan(pose, [float("inf")], 1.0)),
        (IndexError, lambda: ctx.scan((1e6, 0.0, 0.0), ang, 1.0)),
        (ValueError, lambda: ctx.scan(kh.WorldMapPose(70000, 0, 0, 0), ang, 1.0)),
        (ValueError, lambda: ctx.scan([pose, kh.WorldMapPose(0, -70000, 0, 0)], ang, 1.0)),
    ]
    for exc, call in bad_calls:
        with pytest.raises(exc):
            call()
        ok()


# ---- the DVZ on the map's scan ---------------------------------------------------------------------------------------
ZONE = (1.2, 0.8, 0.1, -0.05, 0.3)   # major, minor, centre shift x, y, orientation shift


@pytest.mark.parametrize("n", [1, 64, 65, 1440])
def test_dvz_deform_on_the_map_scan(small, n):
    ctx, cls = small
    ang = beams(n, start=0.0)
    i, j = np.argwhere(cls == EMP)[400]                                    # a start inside an empty cell
    pose = (*xy_of(i + 0.1, j - 0.4), 0.45)
    rmax = range_of(30)
    rng = np.random.default_rng(n)
    with kh.DvzContext(max_beams=1440) as dvz:
        for flags in (0, kh.SCAN_UNKNOWN_BLOCKS):
            for real in (None, np.where(rng.random(n) < 0.5, rng.uniform(0.05, 2.0, n), np.inf)):
                want_r, _ = sref.scan(cls, RES, ORIGIN, [pose], ang, rmax, flags, real)
                want = dvz.deform(ZONE, ang, want_r[0], radii=True)
                got = dvz.deform_worldmap(ZONE, ctx, pose, ang, rmax, real=real, radii=True, flags=flags)
                assert same(got[3], want_r[0])
                assert np.float64(got[:2]).tobytes() == np.float64(want[:2]).tobytes() and got[2] == want[2]
                assert same(got[4], want[3])
                again = dvz.deform_worldmap(ZONE, ctx, pose, ang, rmax, real=real, flags=flags)
                assert np.float64(got[:3]).tobytes() == np.float64(again[:3]).tobytes()
        if n > 1:
            assert want[2] > 0 and math.isfinite(want[0]), "some beam must deform the zone, none from inside a cell"


def test_dvz_refusals_leave_the_context_right(small):
    ctx, cls = small
    ang, pose, rmax = beams(65), (*xy_of(17.6, 13.1), 0.45), range_of(30)
    with kh.DvzContext(max_beams=100) as dvz:
        want = dvz.deform(ZONE, ang, sref.scan(cls, RES, ORIGIN, [pose], ang, rmax)[0][0])

        def ok():
            assert dvz.deform_worldmap(ZONE, ctx, pose, ang, rmax)[:3] == want

        ok()
        for exc, call in [
            (IndexError, lambda: dvz.deform_worldmap(ZONE, ctx, pose, beams(101), rmax)),
            (ValueError, lambda: dvz.deform_worldmap(ZONE, ctx, pose, [], rmax)),
            (ValueError, lambda: dvz.deform_worldmap((1.2, -0.8, 0, 0, 0), ctx, pose, ang, rmax)),
            (ValueError, lambda: dvz.deform_worldmap(ZONE, ctx, pose, ang, -1.0)),
            (IndexError, lambda: dvz.deform_worldmap(ZONE, ctx, pose, ang, 500.0)),
            (ValueError, lambda: dvz.deform_worldmap(ZONE, ctx, pose, ang, rmax, flags=4)),
            (ValueError, lambda: dvz.deform_worldmap(ZONE, ctx, pose, np.full(65, np.nan), rmax)),
            (IndexError, lambda: dvz.deform_worldmap(ZONE, ctx, (1e6, 0.0, 0.0), ang, rmax)),
        ]:
            with pytest.raises(exc):
                call()
            ok()


# ---- the critical zone checker on the map's scan ---------------------------------------------------------------------
SHAPES = [(kh.CYLINDER, [0.2, 0.4]), (kh.BOX, [0.3, 0.25, 0.2]), (kh.SPHERE, [0.2])]


def zone_world(ahead, behind):
    """80 x 80 cells of 0.05 m, the scan frame at cell (40, 40) looking along +x: walls `ahead` and `behind` cells away
    (None: no wall)"""
    cls = np.full((80, 80), EMP, np.int8)
    if ahead is not None:
        cls[40 + ahead, 20:60] = OCC
    if behind is not None:
        cls[40 - behind, 20:60] = OCC
    return cls


@pytest.mark.parametrize("shape,dims", SHAPES)
def test_zone_check_on_the_map_scan(shape, dims):
    ang = beams(180, start=0.0)
    origin = (0.0, 0.0)
    pose = (*xy_of(40, 40, origin=origin), 0.0)
    seen = set()
    with kh.ZoneContext(shape, dims, [0.05, 0.0, 0.1], [0, 0, 0, 1], 160.0, 0.3, 1.0, ang, 0.0, 2.0, 3.0) as zone:
        assert len(zone.indices(True)) > 0 and len(zone.indices(False)) > 0
        cls = zone_world(None, None)
        with world(cls, origin=origin) as ctx:
            for ahead, behind in [(8, None), (16, 38), (38, 16), (None, 9), (None, None), (30, 30)]:
                cls = zone_world(ahead, behind)
                ctx.set_prior(cls)
                for real in (None, np.where(np.arange(180) % 3 == 0, 0.7, np.inf)):
                    want_r, _ = sref.scan(cls, RES, origin, [pose], ang, 3.0, 0, real)
                    for forward in (True, False):
                        want = zone.check(want_r[0], forward)
                        got = zone.check_worldmap(ctx, pose, forward, real=real)
                        assert np.float32(got).tobytes() == np.float32(want).tobytes(), (ahead, behind, forward, got, want)
                        assert got == zone.check_worldmap(ctx, pose, forward, real=real)
                        if real is None:
                            seen.add(0 if got == 0.0 else 2 if got == 1.0 else 1)
            # refusals, each followed by a right call
            for exc, call in [(ValueError, lambda: zone.check_worldmap(ctx, pose, True, flags=2)),
                              (IndexError, lambda: zone.check_worldmap(ctx, (1e6, 0.0, 0.0), True)),
                              (ValueError, lambda: zone.check_worldmap(ctx, kh.WorldMapPose(0, 70000, 0, 0), True))]:
                with pytest.raises(exc):
                    call()
                assert zone.check_worldmap(ctx, pose, True) == zone.check(sref.scan(cls, RES, origin, [pose], ang, 3.0)[0][0], True)
    assert seen == {0, 1, 2}, "factors 0, strictly between 0 and 1, and 1"


def test_contexts_take_turns_on_one_map():
    """A mapper feeds the map; the map's own scan, a DVZ context and a zone checker then read it, each twice in a row,
    and again after the next update."""
    n = 360
    ang = -math.pi + np.arange(n) * (2 * math.pi / n)
    r = float(np.float32(RES))
    c0, c1 = ref.central(200, 200)
    origin = (-c0 * r, -c1 * r)
    scans = [np.full(n, 3.0), np.full(n, 3.0)]
    scans[0][(ang > -0.3) & (ang < 0.3)] = 0.9
    scans[1][(ang > 1.2) & (ang < 1.9)] = 0.6
    pose = (0.1, -0.05, 0.2)
    sang = beams(120, start=0.0)
    m = kh.MapperContext(200, 200, RES, (0, 0, 0), 0.0, n)
    with kh.WorldMapContext(200, 200, RES, origin) as wm, kh.DvzContext(max_beams=128) as dvz, \
            kh.ZoneContext(kh.CYLINDER, [0.2, 0.4], [0, 0, 0], [0, 0, 0, 1], 160.0, 0.3, 1.0, sang, 0.0, 2.0, 2.5) as zone:
        want = ref.WorldMapRef(200, 200, RES, origin)
        seen = []
        for ranges in scans:
            g = m.scan_to_grid(ang, ranges).copy()
            for _ in range(2):
                m.scan_to_grid_device(ang, ranges)
                assert wm.update_from_mapper(m, (0.0, 0.0, 0.0)) == want.update(g, (0.0, 0.0, 0.0))
            want_r, want_c = sref.scan(want.cls, RES, origin, [pose], sang, 2.5)
            for _ in range(2):
                got_r, got_c = wm.scan(pose, sang, 2.5, return_cells=True)
                assert same(got_r, want_r[0]) and same(got_c, want_c[0])
            want_d = dvz.deform(ZONE, sang, want_r[0])
            for _ in range(2):
                assert dvz.deform_worldmap(ZONE, wm, pose, sang, 2.5)[:3] == want_d
            for forward in (True, False, True, False):
                assert zone.check_worldmap(wm, pose, forward) == zone.check(want_r[0], forward)
            seen.append(want_r[0])
        assert not same(seen[0], seen[1])


@pytest.mark.skipif(kh.device_count() < 2, reason="needs a second device")
def test_map_on_another_device_is_refused():
    ang = beams(16)
    with kh.WorldMapContext(64, 48, RES, (-1.0, -1.0), device=1) as wm, kh.DvzContext(max_beams=16) as dvz, \
            kh.ZoneContext(kh.SPHERE, [0.2], [0, 0, 0], [0, 0, 0, 1], 160.0, 0.3, 1.0, ang, 0.0, 2.0, 2.5) as zone:
        with pytest.raises(ValueError, match="device"):
            dvz.deform_worldmap(ZONE, wm, (0.0, 0.0, 0.0), ang, 2.0)
        with pytest.raises(ValueError, match="device"):
            zone.check_worldmap(wm, (0.0, 0.0, 0.0), True)
