"""The correlative match on the device (kc_worldmap_match_*, DESIGN.md 4.11 rules 9 to 15) against
tests/worldmap_match_ref.py: the whole score table, the record and the corrected pose, bit for bit.

The shapes are the smallest at which each mechanism can still go wrong: a 9 x 7 local grid (a gh / gw or c0 / c1 mix-up
shows) over a 37 x 29 world with guesses inside, on every edge and outside; worlds of a few cells under a 64 x 64 local
grid (every weight next to an edge, the scratch plane mostly outside the map); the window of one candidate and the
largest one (16 candidates a lane, the tie key at its limits); 4096 points (16 chunks a rotation: the atomic merge)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import synthetic as syn  # noqa: E402
import worldmap_match_ref as mref  # noqa: E402
import worldmap_ref as ref  # noqa: E402

from helpers import DeviceArray  # noqa: E402
from test_worldmap_gpu import ORIGIN, POSES_IN, POSES_OUT, RES, YAWS, _fetch, local_grid, world_xy  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def seeded(w, h, seed, p_occ=0.15, res=RES, origin=ORIGIN):
    """A context and its reference after the same random prior: about p_occ occupied, some unexplored."""
    rng = np.random.default_rng(seed)
    prior = rng.choice(np.int8([100, 0, -1]), size=(w, h), p=[p_occ, 0.7, 0.3 - p_occ]).astype(np.int8)
    ctx, want = kh.WorldMapContext(w, h, res, origin), ref.WorldMapRef(w, h, res, origin)
    ctx.set_prior(prior)
    want.set_prior(prior)
    return ctx, want


def check(ctx, want, grid, pose, K, step, S, central=None, match=None):
    """One match on both sides: the record, the corrected pose and the whole table must be the reference's."""
    exp, table, _ = mref.match_pose(want, grid, pose, K, step, S, central)
    got = (match or ctx.match)(grid, pose, n_yaw=K, yaw_step=step, reach=S, **({} if central is None else dict(central=central)))
    np.testing.assert_array_equal(ctx.match_scores(K, S), table)
    assert got == exp._asdict(), (pose, got, exp)
    return exp


@pytest.mark.parametrize("yaw", YAWS)
def test_poses_on_the_small_world(yaw):
    ctx, want = seeded(37, 29, 11)
    assert 100 < (want.cls == 100).sum() < 220 and (want.cls == -1).sum() > 50
    with ctx:
        scores = 0
        for k, cell in enumerate(POSES_IN):
            m = check(ctx, want, local_grid(9, 7, 100 + k), world_xy(*cell) + (yaw,), 2, 0.05, 3)
            assert m.points > 5
            scores += m.score
        assert scores > 50
        for cell in POSES_OUT:                          # every point off the map: all zero, the guess wins
            m = check(ctx, want, local_grid(9, 7, 7), world_xy(*cell) + (yaw,), 2, 0.05, 3)
            assert (m.k, m.u, m.v, m.score) == (0, 0, 0, 0) and m.points > 5
        # the central cell anywhere, also outside the grid
        check(ctx, want, local_grid(9, 7, 8), world_xy(18, 14) + (yaw,), 2, 0.05, 3, central=(0, 6))
        check(ctx, want, local_grid(9, 7, 9), world_xy(18, 14) + (yaw,), 2, 0.05, 3, central=(-6, 12))


@pytest.mark.parametrize("shape", [(5, 3), (63, 2), (1, 1)])
def test_tiny_worlds_under_a_large_local_grid(shape):
    ctx, want = seeded(*shape, seed=21, p_occ=0.25)
    if shape == (1, 1):
        ctx.set_prior(np.full((1, 1), 100, np.int8))
        want.set_prior(np.full((1, 1), 100, np.int8))
    assert (want.cls == 100).any()
    with ctx:
        for k, yaw in enumerate(YAWS):
            cell = (shape[0] / 2 + 0.3 * k, shape[1] / 2 - 0.45 * k)
            m = check(ctx, want, local_grid(64, 64, 200 + k), world_xy(*cell) + (yaw,), 1, 0.02, 4)
            assert m.points > 900 and m.score > 0


def test_single_candidate():
    ctx, want = seeded(37, 29, 12)
    with ctx:
        for step in (0.0, 123.0):                       # yaw_step is not used
            m = check(ctx, want, local_grid(9, 7, 31), world_xy(12.37, 9.81) + (0.3,), 0, step, 0)
            assert ctx.match_scores(0, 0).shape == (1, 1, 1) and m.score == m.score_guess > 0


def test_largest_window():
    rng = np.random.default_rng(41)
    g = rng.choice(np.int32([100, 0, -1]), size=(16, 16), p=[0.1, 0.6, 0.3]).astype(np.int32)
    ctx, want = seeded(90, 80, 13)
    with ctx:
        m = check(ctx, want, g, world_xy(44.3, 41.8) + (0.7,), 31, math.radians(1.5), 31)
        assert ctx.match_scores(31, 31).size == 250047 and 15 < m.points < 40
        # the tie key at its limits: no points, so every candidate ties at 0 and the smallest tuple is the guess
        m = check(ctx, want, np.zeros((16, 16), np.int32), world_xy(44.3, 41.8) + (0.7,), 31, math.radians(1.5), 31)
        assert (m.k, m.u, m.v, m.score, m.points) == (0, 0, 0, 0, 0)
    # one occupied cell far out in the corner of the window and of the yaw range: the largest tie fields do win
    ctx, want = kh.WorldMapContext(90, 80, RES, ORIGIN), ref.WorldMapRef(90, 80, RES, ORIGIN)
    prior = np.zeros((90, 80), np.int8)
    prior[44 + 31, 41 + 31] = 100
    ctx.set_prior(prior)
    want.set_prior(prior)
    one = np.zeros((16, 16), np.int32)
    one[ref.central(16, 16)] = 100                      # the point (0, 0): every rotation lands it on the guess's cell
    with ctx:
        m = check(ctx, want, one, world_xy(44.0, 41.0) + (0.7,), 31, 0.01, 31)
        assert (m.k, m.u, m.v, m.score, m.score_guess) == (0, 31, 31, 3, 0)


def test_multiple_chunks_and_a_table_zeroed_again():
    ctx, want = seeded(37, 29, 14)
    g = np.full((64, 64), 100, np.int32)
    with ctx:
        m = check(ctx, want, g, world_xy(18.4, 14.2) + (0.3,), 1, 0.04, 2)
        assert m.points == 4096 and m.score > 300
        first = ctx.match_scores(1, 2)
        assert ctx.match(g, world_xy(18.4, 14.2) + (0.3,), n_yaw=1, yaw_step=0.04, reach=2) == m._asdict()
        np.testing.assert_array_equal(ctx.match_scores(1, 2), first)   # not added onto the first match's sums
        check(ctx, want, local_grid(9, 7, 3), world_xy(18.4, 14.2) + (0.3,), 1, 0.04, 2)   # nor is a smaller one after it
        with pytest.raises(IndexError):
            ctx.match_scores(0, 2)                      # fewer words than the last match's table


def test_no_points_and_an_empty_map():
    ctx, want = seeded(37, 29, 15)
    with ctx:
        g = local_grid(9, 7, 5)
        g[g == 100] = 50
        m = check(ctx, want, g, world_xy(18, 14) + (0.3,), 2, 0.05, 3)
        assert (m.k, m.u, m.v, m.score, m.score_guess, m.points) == (0, 0, 0, 0, 0, 0)
        ctx.clear()
        want.clear()
        m = check(ctx, want, local_grid(9, 7, 5), world_xy(18, 14) + (0.3,), 2, 0.05, 3)
        assert (m.k, m.u, m.v, m.score, m.score_guess) == (0, 0, 0, 0, 0) and m.points > 5
    fresh = kh.WorldMapContext(5, 5, RES, ORIGIN)
    with fresh:
        with pytest.raises(kh.KompassHipError):
            fresh.match_scores(0, 0)                    # no match yet


def test_yaw_tie_goes_to_the_smallest_turn():
    ctx, want = kh.WorldMapContext(37, 29, RES, ORIGIN), ref.WorldMapRef(37, 29, RES, ORIGIN)
    prior = np.zeros((37, 29), np.int8)
    prior[20, 15] = 100
    ctx.set_prior(prior)
    want.set_prior(prior)
    g = np.zeros((9, 7), np.int32)
    g[ref.central(9, 7)[0] + 1, ref.central(9, 7)[1]] = 100      # the point (1, 0): a small turn leaves its cell alone
    with ctx:
        m = check(ctx, want, g, world_xy(18, 14) + (0.0,), 2, 0.01, 3)
        assert (m.k, m.u, m.v, m.score) == (0, 1, 1, 3)
        t = ctx.match_scores(2, 3)
        assert (t[:, 3 + 1, 3 + 1] == 3).all()                    # the peak is tied across all five yaws


def test_same_grid_three_routes():
    gh, gw, res = 40, 40, np.float32(0.1)
    ang, rng = syn.dense_scan(360, 0.25)
    ctx, want = seeded(37, 29, 16, res=res)
    with ctx, kh.MapperContext(gh, gw, res, (0, 0, 0), 0.0, 360) as mapper:
        pose = world_xy(15.2, 12.7) + (0.3,)
        mapper.scan_to_grid_device(ang, rng)
        a = ctx.match_from_mapper(mapper, pose, n_yaw=2, yaw_step=0.02, reach=3)   # no mapper.sync(): the event orders it
        ta = ctx.match_scores(2, 3)
        g = _fetch(mapper, gh, gw)
        assert (g == 100).sum() > 20
        b = ctx.match_device(mapper.grid_device_ptr(), gh, gw, pose, n_yaw=2, yaw_step=0.02, reach=3)
        tb = ctx.match_scores(2, 3)
        exp = check(ctx, want, g, pose, 2, 0.02, 3)
        assert a == b == exp._asdict() and exp.points == (g == 100).sum()
        np.testing.assert_array_equal(ta, tb)
        np.testing.assert_array_equal(ta, ctx.match_scores(2, 3))
        # the refusals of the update's device route are the match's
        flat = np.asfortranarray(g).ravel(order="F")
        with DeviceArray(np.concatenate([flat, flat])) as dev:
            assert ctx.match_device(dev.ptr + flat.nbytes, gh, gw, pose, n_yaw=2, yaw_step=0.02, reach=3) == a   # to the allocation's end
            with pytest.raises(ValueError, match="outside"):
                ctx.match_device(dev.ptr + flat.nbytes + 4, gh, gw, pose, reach=1)
            with pytest.raises(ValueError, match="aligned"):
                ctx.match_device(dev.ptr + 2, gh, gw, pose, reach=1)
            with pytest.raises(ValueError, match="resolution"):
                ctx.match_device(dev.ptr, gh, gw, pose, reach=1, resolution=0.05)
        with pytest.raises(ValueError):
            ctx.match_device(g.ctypes.data, gh, gw, pose, reach=1)               # host memory
        with pytest.raises(ValueError):
            ctx.match(g, pose, n_yaw=32, yaw_step=0.1, reach=1)
        with pytest.raises(ValueError):
            ctx.match(g, pose, n_yaw=1, yaw_step=0.1, reach=32)
        with pytest.raises(ValueError, match="unit vector"):
            ctx.match(g, ctx.quantise_pose(*pose), reach=1, rotations=[(65536, 65536)])
        with kh.MapperContext(gh, gw, 0.05, (0, 0, 0), 0.0, 360) as fine:
            fine.scan_to_grid_device(ang, rng)
            with pytest.raises(ValueError, match="resolution"):
                ctx.match_from_mapper(fine, pose, reach=1)


def test_match_leaves_the_map_alone():
    ctx, want = seeded(37, 29, 17)
    with ctx:
        cls0, ev0 = ctx.planes()
        check(ctx, want, local_grid(9, 7, 6), world_xy(18, 14) + (0.3,), 2, 0.05, 3)
        check(ctx, want, np.full((64, 64), 100, np.int32), world_xy(18, 14) + (-2.5,), 1, 0.05, 5)
        cls1, ev1 = ctx.planes()
        np.testing.assert_array_equal(cls0, cls1)
        np.testing.assert_array_equal(ev0, ev1)
        np.testing.assert_array_equal(cls1, want.cls)
        # and an update after a match is the update it always was
        g = local_grid(9, 7, 6)
        assert ctx.update(g, world_xy(18, 14) + (0.3,)) == want.update(g, world_xy(18, 14) + (0.3,))
        np.testing.assert_array_equal(ctx.planes()[1], want.evidence)


def _recovery():
    world = mref.recovery_world()
    prior = np.where(world.cls == 100, 100, np.where(world.cls == 0, 0, -1)).astype(np.int8)
    return world, prior


def test_the_recovery_scene_on_the_device():
    world, prior = _recovery()
    ctx = kh.WorldMapContext(120, 90, 0.05, (0.0, 0.0))
    ctx.set_prior(prior)
    with ctx:
        np.testing.assert_array_equal(ctx.planes()[0], world.cls)
        for true, guess, off in mref.recovery_draws(3):
            local = mref.gather(world, true, 61, 61, (30, 30))
            m = check(ctx, world, local, guess, 4, math.radians(1.0), 5, central=(30, 30))
            assert (m.k, m.u, m.v) == off


def test_front_end_matches_and_updates_at_the_corrected_pose():
    from kompass_core.mapping import WorldMap
    from kompass_core.models import RobotState

    world, prior = _recovery()
    step = math.radians(1.0)
    true, guess, off = mref.recovery_draws(1)[0]
    # the front end takes the mapper's central cell: a 62 x 62 grid has it at (30, 30)
    assert ref.central(62, 62) == (30, 30)
    local = mref.gather(world, true, 62, 62)
    state = RobotState(x=guess[0], y=guess[1], yaw=guess[2])
    exp, table, pose = mref.match_pose(world, local, guess, 4, step, 5)
    assert (exp.k, exp.u, exp.v) == off and exp.score > exp.score_guess and exp.points >= 30

    def fresh():
        wm, want = WorldMap(120, 90, 0.05, (0.0, 0.0)), ref.WorldMapRef(120, 90, 0.05, (0.0, 0.0))
        wm.set_prior(prior)
        want.set_prior(prior)
        return wm, want

    def same(wm, want):
        np.testing.assert_array_equal(wm.occupancy, want.cls)
        np.testing.assert_array_equal(wm.evidence, want.evidence)

    wm, want = fresh()
    m = wm.match(state, local, n_yaw=4, yaw_step=step, reach=5)
    assert (m.k, m.u, m.v, m.score, m.score_guess, m.points, m.pose) == tuple(exp)
    assert (m.x, m.y, m.yaw) == pose and m.ratio == exp.score / (3.0 * exp.points) and m.applied is None
    np.testing.assert_array_equal(m.scores(), table)
    same(wm, want)                                                      # a match changes nothing
    assert wm.last_match is None
    # trusted: fused at the corrected pose
    n = wm.update(state, local, match=True, n_yaw=4, yaw_step=step, reach=5)
    assert (n, wm.changed_box) == want.update(local, exp.pose)
    assert wm.last_match.applied is True and (wm.last_match.k, wm.last_match.u, wm.last_match.v) == off
    same(wm, want)
    with pytest.raises(RuntimeError):
        m.scores()                                                      # the map's table is the later match's now
    # not trusted: fused at the given pose
    wm, want = fresh()
    n = wm.update(state, local, match=True, min_ratio=2.0, n_yaw=4, yaw_step=step, reach=5)
    assert (n, wm.changed_box) == want.update(local, guess)
    assert wm.last_match.applied is False and (wm.last_match.k, wm.last_match.u, wm.last_match.v) == off
    same(wm, want)
    # more points asked for than there are
    wm, want = fresh()
    wm.update(state, local, match=True, min_points=exp.points + 1, n_yaw=4, yaw_step=step, reach=5)
    want.update(local, guess)
    assert wm.last_match.applied is False
    same(wm, want)
    # without match: today's call and today's result
    wm, want = fresh()
    n = wm.update(state, local)
    assert (n, wm.changed_box) == want.update(local, guess) and wm.last_match is None
    same(wm, want)
    with pytest.raises(TypeError):
        wm.update(state, local, reach=5)
    with pytest.raises(ValueError):
        wm.match(state, local, n_yaw=32)
    # the default window runs too
    d = wm.match(state, local)
    assert d.scores().shape == (21, 21, 21) and d.points == exp.points


def test_front_end_matches_the_mappers_grid_where_it_lies():
    from kompass_core.datatypes.laserscan import LaserScanData
    from kompass_core.mapping import LocalMapper, MapConfig, WorldMap
    from kompass_core.models import RobotState
    from test_worldmap_gpu import _room_scan

    res, origin = 0.05, (-1.0, -1.0)
    wm, want = WorldMap(160, 120, res, origin), ref.WorldMapRef(160, 120, res, origin)
    lm = LocalMapper(MapConfig(width=4.0, height=4.0, resolution=res))
    for k in range(4):
        x, y, yaw = 1.5 + 1.0 * k, 2.0 + 0.1 * k, 0.2 * k - 0.3
        ang, rng = _room_scan(x, y, yaw, None)
        lm.update_from_scan(RobotState(x=x, y=y, yaw=yaw), LaserScanData(angles=ang, ranges=rng, angle_increment=2 * math.pi / 360, range_max=8.0))
        wm.update(RobotState(x=x, y=y, yaw=yaw), lm)
        want.update(np.asarray(lm.occupancy), (x, y, yaw))
    # the last scan again, the pose off by two cells and a degree
    guess = (x + 2 * want.resolution, y - want.resolution, yaw + math.radians(1.0))
    state = RobotState(x=guess[0], y=guess[1], yaw=guess[2])
    exp, table, pose = mref.match_pose(want, np.asarray(lm.occupancy), guess, 4, math.radians(0.5), 5)
    a = wm.match(state, lm, n_yaw=4, yaw_step=math.radians(0.5), reach=5)          # from the device
    np.testing.assert_array_equal(a.scores(), table)
    b = wm.match(state, np.asarray(lm.occupancy), n_yaw=4, yaw_step=math.radians(0.5), reach=5)   # from the host
    for m in (a, b):
        assert (m.k, m.u, m.v, m.score, m.score_guess, m.points, m.pose) == tuple(exp)
        assert (m.x, m.y, m.yaw) == pose
    assert exp.points > 30 and exp.score > exp.score_guess
    n = wm.update(state, lm, match=True, n_yaw=4, yaw_step=math.radians(0.5), reach=5)
    assert wm.last_match.applied == (wm.last_match.ratio >= 0.6)
    assert (n, wm.changed_box) == want.update(np.asarray(lm.occupancy), exp.pose if wm.last_match.applied else guess)
    np.testing.assert_array_equal(wm.evidence, want.evidence)
