"""The correlative match's CPU statement (tests/worldmap_match_ref.py, DESIGN.md 4.11 rules 9 to 15) on cases worked
out by hand, the library's host-only entries against it, and the refusals that need no device.  No GPU needed."""
import math

import numpy as np
import pytest

import kompass_hip as kh
import worldmap_match_ref as mref
import worldmap_ref as ref


def test_window_and_grid_are_refused_before_any_device_is_looked_for():
    kh.worldmap_match_check_window(31, 0.0, 31)
    kh.worldmap_match_check_window(0, 1e300, 0)
    for bad in [(32, 0.01, 5), (-1, 0.01, 5), (4, 0.01, 32), (4, 0.01, -1), (4, -1e-9, 5), (4, float("nan"), 5),
                (4, float("inf"), 5)]:
        with pytest.raises(ValueError):
            kh.worldmap_match_check_window(*bad)
        with pytest.raises(ValueError):
            mref.check_window(*bad)
    kh.worldmap_match_check_grid(0.05, 8192, 8192, ref.central(8192, 8192), 0.05)
    with pytest.raises(IndexError, match="8192"):
        kh.worldmap_match_check_grid(0.05, 8193, 10, ref.central(8193, 10), 0.05)
    with pytest.raises(IndexError, match="8192"):
        kh.worldmap_match_check_grid(0.05, 10, 8193, ref.central(10, 8193), 0.05)
    with pytest.raises(IndexError, match="central"):
        kh.worldmap_match_check_grid(0.05, 10, 10, (-8190, 4), 0.05)      # cell (9, .) is 8199 cells from it
    with pytest.raises(ValueError, match="resolution"):
        kh.worldmap_match_check_grid(0.05, 10, 10, (4, 4), 0.1)           # an update's checks come first
    with pytest.raises(ValueError):
        kh.worldmap_match_rotations(0.3, 32, 0.01)
    with pytest.raises(ValueError):
        kh.worldmap_match_rotations(float("nan"), 2, 0.01)


@pytest.mark.parametrize("K,step", [(0, 0.25), (31, math.radians(0.5)), (31, 0.1), (5, 0.0)])
@pytest.mark.parametrize("yaw", [0.0, math.pi / 2, -2.5, 3.0, 1e-9])
def test_rotation_table(yaw, K, step):
    got = kh.worldmap_match_rotations(yaw, K, step)
    want = [(round(math.cos(yaw + float(k) * step) * 65536.0), round(math.sin(yaw + float(k) * step) * 65536.0))
            for k in range(-K, K + 1)]
    assert got == want == mref.rotations(yaw, K, step)
    assert len(got) == 2 * K + 1
    q = ref.quantise_pose(0.05, (0.0, 0.0), 0.0, 0.0, yaw)
    assert got[K] == q[:2]                       # k = 0 is the guess's own rotation
    if step == 0.0:
        assert len(set(got)) == 1


def test_tie_break_on_hand_made_tables():
    K, S = 2, 3
    z = np.zeros((2 * K + 1, 2 * S + 1, 2 * S + 1), np.uint32)
    at = lambda k, u, v: (k + K, v + S, u + S)   # noqa: E731
    both = lambda t: (mref.winner(t), mref.winner_fast(t))   # noqa: E731
    assert both(z) == ((0, 0, 0),) * 2                                    # all zero: the guess
    t = z.copy(); t[at(0, 2, 1)] = 7; t[at(0, -1, 1)] = 7                 # two equal peaks: the nearer
    assert both(t) == ((0, -1, 1),) * 2
    t = z.copy(); t[at(0, 2, 1)] = 8; t[at(0, -1, 1)] = 7                 # the larger wins however far
    assert both(t) == ((0, 2, 1),) * 2
    t = z.copy(); t[at(1, 1, 0)] = 5; t[at(-1, 1, 0)] = 5                 # mirrored in k: |k| equal, k = -1 first
    assert both(t) == ((-1, 1, 0),) * 2
    t = z.copy(); t[at(2, 1, 0)] = 5; t[at(-1, 1, 0)] = 5; t[at(1, 1, 0)] = 5   # |k| before k
    assert both(t) == ((-1, 1, 0),) * 2
    t = z.copy(); t[at(-2, 1, 0)] = 5; t[at(1, 1, 0)] = 5
    assert both(t) == ((1, 1, 0),) * 2
    t = z.copy(); t[at(0, 1, 2)] = 5; t[at(0, 2, 1)] = 5; t[at(0, -1, 2)] = 5; t[at(0, 2, -1)] = 5   # d2 = 5 four times: v, then u
    assert both(t) == ((0, 2, -1),) * 2
    t = z.copy(); t[at(0, 1, 2)] = 5; t[at(0, -1, 2)] = 5                 # v equal: the smaller u
    assert both(t) == ((0, -1, 2),) * 2
    t = z.copy(); t[at(2, 0, 0)] = 5; t[at(0, 1, 0)] = 5                  # distance in cells before the yaw
    assert both(t) == ((2, 0, 0),) * 2
    rng = np.random.default_rng(3)
    for _ in range(20):                                                    # few distinct values: ties everywhere
        t = rng.integers(0, 3, size=z.shape).astype(np.uint32)
        assert mref.winner(t) == mref.winner_fast(t)
    t = np.full((63, 63, 63), 0xFFFFFFFF, np.uint32)                       # the key's limits
    assert mref.winner_fast(t) == (0, 0, 0)
    t[:, 31, 31] = 0
    t[31] = 0
    assert mref.winner_fast(t) == mref.winner(t) == (-1, 0, -1)


def test_weights_by_hand():
    cls = np.full((5, 4), -1, np.int8)
    cls[1, 1] = 100
    cls[4, 3] = 100
    cls[3, 0] = 0
    want = np.array([[1, 2, 1, 0],
                     [2, 3, 2, 0],
                     [1, 2, 1, 0],
                     [0, 0, 1, 2],
                     [0, 0, 2, 3]], np.uint8)
    np.testing.assert_array_equal(mref.weights(cls), want)
    np.testing.assert_array_equal(mref.weights(np.full((1, 1), 100, np.int8)), [[3]])
    np.testing.assert_array_equal(mref.weights(np.zeros((3, 2), np.int8)), np.zeros((3, 2)))


def test_one_point_by_hand():
    """One occupied map cell, one point: the table is the weight patch mirrored into candidate space."""
    w = ref.WorldMapRef(9, 8, 0.1)
    g = np.zeros((9, 8), np.int8)
    g[6, 2] = 100
    w.set_prior(g)
    local = np.full((5, 5), -1, np.int32)
    assert ref.central(5, 5) == (1, 1)
    local[3, 0] = 100                              # (a, b) = (2, -1)
    # guess: the frame's origin at cell (3.25, 3.0), yaw 0: the point lands at (5.25, 2.0) -> cell (5, 2)
    q = ref.quantise_pose(w.resolution, w.origin, 0.325, 0.3, 0.0)
    assert q == (65536, 0, 3 * 65536 + 16384, 3 * 65536)
    m, t, pose = mref.match_pose(w, local, (0.325, 0.3, 0.0), 0, 0.0, 2)
    assert t.shape == (1, 5, 5) and m.points == 1
    assert t[0, 2, 2] == 2 == m.score_guess        # (5, 2) is an orthogonal neighbour of (6, 2)
    assert (m.k, m.u, m.v, m.score) == (0, 1, 0, 3)
    want = np.zeros((5, 5), np.uint32)             # [v + 2, u + 2]: rule 12 around (6, 2), seen from (5, 2)
    want[1:4, 2:5] = [[1, 2, 1], [2, 3, 2], [1, 2, 1]]
    np.testing.assert_array_equal(t[0], want)
    assert m.pose == (65536, 0, q[2] + 65536, q[3])
    assert pose == (0.325 + w.resolution, 0.3, 0.0)
    # a quarter turn: (a, b) -> (-b, a) = (1, 2): lands at (4.25, 5.0) -> cell (4, 5); reach 2 gets as far as (6, 3)
    m, t, _ = mref.match_pose(w, local, (0.325, 0.3, math.pi / 2), 0, 0.0, 2)
    assert (m.k, m.u, m.v, m.score, m.score_guess) == (0, 2, -2, 2, 0) and int(t.sum()) == 3 and t[0, 0, 3] == 1
    # no points: zeros, the guess, success
    m, t, _ = mref.match_pose(w, np.zeros((5, 5), np.int32), (0.325, 0.3, 0.0), 1, 0.1, 2)
    assert (m.k, m.u, m.v, m.score, m.score_guess, m.points) == (0, 0, 0, 0, 0, 0) and not t.any()
    # points that fall off the map score 0
    m, t, _ = mref.match_pose(w, local, (-5.0, 0.3, 0.0), 1, 0.1, 2)
    assert (m.k, m.u, m.v, m.score) == (0, 0, 0, 0) and m.points == 1


def test_the_rules_recover_a_pose():
    """A property of the statement alone: on the issue's scene the match returns exactly the offsets that were put in,
    in all 12 draws, with a score within 6 of 3 * points."""
    world = mref.recovery_world()
    assert (world.cls[:5] == -1).all() and (world.cls[111:] == -1).all() and (world.cls[5:111] != -1).all()
    step = math.radians(1.0)
    counts = []
    for true, guess, (k0, u0, v0) in mref.recovery_draws(12):
        local = mref.gather(world, true, 61, 61, (30, 30))
        m, t, pose = mref.match_pose(world, local, guess, 4, step, 5, (30, 30))
        assert (m.k, m.u, m.v) == (k0, u0, v0), (true, guess)
        assert 0 <= 3 * m.points - m.score <= 6
        assert m.score == t.max() and mref.winner(t) == (k0, u0, v0)
        assert pose == (guess[0] + u0 * world.resolution, guess[1] + v0 * world.resolution, guess[2] + float(k0) * step)
        counts.append(m.points)
    assert min(counts) == 91 and max(counts) == 180
