"""The world map's obstacle list on the device (kc_worldmap_points, DESIGN.md 4.11 rules 16 to 19) against
tests/worldmap_points_ref.py: the sorted list bit for bit, the count and the index bounds.

The main world is 37 x 29 (neither side a multiple of 4 or 64: the kernel loads bytes of rows that do not start on a
dword); the 300 x 260 worlds spread the window over hundreds of workgroups."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import worldmap_points_ref as pref  # noqa: E402
import worldmap_ref as ref  # noqa: E402

RES, ORIGIN = 0.05, (-0.33, 1.7)
NONE = (-1, -1, -1, -1)


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def seeded_prior(w, h, seed, p_occ=0.3, p_unknown=0.2):
    rng = np.random.default_rng(seed)
    return rng.choice(np.int8([ref.OCCUPIED, ref.UNEXPLORED, ref.EMPTY]), size=(w, h),
                      p=[p_occ, p_unknown, 1.0 - p_occ - p_unknown]).astype(np.int8)


def world(w, h, prior, res=RES, origin=ORIGIN):
    ctx = kh.WorldMapContext(w, h, res, origin)
    ctx.set_prior(prior)
    return ctx


def xy_of(cell_i, cell_j, res=RES, origin=ORIGIN):
    r = float(np.float32(res))
    return origin[0] + cell_i * r, origin[1] + cell_j * r


def range_of(rc, res=RES):
    """A range of rc - 1/2 cells: Rc = rc by rule 16's ceil."""
    return float(np.float32(res)) * (rc - 0.5)


def check(ctx, cls, x, y, rng, res=RES, origin=ORIGIN):
    want, n, bounds = pref.worldmap_points_ref(cls, res, origin, x, y, rng)
    got, got_bounds = ctx.points(x, y, rng)
    assert (len(got), got_bounds) == (n, bounds), (x, y, rng)
    assert pref.sort_points(got, res, origin).tobytes() == want.tobytes(), (x, y, rng)
    assert ctx.points(x, y, rng, count_only=True) == (n, bounds)
    return n


@pytest.fixture(scope="module")
def small():
    prior = seeded_prior(37, 29, 11)
    with world(37, 29, prior) as ctx:
        yield ctx, prior


CENTRES = [(18, 14),                                                          # the middle
           (0, 14), (36, 14), (18, 0), (18, 28),                              # the four edges
           (0, 0), (36, 0), (0, 28), (36, 28),                                # the four corners
           (-1, 14), (37, 14), (18, -1), (18, 29),                            # one cell outside each edge
           (12.37, 9.81), (36.49, 28.49)]                                     # fractions of a cell


@pytest.mark.parametrize("rc", [1, 5, 64])
def test_small_world(small, rc):
    ctx, prior = small
    total = 0
    for cell in CENTRES:
        x, y = xy_of(*cell)
        assert pref.window(RES, ORIGIN, x, y, range_of(rc))[2] == rc
        total += check(ctx, prior, x, y, range_of(rc))
    assert total > 0
    if rc == 64:                                                                # the window holds the whole map
        assert check(ctx, prior, *xy_of(18, 14), range_of(rc)) == int((prior == ref.OCCUPIED).sum())


def test_far_outside_is_empty_and_no_error(small):
    ctx, prior = small
    for cell in [(-200, 14), (18, 400), (5000, -5000)]:
        x, y = xy_of(*cell)
        assert check(ctx, prior, x, y, range_of(5)) == 0
        assert ctx.points(x, y, range_of(5))[1] == NONE


def test_smallest_radius():
    """Rule 16's ceil makes Rc >= 1 for every range it accepts (Rc = 0 would need a range of 0, which it refuses): the
    smallest window is the robot's own cell and its four neighbours.  One occupied cell seen from itself, from a
    neighbour and from a diagonal cell pins that disc; the entry's refusals ride along."""
    prior = np.full((37, 29), ref.EMPTY, np.int8)
    prior[20, 9] = ref.OCCUPIED
    with world(37, 29, prior) as ctx:
        assert check(ctx, prior, *xy_of(20, 9), 1e-6) == 1
        assert check(ctx, prior, *xy_of(21, 9), 1e-6) == 1
        assert check(ctx, prior, *xy_of(21, 10), 1e-6) == 0
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError):
                ctx.points(*xy_of(20, 9), bad)
        with pytest.raises(IndexError):
            ctx.points(*xy_of(20, 9), 103.0)


@pytest.mark.parametrize("shape", [(1, 1), (63, 2), (5, 3)])
def test_tiny_worlds_under_a_large_window(shape):
    prior = seeded_prior(*shape, seed=shape[0], p_occ=0.6)
    prior[0, 0] = ref.OCCUPIED
    with world(*shape, prior) as ctx:
        for cell in [(0, 0), (shape[0] / 2, shape[1] / 2), (shape[0] + 10, -7), (-39.4, 0)]:
            check(ctx, prior, *xy_of(*cell), range_of(40))
        assert check(ctx, prior, *xy_of(0, 0), range_of(40)) > 0


def test_full_disc_over_hundreds_of_workgroups():
    prior = np.full((300, 260), ref.OCCUPIED, np.int8)
    d = np.arange(-100, 101, dtype=np.int64)
    disc = int((d[:, None] ** 2 + d[None, :] ** 2 <= 100 * 100).sum())
    assert disc == 31417 and disc > 16384
    with world(300, 260, prior) as ctx:
        assert check(ctx, prior, *xy_of(150, 130), range_of(100)) == disc    # the whole disc lies inside the map
        assert check(ctx, prior, *xy_of(20, 250.3), range_of(100)) < disc    # clipped at two sides


def test_sparse_world_and_counters_rearmed():
    prior = seeded_prior(300, 260, 21, p_occ=0.01, p_unknown=0.3)
    with world(300, 260, prior) as ctx:
        x, y = xy_of(140.2, 133.7)
        n = check(ctx, prior, x, y, range_of(100))
        assert 100 < n < 1000
        a, ab = ctx.points(x, y, range_of(100))
        b, bb = ctx.points(x, y, range_of(100))
        assert ab == bb and len(a) == len(b) == n
        assert pref.sort_points(a, RES, ORIGIN).tobytes() == pref.sort_points(b, RES, ORIGIN).tobytes()
        check(ctx, prior, *xy_of(3, 3), range_of(30))                            # another window after it


def test_capacity_and_count_only(small):
    ctx, prior = small
    x, y = xy_of(18, 14)
    _, n, bounds = pref.worldmap_points_ref(prior, RES, ORIGIN, x, y, range_of(5))
    assert n > 3
    assert ctx.points(x, y, range_of(5), count_only=True) == (n, bounds)
    with pytest.raises(IndexError, match=str(n)):
        ctx.points(x, y, range_of(5), cap=n - 1)
    # the C entry itself: the count is set, the output untouched
    import ctypes as C
    out = np.full((n - 1, 3), 7.0, np.float32)
    cnt, b = C.c_size_t(0), (C.c_int32 * 4)()
    rc = kh.lib().kc_worldmap_points(ctx.h, x, y, range_of(5), out.ctypes.data, n - 1, C.byref(cnt), b)
    assert rc == -2 and cnt.value == n and (out == 7.0).all()
    got, _ = ctx.points(x, y, range_of(5), cap=n + 5)
    assert len(got) == n


def test_points_follow_an_update():
    with kh.WorldMapContext(37, 29, RES, ORIGIN) as ctx:
        want = ref.WorldMapRef(37, 29, RES, ORIGIN)
        x, y = xy_of(18, 14)
        assert ctx.points(x, y, 2.0, count_only=True) == (0, NONE)
        g = np.zeros((9, 7), np.int32)
        g[2:5, 3] = 100
        g[7, 1] = 100
        pose = (x, y, 0.3)
        assert ctx.update(g, pose) == want.update(g, pose)
        n = check(ctx, want.cls, x, y, 2.0)
        assert n == int((want.cls == ref.OCCUPIED).sum()) and n >= 3
