"""The world map's host pipeline (DESIGN.md 4.11 "Host pipeline"): what the three grid sources, the two flip-flop
records, the staging buffer and the check order have to keep when they are used in combination.

Every result is compared bit for bit with the numpy statements (tests/worldmap_ref.py, worldmap_match_ref.py,
worldmap_points_ref.py).  The world is 37 x 29 at 0.1 m, the local grid the 24 x 20 of a MapperContext after a scan
of 48 beams."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import synthetic as syn  # noqa: E402
import worldmap_match_ref as mref  # noqa: E402
import worldmap_points_ref as pref  # noqa: E402
import worldmap_ref as ref  # noqa: E402

from helpers import DeviceArray, assert_cycle_equal, hip_context, oracle_cycle  # noqa: E402
from test_worldmap_gpu import ORIGIN, RES, _fetch, same_planes, world_xy  # noqa: E402
from test_worldmap_handoff_gpu import _cycle_from_ctx, origin_for  # noqa: E402

W, H = 37, 29
GH, GW, BEAMS = 24, 20, 48
WINDOW = dict(n_yaw=1, yaw_step=0.02, reach=2)
BAD_POSE = (65536, 0, (1 << 36) + 1, 0)            # 2^20 cells and 1 / 65536 of a cell out
BAD_ROTATIONS = [(65536, 65536)]                   # no unit vector


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def scan(k):
    """48 beams that end inside the 2.4 m x 2.0 m grid, a different outline for every k."""
    ang = -math.pi + np.arange(BEAMS, dtype=np.float64) * (2 * math.pi / BEAMS)
    return ang, 0.55 + 0.25 * np.sin(3.0 * ang + 0.9 * k)


def mapper_context(res=RES):
    return kh.MapperContext(GH, GW, res, (0, 0, 0), 0.0, BEAMS)


def scanned(mapper, k):
    """Scans, waits, and returns the mapper's grid as [GH, GW] on the host."""
    mapper.scan_to_grid_device(*scan(k))
    g = _fetch(mapper, GH, GW)
    assert (g == ref.OCCUPIED).sum() >= 8 and (g == ref.EMPTY).sum() >= 8
    return g


def flat(g):
    return np.asfortranarray(g).ravel(order="F")


class Side:
    """One context and the statement's map it has to follow; every call is made on both and compared."""

    def __init__(self):
        self.ctx, self.want = kh.WorldMapContext(W, H, RES, ORIGIN), ref.WorldMapRef(W, H, RES, ORIGIN)

    def update(self, g, pose, call):
        got, exp = call(pose), self.want.update(g, pose)
        assert got == exp, (pose, got, exp)
        same_planes(self.ctx, self.want)
        return got

    def match(self, g, pose, call):
        exp, table, _ = mref.match_pose(self.want, g, pose, WINDOW["n_yaw"], WINDOW["yaw_step"], WINDOW["reach"])
        got = call(pose)
        assert got == exp._asdict(), (pose, got, exp)
        np.testing.assert_array_equal(self.ctx.match_scores(WINDOW["n_yaw"], WINDOW["reach"]), table)
        same_planes(self.ctx, self.want)                       # a match leaves the map alone
        return exp

    def points(self, x, y, max_range, count_only=False):
        exp, n, bounds = pref.worldmap_points_ref(self.want.cls, RES, ORIGIN, x, y, max_range)
        if count_only:
            assert self.ctx.points(x, y, max_range, count_only=True) == (n, bounds)
        else:
            got, got_bounds = self.ctx.points(x, y, max_range)
            assert got_bounds == bounds and len(got) == n
            assert pref.sort_points(got, RES, ORIGIN).tobytes() == exp.tobytes()
        return n

    # the three sources, as (update call, match call) of a pose
    def host(self, g):
        return (lambda p: self.ctx.update(g, p)), (lambda p: self.ctx.match(g, p, **WINDOW))

    def device(self, ptr):
        return (lambda p: self.ctx.update_device(ptr, GH, GW, p)), (lambda p: self.ctx.match_device(ptr, GH, GW, p, **WINDOW))

    def mapper(self, m):
        return (lambda p: self.ctx.update_from_mapper(m, p)), (lambda p: self.ctx.match_from_mapper(m, p, **WINDOW))


POSES = [world_xy(15.2, 12.7) + (0.3,), world_xy(22.6, 16.1) + (-2.5,), world_xy(10.4, 17.8) + (math.pi / 2,),
         world_xy(18.0, 11.5) + (1.1,), world_xy(25.3, 9.2) + (-0.7,)]


def test_sources_and_records_interleaved():
    """update(host), points, match(device), update(mapper, no sync), points(count only), update(device), match(mapper),
    points, update(host): the update's record and the list's counters change parity independently of each other, the
    staging buffer serves update and match in turn, and a second context on the same device works in between."""
    a, b = Side(), Side()
    with a.ctx, b.ctx, mapper_context() as mapper:
        g0 = scanned(mapper, 0)
        with DeviceArray(flat(g0)) as dev0:
            x, y = world_xy(17.0, 13.0)
            assert a.update(g0, POSES[0], a.host(g0)[0])[0] > 0                       # 1
            assert a.points(x, y, 1.5) > 0                                            # 2
            assert a.match(g0, POSES[0], a.device(dev0.ptr)[1]).points > 0            # 3
            # the other context: its own record, counters and staging buffer
            assert b.update(g0, POSES[3], b.host(g0)[0])[0] > 0
            assert b.points(x, y, 3.0) > 0
            mapper.scan_to_grid_device(*scan(1))
            got = a.ctx.update_from_mapper(mapper, POSES[1])                          # 4: no mapper.sync() in between
            g1 = _fetch(mapper, GH, GW)
            assert not np.array_equal(g0, g1)
            assert got == a.want.update(g1, POSES[1]) and got[0] > 0
            same_planes(a.ctx, a.want)
            assert a.points(x, y, 3.0, count_only=True) > 0                           # 5
            b.match(g0, POSES[3], b.host(g0)[1])
            b.points(x, y, 0.4, count_only=True)
            assert a.update(g0, POSES[2], a.device(dev0.ptr)[0])[0] > 0               # 6
            a.match(g1, POSES[1], a.mapper(mapper)[1])                                # 7
            assert b.update(g1, POSES[4], b.mapper(mapper)[0])[0] > 0
            assert a.points(x, y, 3.0) > 0                                            # 8
            a.update(g1, POSES[3], a.host(g1)[0])                                     # 9
            b.points(x, y, 3.0)
            same_planes(b.ctx, b.want)
            assert not np.array_equal(a.want.cls, b.want.cls)


def refusals(ctx, g, dev, host_words):
    """(name, exception, word of the message, the refused call) for the update and the match."""
    p = POSES[0]
    past = dev.ptr + dev.nbytes - flat(g).nbytes + 4           # one cell past the allocation's end
    return [
        ("misaligned", ValueError, "aligned", lambda: ctx.update_device(dev.ptr + 2, GH, GW, p),
         lambda: ctx.match_device(dev.ptr + 2, GH, GW, p, **WINDOW)),
        ("past the allocation", ValueError, "outside", lambda: ctx.update_device(past, GH, GW, p),
         lambda: ctx.match_device(past, GH, GW, p, **WINDOW)),
        ("host memory", ValueError, None, lambda: ctx.update_device(host_words.ctypes.data, GH, GW, p),
         lambda: ctx.match_device(host_words.ctypes.data, GH, GW, p, **WINDOW)),
        ("resolution", ValueError, "resolution", lambda: ctx.update(g, p, resolution=0.05),
         lambda: ctx.match(g, p, resolution=0.05, **WINDOW)),
        ("pose", IndexError, "2\\^20", lambda: ctx.update(g, kh.WorldMapPose(*BAD_POSE)),
         lambda: ctx.match(g, kh.WorldMapPose(*BAD_POSE), reach=1, rotations=[(65536, 0)])),
        ("rotation", ValueError, "unit vector", None,
         lambda: ctx.match(g, ctx.quantise_pose(*p), reach=1, rotations=BAD_ROTATIONS)),
    ]


def test_a_refusal_then_work_from_every_source():
    s = Side()
    with s.ctx, mapper_context() as mapper:
        g = scanned(mapper, 2)
        host_words = flat(g).copy()
        with DeviceArray(np.concatenate([flat(g), flat(g)])) as dev:
            sources = [("host", s.host(g)), ("device", s.device(dev.ptr + flat(g).nbytes)), ("mapper", s.mapper(mapper))]
            k = 0
            for name, exc, word, bad_update, bad_match in refusals(s.ctx, g, dev, host_words):
                for source, (update, match) in sources:
                    for bad, good in ((bad_update, update), (bad_match, match)):
                        if bad is None:
                            continue
                        with pytest.raises(exc, match=word):
                            bad()
                        same_planes(s.ctx, s.want)                                    # a refusal leaves the map alone
                        pose = POSES[k % len(POSES)]
                        k += 1
                        (s.update if good is update else s.match)(g, pose, good)
            assert (s.want.cls == ref.OCCUPIED).sum() > 20


def test_which_check_wins():
    s = Side()
    far = kh.WorldMapPose(*BAD_POSE)
    with s.ctx, mapper_context() as mapper, mapper_context(0.05) as fine:
        g = scanned(mapper, 3)
        fine.scan_to_grid_device(*scan(3))
        with DeviceArray(flat(g)) as dev:
            # an update with a wrong resolution and a pose out of range: the grid check comes first
            for call in (lambda: s.ctx.update(g, far, resolution=0.05),
                         lambda: s.ctx.update_device(dev.ptr, GH, GW, far, resolution=0.05),
                         lambda: s.ctx.update_from_mapper(fine, far)):
                with pytest.raises(ValueError, match="resolution"):
                    call()
            # a match with a bad rotation table and a wrong resolution: the window's checks come first
            q = s.ctx.quantise_pose(*POSES[0])
            for call in (lambda: s.ctx.match(g, q, reach=1, resolution=0.05, rotations=BAD_ROTATIONS),
                         lambda: s.ctx.match_device(dev.ptr, GH, GW, q, reach=1, resolution=0.05, rotations=BAD_ROTATIONS),
                         lambda: s.ctx.match_from_mapper(fine, q, reach=1, rotations=BAD_ROTATIONS)):
                with pytest.raises(ValueError, match="unit vector"):
                    call()
            # no result to write, and everything else wrong as well: the null argument is reported
            L = kh.lib()
            rot = (kh.WorldMapRotation * 1)(kh.WorldMapRotation(*BAD_ROTATIONS[0]))
            for ptr in (flat(g).ctypes.data, dev.ptr + 2):
                for fn in (L.kc_worldmap_update_host, L.kc_worldmap_update_device):
                    with pytest.raises(ValueError, match="null argument"):
                        kh._check(fn(s.ctx.h, ptr, 0, -3, 0, 0, 0.05, C.byref(far), None))
                for fn in (L.kc_worldmap_match_host, L.kc_worldmap_match_device):
                    with pytest.raises(ValueError, match="null argument"):
                        kh._check(fn(s.ctx.h, ptr, 0, -3, 0, 0, 0.05, C.byref(far), rot, 0, 40, None))
            same_planes(s.ctx, s.want)
            s.update(g, POSES[0], s.host(g)[0])


def test_a_window_that_misses_the_map_then_one_that_does_not():
    """kc_dwa_set_worldmap with the robot 100 m outside the world leaves the empty list, the next call with the robot
    inside leaves the statement's list: the controller's cycle is the oracle's on either."""
    inp = syn.make_controller_inputs("cfg1", seed=3, scale=1.0)
    st = inp["state"]
    cell, max_range = (8, 14), 3.0
    origin = origin_for(st, cell, RES)
    cls = np.full((W, H), ref.EMPTY, np.int8)
    cls[cell[0] + 7:cell[0] + 9, cell[1] - 2:cell[1] + 5] = ref.OCCUPIED       # a wall the straight samples run into
    cls[30:, :] = ref.UNEXPLORED
    cls[3, 25] = cls[20, 2] = ref.OCCUPIED
    pts, n, _ = pref.worldmap_points_ref(cls, RES, origin, st[0], st[1], max_range)
    assert 10 < n <= int((cls == ref.OCCUPIED).sum())
    outside = (st[0] + 100.0 + W * RES,) + tuple(st[1:])
    assert pref.worldmap_points_ref(cls, RES, origin, outside[0], outside[1], max_range)[1] == 0
    empty = oracle_cycle(dict(inp, points=np.zeros((0, 3), np.float32), max_range=max_range))
    full = oracle_cycle(dict(inp, points=pts, max_range=max_range))
    assert len(empty["raw"]) == len(inp["vx"]) and 0 < len(full["raw"]) < len(inp["vx"])
    with kh.WorldMapContext(W, H, RES, origin) as wm:
        wm.set_prior(cls)
        ctx = hip_context(kh, dict(inp, points=pts, max_range=max_range))
        for state, want in ((outside, empty), (st, full), (outside, empty), (st, full)):
            ctx.set_worldmap(state, wm, max_range)
            assert_cycle_equal(want, _cycle_from_ctx(ctx, inp))
