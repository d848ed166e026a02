"""The world map on the device (kc_worldmap_*) against tests/worldmap_ref.py: every plane, the changed
count and the changed box, bit for bit, after every call.

The main world is 37 x 29 (not a multiple of 4 wide) and the local grid 9 x 7 (not square: a gh / gw or c0 / c1 mix-up
shows).  A 64 x 64 local grid over the 37 x 29 world, a world 5 cells wide and a world of one cell make the launch box
span the full width, which is where dword stores into the dense byte planes would collide."""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import synthetic as syn  # noqa: E402
import worldmap_ref as ref  # noqa: E402

from helpers import DeviceArray, hip_runtime  # noqa: E402

YAWS = [0.0, math.pi / 2, math.pi, 0.3, -2.5]
RES, ORIGIN = 0.1, (-1.0, 2.0)
NONE = (0, (-1, -1, -1, -1))


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def local_grid(gh, gw, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.int32([-1, 0, 100, 50]), size=(gh, gw)).astype(np.int32)


def pair(w, h, res=RES, origin=ORIGIN, **model):
    """A context and the reference map it has to follow."""
    ctx = kh.WorldMapContext(w, h, res, origin)
    if model:
        ctx.set_model(**model)
    return ctx, ref.WorldMapRef(w, h, res, origin, **model)


def same_planes(ctx, want):
    cls, ev = ctx.planes()
    np.testing.assert_array_equal(ev, want.evidence)
    np.testing.assert_array_equal(cls, want.cls)


def step(ctx, want, grid, pose, update=None):
    """One update on both sides; -> (changed, box)."""
    got = (update or ctx.update)(grid, pose)
    exp = want.update(grid, pose)
    assert got == exp, (pose, got, exp)
    same_planes(ctx, want)
    return got


def world_xy(cell_i, cell_j, res=RES, origin=ORIGIN):
    return origin[0] + cell_i * res, origin[1] + cell_j * res


# the robot's position in cells of the 37 x 29 world: inside, clipped at each of the four sides, fractional offsets
POSES_IN = [(18, 14), (1, 12), (35.5, 14), (20, 0.25), (17, 28), (12.37, 9.81), (30.5, 3.5), (36.49, 28.49)]
POSES_OUT = [(-12, 14), (60, 10), (18, -15), (10, 50), (-8.5, -7.25)]


@pytest.mark.parametrize("yaw", YAWS)
def test_poses_on_the_small_world(yaw):
    ctx, want = pair(37, 29)
    with ctx:
        for k, cell in enumerate(POSES_IN):
            g = local_grid(9, 7, 100 + k)
            n, box = step(ctx, want, g, world_xy(*cell) + (yaw,))
            assert n > 0 and box[0] <= box[2] and box[1] <= box[3]
            if k % 3 == 2:            # now and then from an empty map again
                ctx.clear()
                want.clear()
                same_planes(ctx, want)
        for cell in POSES_OUT:
            assert step(ctx, want, local_grid(9, 7, 7), world_xy(*cell) + (yaw,)) == NONE


@pytest.mark.parametrize("shape", [(37, 29), (5, 29), (5, 3), (1, 1), (4, 4), (63, 2)])
def test_local_grid_larger_than_the_world(shape):
    ctx, want = pair(*shape, **ref.LATEST_WINS_EXACT)
    with ctx:
        for k, yaw in enumerate(YAWS + [0.7]):
            g = local_grid(64, 64, 200 + k)
            cell = (shape[0] / 2 + 0.3 * k, shape[1] / 2 - 0.45 * k)
            step(ctx, want, g, world_xy(*cell) + (yaw,))
        # the local grid covers the whole world, and under this model an observation decides the class
        g = np.zeros((64, 64), np.int32)
        step(ctx, want, g, world_xy(shape[0] / 2, shape[1] / 2) + (0.0,))
        assert (want.cls == 0).all()
        g[:] = 100
        assert step(ctx, want, g, world_xy(shape[0] / 2, shape[1] / 2) + (1.0,)) == (shape[0] * shape[1], (0, 0, shape[0] - 1, shape[1] - 1))


@pytest.mark.parametrize("model", [{}, ref.LATEST_WINS, ref.LATEST_WINS_EXACT], ids=["default", "latest_wins", "latest_wins_exact"])
def test_twenty_updates_in_a_row(model):
    rng = np.random.default_rng(5 + len(model) - model.get("e_min", 0))
    ctx, want = pair(37, 29, **model)
    total = 0
    with ctx:
        for k in range(20):
            gh, gw = (9, 7) if k % 4 else (int(rng.integers(1, 30)), int(rng.integers(1, 30)))
            g = local_grid(gh, gw, 300 + k)
            cell = (rng.uniform(-4, 41), rng.uniform(-4, 33))
            total += step(ctx, want, g, world_xy(*cell) + (rng.uniform(-math.pi, math.pi),))[0]
    assert total > 100
    assert (want.evidence != ref.NEVER).sum() > 200


def test_quantised_pose_and_explicit_central_cell():
    ctx, want = pair(37, 29)
    g = local_grid(9, 7, 1)
    with ctx:
        p = ctx.quantise_pose(1.03, 3.21, 0.3)
        q = (p.cq, p.sq, p.tx, p.ty)
        assert q == ref.quantise_pose(RES, ORIGIN, 1.03, 3.21, 0.3)
        assert ctx.update(g, p) == want.update(g, q)
        same_planes(ctx, want)
        assert ctx.update(g, p, central=(0, 6)) == want.update(g, q, c=(0, 6))   # not the mapper's centre
        same_planes(ctx, want)
        assert ctx.update(g, p, central=(-20, 40)) == want.update(g, q, c=(-20, 40)) == NONE


def test_priors_updates_and_clear():
    rng = np.random.default_rng(9)
    prior = rng.choice(np.int8([-1, 0, 100, 50]), size=(37, 29)).astype(np.int8)
    ctx, want = pair(37, 29)
    with ctx:
        ctx.set_prior(prior)                       # int8 from the host
        want.set_prior(prior)
        same_planes(ctx, want)
        for k in range(3):
            step(ctx, want, local_grid(9, 7, 400 + k), world_xy(10 + 6 * k, 9 + 5 * k) + (0.4 * k,))
        prior32 = np.asfortranarray(rng.choice(np.int32([-1, 0, 100, 7]), size=(37, 29)).astype(np.int32))
        with DeviceArray(prior32) as dev:          # int32 where it lies on the device
            ctx.set_prior_device(dev.ptr, 37, 29, elem_bytes=4)
            with pytest.raises(ValueError, match="outside"):
                ctx.set_prior_device(dev.ptr + 4, 37, 29, elem_bytes=4)
        want.set_prior(prior32)
        same_planes(ctx, want)
        for k in range(3):
            step(ctx, want, local_grid(9, 7, 410 + k), world_xy(30 - 6 * k, 20 - 5 * k) + (-0.9 * k,))
        with pytest.raises(ValueError, match="does not fit"):
            ctx.set_prior(np.zeros((29, 37), np.int8))
        with pytest.raises(ValueError):
            ctx.set_prior_device(prior32.ctypes.data, 37, 29, elem_bytes=4)   # host memory
        same_planes(ctx, want)                     # a refusal leaves the map as it was
        ctx.clear()
        want.clear()
        same_planes(ctx, want)
        step(ctx, want, local_grid(9, 7, 420), world_xy(18, 14) + (2.0,))
        ctx.set_model(hit=5, miss=2, e_min=-3, e_max=9, occ_thr=5)   # clears
        want.set_model(hit=5, miss=2, e_min=-3, e_max=9, occ_thr=5)
        same_planes(ctx, want)
        for k in range(4):
            step(ctx, want, local_grid(9, 7, 430 + k % 2), world_xy(18, 14) + (2.0,))
        with pytest.raises(ValueError):
            ctx.set_model(hit=0)
        step(ctx, want, local_grid(9, 7, 431), world_xy(18, 14) + (2.0,))


def test_update_from_a_grid_on_the_device_and_its_refusals():
    ctx, want = pair(37, 29)
    g = np.asfortranarray(local_grid(9, 7, 21))
    with ctx, DeviceArray(np.concatenate([g.ravel(order="F"), g.ravel(order="F")[::-1]])) as dev:
        pose = world_xy(18.3, 13.6) + (0.3,)
        dev_update = lambda ptr: (lambda grid, p: ctx.update_device(ptr, 9, 7, p))  # noqa: E731
        step(ctx, want, g, pose, dev_update(dev.ptr))
        back = np.asfortranarray(g.ravel(order="F")[::-1].reshape(9, 7, order="F"))
        step(ctx, want, back, pose, dev_update(dev.ptr + g.nbytes))              # the second half, to the allocation's end
        with pytest.raises(ValueError, match="outside"):
            ctx.update_device(dev.ptr + g.nbytes, 9, 8, pose)
        with pytest.raises(ValueError, match="aligned"):
            ctx.update_device(dev.ptr + 2, 9, 7, pose)
        with pytest.raises(ValueError):
            ctx.update_device(g.ctypes.data, 9, 7, pose)                         # host memory
        with pytest.raises(ValueError, match="resolution"):
            ctx.update_device(dev.ptr, 9, 7, pose, resolution=0.05)
        with pytest.raises(ValueError, match="resolution"):
            ctx.update(g, pose, resolution=float(np.nextafter(np.float32(RES), np.float32(1.0))))
        with pytest.raises(IndexError):
            ctx.update(g, kh.WorldMapPose(65536, 0, (1 << 36) + 1, 0))
        same_planes(ctx, want)


def _fetch(mapper, gh, gw):
    """The mapper's device grid, finished, as the [gh, gw] array its scan_to_grid would have returned."""
    mapper.sync()
    out = np.empty(gh * gw, np.int32)
    assert hip_runtime().hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(mapper.grid_device_ptr()), out.nbytes, 2) == 0
    return out.reshape(gw, gh).T


def test_update_from_mapper_without_a_sync():
    gh, gw, res = 40, 30, np.float32(0.1)
    ang, rng = syn.dense_scan(360, 0.25)
    ctx, want = pair(37, 29, res)
    other = kh.WorldMapContext(37, 29, res, ORIGIN)
    with ctx, other, kh.MapperContext(gh, gw, res, (0, 0, 0), 0.0, 360) as mapper:
        seen = []
        for k, (r, pose) in enumerate([(rng, world_xy(15.2, 12.7) + (0.3,)), (rng[::-1] * 0.8, world_xy(22.6, 16.1) + (-2.5,)),
                                       (rng * 0.6, world_xy(10.0, 20.0) + (math.pi / 2,))]):
            mapper.scan_to_grid_device(ang, np.ascontiguousarray(r))
            got = ctx.update_from_mapper(mapper, pose)           # no mapper.sync() in between: the event orders it
            g = _fetch(mapper, gh, gw)
            assert (g == 100).any() and (g == 0).any()
            seen.append(g)
            assert got == other.update(g, pose) == want.update(g, pose)
            same_planes(ctx, want)
            same_planes(other, want)
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])   # three scans, three grids
        with kh.MapperContext(gh, gw, 0.05, (0, 0, 0), 0.0, 360) as fine:
            fine.scan_to_grid_device(ang, rng)
            with pytest.raises(ValueError, match="resolution"):
                ctx.update_from_mapper(fine, (0.0, 3.0, 0.0))


def test_at_size():
    ctx, want = pair(1000, 800, 0.05, (-5.0, -3.0))
    rng = np.random.default_rng(77)
    with ctx:
        for k, (cell, yaw) in enumerate([((500.3, 400.7), 0.3), ((120.0, 700.5), -2.5), ((990.2, 10.1), math.pi / 2)]):
            g = rng.choice(np.int32([-1, 0, 0, 100]), size=(400, 400)).astype(np.int32)
            n, box = step(ctx, want, g, world_xy(*cell, res=0.05, origin=(-5.0, -3.0)) + (yaw,))
            assert n > 20000


class HostGrid:
    """A pointer of the wrong kind: host memory behind the device array protocol."""

    def __init__(self, a):
        self.a = np.asfortranarray(a)
        self.__cuda_array_interface__ = dict(shape=self.a.shape, typestr="|i1", data=(self.a.ctypes.data, False),
                                             strides=self.a.strides, version=3, stream=None)


def _room_scan(x, y, yaw, box, n=360, rmax=8.0):
    """Ranges of n beams from (x, y, yaw) in a 6 m x 4 m room [0, 6] x [0, 4] that holds the axis-aligned `box`
    (x0, y0, x1, y1), or nothing when it is None."""
    ang = -math.pi + np.arange(n) * (2 * math.pi / n)
    dx, dy = np.cos(ang + yaw), np.sin(ang + yaw)
    rects = [(0.0, 0.0, 6.0, 4.0)] + ([box] if box else [])
    best = np.full(n, rmax)
    with np.errstate(divide="ignore", invalid="ignore"):
        for x0, y0, x1, y1 in rects:
            for wall, lo, hi, along_x in [(x0, y0, y1, False), (x1, y0, y1, False), (y0, x0, x1, True), (y1, x0, x1, True)]:
                t = (wall - y) / dy if along_x else (wall - x) / dx
                s = x + t * dx if along_x else y + t * dy
                ok = (t > 1e-9) & (s >= lo) & (s <= hi)
                best = np.where(ok & (t < best), t, best)
    return ang, best


def test_front_end_maps_plans_and_replans():
    from kompass_core.datatypes.laserscan import LaserScanData
    from kompass_core.mapping import LocalMapper, MapConfig, WorldMap
    from kompass_core.models import RobotState
    from kompass_core.planning import GridPlanner
    from test_planner_gpu import _robot

    res, origin = 0.05, (-1.0, -1.0)
    wm = WorldMap(160, 120, res, origin)
    want = ref.WorldMapRef(160, 120, res, origin)
    lm = LocalMapper(MapConfig(width=4.0, height=4.0, resolution=res))

    def see(x, y, yaw, box):
        state = RobotState(x=x, y=y, yaw=yaw)
        ang, rng = _room_scan(x, y, yaw, box)
        lm.update_from_scan(state, LaserScanData(angles=ang, ranges=rng, angle_increment=2 * math.pi / 360, range_max=8.0))
        n = wm.update(state, lm)                              # the mapper's grid where it lies
        exp = want.update(np.asarray(lm.occupancy), (x, y, yaw))
        assert (n, wm.changed_box) == exp and wm.changed == n
        np.testing.assert_array_equal(wm.occupancy, want.cls)
        np.testing.assert_array_equal(wm.evidence, want.evidence)
        return n

    for k in range(5):
        assert see(1.0 + 1.0 * k, 2.0 + 0.1 * k, 0.2 * k - 0.3, None) > 0
    assert (want.cls == 100).sum() > 50 and (want.cls == 0).sum() > 3000
    assert wm.map_meta_data == dict(origin_x=-1.0, origin_y=-1.0, width=160, height=120, resolution=float(np.float32(res)))
    start, goal = (1.0, 1.0), (5.0, 3.0)
    fe = GridPlanner(_robot())
    fe.setup_problem(None, start[0], start[1], 0.0, goal[0], goal[1], 0.0, grid=wm)   # metadata and grid from the map
    first = fe.solve()
    fresh = GridPlanner(_robot())
    fresh.setup_problem(wm.map_meta_data, start[0], start[1], 0.0, goal[0], goal[1], 0.0, grid=wm.occupancy)
    assert first is not None and fresh.solve() is not None
    np.testing.assert_array_equal(fe.path_cells, fresh.path_cells)
    # a crate appears in the middle of the room, across the path
    crate = (2.6, 0.6, 3.2, 3.0)
    changed = sum(see(x, y, yaw, crate) for x, y, yaw in [(1.5, 2.0, 0.0), (2.0, 1.2, 0.4), (1.8, 2.4, -0.2), (4.5, 2.0, math.pi)])
    assert changed > 20
    path = fe.replan(map=wm)
    fresh = GridPlanner(_robot())
    fresh.setup_problem(wm.map_meta_data, start[0], start[1], 0.0, goal[0], goal[1], 0.0, grid=wm.occupancy)
    wpath = fresh.solve()
    assert path is not None and wpath is not None and fe.replanned
    assert fe.status == fresh.status and fe.get_cost() == fresh.get_cost()
    np.testing.assert_array_equal(fe.path_cells, fresh.path_cells)
    np.testing.assert_array_equal(np.asarray(path.x()), np.asarray(wpath.x()))
    np.testing.assert_array_equal(np.asarray(path.y()), np.asarray(wpath.y()))
    assert not np.array_equal(np.asarray(path.y()), np.asarray(first.y()))   # the crate did move the path
    # a local grid from the host is the same update
    n = wm.update(RobotState(x=3.0, y=3.5, yaw=1.0), np.asarray(lm.occupancy))
    assert (n, wm.changed_box) == want.update(np.asarray(lm.occupancy), (3.0, 3.5, 1.0))
    np.testing.assert_array_equal(wm.evidence, want.evidence)
    # a pointer of the wrong kind
    fake = HostGrid(wm.occupancy)
    with pytest.raises(ValueError):
        fe.replan(map=fake)
    with pytest.raises(ValueError):
        wm.set_prior(fake)
    np.testing.assert_array_equal(wm.occupancy, want.cls)
    # a prior through the front end, then the planner on it
    wm.set_prior(np.where(want.cls == 100, 100, 0).astype(np.int8))
    want.set_prior(np.where(want.cls == 100, 100, 0).astype(np.int8))
    np.testing.assert_array_equal(wm.evidence, want.evidence)
    assert fe.replan(map=wm) is not None
