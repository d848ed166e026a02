"""Sensor values at the edges of their types: NaN, +-inf, negative, huge finite ranges and angles.

Mapper: the reference converts the end point of a beam to int without a check (local_mapper.h:210-222) and walks
an int Bresenham (line_drawing.h:55-124), both undefined for NaN, inf and lines beyond 2^30 cells.  The rule
here: a beam whose cell offset x / res or y / res is not below 2^30 in magnitude is skipped, every
other beam keeps the reference's semantics, and the line walks only visit the steps that can land in the grid.
Every device result is compared with the oracle bit for bit, on every execution path of the mapper.

Controller: finite ranges too large for a float (1e39, DBL_MAX) through set_scan's chunk boxes, the largest
device point list in one bucket cell (the rank packing of sensor_points_kernel), and point lists with coordinates at
the octree key window, 1e30, FLT_MAX, -0.0 and denormals on every sensor path.  Point cloud -> laserscan and the
critical zone checker with coordinates whose squares overflow, denormals, +-0, +-inf, negative and DBL_MAX ranges."""
import json
import sys
import time
from pathlib import Path

import numpy as np
import pytest

import synthetic as syn
from oracle import ko

GOLD = Path(__file__).parent / "golden"
BAYES = dict(p_prior=0.6, p_occupied=0.9, p_empty=0.1, range_sure=0.1, range_max=20.0, wall_size=0.2)
FLT_MAX = float(np.finfo(np.float32).max)
DBL_MAX = sys.float_info.max


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _extreme_scan(n, res, ext, seed, orient=0.0):
    """n beams over the circle with ranges up to 1.3 x the grid's extent, and mixed in: NaN / +-inf ranges,
    negative ranges, 1e6 m, FLT_MAX, 1e39 (inf as a float), offsets of just below and just above 2^30 cells along
    the axes (angle 0 and pi: a horizontal / vertical line), and NaN / inf angles."""
    r = np.random.default_rng(seed)
    ang = np.linspace(-np.pi, np.pi, n, endpoint=False) + r.uniform(0, 1e-3)
    rng = r.uniform(0.0, 1.3 * ext, n)
    below, above = (2.0 ** 30) * res * (1 - 1e-6), (2.0 ** 30) * res * (1 + 1e-6)
    special = [np.nan, np.inf, -np.inf, -0.7 * ext, -3.0 * ext, 1e6, -1e6, FLT_MAX, -FLT_MAX, 1e39, DBL_MAX,
               below, above, -below, -above, 0.0]
    idx = r.choice(n, size=3 * len(special), replace=False)
    for k, i in enumerate(idx):
        rng[i] = special[k % len(special)]
    # the 2^30 edge on the axes (orient + angle = 0, pi/2, pi, -pi/2 up to an ulp): one offset decides
    for a, v in ((0.0, below), (0.0, above), (np.pi / 2, below), (np.pi / 2, above), (np.pi, below),
                 (-np.pi / 2, above)):
        j = int(r.integers(n))
        ang[j], rng[j] = a - np.float32(orient), v
    for v in (np.nan, np.inf, -np.inf, 1e30):
        ang[int(r.integers(n))] = v
    return ang, rng


# ---------------------------------------------------------------------------
# oracle (CPU): the rule itself
# ---------------------------------------------------------------------------
def test_oracle_skipped_beams_stamp_nothing():
    """NaN / inf ranges and angles, and beams beyond 2^30 cells, leave the grid as if they were not there."""
    ang, rng = np.linspace(-3, 3, 200), np.linspace(0.1, 9.0, 200)
    want = ko.scan_to_grid(150, 121, 0.05, (0.3, -0.2, 0), 0.4, ang, rng)
    bad_r = np.array([np.nan, np.inf, -np.inf, 1e39, DBL_MAX, FLT_MAX, 0.05 * 2.0 ** 30 * 1.001, 1.0, 2.0])
    bad_a = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6, -0.4, np.nan, np.inf])   # (-0.4: along the x axis)
    got = ko.scan_to_grid(150, 121, 0.05, (0.3, -0.2, 0), 0.4, np.concatenate([bad_a, ang]),
                          np.concatenate([bad_r, rng]))
    np.testing.assert_array_equal(got, want)
    # every beam skipped: nothing at all, not even the start cell
    assert (ko.scan_to_grid(40, 40, 0.05, (0.3, -0.2, 0), 0.4, bad_a, bad_r) == -1).all()
    o = ko.BayesMapper(40, 40, 0.05, (0.3, -0.2, 0), 0.4, **BAYES)
    g, p = o.scan_to_grid_baysian(bad_a, bad_r)
    assert (g == -1).all() and (p == np.float32(BAYES["p_prior"])).all()


def test_oracle_long_beams_equal_their_part_in_the_grid():
    """A beam along an axis whose offset is just below 2^30 cells stamps the same cells as one that just leaves the
    grid (the walk is clipped to the grid, the state at its first step is the closed form); 1e6 m the same; a
    negative range points backwards."""
    H, W, res = 90, 70, 0.05
    for a in (0.0, np.pi / 2, np.pi, -np.pi / 2):
        short = ko.scan_to_grid(H, W, res, (0.1, 0.05, 0), 0.0, [a], [10.0])
        for far in (1e6, (2.0 ** 30) * res * (1 - 1e-6)):
            np.testing.assert_array_equal(ko.scan_to_grid(H, W, res, (0.1, 0.05, 0), 0.0, [a], [far]), short)
    np.testing.assert_array_equal(ko.scan_to_grid(H, W, res, (0, 0, 0), 0.0, [0.0], [-1.0]),
                                  ko.scan_to_grid(H, W, res, (0, 0, 0), 0.0, [np.pi], [1.0]))


# ---------------------------------------------------------------------------
# device: every mapper path against the oracle
# ---------------------------------------------------------------------------
SHAPES = [(200, 200, 0.05, (0.0, 0.0, 0.0), 0.0),
          (257, 131, 0.1, (-0.4, 0.9, 0.0), 0.7),      # odd cell count: the memset fallback of the plain scan
          (96, 333, 0.02, (-1.5, 4.2, 0.0), -2.1)]     # sensor outside the grid


@pytest.mark.gpu
@pytest.mark.parametrize("shape", range(len(SHAPES)))
@pytest.mark.parametrize("staged", ["0", "1"])
@pytest.mark.parametrize("tiles", ["0", "1", "2", "3"])
def test_mapper_extreme_ranges_equal_the_oracle(tiles, staged, shape, monkeypatch):
    """Plain and Bayesian scans with extreme beams on one context (the alternating plain grids, scans queued with
    scan_to_grid_device in between, the Bayesian warp), KC_MAPPER_TILES 0-3 x KC_MAPPER_STAGED 0/1."""
    import kompass_hip as kh
    monkeypatch.setenv("KC_MAPPER_TILES", tiles)
    monkeypatch.setenv("KC_MAPPER_STAGED", staged)
    H, W, res, pos, orient = SHAPES[shape]
    ext = max(H, W) * res
    m = kh.MapperContext(H, W, res, pos, orient, 2048)
    o = ko.BayesMapper(H, W, res, pos, orient, **BAYES)
    for k in range(4):
        ang, rng = _extreme_scan([1440, 361, 2048, 64][k], res, ext, 100 * shape + k, orient)
        want = ko.scan_to_grid(H, W, res, pos, orient, ang, rng)
        assert (want != -1).any()
        np.testing.assert_array_equal(m.scan_to_grid(ang, rng), want)
        m.scan_to_grid_device(ang[::-1].copy(), rng[::-1].copy())   # queued only; the next scan must not see it
    m.enable_bayes(**BAYES)
    for k in range(3):
        ang, rng = _extreme_scan([720, 2048, 97][k], res, ext, 7 + 100 * shape + k, orient)
        want_g, want_p = o.scan_to_grid_baysian(ang, rng)
        got_g, got_p = m.scan_to_grid_baysian(ang, rng)
        np.testing.assert_array_equal(got_g, want_g)
        np.testing.assert_array_equal(_bits(got_p), _bits(want_p))
        o.set_previous(want_p)
        m.set_previous_prob(None)
        o.get_previous_grid_in_current_pose((0.05 * (k + 1), -0.03), 0.1 * (k + 1))
        m.get_previous_grid_in_current_pose((0.05 * (k + 1), -0.03), 0.1 * (k + 1))
        np.testing.assert_array_equal(_bits(m.previous_prob()), _bits(o.previous()))
    # a scan in which every beam is skipped: UNEXPLORED everywhere, the prior everywhere
    ang = np.array([0.0, 1.0, np.nan, 2.0, np.inf, -np.inf])
    rng = np.array([np.nan, np.inf, 1.0, 1e39, 2.0, 1.0])
    want_g, want_p = o.scan_to_grid_baysian(ang, rng)
    assert (want_g == -1).all() and (want_p == np.float32(BAYES["p_prior"])).all()
    got_g, got_p = m.scan_to_grid_baysian(ang, rng)
    np.testing.assert_array_equal(got_g, want_g)
    np.testing.assert_array_equal(_bits(got_p), _bits(want_p))
    np.testing.assert_array_equal(m.scan_to_grid(ang, rng), ko.scan_to_grid(H, W, res, pos, orient, ang, rng))
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tiles", ["0", "1", "2", "3"])
def test_mapper_uncleaned_fixture_scan(tiles, monkeypatch):
    """The reference's fixture as it is, with no nan_to_num / clip, and with the holes a driver leaves in a scan
    (inf: no return, NaN) punched into it."""
    import kompass_hip as kh
    monkeypatch.setenv("KC_MAPPER_TILES", tiles)
    data = json.loads((GOLD / "laserscan_data.json").read_text())
    rng = np.array(data["ranges"], dtype=np.float64)
    ang = data["angle_min"] + np.arange(len(rng)) * data["angle_increment"]
    holed = rng.copy()
    holed[::7], holed[3::11], holed[5::13] = np.inf, np.nan, -np.inf
    m = kh.MapperContext(200, 200, 0.1, (0, 0, 0), 0.0, len(rng))
    m.enable_bayes(**BAYES)
    for r in (rng, holed):
        want = ko.scan_to_grid(200, 200, 0.1, (0, 0, 0), 0.0, ang, r)
        np.testing.assert_array_equal(m.scan_to_grid(ang, r), want)
        assert (want == 100).sum() > 0
        o = ko.BayesMapper(200, 200, 0.1, (0, 0, 0), 0.0, **BAYES)
        want_g, want_p = o.scan_to_grid_baysian(ang, r)
        got_g, got_p = m.scan_to_grid_baysian(ang, r)
        np.testing.assert_array_equal(got_g, want_g)
        np.testing.assert_array_equal(_bits(got_p), _bits(want_p))
    m.close()


@pytest.mark.gpu
def test_mapper_class_surfaces_take_raw_ranges():
    """kompass_cpp.mapping.LocalMapper (plain and Baysian) and kompass_core's LocalMapper.update_from_scan with NaN
    and inf in the scan: the front end clips inf to filter_limit and leaves NaN to the mapper, which skips it."""
    import kompass_cpp
    from kompass_core.datatypes.laserscan import LaserScanData
    from kompass_core.mapping import LocalMapper, MapConfig
    H, W, res = 120, 160, 0.05
    ang, rng = _extreme_scan(720, res, 8.0, seed=3)
    plain = kompass_cpp.mapping.LocalMapper(grid_height=H, grid_width=W, resolution=res,
                                            laserscan_position=[0.1, -0.2, 0.0], laserscan_orientation=0.3,
                                            is_pointcloud=False, scan_size=len(ang), angle_step=0.01,
                                            max_height=10.0, min_height=-10.0, range_max=20.0,
                                            max_points_per_line=400)
    want = ko.scan_to_grid(H, W, res, (0.1, -0.2, 0), 0.3, ang, rng)
    np.testing.assert_array_equal(np.asarray(plain.scan_to_grid(angles=ang, ranges=rng)), want)
    bayes = kompass_cpp.mapping.LocalMapper(grid_height=H, grid_width=W, resolution=res,
                                            laserscan_position=[0.1, -0.2, 0.0], laserscan_orientation=0.3,
                                            is_pointcloud=False, scan_size=len(ang), angle_step=0.01,
                                            max_height=10.0, min_height=-10.0, max_points_per_line=400, **BAYES)
    o = ko.BayesMapper(H, W, res, (0.1, -0.2, 0), 0.3, **BAYES)
    want_g, want_p = o.scan_to_grid_baysian(ang, rng)
    g, p = bayes.scan_to_grid_baysian(angles=list(ang), ranges=list(rng))
    np.testing.assert_array_equal(np.asarray(g), want_g)
    np.testing.assert_array_equal(_bits(np.asarray(p).copy()), _bits(want_p))

    d = json.loads((GOLD / "laserscan_data.json").read_text())
    r = np.array(d["ranges"], float)
    r[5], r[50], r[100] = np.nan, np.inf, np.nan
    a = d["angle_min"] + np.arange(len(r)) * d["angle_increment"]
    scan = LaserScanData(angle_min=d["angle_min"], angle_max=d["angle_max"], angle_increment=d["angle_increment"],
                         range_max=d["range_max"], ranges=r, angles=a)
    m = LocalMapper(MapConfig(width=8.0, height=6.0, resolution=res))
    m.update_from_scan(None, scan)
    lim = m.config.filter_limit
    want = ko.scan_to_grid(H, W, res, (0, 0, 0), 0.0, a, np.clip(r, 0.0, lim))
    np.testing.assert_array_equal(m.occupancy, want)
    # = inf clipped to filter_limit, NaN beams dropped
    keep = ~np.isnan(r)
    np.testing.assert_array_equal(want, ko.scan_to_grid(H, W, res, (0, 0, 0), 0.0, a[keep],
                                                        np.minimum(np.maximum(r[keep], 0.0), lim)))


@pytest.mark.gpu
@pytest.mark.parametrize("bayes", [False, True])
def test_mapper_work_is_bounded_by_the_grid(bayes, monkeypatch):
    """4096 beams of 1e6 m on a 1000 x 1000 grid at 0.02 m: 5e7 steps a beam unclipped, at most ~1000 clipped.
    Measured on an MI355X (whole call, host copies included): median 0.29 ms plain, 1.88 ms Bayesian; the bound is
    50 ms (shared hosts), far below the seconds an unclipped walk would take."""
    import kompass_hip as kh
    monkeypatch.delenv("KC_MAPPER_TILES", raising=False)
    H = W = 1000
    res = 0.02
    ang = np.linspace(-np.pi, np.pi, 4096, endpoint=False)
    rng = np.full(4096, 1e6)
    m = kh.MapperContext(H, W, res, (0.3, -0.1, 0), 0.2, 4096)
    if bayes:
        m.enable_bayes(**BAYES)
        o = ko.BayesMapper(H, W, res, (0.3, -0.1, 0), 0.2, **BAYES)
        want_g, want_p = o.scan_to_grid_baysian(ang, rng)
        run = lambda: m.scan_to_grid_baysian(ang, rng)   # noqa: E731
        got_g, got_p = run()
        np.testing.assert_array_equal(got_g, want_g)
        np.testing.assert_array_equal(_bits(got_p), _bits(want_p))
    else:
        want = ko.scan_to_grid(H, W, res, (0.3, -0.1, 0), 0.2, ang, rng)
        run = lambda: m.scan_to_grid(ang, rng)   # noqa: E731
        np.testing.assert_array_equal(run(), want)
    ts = []
    for _ in range(10):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
    print(f"1e6 m beams, bayes={bayes}: median {np.median(ts) * 1e3:.2f} ms")
    assert np.median(ts) < 0.05
    m.close()


# ---------------------------------------------------------------------------
# controller: finite ranges too large for a float through set_scan's chunk boxes
# ---------------------------------------------------------------------------
def _huge_scan(big, near=0.4):
    """Walls at 5 m, and in the chunk of 64 beams starting at -45 degrees (4096 beams: kc_dwa_set_scan's chunks of
    64): beams at 8 m, the scan's nearest obstacle at `near` in lane 1 of the first eight-wide batch, and beams of
    range `big` in lane 1 of every later batch -- x = +inf, y = -inf as floats, whose placed obstacle has a NaN
    coordinate.  A box that dropped lane 1 behind a NaN would be the 8 m beams' box and prune the chunk."""
    n = 4096
    ang = np.linspace(-np.pi, np.pi, n, endpoint=False)
    rng = np.full(n, 5.0)
    q = 3 * n // 8            # -pi / 4, the first beam of chunk 24
    rng[q:q + 64] = 8.0
    rng[q + 1] = near
    rng[q + 9:q + 64:8] = big
    return ang, rng


@pytest.mark.gpu
@pytest.mark.parametrize("big", [1e39, DBL_MAX])
@pytest.mark.parametrize("yaw", [-0.5, 0.0, 0.6])
def test_scan_chunk_boxes_with_ranges_beyond_float(big, yaw):
    """set_scan + cycle with the near table on and off, single launch and split kernels: the oracle's costs.  The
    scene is checked to depend on the near obstacle (its costs change when the obstacle is moved to 8 m), so a chunk
    box that loses it -- box_avx2 behind a NaN lane -- gives other costs.  At yaw 0 both placed coordinates of a huge
    beam are NaN (0 * inf) and the whole lane is lost: that case fails with the range-based finiteness flag.  At the
    other yaws one coordinate is NaN and the other +-inf, which stretches the box back over the near obstacle."""
    import kompass_hip as kh
    from helpers import assert_cycle_equal, hip_context, hip_cycle, oracle_cycle
    inp = syn.make_controller_inputs("cfg2", seed=4, scale=0.2, scene="open")
    ang, rng = _huge_scan(big)
    cur = dict(inp, state=(0.05, -0.02, yaw, 0.0))
    o = oracle_cycle(cur, scan=(rng, ang))
    far = rng.copy()
    far[3 * len(rng) // 8 + 1] = 8.0
    o_far = oracle_cycle(cur, scan=(far, ang))
    assert len(o["raw"]) > 100 and len(o_far["raw"]) == len(o["raw"])
    assert not np.array_equal(o["costs"], o_far["costs"])
    for opts in (dict(fused_cycle=2), dict(fused_cycle=0, cost_kernel=2), dict(fused_cycle=2, obs_near=0),
                 dict(fused_cycle=0, cost_kernel=2, obs_near=0)):
        ctx = hip_context(kh, cur)
        for k, v in opts.items():
            ctx.set_option(k, v)
        assert_cycle_equal(o, hip_cycle(kh, cur, scan=(rng, ang), ctx=ctx))
        ctx.close()


# ---------------------------------------------------------------------------
# controller: the largest device point list in one bucket cell
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_sensor_rank_packing_at_the_device_maximum():
    """kSensorDeviceMax (2^20) points, all but a few in ONE bucket cell: the ranks inside a workgroup's cell reach
    64 k, packed as id | rank << 12.  Device build (one and two launches) = host build = oracle."""
    import kompass_hip as kh
    from helpers import assert_cycle_equal, hip_context, hip_cycle, oracle_cycle_mt
    n = 1 << 20
    inp = syn.make_controller_inputs("cfg2", seed=1, scale=0.2)
    pts = np.zeros((n, 3), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = 0.9, 0.35, 0.1
    extra = np.float32([[-1.2, 0.4, 0.1], [2.0, -1.5, 0.0], [0.5, -0.6, 0.2], [-0.3, -1.1, 0.1], [3.1, 2.2, 0.1]])
    pts[np.linspace(0, n - 1, len(extra)).astype(int)] = extra
    inp["points"] = pts
    inp["state"] = (0.0, 0.0, 0.1, 0.0)
    o = oracle_cycle_mt(inp)
    assert len(o["raw"]) > 0
    for opt in (None, "sensor_two_launch", "sensor_on_host"):
        ctx = hip_context(kh, inp)
        if opt:
            ctx.set_option(opt, 1)
        assert_cycle_equal(o, hip_cycle(kh, inp, ctx=ctx))
        ctx.close()


# ---------------------------------------------------------------------------
# controller: huge finite coordinates in point lists
# ---------------------------------------------------------------------------
ROBOTS = [(0, [0.1, 0.4]), (1, [0.3, 0.2, 0.4]), (2, [0.15])]


def _edge_points(res, pose):
    """Points at the octree key window (|x / res| < 32768 in sensor_points_kernel) and one cell either side, 1e30,
    FLT_MAX, -0.0 and denormals, among ordinary obstacles around `pose`."""
    px, py = pose
    r = np.random.default_rng(23)
    base = np.column_stack([px + r.uniform(-4, 4, 120), py + r.uniform(-4, 4, 120), r.uniform(-0.1, 0.3, 120)])
    base = base[np.hypot(base[:, 0] - px, base[:, 1] - py) > 1.5]
    w = 32768 * res
    special = []
    for v in (w, -w, w - res, -(w - res), w + res, -(w + res), 1e30, -1e30, FLT_MAX, -FLT_MAX):
        special += [[v, py + 1.0, 0.1], [px + 1.0, v, 0.1], [v, v, 0.1], [px + 0.9, py - 0.7, v]]
    for v in (-0.0, 1e-40, -1e-40, 1e-45):
        special += [[v, py + 0.9, 0.1], [px + 0.8, v, 0.1], [px + 0.7, py + 0.7, v], [v, v, v]]
    return np.vstack([base, np.float32(special)]).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("robot", range(len(ROBOTS)))
@pytest.mark.parametrize("pose", [(0.1, -1.6), (2000.0, -1500.0)])   # the second beyond the key window at 0.05 m
def test_point_lists_with_huge_coordinates(robot, pose):
    """A full cycle on every sensor path (default device build, two launches, host build, split roll-out) for a
    cylinder, a box and a sphere robot: the oracle's admissible set, paths and costs."""
    import kompass_hip as kh
    from helpers import assert_cycle_equal, hip_context, hip_cycle, oracle_cycle
    inp = syn.make_controller_inputs("cfg2", seed=2, scale=0.2)
    shape, dims = ROBOTS[robot]
    inp["robot"] = dict(shape=shape, dims=dims)
    inp["points"] = _edge_points(inp["octree_res"], pose)
    inp["state"] = (pose[0], pose[1], 0.3, 0.0)
    inp["seg_xyz"] = (inp["seg_xyz"] + np.float32([pose[0], pose[1], 0.0])).astype(np.float32)
    o = oracle_cycle(inp)
    for opts in (dict(), dict(sensor_two_launch=1), dict(sensor_on_host=1), dict(force_split=1)):
        ctx = hip_context(kh, inp)
        for k, v in opts.items():
            ctx.set_option(k, v)
        assert_cycle_equal(o, hip_cycle(kh, inp, ctx=ctx))
        ctx.close()


# ---------------------------------------------------------------------------
# point cloud -> laserscan and the critical zone checker
# ---------------------------------------------------------------------------
def _cloud16(xyz):
    rec = np.zeros((len(xyz), 4), np.float32)
    rec[:, :3] = np.asarray(xyz, np.float32)
    return rec.reshape(-1).view(np.int8)


def _extreme_cloud():
    big = [FLT_MAX, -FLT_MAX, 3e19, -3e19, 1.9e19, 1e30]       # x*x overflows to inf beyond ~1.8e19
    tiny = [1e-40, -1e-40, 1e-45, 0.0, -0.0]
    pts = [[a, b, 0.3] for a in big + tiny + [1.0, -2.0] for b in big + tiny + [0.5, -1.5]]
    pts += [[1.0, 0.5, v] for v in big + tiny]
    r = np.random.default_rng(4)
    pts += list(np.column_stack([r.uniform(-6, 6, 500), r.uniform(-6, 6, 500), r.uniform(-0.2, 1.0, 500)]))
    return np.float32(pts)


@pytest.mark.gpu
def test_cloud_to_laserscan_with_huge_and_tiny_coordinates():
    import kompass_hip as kh
    xyz = _extreme_cloud()
    n = len(xyz)
    data = _cloud16(xyz)
    ctx = kh.CloudContext(max_bytes=len(data), max_bins=720)
    for kw in (dict(angle_step=0.0175), dict(num_bins=360)):
        for max_range in (12.0, FLT_MAX):
            want = ko.pointcloud_to_laserscan(data, 16, n * 16, 1, n, 0, 4, 8, max_range, -0.5, 2.0, **kw)
            got = ctx.to_laserscan(data, 16, n * 16, 1, n, 0, 4, 8, max_range, -0.5, 2.0, **kw)
            if "angle_step" in kw:
                np.testing.assert_array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
                got, want = got[0], want[0]
            np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dims", [(0, [0.3, 1.0]), (1, [0.6, 0.4, 1.0]), (2, [0.35])])
def test_zone_checker_with_extreme_ranges_and_points(shape, dims):
    import kompass_hip as kh
    n = 360
    angles = 2.0 * np.pi * np.arange(n) / n
    args = (shape, dims, [0.1, -0.05, 0.3], [0.0, 0.0, np.sin(0.2), np.cos(0.2)], 120.0, 0.2, 0.9, angles, 0.05,
            1.5, 8.0)
    z, o = kh.ZoneContext(*args), ko.CriticalZone(*args)
    r = np.random.default_rng(8)
    for trial in range(24):
        rng = r.uniform(0.3, 3.0, n)
        for k, v in enumerate((np.inf, -np.inf, -0.5, -1e30, DBL_MAX, -DBL_MAX, 1e39, np.nan, 0.0, -0.0, 5e-324)):
            if (trial + k) % 3 == 0:
                rng[r.integers(0, n, 3)] = v
        for fwd in (True, False):
            want, got = o.check(rng, fwd), z.check(rng, fwd)
            assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32), (trial, fwd)
    xyz = _extreme_cloud()
    with np.errstate(over="ignore"):
        outside = xyz[np.hypot(xyz[:, 0], xyz[:, 1]) > 1.0]
    for sub in (xyz, outside):
        c, k = _cloud16(sub), len(sub)
        for fwd in (True, False):
            want = o.check_cloud(c, 16, k * 16, 1, k, 0, 4, 8, fwd)
            got = z.check_cloud(c, 16, k * 16, 1, k, 0, 4, 8, fwd)
            assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32), fwd
