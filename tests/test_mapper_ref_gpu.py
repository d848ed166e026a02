"""GPU: every device path of the mapper against tests/mapper_ref.py (the literal restatement of LocalMapper and
bresenhamEnhanced), not against the oracle: the kernels and the oracle share one derivation of the clipped walk,
so only an independent walk can catch a slip made in it.

The geometry classes of tests/test_mapper_ref_cpu.py run under every KC_MAPPER_TILES (0..3) x KC_MAPPER_STAGED
(0/1), plain and Bayesian; then the exact call sequences bench.py times (--mapper, --mapper --bayes, --ref
mapper400) at its sizes, read back through the device pointers; then sensors far from the grid."""
import ctypes

import numpy as np
import pytest

import mapper_ref as mr
import synthetic as syn
from oracle import ko
from test_mapper_ref_cpu import (BAYES, FAR, RES, WALL, _bits, _random_scene, bayes_edge_scene, far_scene,
                                 slope_half_scene)

pytestmark = pytest.mark.gpu

TILES = ["0", "1", "2", "3"]


class Hip:
    """hipMemcpy through the HIP runtime directly: reads a device buffer this library owns."""

    def __init__(self):
        self.lib = ctypes.CDLL("libamdhip64.so")
        self.lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.lib.hipDeviceSynchronize.argtypes = []

    def read(self, ptr, H, W, dtype):
        """A column-major [H, W] device grid (cell (i, j) at i + j H) -> [H, W]."""
        out = np.empty(H * W, dtype)
        assert ptr
        assert self.lib.hipDeviceSynchronize() == 0
        assert self.lib.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(ptr), out.nbytes, 2) == 0
        return out.reshape(W, H).T


def _ctx(monkeypatch, tiles, staged, H, W, res, pos, n, bayes=None):
    import kompass_hip as kh
    monkeypatch.setenv("KC_MAPPER_TILES", tiles)
    monkeypatch.setenv("KC_MAPPER_STAGED", staged)
    m = kh.MapperContext(H, W, res, pos, 0.0, max(n, 1))
    if bayes:
        m.enable_bayes(**bayes)
    return m


# ---------------------------------------------------------------------------
# geometry classes, every path (expected grids computed once per module)
# ---------------------------------------------------------------------------
def _scenes():
    out = []
    # short lines from the border cells and 1, 2, 3 cells outside (one scan per sensor), 1 x N and N x 1 included
    for H, W in [(12, 9), (1, 13), (13, 1)]:
        for s in mr.border_and_outside_cells(H, W, dists=(1, 2, 3, 64)):
            pos = mr.sensor_pos(H, W, RES, s)
            ang, rng, _ = mr.aim(H, W, RES, pos, [(s[0] + a, s[1] + b) for a in range(-7, 8, 2)
                                                  for b in range(-7, 8, 3)])
            out.append((H, W, pos, ang, rng))
    r = np.random.default_rng(21)
    out += [_random_scene(r) for _ in range(100)]
    return out


@pytest.fixture(scope="module")
def expected():
    r = np.random.default_rng(4)
    res = []
    for H, W, pos, ang, rng in _scenes():
        prev = r.uniform(0.05, 0.95, (H, W)).astype(np.float32)
        g = mr.scan_to_grid(H, W, RES, pos, 0.0, ang, rng)
        bg, bp = mr.scan_to_grid_baysian(H, W, RES, pos, 0.0, ang, rng, prev, WALL)
        res.append((H, W, pos, ang, rng, prev, g, bg, bp))
    return res


@pytest.mark.parametrize("staged", ["0", "1"])
@pytest.mark.parametrize("tiles", TILES)
def test_geometry_classes_every_path(tiles, staged, expected, monkeypatch):
    for k, (H, W, pos, ang, rng, prev, g, bg, bp) in enumerate(expected):
        m = _ctx(monkeypatch, tiles, staged, H, W, RES, pos, len(ang), WALL)
        np.testing.assert_array_equal(m.scan_to_grid(ang, rng), g, err_msg=f"scene {k}")
        m.set_previous_prob(prev)
        got_g, got_p = m.scan_to_grid_baysian(ang, rng)
        np.testing.assert_array_equal(got_g, bg, err_msg=f"scene {k}")
        np.testing.assert_array_equal(_bits(got_p), _bits(bp), err_msg=f"scene {k}")
        m.close()


def test_short_lines_one_at_a_time(monkeypatch):
    """Every line from 7 x 7 offsets around the border and outside cells of a 12 x 9 grid, one scan per line (a cell
    one line misses cannot hide under another's)."""
    H, W = 12, 9
    for s in mr.border_and_outside_cells(H, W, dists=(1, 2)):
        pos = mr.sensor_pos(H, W, RES, s)
        ang, rng, _ = mr.aim(H, W, RES, pos, [(s[0] + a, s[1] + b) for a in range(-3, 4) for b in range(-3, 4)])
        m = _ctx(monkeypatch, "0", "0", H, W, RES, pos, 1)
        for k in range(len(ang)):
            np.testing.assert_array_equal(m.scan_to_grid(ang[k:k + 1], rng[k:k + 1]),
                                          mr.scan_to_grid(H, W, RES, pos, 0.0, ang[k:k + 1], rng[k:k + 1]),
                                          err_msg=f"sensor {s} beam {k}")
        m.close()


# ---------------------------------------------------------------------------
# the call sequences bench.py times, at its sizes
# ---------------------------------------------------------------------------
def test_bench_mapper_sequence():
    """--mapper: 4096 beams into 1000 x 1000, scan_to_grid_device + sync eight times (the context alternates
    between two device grids), the grid read through grid_device_ptr after the last two."""
    import kompass_hip as kh
    H = W = 1000
    ang, rng = syn.dense_scan(4096, 4.0)
    scans = [rng * (1.0 + 0.01 * ((i % 5) - 2)) for i in range(8)]
    m = kh.MapperContext(H, W, 0.05, (0, 0, 0), 0.0, 4096)
    hip = Hip()
    for i in range(8):
        m.scan_to_grid_device(ang, scans[i])
        m.sync()
        if i >= 6:
            np.testing.assert_array_equal(hip.read(m.grid_device_ptr(), H, W, np.int32),
                                          mr.scan_to_grid(H, W, 0.05, (0, 0, 0), 0.0, ang, scans[i]),
                                          err_msg=f"scan {i}")
    m.close()


def test_bench_bayes_sequence():
    """--mapper --bayes: ten steps of warp -> Bayesian scan on the device -> feed the probabilities back -> sync,
    nothing read in between; then the grid, the probabilities (prob_device_ptrs) and previous_prob()."""
    import kompass_hip as kh
    H = W = 1000
    params = dict(p_prior=0.6, p_occupied=0.9, p_empty=0.1, range_sure=0.1, range_max=20.0, wall_size=0.2)
    ang, rng = syn.dense_scan(4096, 4.0)
    scans = [rng * (1.0 + 0.01 * ((i % 5) - 2)) for i in range(8)]
    pose = lambda i: ((0.01 * (i % 7), -0.005 * (i % 5)), 0.002 * (i % 11))
    m = kh.MapperContext(H, W, 0.05, (0, 0, 0), 0.0, 4096)
    m.enable_bayes(**params)
    o = ko.BayesMapper(H, W, 0.05, (0, 0, 0), 0.0, **params)   # for the inverted matrix only
    prev = np.full((H, W), np.float32(params["p_prior"]), np.float32)
    for i in range(10):
        m.get_previous_grid_in_current_pose(*pose(i))
        m.scan_to_grid_baysian_device(ang, scans[i % 8])
        m.set_previous_prob(None)
        m.sync()
        prev = mr.warp_previous(prev, o.warp_matrix(*pose(i)), params["p_prior"])
        g, p = mr.scan_to_grid_baysian(H, W, 0.05, (0, 0, 0), 0.0, ang, scans[i % 8], prev, params)
        prev = p
    hip = Hip()
    np.testing.assert_array_equal(hip.read(m.grid_device_ptr(), H, W, np.int32), g)
    np.testing.assert_array_equal(_bits(hip.read(m.prob_device_ptrs()[0], H, W, np.float32)), _bits(p))
    np.testing.assert_array_equal(_bits(m.previous_prob()), _bits(p))
    assert len(np.unique(p)) > 100
    m.close()


def test_bench_ref_mapper400_sequence():
    """--ref mapper400: 3600 beams into 400 x 400, scan_to_grid_device + sync, read through grid_device_ptr."""
    import kompass_hip as kh
    g = syn.REF_MAPPER400
    H, W, res, n = g["height"], g["width"], g["res"], g["beams"]
    ang, rng = syn.dense_scan(n, 1.0)
    want = mr.scan_to_grid(H, W, res, (0, 0, 0), 0.0, ang, rng)
    m = kh.MapperContext(H, W, res, (0, 0, 0), 0.0, n)
    hip = Hip()
    for _ in range(3):
        m.scan_to_grid_device(ang, rng)
        m.sync()
        np.testing.assert_array_equal(hip.read(m.grid_device_ptr(), H, W, np.int32), want)
    m.close()


# ---------------------------------------------------------------------------
# sensors far from the grid
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def far_expected(tmp_path_factory):
    if not mr.have_gxx():
        pytest.skip("needs g++")
    walker = mr.native_walker(mr.build_native(tmp_path_factory.mktemp("bresenham_literal")))
    out = []
    for dist in FAR:
        H, W = (33, 45) if dist < 2 ** 25 else (301, 299)
        for side in (((-1, 0), (1, 1)) if dist < 2 ** 30 - 1024 else ((-1, 0),)):
            pos, ang, rng = far_scene(dist, side, H, W)
            prev = np.random.default_rng(dist).uniform(0.05, 0.95, (H, W)).astype(np.float32)
            g, p = mr.scan_to_grid_baysian(H, W, 1.0, pos, 0.0, ang, rng, prev, WALL, walker)
            assert (g >= 0).sum() > 10
            out.append((dist, H, W, pos, ang, rng, prev, g, p))
    # |slope| exactly 1/2 from 2^27 cells: the closed-form start needs its remainder test; and the Bayesian cell
    # pass on either side of its switch from the int square to the 64-bit one
    scenes = [("slope 1/2", slope_half_scene())] + [(f"span {v}", bayes_edge_scene(v)) for v in (2 ** 15 - 1, 2 ** 15)]
    for name, (H, W, pos, ang, rng) in scenes:
        prev = np.random.default_rng(len(name)).uniform(0.05, 0.95, (H, W)).astype(np.float32)
        g, p = mr.scan_to_grid_baysian(H, W, 1.0, pos, 0.0, ang, rng, prev, WALL, walker)
        assert (g >= 0).sum() > 30
        out.append((name, H, W, pos, ang, rng, prev, g, p))
    return out


@pytest.mark.parametrize("tiles", TILES)
def test_far_sensors(tiles, far_expected, monkeypatch):
    """Sensors 46 340 / 46 341 cells from the grid centre, 2 * 10^6, 2^25 and just below 2^30; a line of |slope|
    exactly 1/2 from 2^27 cells; the Bayesian cell pass with the far corner 2^15 - 1 and 2^15 cells out."""
    for dist, H, W, pos, ang, rng, prev, g, p in far_expected:
        m = _ctx(monkeypatch, tiles, "0", H, W, 1.0, pos, len(ang), WALL)
        np.testing.assert_array_equal(m.scan_to_grid(ang, rng), g, err_msg=f"{dist}")
        m.set_previous_prob(prev)
        got_g, got_p = m.scan_to_grid_baysian(ang, rng)
        np.testing.assert_array_equal(got_g, g, err_msg=f"{dist}")
        np.testing.assert_array_equal(_bits(got_p), _bits(p), err_msg=f"{dist}")
        m.close()


def test_sensor_at_2_30_cells_is_refused():
    import kompass_hip as kh
    for p in [(2.0 ** 30, 0.0, 0.0), (0.0, -(2.0 ** 30), 0.0), (np.inf, 0, 0), (np.nan, 0, 0)]:
        with pytest.raises(IndexError):   # KC_ERR_RANGE
            kh.MapperContext(10, 10, 1.0, p, 0.0, 4)
    kh.MapperContext(10, 10, 1.0, (2.0 ** 30 - 128, 0, 0), 0.0, 4).close()
