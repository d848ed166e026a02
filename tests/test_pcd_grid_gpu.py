"""Cloud -> occupancy grid on the MI355X (kc_cloud_grid_extent / kc_cloud_grid_fill) against the restatement
pcd_ref.grid: the grid bit for bit, the origin with ==, the cell counts equal, in every case.  Nothing here depends on
the order of the points or on libm, so nothing is tolerated."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kompass_hip as kh
import pcd_ref
import synthetic as syn

pytestmark = pytest.mark.gpu

Z0, ZR = 0.1, 1.0
RESOLUTIONS = [1.0, 0.25, 0.05, 0.013]


@pytest.fixture(scope="module")
def ctx():
    c = kh.CloudContext()
    yield c
    c.close()


def check(ctx, pts, res, zg=Z0, zr=ZR, **kw):
    want, origin = pcd_ref.grid(pts, res, zg, zr)
    got, got_origin = ctx.occupancy_grid(kw.pop("raw", pts), res, zg, zr, **kw)
    assert got.dtype == np.int8 and got.shape == want.shape
    assert [float(v) for v in got_origin] == [float(v) for v in origin]
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8))
    return want


def scattered(n, seed, span=(40.0, 25.0)):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-span[0] / 2, span[0] / 2, n), rng.uniform(-span[1] / 2, span[1] / 2, n),
                     rng.uniform(-0.5, 2.0, n)], axis=1).astype(np.float32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 10**6])
@pytest.mark.parametrize("res", [0.25, 0.05])
def test_sizes(ctx, n, res):
    check(ctx, scattered(n, n), res)


def test_twelve_million_points(ctx):
    want = check(ctx, syn.pcd_indoor_map(12_000_000, seed=3), 0.05)
    assert all((want == v).sum() > 10000 for v in (-1, 0, 100))


@pytest.mark.parametrize("res", RESOLUTIONS)
def test_indoor_map(ctx, res):
    want = check(ctx, syn.pcd_indoor_map(2_000_000 if res >= 0.05 else 300_000, seed=1), res)
    # all three values are exercised where a cell is smaller than the gaps between the points (at 1 m and 0.25 m
    # every cell of the floor holds a ground point)
    assert all((want == v).sum() > 0 for v in ((-1, 0, 100) if res <= 0.05 else (0, 100)))


@pytest.mark.parametrize("res", RESOLUTIONS)
def test_thresholds_swapped(ctx, res):
    want = check(ctx, syn.pcd_indoor_map(200_000, seed=2), res, zg=ZR, zr=Z0)
    assert (want == 100).sum() == 0 and (want == 0).sum() > 0


def test_sparse_outdoor_more_cells_than_points(ctx):
    pts = scattered(5000, 11, span=(900.0, 700.0))
    want = check(ctx, pts, 0.25)
    assert want.size > 1000 * len(pts)


@pytest.mark.parametrize("res", RESOLUTIONS)
def test_every_point_in_one_cell(ctx, res):
    rng = np.random.default_rng(5)
    pts = np.stack([7.0 + rng.uniform(0, 0.9 * res, 100_000), -3.0 + rng.uniform(0, 0.9 * res, 100_000),
                    rng.uniform(-0.5, 2.0, 100_000)], axis=1).astype(np.float32)
    want = check(ctx, pts, res)
    assert want.shape == (1, 1) and want[0, 0] == 100
    check(ctx, pts[pts[:, 2] <= Z0], res)
    check(ctx, pts[pts[:, 2] > ZR], res)


@pytest.mark.parametrize("res", [1.0, 0.25, 0.05])
def test_extent_an_exact_multiple_and_points_on_cell_edges(ctx, res):
    r = np.float32(res)
    k = np.arange(0, 201, dtype=np.float32)
    for base in (np.float32(0.0), np.float32(-37.5), np.float32(1000.0)):
        e = base + k * r  # min + k * res in float
        X, Y = np.meshgrid(e, e[:101], indexing="ij")
        rng = np.random.default_rng(int(abs(base)))
        pts = np.stack([X.ravel(), Y.ravel(), rng.uniform(-0.5, 2.0, X.size).astype(np.float32)], axis=1)
        want = check(ctx, pts.astype(np.float32), res)
        if base == 0.0 and res in (1.0, 0.25):
            assert want.shape == (200, 100)  # the points on the max edges are dropped


@pytest.mark.parametrize("frac", [0.001, 0.5])
def test_non_finite_points(ctx, frac):
    pts = syn.pcd_indoor_map(400_000, seed=4)
    rng = np.random.default_rng(6)
    bad = rng.random(len(pts)) < frac
    kind = rng.integers(0, 6, len(pts))
    for k, (col, v) in enumerate([(0, np.nan), (1, np.nan), (0, np.inf), (1, -np.inf), (2, np.nan), (2, np.inf)]):
        pts[bad & (kind == k), col] = v
    pts[bad & (kind == 0), 1] = 1e6  # a finite y next to a NaN x must not widen the box
    check(ctx, pts, 0.05)
    organised = pts.copy()
    organised[::2] = np.nan
    check(ctx, organised, 0.25)
    check(ctx, np.full((1000, 3), np.nan, np.float32), 0.25)
    check(ctx, np.array([[np.inf, 0, 0], [0, np.nan, 0]], np.float32), 0.25)


@pytest.mark.parametrize("res", [0.25, 0.05])
def test_negative_and_large_coordinates(ctx, res):
    pts = syn.pcd_indoor_map(300_000, seed=7)
    for shift in ((-250.0, -80.0), (1e5, -1e5), (-99990.0, 1e5)):
        check(ctx, (pts + np.array([shift[0], shift[1], 0.0], np.float32)).astype(np.float32), res)
    # all points on one line: an empty grid with the origin of the minimum
    line = pts.copy()
    line[:, 1] = 4.5
    want = check(ctx, line, res)
    assert want.size == 0 and want.shape[0] > 0


def records(pts, step, offs, seed=0):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 255, (len(pts), step), dtype=np.uint8)
    for k in range(3):
        raw[:, offs[k]:offs[k] + 4] = np.ascontiguousarray(pts[:, k]).view(np.uint8).reshape(-1, 4)
    return raw.reshape(-1).view(np.int8)


@pytest.mark.parametrize("step,offs", [(16, (0, 4, 8)), (16, (4, 8, 12)), (32, (20, 4, 12)), (32, (2, 9, 21)),
                                       (12, (8, 0, 4)), (13, (1, 5, 9))])
def test_strided_records(ctx, step, offs):
    for n in (1, 65, 100_003):
        pts = syn.pcd_indoor_map(n, seed=8) if n > 100 else scattered(n, 9)
        check(ctx, pts, 0.05, raw=records(pts, step, offs), point_step=step, offsets=offs, n_points=n)
    # a last record that ends right after its z
    pts = scattered(1000, 10)
    raw = records(pts, step, offs)
    check(ctx, pts, 0.25, raw=raw[:(len(pts) - 1) * step + max(offs) + 4].copy(), point_step=step, offsets=offs,
          n_points=len(pts))
    with pytest.raises(ValueError):  # one byte less: refused, nothing is read
        ctx.occupancy_grid(raw[:(len(pts) - 1) * step + max(offs) + 3].copy(), 0.25, Z0, ZR, point_step=step,
                           offsets=offs, n_points=len(pts))


def test_unaligned_packed_host_array(ctx):
    pts = syn.pcd_indoor_map(50_001, seed=12)
    buf = np.zeros(pts.nbytes + 16, np.int8)
    for shift in (0, 4, 1):
        view = buf[shift:shift + pts.nbytes]
        view[:] = pts.reshape(-1).view(np.int8)
        check(ctx, pts, 0.05, raw=view, n_points=len(pts))


def test_same_context_after_larger_and_smaller_clouds():
    c = kh.CloudContext()
    small, large = scattered(3000, 20, span=(10.0, 6.0)), syn.pcd_indoor_map(1_500_000, seed=21)
    medium = scattered(200_000, 22, span=(60.0, 30.0))
    first = check(c, small, 0.05)
    for pts, res in ((large, 0.05), (small, 0.05), (medium, 0.25), (large, 0.25), (medium, 0.05), (small, 0.05)):
        again = check(c, pts, res)
    np.testing.assert_array_equal(first, again)
    c.close()


def test_grid_stays_on_the_device(ctx):
    pts = syn.pcd_indoor_map(100_000, seed=23)
    want, _ = pcd_ref.grid(pts, 0.05, Z0, ZR)
    dev, shape, origin = ctx.occupancy_grid(pts, 0.05, Z0, ZR, to_host=False)
    assert dev and shape == want.shape
    # copied back with the HIP runtime the library itself is linked to
    import ctypes
    memcpy = kh.lib().hipMemcpy
    memcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    memcpy.restype = ctypes.c_int
    out = np.empty(want.size, np.int8)
    assert memcpy(out.ctypes.data, dev, out.size, 2) == 0  # hipMemcpyDeviceToHost
    np.testing.assert_array_equal(out.reshape(want.shape, order="F"), want)


def test_range_errors_before_any_launch():
    c = kh.CloudContext()
    c.timing_enable(True)
    pts = scattered(1000, 30)
    for res in (0.0, -1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError):
            c.occupancy_grid(pts, res, Z0, ZR)
        o = np.zeros(3, np.float32)
        import ctypes as C
        cx, cy = C.c_int(7), C.c_int(7)
        rc = kh.lib().kc_cloud_grid_extent(c.h, pts.ctypes.data, pts.nbytes, 0, 12, len(pts), 0, 4, 8, res,
                                           o.ctypes.data_as(C.POINTER(C.c_float)), C.byref(cx), C.byref(cy))
        assert rc == -2 and (cx.value, cy.value) == (0, 0)  # KC_ERR_RANGE
    assert c.timings() == []  # nothing was launched
    with pytest.raises(kh.KompassHipError):  # KC_ERR_STATE: no extent to fill
        kh._check(kh.lib().kc_cloud_grid_fill(c.h, Z0, ZR, None, 0))
    # above the cell cap: refused on the host after the bounding box, before the grid is allocated or filled
    far = np.array([[0, 0, 0], [1e6, 1e6, 0]], np.float32)
    for p, res in ((far, 0.001), (np.array([[-3e38, 0, 0], [3e38, 1, 0]], np.float32), 1.0), (far, 1e-30)):
        with pytest.raises(IndexError):
            pcd_ref.grid(p, res, Z0, ZR)
        with pytest.raises(IndexError):
            c.occupancy_grid(p, res, Z0, ZR)
        names = [n for n, _ in c.timings()]
        assert "cloud_grid_scatter_kernel" not in names and "cloud_grid_clear" not in names
        with pytest.raises(kh.KompassHipError):
            kh._check(kh.lib().kc_cloud_grid_fill(c.h, Z0, ZR, None, 0))
    check(c, pts, 0.05)  # and the context still works
    assert [n for n, _ in c.timings() if not n.startswith("host:")] == [
        "cloud_extent_kernel", "cloud_grid_clear", "cloud_grid_scatter_kernel", "cloud_grid_decode_kernel"]
    c.close()


def test_pcd_file_end_to_end(tmp_path):
    import kompass_cpp
    from kompass_core.datatypes import get_occupancy_grid_from_pcd, get_points_from_pcd

    pts = syn.pcd_indoor_map(250_000, seed=31)
    pts[::1000, 0] = np.nan
    f = tmp_path / "map.pcd"
    rng = np.random.default_rng(1)
    pcd_ref.write_pcd(f, ["x", "y", "z", "intensity"], [4, 4, 4, 4], ["F"] * 4,
                      [pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy(), rng.random(len(pts)).astype(np.float32)], True)
    np.testing.assert_array_equal(get_points_from_pcd(str(f)).view(np.uint32), pts.view(np.uint32))
    for res in (0.05, 0.25):
        want, origin = pcd_ref.grid(pcd_ref.read(f), res, Z0, ZR)
        for fn in (kompass_cpp.utils.read_pcd_to_occupancy_grid, get_occupancy_grid_from_pcd):
            grid, o = fn(str(f), res, Z0, ZR)
            assert grid.dtype == np.int8 and grid.shape == want.shape and len(o) == 3
            assert [float(v) for v in o] == [float(v) for v in origin]
            np.testing.assert_array_equal(np.asarray(grid).view(np.uint8), want.view(np.uint8))
            i, j = np.argwhere(want == 100)[0]
            assert grid[i, j] == 100  # grid[i, j] is the cell (i, j)
        grid, o = kompass_cpp.utils.points_to_occupancy_grid(pts, res, Z0, ZR)
        np.testing.assert_array_equal(np.asarray(grid).view(np.uint8), want.view(np.uint8))
    for name in ("pcd_room_ascii.pcd", "pcd_room_binary.pcd"):
        g = Path(__file__).resolve().parent / "golden" / name
        want, origin = pcd_ref.grid(pcd_ref.read(g), 0.25, Z0, ZR)
        grid, o = get_occupancy_grid_from_pcd(str(g), 0.25, Z0, ZR)
        np.testing.assert_array_equal(np.asarray(grid), want)
        assert [float(v) for v in o] == [float(v) for v in origin]
    empty = tmp_path / "empty.pcd"
    pcd_ref.write_pcd(empty, ["x", "y", "z"], [4] * 3, ["F"] * 3, [np.zeros(0, np.float32)] * 3, True)
    grid, o = get_occupancy_grid_from_pcd(str(empty), 0.25, Z0, ZR)
    assert grid.shape == (0, 0) and [float(v) for v in o] == [0.0, 0.0, 0.0]


def test_concurrent_callers_of_the_module_functions():
    """The module functions release the GIL and share one hidden context whose grid state spans several C-ABI calls:
    callers on several threads are serialised by the context's lock, each gets its own grid.  Clouds of
    different sizes and extents, so that a caller that saw another's extent or upload would get a wrong shape or
    wrong cells; laserscan calls on the same context run beside them."""
    import threading

    import kompass_cpp

    clouds = [scattered(3000, 50, span=(10.0, 6.0)), syn.pcd_indoor_map(400_000, seed=51),
              scattered(150_000, 52, span=(60.0, 30.0)), scattered(1, 53), syn.pcd_indoor_map(900_000, seed=54),
              np.zeros((0, 3), np.float32)]
    want = [pcd_ref.grid(c, 0.05, Z0, ZR) for c in clouds]
    scan_cloud = scattered(20_000, 55).copy()
    scan_args = (list(scan_cloud.reshape(-1).view(np.int8)), 12, 12 * len(scan_cloud), 1, len(scan_cloud), 0, 4, 8, 30.0,
                 -1.0, 3.0, 360)
    scan_want = kompass_cpp.utils.pointcloud_to_laserscan_from_raw(*scan_args)
    errors = []

    def grids(k):
        try:
            for r in range(6):
                i = (k + r) % len(clouds)
                g, o = kompass_cpp.utils.points_to_occupancy_grid(clouds[i], 0.05, Z0, ZR)
                assert g.shape == want[i][0].shape and [float(v) for v in o] == [float(v) for v in want[i][1]]
                np.testing.assert_array_equal(np.asarray(g).view(np.uint8), want[i][0].view(np.uint8))
        except BaseException as e:  # noqa: BLE001
            errors.append(repr(e))

    def scans():
        try:
            for _ in range(4):
                assert kompass_cpp.utils.pointcloud_to_laserscan_from_raw(*scan_args) == scan_want
        except BaseException as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=grids, args=(k,)) for k in range(6)] + [threading.Thread(target=scans)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not any(t.is_alive() for t in threads) and not errors, errors


def test_torch_device_tensor_gives_the_host_bits():
    """A torch tensor needs torch's HIP runtime to be the process's only one (torch imported before kompass_cpp,
    DESIGN.md 4.8): the check runs in a fresh process, _torch_pcd_worker.py."""
    pytest.importorskip("torch")
    worker = Path(__file__).resolve().parent / "_torch_pcd_worker.py"
    p = subprocess.run([sys.executable, str(worker)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]
