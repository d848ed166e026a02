"""PCD maps without a device: the reader (kompass_cpp.utils.read_pcd) against files written here and against the
restatement pcd_ref.read, bit for bit; every malformed case as RuntimeError; the two committed fixtures; the
restatement of the occupancy grid (pcd_ref.grid, the yardstick of test_pcd_grid_gpu.py) against grids worked out by
hand; the kompass_core.datatypes front end; and no CPU fallback for the grid."""
import json
from pathlib import Path

import numpy as np
import pytest

import kompass_cpp
import kompass_hip as kh
import pcd_ref
from kompass_cpp.utils import read_pcd

GOLDEN = Path(__file__).resolve().parent / "golden"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def cloud(n, seed=0):
    rng = np.random.default_rng(seed)
    p = rng.normal(0, 30, (n, 3)).astype(np.float32)
    if n > 4:
        p[1] = [np.nan, 1.0, -0.0]
        p[2] = [np.inf, -np.inf, 1e-42]          # a subnormal z
        p[3] = [3.4028235e38, -1.17549435e-38, 0.1]
    return p


def check_read(path, expect):
    got = read_pcd(str(path))
    assert got.dtype == np.float32 and got.shape == expect.shape
    np.testing.assert_array_equal(bits(got), bits(expect))
    np.testing.assert_array_equal(bits(pcd_ref.read(path)), bits(expect))
    return got


def text(col):
    return ["nan" if np.isnan(v) else "%.9g" % v for v in col]


# ------------------------------------------------------------------ reader: well-formed files
@pytest.mark.parametrize("n", [0, 1, 50])
def test_binary_xyz(tmp_path, n):
    p = cloud(n)
    f = tmp_path / "a.pcd"
    pcd_ref.write_pcd(f, ["x", "y", "z"], [4, 4, 4], ["F"] * 3, [p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()], True)
    got = check_read(f, p)
    assert got.flags.c_contiguous and (n == 0 or not got.flags.owndata)  # a view of the reader's vector: no second copy


def test_binary_extra_fields_of_every_size(tmp_path):
    p = cloud(40, 1)
    rng = np.random.default_rng(2)
    cols = [rng.integers(0, 255, 40).astype(np.uint8), p[:, 2].copy(), rng.integers(0, 9999, 40).astype(np.uint16),
            rng.normal(size=40).astype(np.float32), p[:, 0].copy(), rng.normal(size=40), p[:, 1].copy(),
            rng.integers(0, 255, 40).astype(np.uint8)]
    f = tmp_path / "b.pcd"
    pcd_ref.write_pcd(f, ["label", "z", "ring", "intensity", "x", "t", "y", "flag"], [1, 4, 2, 4, 4, 8, 4, 1],
                      ["U", "F", "U", "F", "F", "F", "F", "U"], cols, True)
    check_read(f, p)


@pytest.mark.parametrize("newline", ["\n", "\r\n"])
def test_ascii_xyz(tmp_path, newline):
    p = cloud(30, 3)
    f = tmp_path / "c.pcd"
    pcd_ref.write_pcd(f, ["x", "y", "z"], [4, 4, 4], ["F"] * 3, [text(p[:, 0]), text(p[:, 1]), text(p[:, 2])], False,
                      newline=newline, comments=["# a comment", "#another", "NOBLANKLINE"])
    check_read(f, p)


def test_ascii_fields_by_index(tmp_path):
    """x y z intensity, and z x y: the reference takes the first three tokens of a running stream; here the fields go
    by their index"""
    p = cloud(25, 4)
    inten = [str(i) for i in range(25)]
    f = tmp_path / "d.pcd"
    pcd_ref.write_pcd(f, ["x", "y", "z", "intensity"], [4] * 4, ["F"] * 4,
                      [text(p[:, 0]), text(p[:, 1]), text(p[:, 2]), inten], False)
    check_read(f, p)
    g = tmp_path / "e.pcd"
    pcd_ref.write_pcd(g, ["z", "x", "y"], [4] * 3, ["F"] * 3, [text(p[:, 2]), text(p[:, 0]), text(p[:, 1])], False)
    check_read(g, p)


def test_ascii_number_rules(tmp_path):
    """std::from_chars<float>: one rounding; subnormals; out of range and unparsable tokens leave 0"""
    toks = ["1e-45", "1e-40", "1.17549435e-38", "3.4028235e38", "1e39", "-1e39", "3.4028236e38", "1e-46", "nan", "-0.0",
            "0.100000001", "16777217", "1.00000012", "0.333333343", "abc", "-inf", "inf", ".5", "5.",
            "123456789.123456789", "-7.00649232e-46", "2.5e-1", "NaN"]
    want = {"1e39": 0.0, "-1e39": 0.0, "3.4028236e38": 0.0, "1e-46": 0.0, "abc": 0.0, "-7.00649232e-46": 0.0}
    col = np.array([np.float32(want[t]) if t in want else np.float32(t) for t in toks], np.float32)
    assert col[0].view(np.uint32) == 1 and col[1].view(np.uint32) == 0x000116C2 and np.isnan(col[8])
    assert np.signbit(col[9]) and col[11] == 16777216.0
    n = len(toks)
    p = np.stack([col, np.roll(col, 1), np.roll(col, 2)], axis=1)
    f = tmp_path / "f.pcd"
    pcd_ref.write_pcd(f, ["x", "y", "z"], [4] * 3, ["F"] * 3,
                      [toks, list(np.roll(np.array(toks, object), 1)), list(np.roll(np.array(toks, object), 2))], False)
    assert check_read(f, p).shape == (n, 3)


def test_ascii_partly_numeric_tokens(tmp_path):
    """from_chars stops at the first character that cannot continue the number and the reader, like the reference,
    does not look at where it stopped: the longest numeric prefix counts.  Values by hand."""
    toks = ["1.5abc", "1e", "2.5e+", "-3.25x7", "0x10", "7,5", "1.2.3", "nan(7)", "infinity", "-infx", "+1.5", "e5",
            "--2", "-.5e1q", "1e39z"]
    want = [1.5, 1.0, 2.5, -3.25, 0.0, 7.0, 1.2, np.nan, np.inf, -np.inf, 0.0, 0.0, 0.0, -5.0, 0.0]
    col = np.array(want, np.float32)
    for t, w in zip(toks, col):
        assert bits(pcd_ref.parse_float(t)) == bits(w), t
    p = np.stack([col, col[::-1], np.roll(col, 3)], axis=1)
    f = tmp_path / "k.pcd"
    pcd_ref.write_pcd(f, ["x", "y", "z"], [4] * 3, ["F"] * 3,
                      [toks, toks[::-1], list(np.roll(np.array(toks, object), 3))], False)
    check_read(f, p)


def test_repeated_field_name_takes_the_last(tmp_path):
    """FIELDS x y z x: the reference's loop overwrites x_idx, so the last x is the one that is read"""
    p = cloud(15, 10)
    other = np.arange(15, dtype=np.float32)
    for binary in (True, False):
        f = tmp_path / f"l{int(binary)}.pcd"
        cols = [other, p[:, 1].copy(), p[:, 2].copy(), p[:, 0].copy()]
        pcd_ref.write_pcd(f, ["x", "y", "z", "x"], [4] * 4, ["F"] * 4, cols if binary else [text(c) for c in cols],
                          binary)
        check_read(f, p)


def test_data_line_with_trailing_blanks(tmp_path):
    p = cloud(10, 5)
    f = tmp_path / "g.pcd"
    pcd_ref.write_pcd(f, ["x", "y", "z"], [4] * 3, ["F"] * 3, [p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()], True,
                      data_tag="binary  ", newline="\r\n")
    check_read(f, p)


def test_golden_fixtures():
    want = np.array(json.loads((GOLDEN / "pcd_room_expected.json").read_text())["points_f32_bits"], np.uint32)
    for name in ("pcd_room_ascii.pcd", "pcd_room_binary.pcd"):
        got = read_pcd(str(GOLDEN / name))
        np.testing.assert_array_equal(bits(got), want)
        np.testing.assert_array_equal(bits(pcd_ref.read(GOLDEN / name)), want)


# ------------------------------------------------------------------ reader: malformed files
def _xyz(p):
    return [p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()]


def malformed(tmp_path):
    p = cloud(20, 6)
    out = {}

    def mk(name, *a, **k):
        out[name] = tmp_path / (name + ".pcd")
        pcd_ref.write_pcd(out[name], *a, **k)

    mk("truncated_binary", ["x", "y", "z"], [4] * 3, ["F"] * 3, _xyz(p), True)
    out["truncated_binary"].write_bytes(out["truncated_binary"].read_bytes()[:-5])
    mk("points_beyond_binary", ["x", "y", "z"], [4] * 3, ["F"] * 3, _xyz(p), True, points=10**12)
    mk("points_beyond_ascii", ["x", "y", "z"], [4] * 3, ["F"] * 3, [text(c) for c in _xyz(p)], False, points=21)
    mk("points_huge_ascii", ["x", "y", "z"], [4] * 3, ["F"] * 3, [text(c) for c in _xyz(p)], False, points=2**62)
    mk("missing_z", ["x", "y", "w"], [4] * 3, ["F"] * 3, _xyz(p), True)
    mk("fields_size_mismatch", ["x", "y", "z", "i"], [4] * 3, ["F"] * 3, _xyz(p), True)
    mk("binary_compressed", ["x", "y", "z"], [4] * 3, ["F"] * 3, _xyz(p), True, data_tag="binary_compressed")
    mk("count_3", ["x", "y", "z", "normal"], [4] * 4, ["F"] * 4, _xyz(p) + [p[:, 0].copy()], True, counts=[1, 1, 1, 3])
    mk("double_xyz", ["x", "y", "z"], [8] * 3, ["F"] * 3, [c.astype(np.float64) for c in _xyz(p)], True)
    mk("no_data_line", ["x", "y", "z"], [4] * 3, ["F"] * 3, _xyz(p), True)
    raw = out["no_data_line"].read_bytes()
    out["no_data_line"].write_bytes(raw[:raw.index(b"DATA")])
    mk("no_points_line", ["x", "y", "z"], [4] * 3, ["F"] * 3, _xyz(p), True)
    out["no_points_line"].write_bytes(out["no_points_line"].read_bytes().replace(b"POINTS 20\n", b""))
    mk("bad_points", ["x", "y", "z"], [4] * 3, ["F"] * 3, _xyz(p), True)
    out["bad_points"].write_bytes(out["bad_points"].read_bytes().replace(b"POINTS 20\n", b"POINTS many\n"))
    out["absent"] = tmp_path / "absent.pcd"
    return out


CASES = ["truncated_binary", "points_beyond_binary", "points_beyond_ascii", "points_huge_ascii", "missing_z",
         "fields_size_mismatch", "binary_compressed", "count_3", "double_xyz", "no_data_line", "no_points_line",
         "bad_points", "absent"]


@pytest.mark.parametrize("case", CASES)
def test_malformed_is_runtime_error(tmp_path, case):
    path = malformed(tmp_path)[case]
    with pytest.raises(RuntimeError, match="Failed to read PCD file"):
        read_pcd(str(path))
    with pytest.raises(RuntimeError, match="Failed to read PCD file"):
        kompass_cpp.utils.read_pcd_to_occupancy_grid(str(path), 0.1, 0.1, 1.0)  # the reader fails before any device use
    if case != "absent":
        with pytest.raises(pcd_ref.PcdError):
            pcd_ref.read(path)


# ------------------------------------------------------------------ the restatement of the grid, by hand
Z0, ZR = 0.1, 1.0  # z_ground_limit, robot_height


def test_ref_square():
    """(0,0) (1,0) (0,1) (1,1) at 0.25 m: ceil(1 / 0.25) = 4 cells an axis; (int)(1 * 4) = 4 is outside [0, 4), so
    the three points with a coordinate on the max edge are dropped and only cell (0, 0) holds a point"""
    g, o = pcd_ref.grid([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], 0.25, Z0, ZR)
    want = np.full((4, 4), -1, np.int8)
    want[0, 0] = 0
    np.testing.assert_array_equal(g, want)
    assert list(o) == [0.0, 0.0, 0.0]


def test_ref_classes_and_maximum():
    """a 3 x 2 m cloud at 1 m (the corner points only span it and are overhead, class -1)"""
    span = [[0, 0, 5], [3.5, 2.5, 5]]  # 4 x 3 cells; (3.5, 2.5) is in cell (3, 2)

    def one(zs, cell=(1, 1)):
        pts = span + [[cell[0] + 0.5, cell[1] + 0.5, z] for z in zs]
        g, o = pcd_ref.grid(pts, 1.0, Z0, ZR)
        assert g.shape == (4, 3) and list(o) == [0.0, 0.0, 0.0]
        assert (g == -1).sum() == 11 or g[cell] == -1
        return int(g[cell])

    assert one([0.0, 0.5, 2.0]) == 100      # ground + occupied + overhead
    assert one([2.0, 0.5, 0.0]) == 100      # ... in any order
    assert one([0.0, 2.0]) == 0             # ground + overhead
    assert one([2.0]) == -1                 # overhead only
    assert one([Z0]) == 0                   # z == z_ground_limit: z <= limit is ground
    assert one([ZR]) == 100                 # z == robot_height: z <= height is occupied
    assert one([np.nextafter(np.float32(ZR), np.float32(2))]) == -1
    assert one([np.nextafter(np.float32(Z0), np.float32(2))]) == 100
    assert one([np.nan]) == -1              # every comparison with NaN is false
    assert one([-np.inf]) == 0 and one([np.inf]) == -1
    # thresholds swapped (ground limit 1.0, height 0.1): z = 0.5 is not above the limit, so it is ground; 1.5 is above
    # both; nothing can be occupied
    g, _ = pcd_ref.grid(span + [[1.5, 1.5, 0.5], [2.5, 1.5, 1.5], [0.5, 1.5, 0.05]], 1.0, ZR, Z0)
    assert g[1, 1] == 0 and g[2, 1] == -1 and g[0, 1] == 0 and (g == 100).sum() == 0


def test_ref_layout_and_origin():
    pts = [[-2.0, 10.0, 0.0], [1.2, 10.6, 0.5], [-0.9, 10.3, 0.0], [-0.9, 10.3, 3.0]]
    g, o = pcd_ref.grid(pts, 0.5, Z0, ZR)
    # x extent 3.2 -> ceil(6.4) = 7, y extent 0.6 (float: 0.6000004) -> ceil(1.2) = 2
    assert g.shape == (7, 2) and list(o) == [-2.0, 10.0, 0.0]
    want = np.full((7, 2), -1, np.int8)
    want[0, 0] = 0      # (-2, 10)
    want[6, 1] = 100    # (3.2 * 2, 0.6 * 2) = (6.4, 1.2)
    want[2, 0] = 0      # (1.1 * 2, 0.3 * 2) = (2.2, 0.6); the overhead point of the same cell changes nothing
    np.testing.assert_array_equal(g, want)


def test_ref_non_finite_and_degenerate():
    nan, inf = np.nan, np.inf
    # NaN / inf x or y are skipped in the bounding box and in the fill
    g, o = pcd_ref.grid([[nan, 50, 0], [0, 0, 0], [inf, 1, 0.5], [2, -inf, 0.5], [1.5, 1.5, 0.5], [-100, nan, 0]], 1.0,
                        Z0, ZR)
    assert g.shape == (2, 2) and list(o) == [0.0, 0.0, 0.0]
    np.testing.assert_array_equal(g, np.array([[0, -1], [-1, 100]], np.int8))
    # all points on one line: no extent on y, an empty grid, the origin still the minimum
    g, o = pcd_ref.grid([[0, 2, 0], [1, 2, 0], [5, 2, 0]], 1.0, Z0, ZR)
    assert g.shape == (5, 0) and g.size == 0 and list(o) == [0.0, 2.0, 0.0]
    # empty, and nothing finite
    for pts in ([], [[nan, 0, 0], [0, inf, 0]]):
        g, o = pcd_ref.grid(np.array(pts, np.float32).reshape(-1, 3), 1.0, Z0, ZR)
        assert g.shape == (0, 0) and list(o) == [0.0, 0.0, 0.0]
    for res in (0.0, -1.0, nan, inf):
        with pytest.raises(IndexError):
            pcd_ref.grid([[0, 0, 0], [1, 1, 0]], res, Z0, ZR)
    with pytest.raises(IndexError):
        pcd_ref.grid([[0, 0, 0], [1e6, 1e6, 0]], 0.001, Z0, ZR)   # 10^9 x 10^9 cells
    with pytest.raises(IndexError):
        pcd_ref.grid([[-3e38, 0, 0], [3e38, 1, 0]], 1.0, Z0, ZR)  # the extent itself overflows


# ------------------------------------------------------------------ front end
def test_datatypes_front_end(tmp_path):
    from kompass_core.datatypes import PointCloudData, get_occupancy_grid_from_pcd, get_points_from_pcd
    from kompass_core.datatypes import pointcloud

    assert pointcloud.get_occupancy_grid_from_pcd is get_occupancy_grid_from_pcd
    p = cloud(12, 7)
    f = tmp_path / "h.pcd"
    pcd_ref.write_pcd(f, ["x", "y", "z"], [4] * 3, ["F"] * 3, _xyz(p), True)
    np.testing.assert_array_equal(bits(get_points_from_pcd(str(f))), bits(p))
    d = PointCloudData(data=np.zeros(64, np.int8), point_step=16, row_step=64, height=1, width=4, x_offset=0,
                       y_offset=4, z_offset=8)
    assert d.point_step == 16 and d.z_offset == 8
    assert PointCloudData(data=np.zeros(16, np.int8), point_step=16, row_step=16, height=1, width=1).x_offset is None
    for bad in ("point_step", "row_step", "height", "width"):
        kw = dict(data=np.zeros(16, np.int8), point_step=16, row_step=16, height=1, width=1)
        for v in (0, -4):
            kw[bad] = v
            with pytest.raises(ValueError):
                PointCloudData(**kw)


def test_argument_validation_precedes_device_use(tmp_path):
    p = cloud(12, 8)
    f = tmp_path / "i.pcd"
    pcd_ref.write_pcd(f, ["x", "y", "z"], [4] * 3, ["F"] * 3, _xyz(p), True)
    for res in (0.0, -0.5, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError):
            kompass_cpp.utils.read_pcd_to_occupancy_grid(str(f), res, 0.1, 1.0)
        with pytest.raises(ValueError):
            kompass_cpp.utils.points_to_occupancy_grid(p, res, 0.1, 1.0)
    with pytest.raises(ValueError):
        kompass_cpp.utils.points_to_occupancy_grid(np.zeros((4, 2), np.float32), 0.1, 0.1, 1.0)


def test_no_cpu_fallback_without_device(tmp_path):
    if kh.device_count() > 0:
        pytest.skip("a HIP device is visible here")
    p = cloud(12, 9)
    f = tmp_path / "j.pcd"
    pcd_ref.write_pcd(f, ["x", "y", "z"], [4] * 3, ["F"] * 3, _xyz(p), True)
    with pytest.raises(RuntimeError, match="(?i)hip|device"):
        kompass_cpp.utils.read_pcd_to_occupancy_grid(str(f), 0.1, 0.1, 1.0)
    with pytest.raises(RuntimeError, match="(?i)hip|device"):
        kompass_cpp.utils.points_to_occupancy_grid(p, 0.1, 0.1, 1.0)
    with pytest.raises(kh.KompassHipError):
        kh.CloudContext().occupancy_grid(p, 0.1, 0.1, 1.0)
