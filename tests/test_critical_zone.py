"""CriticalZoneChecker.

The 14 cases of the reference's tests/critical_zone_test.cpp:12-330 pin the
oracle restatement (CPU) and run against the HIP path through the C ABI and
the kompass_cpp module (GPU); random scans / clouds compare HIP with the oracle
bit for bit."""
import numpy as np
import pytest

from oracle import ko

N = 360
ANGLES = 2.0 * np.pi * np.arange(N) / N  # test.h:55-63 initLaserscan
CYL, BOX, SPH = 0, 1, 2


def set_at(ranges, angle, value):
    """test.h:65-95 setLaserscanAtAngle"""
    a = np.fmod(angle, 2.0 * np.pi)
    if a < 0:
        a += 2.0 * np.pi
    ranges[int(np.argmin(np.abs(ANGLES - a)))] = value


def cloud(points):
    """test.h:97-125: PointXYZ{x, y, z, padding}, 16 bytes"""
    rec = np.zeros((len(points), 4), np.float32)
    if len(points):
        rec[:, :3] = np.asarray(points, np.float32)
    return rec.reshape(-1).view(np.int8)


def laserscan_cases():
    """(ranges, forward, predicate) in the order of critical_zone_test.cpp:37-187"""
    out = []
    r = np.full(N, 10.0)
    for a in (0.0, 0.1, -0.1):
        set_at(r, a, 0.2)
    out.append((r.copy(), True, lambda v: v == 1.0))                       # 1 behind, moving forward
    r = np.full(N, 10.0)
    out.append((r.copy(), True, lambda v: v == 1.0))                       # 2 far
    for a in (np.pi, np.pi + 0.1, np.pi - 0.1):
        set_at(r, a, 0.2)
    out.append((r.copy(), True, lambda v: v == 0.0))                       # 3 front close, forward
    out.append((r.copy(), False, lambda v: v == 1.0))                      # 4 front close, backward
    for a in (0.0, 0.1, -0.1):
        set_at(r, a, 0.2)
    out.append((r.copy(), False, lambda v: v == 0.0))                      # 5 back close, backward
    r = np.full(N, 10.0)
    set_at(r, 0.0, 1.3)
    out.append((r.copy(), False, lambda v: 0.0 < v < 1.0))                 # 6 back slowdown, backward
    out.append((r.copy(), True, lambda v: v == 1.0))                       # 7 back slowdown, forward
    set_at(r, np.pi, 0.7)
    out.append((r.copy(), True, lambda v: 0.0 < v < 1.0))                  # 8 front slowdown, forward
    return out


def cloud_cases():
    """critical_zone_test.cpp:230-330"""
    junk = [(-0.1, -0.1, 3.0), (-0.1, -0.1, -3.0), (0.1, 0.2, 4.0), (0.1, 0.2, -4.0)]
    return [
        ([], True, lambda v: v == 1.0),                                                      # 9 empty
        ([(0.7, 0.0, 0.5)], True, lambda v: v == 0.0),                                       # 10 critical
        ([(0.7, 0.0, 3.0)], True, lambda v: v == 1.0),                                       # 11 too high
        ([(0.95, 0.0, 0.5)], True, lambda v: 0.4 < v < 0.6),                                 # 12 slowdown
        ([(0.95, 0.0, 0.5), (1.0, 1.0, 0.5), (-1.0, -1.0, 0.5)] + junk + [(0.75, 0.0, 0.5)],
         True, lambda v: v == 0.0),                                                          # 13 complex stop
        ([(0.95, 0.0, 0.5), (-0.95, 0.0, 0.5), (1.0, 1.0, 0.5), (-1.0, -1.0, 0.5)] + junk,
         False, lambda v: 0.4 < v < 0.6),                                                    # 14 complex slowdown
    ]


SCAN_ARGS = (CYL, [0.51, 2.0], [0.22, 0.0, 0.4], [0, 0, 0.99, 0.0], 160.0, 0.3, 0.6, ANGLES, 0.1, 2.0, 20.0)
CLOUD_ARGS = (CYL, [0.51, 2.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0], 160.0, 0.3, 0.6, ANGLES, 0.1, 2.0, 20.0)


def test_oracle_reference_cases():
    z = ko.CriticalZone(*SCAN_ARGS)
    for k, (r, fwd, ok) in enumerate(laserscan_cases(), 1):
        assert ok(z.check(r, fwd)), f"laserscan case {k}"
    zc = ko.CriticalZone(*CLOUD_ARGS)
    for k, (pts, fwd, ok) in enumerate(cloud_cases(), 9):
        c = cloud(pts)
        n = len(pts)
        assert ok(zc.check_cloud(c, 16, n * 16, 1, n, 0, 4, 8, fwd)), f"cloud case {k}"


def test_oracle_rejects_bad_distances():
    with pytest.raises(ValueError):
        ko.CriticalZone(CYL, [0.5, 1.0], [0, 0, 0], [0, 0, 0, 1], 90.0, 0.6, 0.6, ANGLES, 0.0, 1.0, 10.0)


@pytest.mark.gpu
def test_gpu_reference_cases_abi_and_module():
    import kompass_hip as kh
    from kompass_cpp.types import RobotGeometry
    from kompass_cpp.utils import CriticalZoneChecker, CriticalZoneCheckerGPU

    z = kh.ZoneContext(*SCAN_ARGS)
    o = ko.CriticalZone(*SCAN_ARGS)
    np.testing.assert_array_equal(z.indices(True), o.indices(True))
    np.testing.assert_array_equal(z.indices(False), o.indices(False))
    for k, (r, fwd, ok) in enumerate(laserscan_cases(), 1):
        v = z.check(r, fwd)
        assert ok(v), f"laserscan case {k}: {v}"
        assert np.float32(v) == np.float32(o.check(r, fwd))
    zc, oc = kh.ZoneContext(*CLOUD_ARGS), ko.CriticalZone(*CLOUD_ARGS)
    for k, (pts, fwd, ok) in enumerate(cloud_cases(), 9):
        c, n = cloud(pts), len(pts)
        v = zc.check_cloud(c, 16, n * 16, 1, n, 0, 4, 8, fwd)
        assert ok(v), f"cloud case {k}: {v}"
        assert np.float32(v) == np.float32(oc.check_cloud(c, 16, n * 16, 1, n, 0, 4, 8, fwd))
    # the reference's Python surface (bindings_utils.cpp:47-73, bindings_gpu.cpp:40-68)
    for cls in (CriticalZoneChecker, CriticalZoneCheckerGPU):
        m = cls(input_type=CriticalZoneChecker.InputType.LASERSCAN, robot_shape=RobotGeometry.CYLINDER,
                robot_dimensions=[0.51, 2.0], sensor_position_body=np.array([0.22, 0.0, 0.4], np.float32),
                sensor_rotation_body=np.array([0, 0, 0.99, 0.0], np.float32), critical_angle=160.0,
                critical_distance=0.3, slowdown_distance=0.6, scan_angles=list(ANGLES), min_height=0.1,
                max_height=2.0, range_max=20.0)
        for k, (r, fwd, ok) in enumerate(laserscan_cases(), 1):
            assert ok(m.check(ranges=list(r), forward=fwd)), f"{cls.__name__} case {k}"
        mc = cls(input_type=CriticalZoneChecker.InputType.POINTCLOUD, robot_shape=RobotGeometry.CYLINDER,
                 robot_dimensions=[0.51, 2.0], sensor_position_body=np.zeros(3, np.float32),
                 sensor_rotation_body=np.array([0, 0, 0, 1.0], np.float32), critical_angle=160.0,
                 critical_distance=0.3, slowdown_distance=0.6, scan_angles=list(ANGLES), min_height=0.1,
                 max_height=2.0, range_max=20.0)
        for k, (pts, fwd, ok) in enumerate(cloud_cases(), 9):
            c, n = cloud(pts), len(pts)
            assert ok(mc.check(data=c, point_step=16, row_step=n * 16, height=1, width=n, x_offset=0, y_offset=4,
                               z_offset=8, forward=fwd)), f"{cls.__name__} cloud case {k}"
    with pytest.raises((ValueError, kh.KompassHipError)):
        kh.ZoneContext(CYL, [0.5, 1.0], [0, 0, 0], [0, 0, 0, 1], 90.0, 0.6, 0.6, ANGLES, 0.0, 1.0, 10.0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dims", [(CYL, [0.3, 1.0]), (BOX, [0.6, 0.4, 1.0]), (SPH, [0.35])])
def test_gpu_random_scans_and_clouds_match_oracle(shape, dims):
    import kompass_hip as kh

    rng = np.random.default_rng(17 + shape)
    n = 720
    angles = np.sort(rng.uniform(0, 2 * np.pi, n))
    yaw = 0.4
    args = (shape, dims, [0.1, -0.05, 0.3], [0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)], 120.0, 0.2, 0.9,
            angles, 0.05, 1.5, 8.0)
    z, o = kh.ZoneContext(*args), ko.CriticalZone(*args)
    np.testing.assert_array_equal(z.indices(True), o.indices(True))
    np.testing.assert_array_equal(z.indices(False), o.indices(False))
    seen = set()
    for trial in range(60):
        lo = [0.05, 0.4, 0.7, 1.5][trial % 4]
        r = rng.uniform(lo, lo + 2.0, n)
        if trial % 7 == 0:
            r[rng.integers(0, n, 5)] = np.nan
        for fwd in (True, False):
            want, got = o.check(r, fwd), z.check(r, fwd)
            assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32)
            seen.add("stop" if want == 0 else "clear" if want == 1 else "slow")
    assert seen == {"stop", "clear", "slow"}
    for trial in range(10):
        m = 3000
        d = [0.3, 0.8, 1.2, 3.0][trial % 4]
        pts = np.column_stack([rng.uniform(-1, 1, m) * (d + 2), rng.uniform(-1, 1, m) * (d + 2), rng.uniform(-0.5, 2.0, m)])
        pts = pts[np.hypot(pts[:, 0], pts[:, 1]) > d]
        c, k = cloud(pts), len(pts)
        for fwd in (True, False):
            want = o.check_cloud(c, 16, k * 16, 1, k, 0, 4, 8, fwd)
            got = z.check_cloud(c, 16, k * 16, 1, k, 0, 4, 8, fwd)
            assert np.float32(got).view(np.uint32) == np.float32(want).view(np.uint32)


# ---- more than one workgroup of the check kernel, the thresholds, odd ranges --------------------------------------
# zone_check_kernel runs one lane per entry of the preset index set, 256 a workgroup, and takes the minimum across
# all of them: the sets below span two to four workgroups, the last of them partly filled.
SHAPES = [(CYL, [0.3, 1.0]), (BOX, [0.6, 0.4, 1.0]), (SPH, [0.35])]
YAW = 0.4
MOUNT = ([0.1, -0.05, 0.3], [0.0, 0.0, np.sin(YAW / 2), np.cos(YAW / 2)])


def _bits(v):
    return np.float32(v).view(np.uint32)


def _kind(v):
    return "stop" if v == 0.0 else "clear" if v == 1.0 else "slow"


@pytest.mark.gpu
@pytest.mark.parametrize("n,critical_angle", [(2048, 170.0), (1100, 90.0)])
@pytest.mark.parametrize("shape,dims", SHAPES)
def test_gpu_index_sets_of_several_workgroups(shape, dims, n, critical_angle):
    import kompass_hip as kh

    rng = np.random.default_rng(33 + n)
    angles = np.sort(rng.uniform(0, 2 * np.pi, n))
    # (a sensor 2 cm off the centre: further out the backward set of 1100 angles at 90 degrees drops below 256)
    args = (shape, dims, [0.02, -0.01, 0.3], MOUNT[1], critical_angle, 0.2, 0.9, angles, 0.05, 1.5, 8.0)
    z, o = kh.ZoneContext(*args), ko.CriticalZone(*args)
    seen = set()
    for fwd in (True, False):
        idx = o.indices(fwd)
        assert len(idx) > 256 and len(idx) % 256 != 0, len(idx)
        np.testing.assert_array_equal(z.indices(fwd), idx)
        for trial in range(40):
            lo = [0.05, 0.4, 0.7, 1.5][trial % 4]
            r = rng.uniform(lo, lo + 2.0, n)
            if trial % 7 == 0:
                r[rng.integers(0, n, 5)] = np.nan
            want = o.check(r, fwd)
            assert _bits(z.check(r, fwd)) == _bits(want)
            seen.add(_kind(want))
        # one short beam, everything else far: the last entry of the set (the last lane of the partly filled
        # workgroup), the entries either side of the first workgroup boundary, the first entry
        for k in (len(idx) - 1, 256, 255, 0):
            for short in (0.05, 0.75):
                r = np.full(n, 10.0)
                r[idx[k]] = short
                want = o.check(r, fwd)
                assert want < 1.0, (k, short)  # the beam alone decides (oracle)
                assert _bits(z.check(r, fwd)) == _bits(want), (k, short)
                seen.add(_kind(want))
        assert o.check(np.full(n, 10.0), fwd) == 1.0 and z.check(np.full(n, 10.0), fwd) == 1.0
    assert seen == {"stop", "clear", "slow"}
    z.close()


def _next_doubles(v, count, direction):
    out = []
    for _ in range(count):
        v = float(np.nextafter(v, direction))
        out.append(v)
    return out


def _bisect_boundary(check, lo, hi, below):
    """Adjacent doubles lo < hi with below(check(lo)) and not below(check(hi)), by bisection over the doubles'
    bit patterns (positive doubles order like their bits)."""
    assert below(check(lo)) and not below(check(hi))
    a, b = (int(np.float64(v).view(np.uint64)) for v in (lo, hi))
    while b - a > 1:
        m = (a + b) // 2
        if below(check(float(np.uint64(m).view(np.float64)))):
            a = m
        else:
            b = m
    return float(np.uint64(a).view(np.float64)), float(np.uint64(b).view(np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dims", SHAPES)
def test_gpu_thresholds_at_adjacent_doubles(shape, dims):
    """`distance <= critical_distance` and `distance <= slowdown_distance` at equality and next to it: one beam of the
    forward set carries the range, found with the oracle alone by bisection down to two adjacent doubles that
    straddle the stop / slow boundary (and the slow / clear one); the kernel has to agree at the eight doubles
    either side of each."""
    import kompass_hip as kh

    n = 360
    args = (shape, dims, *MOUNT, 120.0, 0.2, 0.9, ANGLES, 0.05, 1.5, 8.0)
    z, o = kh.ZoneContext(*args), ko.CriticalZone(*args)
    fwd_set = o.indices(True)
    for beam in (int(fwd_set[0]), int(fwd_set[len(fwd_set) // 2])):
        def check(v, ctx=o):
            r = np.full(n, 10.0)
            r[beam] = v
            return ctx.check(r, True)

        stop_slow = _bisect_boundary(check, 0.01, 0.9, lambda f: f == 0.0)
        slow_clear = _bisect_boundary(check, stop_slow[1], 9.0, lambda f: f < 1.0)
        assert check(stop_slow[0]) == 0.0 and 0.0 < check(stop_slow[1]) < 1.0
        assert 0.0 < check(slow_clear[0]) < 1.0 and check(slow_clear[1]) == 1.0
        for lo, hi in (stop_slow, slow_clear):
            values = _next_doubles(lo, 7, -np.inf)[::-1] + [lo, hi] + _next_doubles(hi, 7, np.inf)
            assert len(values) == 16 and values == sorted(values)
            kinds = set()
            for v in values:
                want = check(v)
                assert _bits(check(v, z)) == _bits(want), (beam, v.hex(), want)
                kinds.add(_kind(want))
            assert len(kinds) == 2
        # ... and the float neighbours of the boundary ranges: each a different distance in the kernel's float
        for lo, hi in (stop_slow, slow_clear):
            f = np.float32(hi)
            for _ in range(4):
                f = np.nextafter(f, np.float32(np.inf))
                assert _bits(check(float(f), z)) == _bits(check(float(f)))
            f = np.float32(lo)
            for _ in range(4):
                f = np.nextafter(f, np.float32(-np.inf))
                assert _bits(check(float(f), z)) == _bits(check(float(f)))
    z.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dims", SHAPES)
def test_gpu_odd_ranges_on_index_set_beams(shape, dims):
    """+-inf, 0, a negative range, a range whose product with the float trig overflows the float it is stored in, NaN:
    alone on a beam of the set and next to a short beam.  Angles 0 and pi / 2 are in the preset (sin / cos exactly 0:
    inf * 0).  The expected value is whatever the reference's expression gives."""
    import kompass_hip as kh

    rng = np.random.default_rng(53 + shape)
    n = 700
    angles = np.sort(np.concatenate([[0.0, np.pi / 2, np.pi, 3 * np.pi / 2], rng.uniform(0, 2 * np.pi, n - 4)]))
    args = (shape, dims, *MOUNT, 170.0, 0.2, 0.9, angles, 0.05, 1.5, 8.0)
    z, o = kh.ZoneContext(*args), ko.CriticalZone(*args)
    odd = [np.inf, -np.inf, 0.0, -0.0, -1.0, 1e308, -1e308, np.nan, 1e39, 3.5e38, 5e-324]
    seen = set()
    for fwd in (True, False):
        idx = o.indices(fwd)
        assert len(idx) > 256
        axis = [int(i) for i in idx if angles[i] in (0.0, np.pi / 2, np.pi, 3 * np.pi / 2)]
        assert axis
        beams = axis + [int(idx[0]), int(idx[255]), int(idx[256]), int(idx[-1])]
        for b in beams:
            for v in odd:
                for short in (None, 0.05, 0.75):
                    r = np.full(n, 10.0)
                    r[b] = v
                    if short is not None:
                        r[idx[(list(idx).index(b) + 100) % len(idx)]] = short
                    with np.errstate(all="ignore"):
                        want = o.check(r, fwd)
                    assert _bits(z.check(r, fwd)) == _bits(want), (b, v, short, want)
                    seen.add(_kind(want))
        for trial in range(10):  # mixed
            r = rng.uniform(0.7, 3.0, n)
            r[rng.choice(idx, 12, replace=False)] = rng.choice(odd, 12)
            want = o.check(r, fwd)
            assert _bits(z.check(r, fwd)) == _bits(want), (trial, want)
    assert seen == {"stop", "clear", "slow"}
    z.close()
