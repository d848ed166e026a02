"""The Monte-Carlo localiser through its three front ends (DESIGN.md 4.11 rules 28 to 41): `kompass_core.mapping.MCL`,
`kompass_cpp.mapping.MCL` and the ctypes owner `kompass_hip.MclContext` give one record and one estimate, the estimate's
doubles are the statement's from the same integers, the resample decision is the statement's on either side of its
threshold, and a closed loop runs with the map updated on the device at the localiser's own estimate."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_cpp  # noqa: E402
import kompass_hip as kh  # noqa: E402
import worldmap_mcl_ref as mref  # noqa: E402
import worldmap_ref as ref  # noqa: E402
import worldmap_scan_ref as sref  # noqa: E402

RES, ORIGIN = 0.05, (-1.0, -1.0)
W, H = 160, 120
RANGE_MAX = 3.0
ANGLES = np.arange(24) * (2 * math.pi / 24) + 0.02
NOISE = (0.02, 0.01, 0.01)
SIGMA_HIT = 0.1
START = (2.0, 2.5, 0.4)


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def room_cls():
    c = np.full((W, H), ref.EMPTY, np.int8)
    c[4, :] = c[150, :] = ref.OCCUPIED
    c[:, 5] = c[:, 110] = ref.OCCUPIED
    c[:4, :] = c[151:, :] = ref.UNEXPLORED
    c[70, 5:60] = ref.OCCUPIED
    c[100:150, 70] = ref.OCCUPIED
    return c


def drive(n):
    out = [START]
    for _ in range(n):
        x, y, yaw = out[-1]
        out.append((x + 0.1 * math.cos(yaw), y + 0.1 * math.sin(yaw), yaw + 0.06))
    return out


def true_scans(cls, path):
    table = sref.scan_table(ANGLES)
    return [sref.scan_pose(cls, RES, ref.quantise_pose(RES, ORIGIN, *p), table, RANGE_MAX)[0] for p in path]


def scales():
    cells = 65536.0 / float(np.float32(RES))
    return (mref.noise_scale(NOISE[0] * cells), mref.noise_scale(NOISE[1] * cells),
            mref.noise_scale(NOISE[2] / (2 * math.pi) * 65536.0))


def init_args(state, sigma_xy, sigma_yaw):
    _, _, tx, ty = ref.quantise_pose(RES, ORIGIN, state[0], state[1], 0.0)
    cells = 65536.0 / float(np.float32(RES))
    return tx, ty, mref.quantise_heading(state[2]), mref.noise_scale(sigma_xy * cells), mref.noise_scale(sigma_yaw / (2 * math.pi) * 65536.0)


def statement(cls, n, seed):
    m = mref.MclRef(cls, RES, n, ANGLES, RANGE_MAX, seed)
    m.set_model(*mref.sensor_tables(RES, SIGMA_HIT))
    return m


def statement_step(m, a, b, ranges, resample=(1, 2)):
    rec = m.step(*mref.odometry_increment(RES, a, b), *scales(), mref.quantise_ranges(ranges, RES, RANGE_MAX))
    est = mref.estimate(rec, RES, ORIGIN)
    est["spread"] = mref.spread(m.tx, m.ty, m.w, est, RES)
    est["resampled"] = mref.should_resample(rec, m.n, *resample)
    if est["resampled"]:
        m.resample()
    return rec, est


def same_estimate(e, rec, est):
    assert tuple(e.record) == rec.as_tuple()
    assert (e.x, e.y, e.yaw, e.n_eff) == (est["x"], est["y"], est["yaw"], est["n_eff"])        # the very doubles
    assert e.resampled == est["resampled"] and e.best_cost == rec.amin
    assert e.spread == pytest.approx(est["spread"], rel=1e-12)


def test_three_front_ends_one_record():
    from kompass_core.mapping import MCL, WorldMap
    from kompass_core.models import RobotState

    cls, n, seed = room_cls(), 200, 7
    path = drive(4)
    scans = true_scans(cls, path)
    guess = (START[0] + 0.08, START[1] - 0.05, START[2] + 0.03)

    fe_map = WorldMap(W, H, RES, ORIGIN)
    fe_map.set_prior(cls)
    fe = MCL(fe_map, n, ANGLES, RANGE_MAX, sigma_hit=SIGMA_HIT, seed=seed, motion_noise=NOISE)
    cpp_map = kompass_cpp.mapping.WorldMap(width=W, height=H, resolution=RES, origin_x=ORIGIN[0], origin_y=ORIGIN[1])
    cpp_map.set_prior(cls)
    cpp = kompass_cpp.mapping.MCL(cpp_map, n, ANGLES, RANGE_MAX, seed)
    cpp.set_model(sigma_hit=SIGMA_HIT)
    cpp.set_motion_noise(*NOISE)
    with kh.WorldMapContext(W, H, RES, ORIGIN) as ct_map:
        ct_map.set_prior(cls)
        with kh.MclContext(ct_map, n, ANGLES, RANGE_MAX, seed) as ct:
            ct.set_model(*mref.sensor_tables(RES, SIGMA_HIT))
            want = statement(cls, n, seed)
            fe.init(RobotState(x=guess[0], y=guess[1], yaw=guess[2]), 0.1, 0.05)
            cpp.init(*guess, 0.1, 0.05)
            ct.init_pose(*init_args(guess, 0.1, 0.05))
            want.init_pose(*init_args(guess, 0.1, 0.05))
            for k in range(1, len(path)):
                rec, est = statement_step(want, path[k - 1], path[k], scans[k])
                e_fe = fe.step(RobotState(x=path[k - 1][0], y=path[k - 1][1], yaw=path[k - 1][2]), path[k], scans[k])
                e_cpp = cpp.step(path[k - 1], path[k], scans[k])
                r_ct = ct.step(*mref.odometry_increment(RES, path[k - 1], path[k]), *scales(),
                               kh.mcl_quantise_ranges(scans[k], RES, RANGE_MAX))
                same_estimate(e_fe, rec, est)
                same_estimate(e_cpp, rec, est)
                assert r_ct.as_tuple() == rec.as_tuple()
                if est["resampled"]:
                    ct.resample()
                for got in (cpp.particles(), ct.particles()):
                    assert all(np.array_equal(g, w) for g, w in zip(got, want.particles()))
            x, y, yaw, acc = fe.particles()
            assert x.shape == (n,) and np.array_equal(acc, want.particles()[3])
            assert abs(np.average(x) - path[-1][0]) < 0.5 and fe.n_particles == n
            # the estimate is a robot state to the map
            assert fe_map.scan(e_fe, ANGLES, RANGE_MAX).shape == (24,)
            assert fe_map.points(e_fe, 1.0).shape[1] == 3
    with pytest.raises(TypeError):
        MCL(object(), n, ANGLES, RANGE_MAX)
    with pytest.raises(ValueError):
        fe.step(path[0], path[1], scans[1][:5])


def test_resample_decision_on_either_side_of_the_threshold():
    cls, n, seed = room_cls(), 300, 2
    path = drive(1)
    scans = true_scans(cls, path)
    cpp_map = kompass_cpp.mapping.WorldMap(width=W, height=H, resolution=RES, origin_x=ORIGIN[0], origin_y=ORIGIN[1])
    cpp_map.set_prior(cls)

    def run(ratio):
        m = kompass_cpp.mapping.MCL(cpp_map, n, ANGLES, RANGE_MAX, seed)
        m.set_model(sigma_hit=SIGMA_HIT)
        m.set_motion_noise(*NOISE)
        m.set_resample_ratio(*ratio)
        m.init(*START, 0.2, 0.1)
        want = statement(cls, n, seed)
        want.init_pose(*init_args(START, 0.2, 0.1))
        rec, est = statement_step(want, path[0], path[1], scans[1], ratio)
        e = m.step(path[0], path[1], scans[1])
        same_estimate(e, rec, est)
        assert all(np.array_equal(g, w) for g, w in zip(m.particles(), want.particles()))
        return rec, e.resampled

    rec, _ = run((0, 1))
    den = 65536
    num = rec.w1 * rec.w1 * den // (n * rec.w2)            # the largest num with w1^2 den >= num n w2: no resample
    assert 0 < num < den
    assert run((num, den))[1] is False
    assert run((num + 1, den))[1] is True


def test_closed_loop_with_the_map_updated_at_the_estimate():
    """A dozen steps: the mapper's grid is fused into the map at the localiser's estimate where it lies on the device, and
    the next step ray-casts the updated map.  The statement follows with a host copy; the device path has none."""
    from kompass_core.datatypes.laserscan import LaserScanData
    from kompass_core.mapping import MCL, LocalMapper, MapConfig, WorldMap
    from kompass_core.models import RobotState

    truth_cls, n, seed = room_cls(), 64, 1
    path = drive(12)
    scans = true_scans(truth_cls, path)
    wm = WorldMap(W, H, RES, ORIGIN)
    want_map = ref.WorldMapRef(W, H, RES, ORIGIN)
    prior = truth_cls.copy()
    prior[:, 60:] = ref.UNEXPLORED                            # half of the room is still to be mapped
    wm.set_prior(prior)
    want_map.set_prior(prior)
    lm = LocalMapper(MapConfig(width=4.0, height=4.0, resolution=RES))
    fe = MCL(wm, n, ANGLES, RANGE_MAX, sigma_hit=SIGMA_HIT, seed=seed, motion_noise=NOISE)
    want = statement(want_map.cls, n, seed)
    fe.init(START, 0.05, 0.02)
    want.init_pose(*init_args(START, 0.05, 0.02))
    changed = 0
    for k in range(1, len(path)):
        want.cls = want_map.cls
        rec, est = statement_step(want, path[k - 1], path[k], scans[k])
        e = fe.step(path[k - 1], path[k], LaserScanData(angles=ANGLES, ranges=scans[k], angle_increment=2 * math.pi / 24,
                                                        range_max=RANGE_MAX))
        same_estimate(e, rec, est)
        lm.update_from_scan(RobotState(x=e.x, y=e.y, yaw=e.yaw),
                            LaserScanData(angles=ANGLES, ranges=scans[k], angle_increment=2 * math.pi / 24, range_max=RANGE_MAX))
        got = wm.update(e, lm)                                 # the estimate as the robot state, the grid where it lies
        exp = want_map.update(np.asarray(lm.occupancy), (e.x, e.y, e.yaw))
        assert got == exp[0]
        changed += got
    assert changed > 0
    np.testing.assert_array_equal(wm.occupancy, want_map.cls)
    assert math.isfinite(e.spread) and e.n_eff >= 1.0
