"""Scan integration on the device (kc_worldmap_integrate, kc_worldmap_integrate_marks; DESIGN.md 4.11 rules 52 to 57)
against the Python statement tests/worldmap_integrate_ref.py: the mark plane, evidence, class and the result record bit
for bit.

The main world is 37 x 29: no side a multiple of 4, and 1073 cells, so that the last dword of the mark plane is partial.
The 130 x 70 world spans several workgroups of the apply kernel (64 cells by 4 rows each)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import worldmap_dist_ref as dref  # noqa: E402
import worldmap_integrate_ref as iref  # noqa: E402
import worldmap_ref as ref  # noqa: E402
import worldmap_scan_ref as sref  # noqa: E402
import worldmap_shift_ref as shref  # noqa: E402

RES, ORIGIN = 0.05, (-0.33, 1.7)
W, H = 37, 29
OCC, UNK, EMP = ref.OCCUPIED, ref.UNEXPLORED, ref.EMPTY
CLEAR = kh.INTEGRATE_CLEAR_NO_RETURN
CELL = 65536
NOTHING = (0, (-1, -1, -1, -1))

# test_worldmap_scan_gpu.py's list
ORIGINS = [(18, 14),                                                          # the middle
           (0, 14), (36, 14), (18, 0), (18, 28),                              # the four edges
           (0, 0), (36, 0), (0, 28), (36, 28),                                # the four corners
           (-1, 14), (37, 14), (18, -1), (18, 29),                            # one cell outside each edge
           (12.37, 9.81), (36.49, 28.49), (17.5, 13.5),                       # fractions of a cell, a cell corner
           (-200, 14), (18, 400), (5000, -5000)]                              # far outside


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def seeded_prior(w, h, seed, p_occ=0.08, p_unknown=0.2):
    rng = np.random.default_rng(seed)
    return rng.choice(np.int8([OCC, UNK, EMP]), size=(w, h), p=[p_occ, p_unknown, 1.0 - p_occ - p_unknown]).astype(np.int8)


def xy_of(cell_i, cell_j, res=RES, origin=ORIGIN):
    r = float(np.float32(res))
    return origin[0] + cell_i * r, origin[1] + cell_j * r


def range_of(rc, res=RES):
    """A range of rc - 1/2 cells: Rc = rc by rule 20's ceil."""
    return float(np.float32(res)) * (rc - 0.5)


def beams(n, start=-math.pi + 0.013):
    return start + np.arange(n) * (2 * math.pi / n)


def seeded_zq(n, range_max, seed, res=RES):
    """Measured ranges up to 1.3 range_max with a NaN, an inf and a negative one among them, through rule 52's quantiser"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.0, 1.3 * range_max, n)
    r[rng.random(n) < 0.08] = np.nan
    r[rng.random(n) < 0.08] = np.inf
    r[rng.random(n) < 0.04] = -1.0
    return kh.worldmap_quantise_ranges(r, res, range_max)


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


class Pair:
    """A device map and the statement side by side, under one prior and one model"""

    def __init__(self, w=W, h=H, res=RES, origin=ORIGIN, prior=None, model=None):
        self.ctx = kh.WorldMapContext(w, h, res, origin)
        self.want = iref.IntegrateRef(w, h, res, origin)
        if model:
            self.ctx.set_model(**model)
            self.want.set_model(**model)
        if prior is not None:
            self.ctx.set_prior(prior)
            self.want.set_prior(prior)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()

    def quantised(self, pose):
        p = pose if isinstance(pose, kh.WorldMapPose) else self.ctx.quantise_pose(*pose)
        return p, (int(p.cq), int(p.sq), int(p.tx), int(p.ty))

    def planes_equal(self):
        cls, ev = self.ctx.planes()
        assert np.array_equal(cls, self.want.cls), np.argwhere(cls != self.want.cls)[:5]
        assert np.array_equal(ev, self.want.evidence), np.argwhere(ev != self.want.evidence)[:5]

    def marks_zero(self):
        """the mark plane between calls, read through a scan that says nothing"""
        z = self.ctx.integrate_marks((self.ctx.origin[0], self.ctx.origin[1], 0.0), [0.0, 1.0], [-1, -1], 1.0)
        assert z.shape == self.ctx.shape and not z.any()

    def integrate(self, pose, angles, zq, range_max, flags=0, marks=None):
        """the mark launch alone, then the whole call -> the statement's (marks, changed, box)"""
        p, q = self.quantised(pose)
        if marks is None:
            marks, _ = self.want.marks(q, angles, zq, range_max, flags)
        before = self.ctx.planes()
        got_marks = self.ctx.integrate_marks(p, angles, zq, range_max, flags)
        assert same(got_marks, marks), (q, np.argwhere(got_marks != marks)[:5])
        after = self.ctx.planes()
        assert same(after[0], before[0]) and same(after[1], before[1])      # the marks entry leaves the map alone
        changed, box = self.want.apply(marks)
        got = self.ctx.integrate(p, angles, zq, range_max, flags)
        assert got == (changed, box), (q, got, changed, box)
        self.planes_equal()
        return marks, changed, box


@pytest.mark.parametrize("rc", [1, 5, 64])
@pytest.mark.parametrize("flags", [0, CLEAR])
def test_small_world_from_every_origin(rc, flags):
    ang, rmax = beams(40), range_of(rc)
    assert kh.worldmap_integrate_check(RES, len(ang), rmax, flags)[0] == rc
    total = hits = 0
    with Pair(prior=seeded_prior(W, H, 11)) as p:
        for k, cell in enumerate(ORIGINS):
            x, y = xy_of(*cell)
            marks, changed, _ = p.integrate((x, y, 0.37 * k), ang, seeded_zq(len(ang), rmax, 100 + k), rmax, flags)
            total += changed
            hits += int((marks & iref.HIT != 0).sum())
            if k >= 16:
                assert not marks.any() and changed == 0                     # far outside: nothing is launched
        p.marks_zero()
    assert total > 0 and hits > 0


@pytest.mark.parametrize("precheck", [True, False])
@pytest.mark.parametrize("n", [1, 40, 257, 1024])
def test_beam_counts(n, precheck):
    """257: just over one workgroup.  1024 beams from one cell at Rc = 5: every beam's first atomics land in the same few
    dwords.  The byte load in front of the atomic plays no part in the result."""
    ang, rmax = beams(n), range_of(5)
    with Pair(prior=seeded_prior(W, H, 12)) as p:
        p.ctx.integrate_set_precheck(precheck)
        for k, cell in enumerate([(18, 14), (12.37, 9.81), (36, 28)]):
            x, y = xy_of(*cell)
            p.integrate((x, y, 0.2 + k), ang, seeded_zq(n, rmax, 200 + k), rmax, CLEAR)
        p.marks_zero()


def centre_pose(i, j, yaw):
    return kh.WorldMapPose(round(math.cos(yaw) * 65536.0), round(math.sin(yaw) * 65536.0), i * CELL, j * CELL)


def test_axis_beams_and_exact_diagonals():
    """dx == 0 and dy == 0 in both directions, by the beam angle and by the yaw; the exact diagonals, where every step ties;
    ranges that end on a cell boundary, one unit before and one after"""
    ang = np.arange(8) * (math.pi / 4)
    table = sref.scan_table(ang)
    assert (table[0][1], table[2][0], table[4][1], table[6][0]) == (0, 0, 0, 0) and abs(table[1][0]) == abs(table[1][1])
    rmax = range_of(5)
    zmax = kh.worldmap_integrate_check(RES, 8, rmax)[1]
    with Pair(prior=seeded_prior(W, H, 13)) as p:
        for yaw in (0.0, math.pi / 2, math.pi, -math.pi / 2):
            for cell in ((18, 14), (1, 1), (35, 27)):
                pose = centre_pose(cell[0], cell[1], yaw)
                for z in (0, CELL // 2 - 1, CELL // 2, CELL // 2 + 1, 46340, 46341, 5 * CELL // 2, 3 * CELL, zmax - 1, zmax):
                    marks, _, _ = p.integrate(pose, ang, np.full(8, z, np.int32), rmax, CLEAR)
                    if z == 0:
                        assert marks[cell] == iref.HIT and np.count_nonzero(marks) == 1
        # the same beams over several 8-step segments of the mark kernel: ranges around the first steps of two of them, along the
        # axes (16 and 32 cells less the half cell to the first boundary) and along the diagonals (times sqrt 2)
        rmax = range_of(40)
        zmax = kh.worldmap_integrate_check(RES, 8, rmax)[1]
        for yaw in (0.0, math.pi / 2):
            for cell in ((18, 14), (1, 27)):
                pose = centre_pose(cell[0], cell[1], yaw)
                for z in (31 * CELL // 2 - 1, 31 * CELL // 2, 33 * CELL // 2, 63 * CELL // 2 - 1, 63 * CELL // 2, 1436568, 1436569,
                          1436570, 1529250, 1529251, 1529252, 35 * CELL, zmax - 1, zmax):
                    p.integrate(pose, ang, np.full(8, z, np.int32), rmax, CLEAR)
        p.marks_zero()


@pytest.mark.parametrize("flags", [0, CLEAR])
def test_measurement_limits(flags):
    n, rmax = 40, range_of(5)
    ang = beams(n)
    zmax = kh.worldmap_integrate_check(RES, n, rmax, flags)[1]
    mix = np.resize(np.int32([-1, zmax, 0]), n)
    with Pair(prior=seeded_prior(W, H, 14)) as p:
        x, y = xy_of(12.37, 9.81)
        for zq in (np.full(n, -1, np.int32), np.full(n, zmax, np.int32), np.zeros(n, np.int32), mix):
            marks, changed, box = p.integrate((x, y, 0.4), ang, zq, rmax, flags)
            if zq[0] == -1 and zq[1] == -1:
                assert not marks.any() and (changed, box) == NOTHING
            elif zq[0] == zmax and zq[1] == zmax:
                assert not (marks & iref.HIT).any() and marks.any() == bool(flags)
            elif zq[1] == 0:
                assert np.count_nonzero(marks) == 1 and marks[12, 10] == iref.HIT
            else:
                assert marks[12, 10] == (iref.HIT | iref.MISS if flags else iref.HIT)
        p.marks_zero()


def test_a_hit_and_a_miss_on_one_cell():
    with Pair() as p:
        pose = centre_pose(10, 10, 0.0)
        marks, changed, box = p.integrate(pose, [0.0, 0.0], [2 * CELL, 4 * CELL], range_of(8))
        assert marks[12, 10] == iref.HIT | iref.MISS and marks[14, 10] == iref.HIT and marks[13, 10] == iref.MISS
        assert p.want.cls[12, 10] == OCC and p.want.cls[13, 10] == EMP and p.want.evidence[12, 10] == 3
        assert (changed, box) == (5, (10, 10, 14, 10))


def check_distance(p, reach=6):
    assert np.array_equal(p.ctx.distance(), dref.dist2_plane(p.want.cls, reach))


def test_sequences_on_one_context():
    """three scans in a row; integrate interleaved with the update of a local grid; a shift followed by an integrate; the
    mark plane all zero after each, the distance plane at reach 6 equal to a full recompute after each"""
    rng = np.random.default_rng(21)
    ang, rmax = beams(90), range_of(9)
    with Pair() as p:
        p.ctx.set_distance(6)
        check_distance(p)
        for k, cell in enumerate([(18, 14), (30.2, 20.7), (3.5, 3.5)]):
            x, y = xy_of(*cell)
            _, changed, _ = p.integrate((x, y, 0.9 * k), ang, seeded_zq(90, rmax, 300 + k), rmax, CLEAR if k != 1 else 0)
            assert changed > 0
            p.marks_zero()
            check_distance(p)
        local = rng.choice(np.int32([OCC, UNK, EMP]), size=(21, 17), p=[0.1, 0.3, 0.6]).astype(np.int32)
        for k, cell in enumerate([(10, 20), (25, 8)]):
            x, y = xy_of(*cell)
            assert p.ctx.update(local, (x, y, 0.5 + k)) == p.want.update(local, (x, y, 0.5 + k))
            p.planes_equal()
            check_distance(p)
            p.integrate((x + 0.11, y - 0.07, -0.4 * k), ang, seeded_zq(90, rmax, 310 + k), rmax, CLEAR)
            p.marks_zero()
            check_distance(p)
        for k, (di, dj) in enumerate([(5, -3), (-9, 4)]):
            p.ctx.shift(di, dj)
            p.want.evidence, p.want.cls = shref.shift_planes(p.want.evidence, p.want.cls, di, dj)
            p.want.origin = p.ctx.origin                                     # rule 46's, as the library holds it
            p.planes_equal()
            x, y = xy_of(14 + 3 * k, 12, origin=p.ctx.origin)
            _, changed, _ = p.integrate((x, y, 2.0 + k), ang, seeded_zq(90, rmax, 320 + k), rmax, CLEAR)
            assert changed > 0
            p.marks_zero()
            check_distance(p)
        assert p.ctx.offset() == (-4, 1)


@pytest.mark.parametrize("model", [ref.DEFAULT_MODEL, ref.LATEST_WINS_EXACT], ids=["default", "latest_wins_exact"])
def test_both_models_held_until_the_evidence_saturates(model):
    ang, rmax = beams(64), range_of(6)
    x, y = xy_of(17.3, 13.6)
    zq = seeded_zq(64, rmax, 400)
    prior = seeded_prior(W, H, 15)
    with Pair(prior=prior, model=model) as p:
        marks, _ = p.want.marks(p.quantised((x, y, 0.7))[1], ang, zq, rmax, CLEAR)
        assert (marks & iref.HIT).any() and (marks == iref.MISS).any()
        reps = (model["e_max"] - model["e_min"]) // min(model["hit"], model["miss"]) + 2
        last = None
        for _ in range(reps):
            last = p.integrate((x, y, 0.7), ang, zq, rmax, CLEAR, marks=marks)
        assert last[1] == 0                                                  # saturated: nothing changes any more
        assert set(np.unique(p.want.evidence[marks & iref.HIT != 0])) == {model["e_max"]}
        assert set(np.unique(p.want.evidence[marks == iref.MISS])) == {model["e_min"]}
        p.marks_zero()


def test_every_refusal_leaves_the_map_and_the_mark_plane_untouched():
    ang, rmax = beams(40), range_of(5)
    x, y = xy_of(18, 14)
    with Pair(prior=seeded_prior(W, H, 16)) as p:
        zq = seeded_zq(40, rmax, 500)
        zmax = kh.worldmap_integrate_check(RES, 40, rmax)[1]
        p.integrate((x, y, 0.1), ang, zq, rmax, CLEAR)
        bad_angles = ang.copy()
        bad_angles[7] = np.nan
        bad_zq = zq.copy()
        bad_zq[3] = zmax + 1
        low_zq = zq.copy()
        low_zq[39] = -2
        far = kh.WorldMapPose(65536, 0, (1 << 36) + 1, 0)
        skew = kh.WorldMapPose(65537, 0, 0, 0)
        refusals = [
            (ValueError, ((x, y, 0.1), ang[:0], zq[:0], rmax, 0)),                       # no beam
            (IndexError, ((x, y, 0.1), beams(65537), np.zeros(65537, np.int32), rmax, 0)),
            (ValueError, ((x, y, 0.1), ang, zq, float("nan"), 0)),
            (ValueError, ((x, y, 0.1), ang, zq, -1.0, 0)),
            (IndexError, ((x, y, 0.1), ang, zq, 103.0, 0)),                              # Rc = 2060
            (ValueError, ((x, y, 0.1), ang, zq, rmax, 2)),
            (ValueError, ((x, y, 0.1), ang, zq, rmax, 0x80000001)),
            (ValueError, ((x, y, 0.1), ang, bad_zq, rmax, CLEAR)),
            (ValueError, ((x, y, 0.1), ang, low_zq, rmax, CLEAR)),
            (ValueError, ((x, y, 0.1), bad_angles, zq, rmax, CLEAR)),
            (ValueError, (skew, ang, zq, rmax, CLEAR)),
            (IndexError, (far, ang, zq, rmax, CLEAR)),
            (ValueError, ((x, y, 0.1), ang, zq[:39], rmax, CLEAR)),                      # one range a beam
        ]
        for exc, args in refusals:
            for entry in (p.ctx.integrate, p.ctx.integrate_marks):
                with pytest.raises(exc):
                    entry(*args)
                p.planes_equal()
                p.marks_zero()
        # the order: counts, range_max, flags, zq, then the angles and the pose
        with pytest.raises(IndexError, match="2048"):
            p.ctx.integrate(far, bad_angles, bad_zq, 103.0, 2)
        with pytest.raises(ValueError, match="flag"):
            p.ctx.integrate(far, bad_angles, bad_zq, rmax, 2)
        with pytest.raises(ValueError, match="quantised range 3 "):
            p.ctx.integrate(far, bad_angles, bad_zq, rmax, CLEAR)
        with pytest.raises(ValueError, match="angle 7 "):
            p.ctx.integrate(far, bad_angles, zq, rmax, CLEAR)
        p.planes_equal()
        p.integrate((x, y, 0.1), ang, zq, rmax, CLEAR)                                   # and a right call works as before
        p.marks_zero()


def test_a_world_of_several_apply_workgroups():
    w, h = 130, 70
    ang = beams(257)
    with Pair(w, h, prior=seeded_prior(w, h, 17)) as p:
        for k, (cell, rc) in enumerate([((65, 35), 64), ((129.3, 0.2), 64), ((40.5, 60.5), 30)]):
            rmax = range_of(rc)
            x, y = xy_of(*cell)
            marks, changed, box = p.integrate((x, y, 1.1 * k), ang, seeded_zq(257, rmax, 600 + k), rmax, CLEAR)
            assert changed > 0
            if k == 0:
                assert box[2] - box[0] >= 64 and box[3] - box[1] >= 8            # the record spans workgroups both ways
        p.marks_zero()


def wall_scan(truth, res, origin, pose, angles, range_max):
    """what a lidar at `pose` would measure in the world `truth`: the virtual scan's statement, inf where nothing returns"""
    q = ref.quantise_pose(res, origin, *pose)
    ranges, cells = sref.scan_pose(truth, res, q, sref.scan_table(angles), range_max)
    return np.where(cells >= 0, ranges, np.inf)


def test_front_ends_give_the_planes_of_the_c_abi():
    import kompass_cpp
    from kompass_core.datatypes.laserscan import LaserScanData
    from kompass_core.mapping import WorldMap
    from kompass_core.models import RobotState

    w, h, res, origin, rmax = 90, 60, 0.05, (-1.0, -0.5), 3.0
    truth = np.full((w, h), EMP, np.int8)
    truth[0, :] = truth[-1, :] = truth[:, 0] = truth[:, -1] = OCC
    truth[50:53, 10:40] = OCC
    ang = beams(120)
    fe = WorldMap(w, h, res, origin)
    cpp = kompass_cpp.mapping.WorldMap(width=w, height=h, resolution=res, origin_x=origin[0], origin_y=origin[1])
    with Pair(w, h, res, origin) as p:
        for k, pose in enumerate([(0.5, 0.7, 0.3), (1.2, 1.9, -2.0), (3.1, 1.0, 3.0)]):
            ranges = wall_scan(truth, res, origin, pose, ang, rmax)
            ranges[5] = np.nan
            ranges[6] = 0.01                                                  # below range_min
            clear = k != 1
            zq = kh.worldmap_quantise_ranges(ranges, res, rmax, 0.02)
            _, changed, box = p.integrate(pose, ang, zq, rmax, CLEAR if clear else 0)
            state = RobotState(x=pose[0], y=pose[1], yaw=pose[2])
            if k == 0:
                scan = LaserScanData(angles=ang, ranges=ranges, angle_increment=2 * math.pi / 120, range_min=0.02, range_max=rmax)
                got = fe.integrate_scan(state, scan, clear_no_return=clear)
            elif k == 1:
                got = fe.integrate_scan(pose, ranges, angles=ang, range_max=rmax, range_min=0.02, clear_no_return=clear)
            else:
                got = fe.integrate_scan(state, ranges, angles=ang, range_max=rmax, range_min=0.02, clear_no_return=clear, follow=(2, 1))
            assert got == changed and fe.changed == changed and fe.changed_box == box
            assert cpp.integrate_scan(pose[0], pose[1], pose[2], ang, ranges, rmax, 0.02, clear) == changed
            assert cpp.get_changed_box() == box
            for m in (fe.occupancy, cpp.get_cls()):
                assert np.array_equal(m, p.want.cls)
            for m in (fe.evidence, cpp.get_evidence()):
                assert np.array_equal(m, p.want.evidence)
        assert fe.offset == (0, 0)                                            # every pose was inside the margin
        q = p.quantised((1.0, 1.0, 0.5))[1]
        ranges = wall_scan(truth, res, origin, (1.0, 1.0, 0.5), ang, rmax)
        p.integrate(kh.WorldMapPose(*q), ang, kh.worldmap_quantise_ranges(ranges, res, rmax), rmax)
        cpp.integrate_scan_at(q, ang, ranges, rmax)
        assert np.array_equal(cpp.get_cls(), p.want.cls) and np.array_equal(cpp.get_evidence(), p.want.evidence)
        with pytest.raises(ValueError):
            cpp.integrate_scan(1.0, 1.0, 0.5, ang, ranges[:-1], rmax)
        with pytest.raises(TypeError):
            fe.integrate_scan((1.0, 1.0, 0.5), ranges)
        assert np.array_equal(cpp.get_cls(), p.want.cls)


def test_replan_routes_around_an_integrated_wall():
    from kompass_core.mapping import WorldMap
    from kompass_core.planning import GridPlanner
    from test_planner_gpu import _robot

    w, h, res, origin, rmax = 160, 120, 0.05, (-1.0, -1.0), 6.0
    wm = WorldMap(w, h, res, origin)                                          # nothing observed yet: the planner may cross it
    start, goal = (1.0, 2.0), (5.0, 2.0)
    fe = GridPlanner(_robot())
    fe.setup_problem(None, start[0], start[1], 0.0, goal[0], goal[1], 0.0, grid=wm)
    first = fe.solve()
    assert first is not None
    truth = np.zeros((w, h), np.int8)
    truth[78:81, 30:90] = OCC                                                 # a wall across the straight line, x = 2.9 .. 3.0 m
    ang = beams(720)
    for pose in [(1.0, 2.0, 0.0), (1.5, 1.0, 0.5), (1.5, 3.2, -0.5), (5.0, 2.0, math.pi)]:
        assert wm.integrate_scan(pose, wall_scan(truth, res, origin, pose, ang, rmax), angles=ang, range_max=rmax) >= 0
    occ = wm.occupancy == OCC
    assert occ[78, 35:85].all() and not (occ & (truth != OCC)).any()          # the faces seen, and nothing but the wall
    path = fe.replan(map=wm)
    assert path is not None
    cells = np.asarray(fe.path_cells)
    assert not occ[cells[:, 0], cells[:, 1]].any()
    assert not np.array_equal(np.asarray(path.y()), np.asarray(first.y()))    # the wall did move the path
    ys = np.asarray(path.y())
    assert ys.min() < -1.0 + 30 * res or ys.max() > -1.0 + 89 * res          # round one of its ends
