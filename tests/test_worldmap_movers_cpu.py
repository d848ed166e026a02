"""Finding and tracking movers without a GPU (DESIGN.md 4.11 rules 64 to 70 and the tracker): the statement
tests/worldmap_movers_ref.py against answers worked out by hand, the host-only entry kc_worldmap_movers_check against
the statement, the geometry of a disc's cluster, the tracker on an exactly linear input, and the burn-in scene: a walker's
beams integrated as they come leave phantom cells in the map, and kept out by the skip mask leave none."""
import math

import numpy as np
import pytest

import kompass_hip as kh
import mppi_movers_ref as mvref
import mppi_ref as mp
import worldmap_dist_ref as dref
import worldmap_integrate_ref as iref
import worldmap_movers_cases as cases
import worldmap_movers_ref as wm
import worldmap_ref as ref
import worldmap_scan_ref as sref

CELL = 65536


def run_case(c):
    plane = dref.dist2_plane(c["cls"], c["reach"])
    return wm.detect(c["cls"], plane, c["reach"], cases.RES, c["pose"], c["angles"], c["zq"], c["range_max"], **c["cfg"])


# ---- rule 70 ----
GOOD = dict(resolution=0.05, n_beams=4, range_max=2.0, zq=None, m2=4, gap=2, join_q=9 << 16, min_beams=3)
# each case breaks two rules; the one earlier in rule 70's order must be the one reported
ORDER = [
    (dict(n_beams=0, m2=0), ValueError, "beam"),                       # counts before m2
    (dict(n_beams=65537, m2=0), IndexError, "beam"),
    (dict(range_max=float("nan"), gap=65), ValueError, "range_max"),   # range_max before gap
    (dict(range_max=2048.5 * 0.05, m2=0), IndexError, "2048"),         # Rc before m2
    (dict(zq=[0, 0, -2, 0], m2=0), ValueError, "quantised"),           # zq before m2
    (dict(m2=0, gap=65), ValueError, "m2"),                            # m2 before gap
    (dict(gap=65, join_q=(1 << 40) + 1), IndexError, "gap"),           # gap before join_q
    (dict(join_q=(1 << 40) + 1, min_beams=0), IndexError, "join_q"),   # join_q before min_beams
    (dict(min_beams=0, n_beams=4), ValueError, "min_beams"),
    (dict(min_beams=65537, n_beams=4), IndexError, "min_beams"),
]


@pytest.mark.parametrize("change,exc,word", ORDER)
def test_refusal_order(change, exc, word):
    args = dict(GOOD, **change)
    with pytest.raises(exc, match=word):
        wm.movers_check(**args)
    with pytest.raises(exc, match=word):
        kh.worldmap_movers_check(**args)


def test_check_accepts_the_limits():
    for change in (dict(m2=1), dict(gap=0), dict(gap=64), dict(join_q=0), dict(join_q=1 << 40), dict(min_beams=1),
                   dict(min_beams=65536), dict(zq=[-1, 0, 5, round(2.0 / float(np.float32(0.05)) * 65536.0)])):
        args = dict(GOOD, **change)
        assert kh.worldmap_movers_check(**args) == wm.movers_check(**args)


# ---- rules 66 and 67 ----
def test_rule_66_edges():
    c = cases.rule66_case()
    labels, rec, clusters = run_case(c)
    assert labels.tolist() == c["labels"].tolist()
    assert rec == wm.Record(4, 4, 4, 4)
    assert [(k.k_first, k.k_last, k.n) for k in clusters] == [(2, 2, 1), (4, 4, 1), (5, 5, 1), (10, 10, 1)]
    # the zero-range beam ends at the sensor itself: rule 65's half cell
    tx, ty = c["pose"][2:]
    assert (clusters[3].sx, clusters[3].sy) == (tx + 32768, ty + 32768)
    assert clusters[3].min_x == clusters[3].max_x == clusters[3].sx


@pytest.mark.parametrize("name", sorted(cases.rule67_cases()))
def test_rule_67_edges(name):
    c = cases.rule67_cases()[name]
    labels, rec, clusters = run_case(c)
    assert labels.tolist() == c["labels"].tolist()
    assert rec.n_dynamic == int((c["zq"] >= 0).sum())
    assert rec.n_kept == len(clusters) == int(c["labels"].max()) + 1


def test_sums_and_box_of_a_run():
    c = cases.rule67_cases()["gap_plus_1"]
    _, _, (k,) = run_case(c)
    x0 = c["pose"][2] + 32768
    xs = [x0 + int(z) for z in c["zq"] if z >= 0]
    y = c["pose"][3] + 32768
    assert k == wm.Cluster(0, 4, 3, sum(xs), 3 * y, min(xs), max(xs), y, y)


def test_alternating_beams_beyond_the_returned_clusters():
    c = cases.alternating_case()
    labels, rec, clusters = run_case(c)
    assert labels.tolist() == c["labels"].tolist() and labels.max() == 511
    assert rec == wm.Record(512, 512, 512, 256) and len(clusters) == 256


def test_state_refusals():
    c = cases.rule66_case()
    with pytest.raises(wm.StateError):
        wm.detect(c["cls"], None, 0, cases.RES, c["pose"], c["angles"], c["zq"], c["range_max"])
    plane = dref.dist2_plane(c["cls"], 2)
    with pytest.raises(wm.StateError):
        wm.detect(c["cls"], plane, 2, cases.RES, c["pose"], c["angles"], c["zq"], c["range_max"], m2=5)
    wm.detect(c["cls"], plane, 2, cases.RES, c["pose"], c["angles"], c["zq"], c["range_max"], m2=4)


# ---- geometry: a disc against free space ----
# the sensor stands in the middle of cell (30, 30) of an open 64 x 64 map; (disc centre in cells, r in cells, yaw): along an
# axis and off it, near (the disc fills a third of the view) and far, a disc of less than a cell, and the view along the
# diagonal, where the endpoints' box is widest for what the sensor sees
DISCS = [((40.0, 30.0), 2.0, 0.0), ((12.25, 50.5), 2.0, 1.1), ((30.0, 8.0), 0.75, -2.3), ((33.0, 33.0), 3.5, 0.5),
         ((58.0, 31.0), 1.0, 0.1), ((50.0, 50.0), 2.0, 0.0)]
SLACK = 2.0 ** -10


def disc_cluster(centre, r, yaw):
    W = H = 64
    cls = np.full((W, H), ref.EMPTY, np.int8)
    plane = np.full((W, H), dref.FAR, np.uint16)
    pose = cases.centre_pose(30.0, 30.0, yaw)
    angles = -math.pi + np.arange(360) * (2 * math.pi / 360)
    rmax = 60.0
    disc = (round(centre[0] * CELL), round(centre[1] * CELL), r)
    ranges = wm.shorten_by_discs(np.full(360, rmax), 1.0, pose, angles, [disc])
    zq = wm.quantise_ranges(ranges, 1.0, rmax)
    labels, rec, clusters = wm.detect(cls, plane, 8, 1.0, pose, angles, zq, rmax)
    assert rec.n_kept == rec.n_runs == 1 and rec.n_dynamic == clusters[0].n >= 3
    return disc, clusters[0]


@pytest.mark.parametrize("centre,r,yaw", DISCS)
def test_a_disc_comes_back_where_it_stands(centre, r, yaw):
    """Every endpoint lies on the disc's rim up to rule 44's rounding (2^-16 of a cell a coordinate, the range's 2^-17), and
    a mean of points of a convex set lies inside it: the centre lies within r + 2^-10 cells of the disc's."""
    disc, k = disc_cluster(centre, r, yaw)
    cx, cy = wm.cluster_centre_q(k)
    print("centre off by", math.hypot(cx - disc[0], cy - disc[1]) / CELL, "cells of", r)
    assert math.hypot(cx - disc[0], cy - disc[1]) / CELL <= r + SLACK
    # metres: the front ends' formula with the origin and the resolution
    x, y, rad = wm.cluster_world(k, 0.25, (-3.0, 7.0))
    assert x == -3.0 + cx / 65536.0 * 0.25 and y == 7.0 + cy / 65536.0 * 0.25 and rad == wm.cluster_radius_q(k) / 65536.0 * 0.25


@pytest.mark.parametrize("centre,r,yaw", DISCS)
def test_a_discs_radius(centre, r, yaw):
    """The radius is at most r + 2^-10 cells.  Every endpoint lies on the rim up to its rounding, points of a rim of radius r
    span at most 2 r along an axis, and the radius is half the longer side of the endpoints' box.  Half the box's DIAGONAL,
    the first formula this feature had, is bounded by sqrt(2) r only and gave 2.155 cells for the last case (r = 2, seen
    along the map's diagonal from 28.3 cells): that is why the diagonal is not what the front ends use, and the second
    assertion keeps the reason in view."""
    _, k = disc_cluster(centre, r, yaw)
    print("radius", wm.cluster_radius_q(k) / CELL, "of", r)
    assert wm.cluster_radius_q(k) / CELL <= r + SLACK
    assert wm.cluster_radius_q(k) * 2.0 == max(k.max_x - k.min_x, k.max_y - k.min_y)
    if centre == (50.0, 50.0):
        assert math.hypot(k.max_x - k.min_x, k.max_y - k.min_y) / 2.0 / CELL > r + SLACK


def test_a_cluster_in_one_cell_centre_comes_back_at_that_cell():
    """4.12 rule 1 puts cell I's centre at TX = I << 16; rule 65's EX of a return in the middle of cell I is (I << 16) +
    2^15.  The front ends' - 32768 is that half cell: three returns in the middle of cell (12, 8) are a mover at
    (12 << 16, 8 << 16), the cell MPPI's (TX + 2^15) >> 16 names."""
    c = cases._open_row([10 * CELL] * 3, dict(m2=4, gap=0, join_q=0, min_beams=3), [0, 0, 0])
    _, _, (k,) = run_case(c)
    cx, cy = wm.cluster_centre_q(k)
    assert (cx, cy) == (12.0 * CELL, 8.0 * CELL)
    assert mp.cell(int(cx), int(cy)) == (12, 8)
    assert wm.cluster_radius_q(k) == 0.0


# ---- the tracker ----
def test_tracker_on_a_line():
    """Centres exactly on a line at a constant velocity of dyadic numbers: the two-point start gives the velocity exactly,
    every later residual is zero."""
    tr = wm.MoverTracker()
    dt, v = 0.5, (0.5, -1.0)
    for n in range(12):
        tr.update([(100.0 + v[0] * dt * n, 50.0 + v[1] * dt * n, 0.25 + 0.125 * (n == 3))], dt)
        assert len(tr.tracks) == 1 and tr.tracks[0].id == 0
        x, y, vx, vy, rad = tr.moving_obstacles()[0]
        assert abs(x - (100.0 + v[0] * dt * n)) <= 1e-9 and abs(y - (50.0 + v[1] * dt * n)) <= 1e-9
        if n >= 1:
            assert abs(vx - v[0]) <= 1e-9 and abs(vy - v[1]) <= 1e-9
        assert rad == (0.375 if n >= 3 else 0.25)                       # the largest seen


def test_tracker_association_coasting_and_ids():
    tr = wm.MoverTracker(gate=2.0, max_misses=2)
    tr.update([(0.0, 0.0, 1.0), (10.0, 0.0, 1.0)], 1.0)
    assert [t.id for t in tr.tracks] == [0, 1]
    tr.update([(11.0, 0.0, 1.0), (1.0, 0.0, 1.0), (50.0, 50.0, 1.0)], 1.0)   # cluster order does not decide, nearness does
    assert [(t.id, t.x, t.vx) for t in tr.tracks] == [(0, 1.0, 1.0), (1, 11.0, 1.0), (2, 50.0, 0.0)]
    tr.update([(1.5, 0.0, 1.0), (2.5, 0.0, 1.0)], 1.0)                        # equally near the prediction 2.0: the lowest index
    t0 = tr.tracks[0]
    assert (t0.x, t0.vx) == (2.0 + 0.5 * -0.5, 1.0 + 0.3 * -0.5)
    assert [t.id for t in tr.tracks] == [0, 1, 2, 3]                          # 2.5 opened a track; 1 and 2 coast
    assert tr.tracks[1].x == 12.0 and tr.tracks[1].misses == 1
    tr.update([], 1.0)
    tr.update([], 1.0)
    assert [t.id for t in tr.tracks] == [0, 3]                                # 1 and 2 missed three times in a row
    tr.update([], 1.0)
    assert tr.tracks == []


# ---- the host classes, which need no device for this ----
def test_cluster_to_world_and_the_half_cell_against_movers_of():
    """A mover the statement places in the middle of cell (12, 8) comes back there: WorldMap.cluster_to_world gives origin +
    12 res, and MPPI.movers_of, which quantises as the pose is quantised (4.12 rule 1), turns that into OX = 12 << 16, the
    cell MPPI's (TX + 2^15) >> 16 names.  Without the - 32768 it would be half a cell off."""
    import kompass_cpp
    from kompass_core.control import MPPIConfig
    c = cases._open_row([10 * CELL] * 3, dict(m2=4, gap=0, join_q=0, min_beams=3), [0, 0, 0])
    _, _, (k,) = run_case(c)
    for origin in ((0.0, 0.0), (-0.33, 1.7), (-0.33 + 3 * 0.05, 1.7 - 2 * 0.05)):   # the last: a window shifted by (3, -2) cells
        got = kompass_cpp.mapping.WorldMap.cluster_to_world(tuple(k), 0.05, *origin)
        want = wm.cluster_world(k, 0.05, origin)
        assert (got.x, got.y, got.radius) == want and got.raw == tuple(k)
        mv = kompass_cpp.control.MPPI.movers_of([kompass_cpp.control.MovingObstacle(got.x, got.y, 0.0, 0.0, got.radius)], 0.1, 0.05,
                                                *origin, 0.0, 0.0, MPPIConfig().to_kompass_cpp())
        assert (mv[0][0], mv[1][0]) == (12 * CELL, 8 * CELL)
        assert mp.cell(mv[0][0], mv[1][0]) == (12, 8)


def scene_detections(n_scans=40):
    """The burn-in scene's detections as [(x, y, radius)] in metres at 0.05 m a cell, a list a scan"""
    static = mp.scene_cls()
    plane = dref.dist2_plane(static, mp.SCENE_REACH)
    pose = (65536, 0, 75 * CELL, 56 * CELL + 32768)
    angles = -math.pi + np.arange(SCENE_BEAMS) * (2 * math.pi / SCENE_BEAMS)
    table = sref.scan_table(angles)
    out = []
    for n in range(n_scans):
        walker = (mvref.CROSS_START[0] + n * mvref.CROSS_V[0], mvref.CROSS_START[1] + n * mvref.CROSS_V[1])
        zq = scene_scan(static, pose, angles, table, walker)
        _, _, clusters = wm.detect(static, plane, mp.SCENE_REACH, SCENE_RES, pose, angles, zq, SCENE_RMAX)
        out.append([wm.cluster_world(k, 0.05, (-0.33, 1.7)) for k in clusters])
    return out


def test_cpp_tracker_equals_the_statement():
    """On the scene's detections, with every fifth scan's dropped (coasting) and a second, made-up mover that comes and goes
    (tracks opening and being dropped): within 1e-9, the margin being there because a compiler may fuse multiply-adds."""
    import kompass_cpp
    got = kompass_cpp.mapping.MoverTracker(alpha=0.5, beta=0.3, max_misses=3, gate=6 * 0.05)
    want = wm.MoverTracker(gate=6 * 0.05)
    seen = 0
    for n, clusters in enumerate(scene_detections()):
        if n % 5 == 4:
            clusters = []
        if 8 <= n < 14 or 22 <= n < 30:
            clusters = clusters + [(1.0 + 0.01 * n, 2.0 - 0.02 * n, 0.07)]
        got.update([kompass_cpp.mapping.MoverCluster(*c) for c in clusters], 0.1)
        want.update(clusters, 0.1)
        a = [(t.id, t.hits, t.misses) for t in got.tracks]
        assert a == [(t.id, t.hits, t.misses) for t in want.tracks], n
        g = np.array([(t.x, t.y, t.vx, t.vy, t.radius) for t in got.tracks]).reshape(-1, 5)
        assert np.allclose(g, np.array(want.moving_obstacles()).reshape(-1, 5), rtol=0.0, atol=1e-9), n
        assert [(o.x, o.y, o.vx, o.vy, o.radius) for o in got.moving_obstacles()] == [tuple(r) for r in g]
        seen += len(a)
    assert seen > 40 and want.next_id >= 3
    assert kompass_cpp.mapping.MoverTracker.skip_mask([0, -1, -2, 7]).tolist() == [1, 0, 0, 1]
    with pytest.raises(ValueError):
        got.update([], 0.0)


# ---- the burn-in scene ----
SCENE_RES, SCENE_RMAX, SCENE_BEAMS = 1.0, 60.0, 360
WALKER_R = 2.0


def scene_scan(static, pose, angles, table, walker):
    """The static scene's ranges by the virtual scan, shortened by the walker's disc -> zq"""
    ranges, _ = sref.scan_pose(static, SCENE_RES, pose, table, SCENE_RMAX)
    ranges = wm.shorten_by_discs(ranges, SCENE_RES, pose, angles, [(walker[0], walker[1], WALKER_R)])
    return wm.quantise_ranges(ranges, SCENE_RES, SCENE_RMAX)


def burn_in(with_mask):
    """40 scans from a standing robot -> (phantom occupied cells after each scan, static cells lost after each scan)"""
    static = mp.scene_cls()
    world = iref.IntegrateRef(mp.SCENE_W, mp.SCENE_H, SCENE_RES)
    world.set_prior(static)
    dist = dref.DistRef(world.cls, mp.SCENE_REACH)
    det = wm.MoversRef(world, dist)
    pose = (65536, 0, 75 * CELL, 56 * CELL + 32768)
    angles = -math.pi + np.arange(SCENE_BEAMS) * (2 * math.pi / SCENE_BEAMS)
    table = sref.scan_table(angles)
    occ = static == ref.OCCUPIED
    phantom, lost = [], []
    for n in range(40):
        walker = (mvref.CROSS_START[0] + n * mvref.CROSS_V[0], mvref.CROSS_START[1] + n * mvref.CROSS_V[1])
        zq = scene_scan(static, pose, angles, table, walker)
        if with_mask:
            labels, _, _ = det.detect(pose, angles, zq, SCENE_RMAX)
            zq = wm.apply_skip(zq, wm.skip_mask(labels))
        _, changed, box = world.integrate(pose, angles, zq, SCENE_RMAX)
        dist.mark(changed, box)
        now = np.asarray(world.cls) == ref.OCCUPIED
        phantom.append(int((now & ~occ).sum()))
        lost.append(int((occ & ~now).sum()))
    return phantom, lost


def mover_rows(tracks, pen=mvref.CROSS_PEN):
    """MPPI::moversOf in cells: a hit inside 3 + the tracked radius, the ramp 4 cells wider, g as moversOf forms it"""
    rows = []
    for x, y, vx, vy, rad in tracks:
        hit = 3.0 + rad / CELL
        hq, sq = round(hit * hit * 65536.0), round((hit + 4.0) ** 2 * 65536.0)
        rows.append((round(x), round(y), round(vx), round(vy), hq, sq, (200 * 65536) // (((sq - hq) >> 16) + 1)))
    return mvref.movers(rows, pen)


def closed_loop_on_scans(seed, max_steps=200, log=None):
    """mppi_movers_ref.closed_loop with the list of movers made from a simulated scan each step: detect, track, integrate
    with the skip mask, control.  Lengths in 2^-16 cells, dt = 1 step.  -> (steps or None, smallest d2, smallest q - hq
    against the walker's true centre with the scene's own hq, most clusters in one scan)"""
    static = mp.scene_cls()
    static_plane = dref.dist2_plane(static, mp.SCENE_REACH)
    world = iref.IntegrateRef(mp.SCENE_W, mp.SCENE_H, SCENE_RES)
    world.set_prior(static)
    dist = dref.DistRef(world.cls, mp.SCENE_REACH)
    det = wm.MoversRef(world, dist)
    tracker = wm.MoverTracker(gate=wm.GATE * CELL)
    angles = -math.pi + np.arange(SCENE_BEAMS) * (2 * math.pi / SCENE_BEAMS)
    table = sref.scan_table(angles)
    heads = mp._heads()
    m, c = mp.scene_model(), mp.scene_costs()
    px, py = mp.quantise_points(mp.polyline_points())
    tx, ty, h = px[0], py[0], 0
    U = [(0, 0, 0)] * mp.SCENE_T
    walker = list(mvref.CROSS_START)
    d2_min, margin, most = dref.FAR, None, 0
    for n in range(max_steps):
        pose = (int(heads[h, 0]), int(heads[h, 1]), tx, ty)
        zq = scene_scan(static, pose, angles, table, walker)
        labels, rec, clusters = det.detect(pose, angles, zq, SCENE_RMAX)
        most = max(most, rec.n_kept)
        tracker.update([wm.cluster_centre_q(k) + (wm.cluster_radius_q(k),) for k in clusters], 1.0)
        _, changed, box = world.integrate(pose, angles, wm.apply_skip(zq, wm.skip_mask(labels)), SCENE_RMAX)
        dist.mark(changed, box)
        mv = mover_rows(tracker.moving_obstacles())
        if log is not None:
            log.append((n, walker[0], walker[1], tracker.moving_obstacles()))
        wx, wy = mp.window_from(px, py, tx, ty)
        new = mvref.step(dist.field(), mp.SCENE_K, seed, m, c, wx, wy, tx, ty, h, U, n, mv)[0]
        tx, ty, h = mp.advance(tx, ty, h, *new[0])
        walker[0] += mvref.CROSS_V[0]
        walker[1] += mvref.CROSS_V[1]
        U = mp.shift(new)
        I, J = mp.cell(tx, ty)
        d2 = int(static_plane[I, J])
        d2_min = min(d2_min, d2)
        q = ((tx - walker[0]) >> 8) ** 2 + ((ty - walker[1]) >> 8) ** 2
        here = min(q, mvref.MAX_Q) - mvref.CROSS_HQ
        margin = here if margin is None else min(margin, here)
        assert here > 0 and d2 > 9, (n, here, d2)                         # at every step
        if (tx - px[-1]) ** 2 + (ty - py[-1]) ** 2 <= (3 << 15) ** 2:
            return n + 1, d2_min, margin, most
    return None, d2_min, margin, most


@pytest.mark.parametrize("seed", range(6))
def test_closed_loop_on_raw_scans(seed):
    """The crossing scene with the controller given only what detection and tracker make of a scan: arrival within 200
    steps, never inside the walker's hit distance (q > hq against its true centre, hq = 25 << 16), never within 3 cells
    of a wall (d2 > 9).  The bounds are the MPPI scene's own."""
    steps, d2_min, margin, most = closed_loop_on_scans(seed)
    print(f"seed {seed}: {steps} steps, d2 >= {d2_min}, q - hq >= {margin / 65536.0:.1f} cells^2, at most {most} clusters a scan")
    assert steps is not None and steps <= 200
    assert margin > 0 and d2_min > 9


def test_burn_in_without_the_mask_leaves_phantom_cells():
    phantom, _ = burn_in(False)
    print("phantom cells a scan, no mask:", phantom)
    assert max(phantom) >= 1


def test_burn_in_with_the_mask_leaves_the_map_as_it_was():
    phantom, lost = burn_in(True)
    print("phantom / lost a scan, masked:", phantom, lost)
    assert max(phantom) == 0 and max(lost) == 0
