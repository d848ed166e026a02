"""Finding movers in a scan on the device (kc_worldmap_movers; DESIGN.md 4.11 rules 64 to 69) against the Python statement
tests/worldmap_movers_ref.py: labels, record and clusters bit for bit.  The distance plane the statement reads is the
brute-force one of the whole map (worldmap_dist_ref.dist2_plane), so the device's lazy refresh is under test as well.

The flag kernel's workgroups are 256 beams of four wavefronts; the cluster kernel's lane t owns the beams [t C, (t + 1) C)
with C = ceil(B / 1024): one beam a lane up to 1024 beams, two from 1025 on, five at 4097, 64 at 65536."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import kompass_hip as kh  # noqa: E402
import worldmap_dist_ref as dref  # noqa: E402
import worldmap_integrate_ref as iref  # noqa: E402
import worldmap_movers_cases as cases  # noqa: E402
import worldmap_movers_ref as wm  # noqa: E402
import worldmap_ref as ref  # noqa: E402
import worldmap_shift_ref as shref  # noqa: E402

RES, CELL = cases.RES, cases.CELL


@pytest.fixture(scope="module", autouse=True)
def _device():
    assert kh.device_count() >= 1, "no HIP device visible"


def pose_of(q):
    return kh.WorldMapPose(int(q[0]), int(q[1]), int(q[2]), int(q[3]))


def want_of(cls, reach, q, angles, zq, range_max, cfg):
    return wm.detect(cls, dref.dist2_plane(cls, reach), reach, RES, q, angles, zq, range_max, **cfg)


def assert_same(got, want, what=""):
    labels, rec, clusters = got
    w_labels, w_rec, w_clusters = want
    assert rec == tuple(w_rec), (what, rec, w_rec)
    assert clusters == [tuple(c) for c in w_clusters], what
    assert labels.dtype == np.int32 and labels.tobytes() == w_labels.tobytes(), (what, np.flatnonzero(labels != w_labels)[:8])


def run(c, ctx=None):
    """the case on a fresh map (or on ctx) -> the statement's answer, after the device's has been found equal"""
    own = ctx is None
    if own:
        ctx = kh.WorldMapContext(c["cls"].shape[0], c["cls"].shape[1], RES, (0.0, 0.0))
        ctx.set_prior(c["cls"])
        ctx.set_distance(c["reach"])
    try:
        got = ctx.movers(pose_of(c["pose"]), c["angles"], c["zq"], c["range_max"], **c["cfg"])
        want = want_of(c["cls"], c["reach"], c["pose"], c["angles"], c["zq"], c["range_max"], c["cfg"])
        assert_same(got, want)
        if c["labels"] is not None:
            assert got[0].tolist() == c["labels"].tolist()
        return want
    finally:
        if own:
            ctx.close()


def test_rule_66_edges():
    _, rec, _ = run(cases.rule66_case())
    assert rec.n_dynamic == 4


@pytest.mark.parametrize("name", sorted(cases.rule67_cases()))
def test_rule_67_edges(name):
    run(cases.rule67_cases()[name])


def test_room_scene_360_beams():
    _, rec, _ = run(cases.pattern_case(360, 1))
    assert rec.n_kept >= 4 and rec.n_runs > rec.n_kept          # kept and dropped runs both occur


@pytest.mark.parametrize("n_beams", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_beam_counts(n_beams):
    _, rec, _ = run(cases.pattern_case(n_beams, 100 + n_beams))
    assert rec.n_dynamic >= 1


def test_runs_across_wavefront_workgroup_and_chunk_boundaries():
    """No beam knocked out around beams 63 | 64 (a wavefront of the flag kernel), 255 | 256 (its workgroup) and, at 4097
    beams with five a lane, 1279 | 1280 and 2559 | 2560 (chunks of the cluster kernel; every one of the others is a chunk
    boundary up to 1024 beams): the runs there must cross."""
    for n_beams, edges in ((512, (64, 256)), (4097, (64, 256, 1280, 2560))):
        c = cases.pattern_case(n_beams, 7, jump=0.0)
        for e in edges:
            c["zq"][e - 6:e + 6] = np.rint((10.0 + 3.0 * np.sin(5.0 * c["angles"][e - 6:e + 6])) * CELL).astype(np.int32)
        labels, _, _ = run(c)
        for e in edges:
            assert labels[e - 1] == labels[e] >= 0, (n_beams, e)


def test_alternating_beams_beyond_the_returned_clusters():
    labels, rec, clusters = run(cases.alternating_case())
    assert rec == wm.Record(512, 512, 512, 256) and len(clusters) == 256 and labels.max() == 511


def test_65536_beams_in_one_run():
    c = cases.pattern_case(65536, 3, knock=0.0, jump=0.0)
    _, rec, (k,) = run(c)
    assert rec == wm.Record(65536, 1, 1, 1) and (k.k_first, k.k_last, k.n) == (0, 65535, 65536)
    assert abs(k.sx) > 1 << 36                                    # the sums pass 32 bits by far


def test_no_dynamic_beam():
    c = cases.pattern_case(300, 5)
    zmax = kh.worldmap_movers_check(RES, 300, c["range_max"])
    c["zq"][:] = zmax
    c["zq"][::3] = -1
    labels, rec, clusters = run(c)
    assert rec == wm.Record(0, 0, 0, 0) and clusters == [] and (labels == -1).all()
    # and returns that all end in the wall
    c = cases.pattern_case(300, 5)
    c["zq"][:] = np.int32(23.4 * CELL)
    c["angles"] = np.linspace(-0.2, 0.2, 300)
    c["pose"] = cases.centre_pose(24, 24, 0.0)
    _, rec, _ = run(c)
    assert rec.n_dynamic == 0


def test_pose_outside_the_map():
    far = cases.pattern_case(200, 9, pose_cell=(-30.0, 24.0))     # no endpoint reaches the map
    _, rec, _ = run(far)
    assert rec.n_dynamic == 0
    near = cases.pattern_case(200, 9, pose_cell=(-4.0, 24.0))     # some do
    _, rec, _ = run(near)
    assert 0 < rec.n_dynamic < 200


def test_behind_an_integration_and_a_shift():
    """One context: a detection, an integrate that changes cells and leaves the plane's box dirty, a detection (the lazy
    refresh), a shift of the window, a detection with the pose re-expressed by the caller (rule 46)."""
    c = cases.pattern_case(360, 11)
    W, H = c["cls"].shape
    with kh.WorldMapContext(W, H, RES, (0.0, 0.0)) as ctx:
        world = iref.IntegrateRef(W, H, RES, (0.0, 0.0))
        ctx.set_model(hit=12)                                     # one hit turns a cell of the prior's e_min = -8
        world.set_model(hit=12)
        ctx.set_prior(c["cls"])
        world.set_prior(c["cls"])
        ctx.set_distance(c["reach"])
        p = pose_of(c["pose"])
        run(dict(c, cls=np.array(world.cls)), ctx)
        # a scan of short returns burns occupied cells in: the next detection sees fewer dynamic beams around them
        zq_in = c["zq"].copy()
        changed, box = ctx.integrate(p, c["angles"], zq_in, c["range_max"])
        _, w_changed, w_box = world.integrate(c["pose"], c["angles"], zq_in, c["range_max"])
        assert (changed, box) == (w_changed, w_box) and changed > 0
        _, rec, _ = run(dict(c, cls=np.array(world.cls)), ctx)
        assert rec.n_dynamic < int((c["zq"] >= 0).sum())
        assert ctx.distance_info()[2][0] >= 0                     # the call refreshed a box
        run(dict(c, cls=np.array(world.cls)), ctx)                # and a clean plane launches no refresh
        assert ctx.distance_info()[2] == (-1, -1, -1, -1)
        di, dj = 5, -3
        ctx.shift(di, dj)
        world.evidence, world.cls = shref.shift_planes(world.evidence, world.cls, di, dj)
        q = c["pose"]
        moved = (q[0], q[1], q[2] - di * CELL, q[3] - dj * CELL)
        assert ctx.offset() == (di, dj)
        run(dict(c, cls=np.array(world.cls), pose=moved), ctx)    # the same returns end in or beside the cells they burnt in
        nearer = np.where(c["zq"] >= 0, c["zq"] - 3 * CELL, -1).astype(np.int32)   # three cells in front of them: free, dist2 >= 9
        _, rec, _ = run(dict(c, cls=np.array(world.cls), pose=moved, zq=nearer), ctx)
        assert rec.n_dynamic > 0


def test_state_refusals_queue_nothing():
    c = cases.rule66_case()
    with kh.WorldMapContext(c["cls"].shape[0], c["cls"].shape[1], RES, (0.0, 0.0)) as ctx:
        ctx.set_prior(c["cls"])
        p = pose_of(c["pose"])
        with pytest.raises(kh.KompassHipError, match="distance plane"):
            ctx.movers(p, c["angles"], c["zq"], c["range_max"])
        ctx.set_distance(2)
        with pytest.raises(kh.KompassHipError, match="reach"):
            ctx.movers(p, c["angles"], c["zq"], c["range_max"], m2=5)
        assert ctx.distance_info()[2:] == ((-1, -1, -1, -1), False)   # the refused call did not refresh the plane
        got = ctx.movers(p, c["angles"], c["zq"], c["range_max"], m2=4, gap=0, join_q=0, min_beams=1)
        assert ctx.distance_info()[3]                                  # this one did, the whole map
        assert_same(got, want_of(c["cls"], 2, c["pose"], c["angles"], c["zq"], c["range_max"], dict(m2=4, gap=0, join_q=0, min_beams=1)))
        # rule 70 and the pose, through the call
        with pytest.raises(ValueError):
            ctx.movers(p, c["angles"], c["zq"], c["range_max"], m2=0)
        with pytest.raises(IndexError):
            ctx.movers(kh.WorldMapPose(65536, 0, (1 << 36) + 1, 0), c["angles"], c["zq"], c["range_max"])
        with pytest.raises(ValueError):
            ctx.movers(p, [float("nan")] * len(c["zq"]), c["zq"], c["range_max"])


def test_without_labels_and_timing():
    c = cases.pattern_case(360, 1)
    with kh.WorldMapContext(48, 48, RES, (0.0, 0.0)) as ctx:
        ctx.set_prior(c["cls"])
        ctx.set_distance(c["reach"])
        with pytest.raises(kh.KompassHipError):
            ctx.movers_times()
        ctx.movers_set_timing(True)
        labels, rec, clusters = ctx.movers(pose_of(c["pose"]), c["angles"], c["zq"], c["range_max"], return_labels=False, **c["cfg"])
        want = want_of(c["cls"], c["reach"], c["pose"], c["angles"], c["zq"], c["range_max"], c["cfg"])
        assert labels is None and rec == tuple(want[1]) and clusters == [tuple(k) for k in want[2]]
        flag_ms, cluster_ms = ctx.movers_times()
        assert flag_ms > 0.0 and cluster_ms > 0.0
