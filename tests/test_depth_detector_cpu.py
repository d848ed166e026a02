"""DepthDetector surface without a GPU: the vision types with the reference's constructors, fields and validation
(datatypes/tracking.h, bindings_types.cpp:188-235), Bbox2D(PointsOfInterest) against the restatement, the
restatement against closed-form answers of the reference test's scenarios (tests/test_depth_detector.py), the
conversion-factor and frame checks, no CPU fallback, and the claims, raw intervals and chunk sizes of the edge scenes
(depth_scenes.py) that test_depth_detector_edges_gpu.py runs on the device."""
import math

import numpy as np
import pytest

import kompass_cpp
import depth_scenes
import kompass_hip as kh
from depth_detector_ref import Detector, box_from_pois
from kompass_core.datatypes import Bbox2D, Bbox3D, PointsOfInterest
from kompass_core.vision import DepthDetector

CAM = dict(depth_range=np.array([0.1, 10.0], np.float32), focal=np.array([500.0, 500.0], np.float32),
           principal=np.array([320.0, 240.0], np.float32))


def test_module_layout():
    assert kompass_cpp.vision.DepthDetector is DepthDetector
    for n in ("Bbox2D", "Bbox3D", "PointsOfInterest"):
        assert hasattr(kompass_cpp.types, n)


def test_bbox2d_fields_and_validation():
    b = Bbox2D()
    assert list(b.top_left_corner) == [0, 0] and list(b.size) == [0, 0] and list(b.img_size) == [640, 480]
    b = Bbox2D(top_left_corner=np.array([3, 4], np.int32), size=[10, 20], timestamp=1.5, label="person")
    assert list(b.top_left_corner) == [3, 4] and list(b.size) == [10, 20]
    assert b.timestamp == 1.5 and b.label == "person"
    b.size = np.array([-1, 0], np.int32)  # fields are unchecked, as in the reference
    assert list(b.size) == [-1, 0]
    c = Bbox2D(b)
    assert list(c.size) == [-1, 0] and c.label == "person"
    for bad in ([0, 5], [5, 0], [-2, 5]):
        with pytest.raises(ValueError):
            Bbox2D(top_left_corner=[0, 0], size=bad)
    with pytest.raises(ValueError):
        b.set_img_size([0, 10])
    b.set_img_size([1280, 720])
    assert list(b.img_size) == [1280, 720]
    b.set_vel([1.0, 2.0, 3.0])


def test_points_of_interest_and_bbox3d():
    p = PointsOfInterest(points=[np.array([1, 2], np.int32), [3, 4]], img_size=[10, 10], timestamp=2.0, label="x")
    assert [list(v) for v in p.points_2d] == [[1, 2], [3, 4]] and list(p.img_size) == [10, 10]
    assert p.timestamp == 2.0 and p.label == "x"
    p.set_vel([1, -1])
    assert list(p.vel) == [1, -1]
    with pytest.raises(ValueError):
        PointsOfInterest(points=[[10, 0]], img_size=[10, 10])
    with pytest.raises(ValueError):
        PointsOfInterest(points=[[0, -1]], img_size=[10, 10])
    with pytest.raises(ValueError):
        PointsOfInterest(points=[[0, 0]], img_size=[0, 10])
    with pytest.raises(ValueError):
        p.set_img_size([10, -1])
    b = Bbox3D(center=[1, 2, 3], size=[4, 5, 6], center_img_frame=[7, 8], size_img_frame=[9, 10], timestamp=0.5,
               label="y", pc_points=[[1, 1, 1]])
    assert list(b.center) == [1, 2, 3] and list(b.size) == [4, 5, 6] and list(b.center_img_frame) == [7, 8]
    assert list(b.size_img_frame) == [9, 10] and len(b.pc_points) == 1 and b.label == "y"
    assert Bbox3D(b).label == "y" and len(Bbox3D().pc_points) == 0


def test_bbox_from_pois_restatement():
    rng = np.random.default_rng(5)
    cases = [([[320, 240]], (640, 480)), ([[0, 0]], (640, 480)), ([[639, 479]], (640, 480)),
             ([[290, 220], [310, 230], [320, 240], [330, 250], [350, 260]], (640, 480))]
    for _ in range(20):
        w, h = int(rng.integers(1, 700)), int(rng.integers(1, 500))
        n = int(rng.integers(1, 30))
        cases.append((np.stack([rng.integers(0, w, n), rng.integers(0, h, n)], 1).tolist(), (w, h)))
    # the 5-point cluster: medians (320, 240), MADs (10, 10) -> half sizes 20: box (300, 220) + (40, 40)
    assert box_from_pois(cases[3][0], cases[3][1]) == (300, 220, 40, 40)
    assert box_from_pois([[320, 240]], (640, 480)) == (315, 235, 10, 10)
    assert box_from_pois([[0, 0]], (640, 480)) == (0, 0, 5, 5)
    for pts, size in cases:
        poi = PointsOfInterest(points=pts, img_size=list(size))
        assert poi.points_2d is not None
        assert box_from_pois(pts, size)[0] >= 0
    with pytest.raises(ValueError):
        box_from_pois([], (640, 480))


def test_restatement_closed_forms():
    """The reference test's scenarios, answered in closed form: a 3 m box on the principal point."""
    img = np.zeros((480, 640), np.uint16, order="F")
    img[190:290, 270:370] = 3000
    det = Detector(CAM["depth_range"], [0, 0, 0], [0, 0, 0, 1], CAM["focal"], CAM["principal"], 1e-3)
    box = (270, 190, 100, 100)  # covers rows / columns 190..290, 270..370 inclusive: 101 x 101 pixels
    (n, med, mad, mn, mx), = det.stats(img, [box])
    d3 = np.float32(3000) * np.float32(1e-3)
    assert n == 100 * 100 and med == d3 and mad == 0 and mn == mx == d3
    c, s, idx = det.boxes(img, [box], state=(0.0, 0.0, 0.0))
    assert list(idx) == [0]
    np.testing.assert_allclose(c[0], [3.0, 0.0, 0.0], atol=1e-6)
    np.testing.assert_allclose(s[0], [0.0, 100 * 3.0 / 500, 100 * 3.0 / 500], rtol=1e-6, atol=0)
    c, _, _ = det.boxes(img, [box], state=(10.0, 5.0, 0.0))
    np.testing.assert_allclose(c[0], [13.0, 5.0, 0.0], atol=1e-5)
    # yaw = pi/2: 3 m ahead of the robot is +y in the world
    c, _, _ = det.boxes(img, [box], state=(1.0, 2.0, math.pi / 2))
    np.testing.assert_allclose(c[0], [1.0, 5.0, 0.0], atol=1e-5)
    # None keeps the previous body_in_world
    c2, _, _ = det.boxes(img, [box])
    np.testing.assert_array_equal(c, c2)
    # the POI variants: one point on the principal point, and a symmetric 5-point cluster
    poi_img = np.zeros((480, 640), np.uint16, order="F")
    poi_img[80:400, 160:480] = 3000
    for pts in ([[320, 240]], [[290, 220], [310, 230], [320, 240], [330, 250], [350, 260]]):
        b = box_from_pois(pts, (640, 480))
        c, _, _ = det.boxes(poi_img, [b], state=(10.0, 5.0, 0.0))
        np.testing.assert_allclose(c[0], [13.0, 5.0, 0.0], atol=1e-5)
    # nothing in range, and one value only: dropped
    assert len(det.boxes(np.zeros((480, 640), np.uint16), [box])[2]) == 0
    one = np.zeros((480, 640), np.uint16)
    one[200, 300] = 3000
    assert det.stats(one, [box])[0][0] == 1 and len(det.boxes(one, [box])[2]) == 0


def test_restatement_median_and_band():
    img = np.array([[1, 2, 3, 4, 10]], np.uint16)  # 1, 2, 3, 4, 10 m
    det = Detector([0.0, 100.0], [0, 0, 0], [0, 0, 0, 1], [1, 1], [0, 0], 1.0)
    (n, med, mad, mn, mx), = det.stats(img, [(0, 0, 4, 0)])
    # median 3, |dev| = 2, 1, 0, 1, 7 -> MAD 1; band [1.5, 4.5]: min 2, max 4
    assert (n, float(med), float(mad), float(mn), float(mx)) == (5, 3.0, 1.0, 2.0, 4.0)
    (n, med, mad, _, _), = det.stats(img, [(0, 0, 3, 0)])  # 1, 2, 3, 4: even
    assert (n, float(med), float(mad)) == (4, 2.5, 1.0)


def scene_on_restatement(name):
    """(stats, kept) of every box of a scene, from the restatement alone."""
    frame, boxes, depth_range, factor, claim = depth_scenes.SCENES[name].build()
    det = Detector(np.array(depth_range, np.float32), [0, 0, 0], [0, 0, 0, 1], [1, 1], [0, 0], factor)
    kept = [depth_scenes.kept_values(frame, b, depth_range, factor) for b in boxes]
    return det.stats(frame, boxes), kept, claim


@pytest.mark.parametrize("name", list(depth_scenes.SCENES))
def test_scene_claims_hold_on_the_restatement(name):
    """Every edge scene of test_depth_detector_edges_gpu.py is what it says it is: its claim holds on the
    restatement's statistics and on the kept values, and the restatement counted exactly the kept values."""
    assert depth_scenes.SCENES[name].build()[3] in (1.0, 0.5)
    stats, kept, claim = scene_on_restatement(name)
    assert [s[0] for s in stats] == [len(k) for k in kept]
    assert claim(stats, kept)


@pytest.mark.parametrize("name", list(depth_scenes.SCENES))
def test_scene_raw_interval_and_chunk(name):
    """The raw interval [d_lo, d_lo + nbins) by the rule of kc_depth_create (convert all 65536 values, keep
    min <= v <= max), recomputed value by value, and the chunk size it selects."""
    scene = depth_scenes.SCENES[name]
    _, _, depth_range, factor, _ = scene.build()
    lo, hi = -1, -2
    for d in range(65536):
        v = np.float32(d) * np.float32(factor)
        if v <= np.float32(depth_range[1]) and v >= np.float32(depth_range[0]):
            lo, hi = (d if lo < 0 else lo), d
        elif lo >= 0:
            break  # float(d) * factor is non-decreasing: nothing is kept after the first value above max
    assert (lo, hi - lo + 1) == depth_scenes.raw_interval(depth_range, factor)
    assert hi - lo + 1 == scene.nbins
    assert scene.chunk == (8192 if scene.nbins <= 16384 else 32768)
    if name.startswith(("counter_", "chunk_")):  # named after the chunk size they are built for
        assert scene.chunk == next(int(t) for t in name.split("_") if t in ("8192", "32768"))


def test_conversion_factor_and_frame_checks():
    args = (CAM["depth_range"], [0, 0, 0], [0, 0, 0, 1], CAM["focal"], CAM["principal"])
    for bad in (0.0, -1e-3, float("nan"), float("inf"), 1e36):
        with pytest.raises(ValueError):
            DepthDetector(*args, bad)
        with pytest.raises(ValueError):
            kh.DepthContext(*args, bad)
        with pytest.raises(ValueError):
            Detector(*args, bad)
    DepthDetector(*args, 1.0)
    DepthDetector([5.0, 1.0], [0, 0, 0], [0, 0, 0, 1], [1, 1], [0, 0])  # min > max: accepted (yields no boxes)
    d = DepthDetector(*args)
    b = Bbox2D(top_left_corner=[0, 0], size=[4, 4])
    with pytest.raises(TypeError):
        d.compute_3d_detections(np.zeros((8, 8), np.int32), [b], 0.0, 0.0, 0.0, 0.0)
    with pytest.raises(TypeError):
        d.compute_3d_detections(np.zeros((8, 8), np.float32), [b], 0.0, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        d.compute_3d_detections(np.zeros((2, 8, 8), np.uint16), [b], 0.0, 0.0, 0.0, 0.0)
    ctx = kh.DepthContext(*args)
    with pytest.raises(TypeError):
        ctx.boxes(np.zeros((8, 8), np.float64), [[0, 0, 4, 4]])


def test_no_cpu_fallback():
    """Without a visible device the compute call raises; with one it computes (there is no CPU path)."""
    img = np.full((16, 16), 1000, np.uint16)
    d = DepthDetector(CAM["depth_range"], [0, 0, 0], [0, 0, 0, 1], CAM["focal"], CAM["principal"])
    ctx = kh.DepthContext(CAM["depth_range"], [0, 0, 0], [0, 0, 0, 1], CAM["focal"], CAM["principal"])
    b = Bbox2D(top_left_corner=[2, 2], size=[4, 4])
    if kh.device_count() == 0:
        with pytest.raises(RuntimeError):
            d.compute_3d_detections(img, [b], 0.0, 0.0, 0.0, 0.0)
        with pytest.raises(kh.KompassHipError):
            ctx.boxes(img, [[2, 2, 4, 4]])
    else:
        assert len(d.compute_3d_detections(img, [b], 0.0, 0.0, 0.0, 0.0)) == 1
        assert len(ctx.boxes(img, [[2, 2, 4, 4]])[2]) == 1
