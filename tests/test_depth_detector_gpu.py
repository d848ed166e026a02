"""DepthDetector on the MI355X against the independent restatement (depth_detector_ref.py), bit for bit: every
centre and size float, the kept-index list, and the five per-box statistics of kc_depth_box_stats.

golden/bag_image_depth.npz (key "depth") is the reference's test frame tests/resources/control/bag_image_depth.tif,
a real 1280x720 uint16 depth frame in mm, converted once to npz (data only)."""
import math
from pathlib import Path

import numpy as np
import pytest

from depth_detector_ref import Detector, box_from_pois
from helpers import DeviceArray

pytestmark = pytest.mark.gpu

FIXTURE = Path(__file__).resolve().parent / "golden" / "bag_image_depth.npz"
FOCAL, PRINCIPAL = [911.0, 910.5], [640.5, 360.25]
TILT = [0.1, 0.02, 0.3], [0.0, 0.2588190451, 0.0, 0.9659258263]  # camera 30 degrees pitched, off-centre
STATES = [(0.0, 0.0, 0.0), (10.0, 5.0, 0.0), (-3.5, 2.25, 1.0), (1.0, -2.0, math.pi), (0.5, 0.5, -math.pi),
          (100.0, -40.0, -2.5)]


def fixture():
    return np.load(FIXTURE)["depth"]


def synthetic(seed, h=240, w=320):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 6000, (h, w)).astype(np.uint16)
    img[rng.random((h, w)) < 0.1] = 0
    img[h // 4:h // 2, w // 4:w // 2] = 2500  # a constant block (MAD = 0)
    return img


def edge_boxes(h, w):
    return [(0, 0, 0, 0), (0, 0, w - 1, h - 1), (0, 0, w, h), (-5, -7, w + 20, h + 30), (w - 3, 10, 10, 10),
            (10, h - 2, 30, 5), (w - 1, h - 1, 0, 0), (w, 0, 5, 5), (0, h, 5, 5), (-10, -10, 5, 5), (-3, 5, 5, 5),
            (5, -3, 5, 5), (20, 20, -1, 10), (20, 20, 10, -4), (20, 20, 0, 40), (20, 20, 40, 0), (3, 4, 1, 1),
            (2**31 - 10, 5, 100, 100), (5, 2**31 - 10, 100, 100), (-2**31, -2**31, 2**31 - 1, 2**31 - 1),
            (-2**31, 5, 2**31 - 1, 8), (w // 3, h // 3, w // 2, h // 2)]


def random_boxes(rng, n, h, w, big=False):
    out = []
    for _ in range(n):
        sx = int(rng.integers(0, w if big else 80))
        sy = int(rng.integers(0, h if big else 80))
        out.append((int(rng.integers(-20, w)), int(rng.integers(-20, h)), sx, sy))
    return out


def check(ctx, det, img, boxes, state=None, host=None, **frame):
    """Statistics and boxes of one call against the restatement; `host` is the frame when `img` lives on the
    device.  Returns the number of kept boxes."""
    ref_img = img if host is None else host
    cnt, st = ctx.box_stats(img, boxes, **frame)
    for i, r in enumerate(det.stats(ref_img, boxes)):
        assert cnt[i] == r[0], f"box {i} {boxes[i]}: count {cnt[i]} vs {r[0]}"
        if r[0] > 1:
            np.testing.assert_array_equal(st[i].view(np.uint32), np.array(r[1:], np.float32).view(np.uint32),
                                          err_msg=f"box {i} {boxes[i]}")
    c, s, idx = ctx.boxes(img, boxes, state=state, **frame)
    rc, rs, ridx = det.boxes(ref_img, boxes, state=state)
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(c.view(np.uint32), rc.view(np.uint32))
    np.testing.assert_array_equal(s.view(np.uint32), rs.view(np.uint32))
    return len(idx)


def pair(depth_range=(0.1, 10.0), factor=1e-3, mount=([0, 0, 0], [0, 0, 0, 1])):
    import kompass_hip as kh

    args = (np.array(depth_range, np.float32), mount[0], mount[1], FOCAL, PRINCIPAL, factor)
    return kh.DepthContext(*args), Detector(*args)


@pytest.mark.parametrize("depth_range,factor", [((0.1, 10.0), 1e-3), ((0.0, 1e3), 1e-3), ((0.05, 3.0), 2.5e-4),
                                                ((0.0, 4000.0), 1.0), ((1.0, 2.0), 1e-3)])
def test_fixture_boxes(depth_range, factor):
    img = fixture()
    ctx, det = pair(depth_range, factor)
    rng = np.random.default_rng(int(factor * 1e4) + int(depth_range[1]))
    h, w = img.shape
    boxes = edge_boxes(h, w) + random_boxes(rng, 24, h, w) + random_boxes(rng, 6, h, w, big=True)
    kept = check(ctx, det, img, boxes, state=(1.0, 2.0, 0.3))
    assert kept > 5


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_synthetic_frames_every_count(seed):
    img = synthetic(seed)
    h, w = img.shape
    ctx, det = pair((0.0, 1e3), 1e-3)
    rng = np.random.default_rng(seed)
    for n in (1, 8, 64, 256):
        boxes = random_boxes(rng, n, h, w, big=(n == 8))
        if n == 64:
            boxes[10:20] = boxes[:10]  # duplicated
        check(ctx, det, img, boxes, state=STATES[n % len(STATES)])
    check(ctx, det, img, edge_boxes(h, w))


def test_kept_pixel_counts_and_constant_depth():
    ctx, det = pair((0.0, 10.0), 1e-3)
    img = np.zeros((64, 64), np.uint16)
    img[10, 10] = 2000          # one kept pixel (min_depth = 0 keeps the zeros too)
    img[30:40, 30:40] = 1234    # constant depth: MAD 0
    img[50, 50:52] = (1000, 3000)
    boxes = [(10, 10, 0, 0), (9, 9, 2, 2), (30, 30, 9, 9), (30, 30, 10, 10), (50, 50, 1, 0), (49, 49, 3, 3)]
    check(ctx, det, img, boxes, state=(0.0, 0.0, 0.0))
    ctx2, det2 = pair((0.5, 10.0), 1e-3)  # zeros out of range: 1, 1, 100, 100, 2 and 2 kept pixels
    cnt, _ = ctx2.box_stats(img, boxes)
    assert list(cnt) == [1, 1, 100, 100, 2, 2]
    assert check(ctx2, det2, img, boxes) == 4
    # min > max: accepted, nothing kept
    ctx3, det3 = pair((5.0, 1.0), 1e-3)
    assert check(ctx3, det3, img, boxes) == 0


def test_full_value_range_and_large_boxes():
    rng = np.random.default_rng(9)
    img = rng.integers(0, 65536, (720, 1280)).astype(np.uint16)
    for depth_range, factor in (((0.0, 1e3), 1e-3), ((0.0, 70000.0), 1.0)):
        ctx, det = pair(depth_range, factor)
        check(ctx, det, img, [(0, 0, 1279, 719), (100, 100, 600, 400), (5, 5, 63, 63), (0, 0, 2000, 2000)],
              state=(0.0, 0.0, 0.0))


def test_memory_orders_and_views():
    base = fixture()
    ctx, det = pair((0.1, 10.0), 1e-3)
    h, w = base.shape
    boxes = edge_boxes(h, w)[:12] + [(100, 50, 300, 200), (600, 300, 200, 200)]
    for img in (base, np.asfortranarray(base), base[::2, ::3], np.asfortranarray(base)[1::3, ::2], base[::-1, :],
                base[:, 100:900], base.T.copy().T):
        hh, ww = img.shape
        bx = [b for b in boxes] + [(ww // 4, hh // 4, ww // 2, hh // 2)]
        check(ctx, det, img, bx, state=(1.0, 2.0, 0.5))


def device_frame(host, order="C"):
    """A device copy of a host frame in the given memory order, and the keywords that describe it."""
    a = np.ascontiguousarray(host) if order == "C" else np.asfortranarray(host)
    dev = DeviceArray(a)
    return dev, dict(device_ptr=dev.ptr, shape=a.shape, strides=[v // 2 for v in a.strides])


def test_device_resident_frame():
    img = fixture()
    ctx, det = pair((0.1, 10.0), 1e-3)
    boxes = edge_boxes(*img.shape) + [(100, 50, 300, 200)]
    for order in ("C", "F"):
        dev, frame = device_frame(img, order)
        with dev:
            check(ctx, det, None, boxes, state=(3.0, 4.0, -1.0), host=img, **frame)
            assert ctx.last_upload() == 0


def test_states_mount_and_repeated_calls():
    img = fixture()
    ctx, det = pair((0.1, 10.0), 1e-3, TILT)
    rng = np.random.default_rng(4)
    h, w = img.shape
    for k, st in enumerate(STATES):
        boxes = random_boxes(rng, [3, 40, 1, 7, 120, 2][k], h, w, big=(k % 2 == 0))
        check(ctx, det, img, boxes, state=st)
        check(ctx, det, img, boxes[:1], state=None)  # keeps the previous body_in_world
    assert check(ctx, det, img, [], state=(1.0, 1.0, 1.0)) == 0


def test_upload_is_the_bounding_rectangle():
    img = fixture()
    ctx, _ = pair((0.1, 10.0), 1e-3)
    cases = [([(100, 50, 63, 63)], 64 * 64), ([(100, 50, 63, 63), (300, 200, 9, 9)], 210 * 160),
             ([(-10, -10, 19, 9), (1270, 710, 50, 50)], 10 * 10), ([(-10, -10, 19, 19), (1270, 710, 50, 50)], 1280 * 720), ([(0, 0, 1279, 719)] * 8, 1280 * 720),
             ([(2000, 0, 5, 5)], 0), ([(5, 5, -1, 3)], 0)]
    for boxes, pixels in cases:
        for frame in (img, np.asfortranarray(img), img[::1, ::1]):
            ctx.box_stats(frame, boxes)
            assert ctx.last_upload() == 2 * pixels, (boxes, ctx.last_upload())
    ctx.box_stats(img[::2, ::3], [(10, 10, 9, 19)])
    assert ctx.last_upload() == 2 * 10 * 20


def test_compute_3d_detections_both_overloads():
    from kompass_core.datatypes import Bbox2D, PointsOfInterest
    from kompass_core.vision import DepthDetector

    img = fixture()
    mount = TILT
    d = DepthDetector(np.array([0.1, 10.0], np.float32), mount[0], mount[1], FOCAL, PRINCIPAL, 1e-3)
    det = Detector(np.array([0.1, 10.0], np.float32), mount[0], mount[1], FOCAL, PRINCIPAL, 1e-3)
    rng = np.random.default_rng(2)
    boxes = random_boxes(rng, 12, *img.shape) + [(1270, 700, 30, 30), (5, 5, -2, 4)]
    b2 = []
    for tx, ty, sx, sy in boxes:
        b = Bbox2D()
        b.top_left_corner = np.array([tx, ty], np.int32)
        b.size = np.array([sx, sy], np.int32)
        b.label, b.timestamp = f"b{tx}", 0.25
        b2.append(b)
    for st in STATES[:4]:
        fst = tuple(float(np.float32(v)) for v in st)
        for frame in (img, np.asfortranarray(img)):
            res = d.compute_3d_detections(frame, b2, *st, 0.0)
            c, s, idx = det.boxes(img, boxes, state=fst)
            assert len(res) == len(idx)
            for r, i, cc, ss in zip(res, idx, c, s):
                np.testing.assert_array_equal(np.asarray(r.center, np.float32).view(np.uint32), cc.view(np.uint32))
                np.testing.assert_array_equal(np.asarray(r.size, np.float32).view(np.uint32), ss.view(np.uint32))
                tx, ty, sx, sy = boxes[i]
                assert list(r.center_img_frame) == [tx + int(sx / 2), ty + int(sy / 2)]
                assert list(r.size_img_frame) == [sx, sy] and r.label == f"b{tx}" and len(r.pc_points) == 0
    pts = [[600, 300], [640, 360], [700, 380], [650, 350], [620, 330]]
    poi = PointsOfInterest(points=pts, img_size=[1280, 720])
    res = d.compute_3d_detections(img, poi, 2.0, 1.0, 0.5, 0.0)
    c, s, idx = det.boxes(img, [box_from_pois(pts, (1280, 720))], state=(2.0, 1.0, 0.5))
    assert len(res) == len(idx) == 1
    np.testing.assert_array_equal(np.asarray(res[0].center, np.float32).view(np.uint32), c[0].view(np.uint32))
    np.testing.assert_array_equal(np.asarray(res[0].size, np.float32).view(np.uint32), s[0].view(np.uint32))
    assert d.compute_3d_detections(img, [], 0.0, 0.0, 0.0, 0.0) == []


def test_reference_scenarios_on_device():
    """tests/test_depth_detector.py of the reference: a 3 m box on the principal point."""
    from kompass_core.datatypes import Bbox2D
    from kompass_core.vision import DepthDetector

    d = DepthDetector(np.array([0.1, 10.0], np.float32), np.zeros(3, np.float32),
                      np.array([0, 0, 0, 1], np.float32), np.array([500.0, 500.0], np.float32),
                      np.array([320.0, 240.0], np.float32), 1e-3)
    img = np.zeros((480, 640), np.uint16, order="F")
    img[190:290, 270:370] = 3000
    b = Bbox2D()
    b.top_left_corner = np.array([270, 190], np.int32)
    b.size = np.array([100, 100], np.int32)
    r = d.compute_3d_detections(img, [b], 0.0, 0.0, 0.0, 0.0)
    np.testing.assert_allclose(r[0].center, [3.0, 0.0, 0.0], atol=1e-5)
    r = d.compute_3d_detections(img, [b], 10.0, 5.0, 0.0, 0.0)
    np.testing.assert_allclose(r[0].center, [13.0, 5.0, 0.0], atol=1e-5)
