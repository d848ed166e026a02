"""RGBDFollower on the MI355X: closed loops on depth frames rendered inside the test (a background, the target box
at its depth, distractors of the same and of other labels, re-rendered as the robot moves) against the
restatement (rgbd_follower_ref.py, the pixel part by depth_detector_ref.py) step by step; initial tracking by a
click on the reference's depth frame; a torch device frame against the same host frame; the upload and the
one-call-per-frame rules."""
import math
from pathlib import Path

import numpy as np
import pytest

import kompass_cpp
import rgbd_follower_ref as ref
from depth_detector_ref import Detector
from test_vision_follower_cpu import ATOL, RTOL, cpp_box, limits, params, step_both

pytestmark = pytest.mark.gpu

C = kompass_cpp.control
T = kompass_cpp.types
FIXTURE = Path(__file__).resolve().parent / "golden" / "bag_image_depth.npz"
W, H = 640, 480
FOCAL, PRINCIPAL = (525.0, 525.0), (319.5, 239.5)
DEPTH_RANGE = (0.1, 10.0)
MOUNT = ([0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0])


def make(cfg, mount=MOUNT):
    f = C.RGBDFollower(C.ControlType.DIFFERENTIAL_DRIVE, limits(), T.RobotGeometry.CYLINDER, [0.3, 0.6], mount[0],
                       mount[1], params(cfg))
    f.set_camera_intrinsics(FOCAL[0], FOCAL[1], PRINCIPAL[0], PRINCIPAL[1])
    r = ref.Follower(cfg, 0.3, 1.0, 2.0)
    det = Detector(np.array(DEPTH_RANGE, np.float32), mount[0], mount[1], FOCAL, PRINCIPAL, 1e-3)
    return f, r, det


def render(objects, rng=None):
    """objects: (x_body, y_body, width, height, label) seen by a forward camera at the body origin; returns the
    uint16 frame in mm and the 2-D boxes (top.x, top.y, size.x, size.y, label) of the visible ones."""
    img = np.full((H, W), 7000, np.uint16)
    if rng is not None:
        img[rng.random((H, W)) < 0.02] = 0  # holes
    boxes = []
    for x, y, w, h, label in sorted(objects, key=lambda o: -o[0]):  # far to near
        if x <= 0.2:
            continue
        u = PRINCIPAL[0] - y * FOCAL[0] / x
        sx, sy = int(w * FOCAL[0] / x), int(h * FOCAL[1] / x)
        tx, ty = int(u - sx / 2), int(PRINCIPAL[1] - sy / 2)
        x0, x1, y0, y1 = max(tx, 0), min(tx + sx, W - 1), max(ty, 0), min(ty + sy, H - 1)
        if x0 > x1 or y0 > y1 or sx < 2 or sy < 2:
            continue
        img[y0:y1 + 1, x0:x1 + 1] = int(x * 1000)
        boxes.append((tx, ty, sx, sy, label))
    return img, boxes


def to_2d(boxes):
    return [T.Bbox2D([b[0], b[1]], [b[2], b[3]], 0.0, b[4]) for b in boxes]


def ref_boxes(det, img, boxes, label, state=None):
    """The restatement's 3-D boxes of the tracked label (what the follower sends to the device)."""
    same = [b for b in boxes if b[4] == label]
    cs, ss, idx = det.boxes(img, [b[:4] for b in same], state=state)
    out = []
    for c, s, i in zip(cs, ss, idx):
        tx, ty, sx, sy, lab = same[i]
        out.append(ref.Box(c, s, lab, 0.0, (tx + int(sx / 2), ty + int(sy / 2)), (sx, sy)))
    return out


def body_of(px, py, x, y, yaw):
    dx, dy = px - x, py - y
    return math.cos(yaw) * dx + math.sin(yaw) * dy, -math.sin(yaw) * dx + math.cos(yaw) * dy


SCENES = [
    ("local", ref.Config(prediction_horizon=10, target_distance=0.8, distance_tolerance=0.05)),
    ("local-search", ref.Config(prediction_horizon=8, control_horizon=3, target_distance=0.6, enable_search=True,
                                target_search_timeout=1.5)),
    ("global", ref.Config(prediction_horizon=10, use_local_coordinates=False, target_distance=0.7,
                          target_orientation=-0.2)),
]


@pytest.mark.parametrize("name,cfg", SCENES, ids=[s[0] for s in SCENES])
def test_closed_loop_matches_the_restatement(name, cfg):
    rng = np.random.default_rng(len(name))
    f, r, det = make(cfg)
    x = y = yaw = 0.0
    target = [3.0, 0.4]

    def scene(k):
        tb = body_of(target[0], target[1], x, y, yaw)
        objs = [(tb[0], tb[1], 0.5, 1.2, "person")]
        d1 = body_of(target[0] + 2.0, target[1] - 1.2, x, y, yaw)
        objs.append((d1[0], d1[1], 0.4, 1.0, "person"))  # a second person further away
        d2 = body_of(target[0] - 0.8, target[1] + 1.0, x, y, yaw)
        objs.append((d2[0], d2[1], 0.9, 0.6, "chair"))
        if 15 <= k < 24:
            objs = objs[2:]  # both people leave the view (one of them alone would be taken as the target)
        return render(objs, rng)

    img, boxes = scene(0)
    state = (x, y, yaw) if not cfg.use_local_coordinates else None
    if state is not None:
        f.set_current_state(x, y, yaw, 0.0)
    assert f.set_initial_tracking(img, to_2d(boxes)[0])
    first = ref_boxes(det, img, boxes[:1], "person", state=state)
    r.set_initial(first[0])
    kinds = []
    for k in range(1, 45):
        target[0] += 0.02
        target[1] += 0.01 * math.sin(0.2 * k)
        img, boxes = scene(k)
        st = (x, y, yaw) if not cfg.use_local_coordinates else None
        if st is not None:
            f.set_current_state(x, y, yaw, 0.0)
            r.state = st
        calls = f.depth_calls()
        res = f.get_tracking_ctrl(img, to_2d(boxes), T.Velocity2D())
        assert f.depth_calls() == calls + (1 if boxes else 0)
        kind, vx, om = r.step(ref_boxes(det, img, boxes, "person", state=st))
        kinds.append(kind)
        if kind == "give_up":
            assert not res.is_found
            continue
        v = res.trajectory.velocities
        np.testing.assert_allclose(v.vx, vx, rtol=RTOL, atol=ATOL, err_msg=f"{kind} at {k}")
        np.testing.assert_allclose(v.omega, om, rtol=RTOL, atol=ATOL, err_msg=f"{kind} at {k}")
        np.testing.assert_allclose(f.get_tracked_state(), r.tracker.kf.x, rtol=RTOL, atol=ATOL)
        assert len(f.pending_search_commands()) == len(r.queue)
        if len(v.vx):  # the robot drives the first command
            x += float(v.vx[0]) * math.cos(yaw) * cfg.control_time_step
            y += float(v.vx[0]) * math.sin(yaw) * cfg.control_time_step
            yaw += float(v.omega[0]) * cfg.control_time_step
    assert "found" in kinds and "hold" in kinds


def test_initial_tracking_by_a_click_on_the_reference_frame():
    img = np.load(FIXTURE)["depth"]
    focal, principal = (911.0, 910.5), (640.5, 360.25)
    cfg = ref.Config()
    f = C.RGBDFollower(C.ControlType.DIFFERENTIAL_DRIVE, limits(), T.RobotGeometry.CYLINDER, [0.3, 0.6], *MOUNT,
                       params(cfg))
    f.set_camera_intrinsics(focal[0], focal[1], principal[0], principal[1])
    det = Detector(np.array(DEPTH_RANGE, np.float32), *MOUNT, focal, principal, 1e-3)
    boxes = [(100, 50, 200, 150, "chair"), (600, 300, 120, 250, "person"), (650, 350, 60, 60, "person")]
    for px, py, want in [(660, 400, 1), (700, 360, 1), (150, 100, 0), (1000, 100, None), (720, 550, 1)]:
        ok = f.set_initial_tracking(px, py, img, to_2d(boxes))
        assert ok == (want is not None)
        if ok:
            c, s, _ = det.boxes(img, [boxes[want][:4]])
            raw = f.get_raw_tracking()
            np.testing.assert_array_equal(np.asarray(raw.center, np.float32).view(np.uint32), c[0].view(np.uint32))
            assert raw.label == boxes[want][4]
            assert f.target_radius() == np.float32(0.5) * max(np.float32(s[0][0]), np.float32(s[0][1]))


def _torch_worker(check):
    """A torch frame needs torch's HIP runtime to be the process's only one (torch imported before kompass_cpp,
    DESIGN.md 4.8): the torch checks run in a fresh process, _torch_frame_worker.py."""
    pytest.importorskip("torch")
    import subprocess
    import sys

    worker = Path(__file__).resolve().parent / "_torch_frame_worker.py"
    p = subprocess.run([sys.executable, str(worker), check], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout[-3000:] + p.stderr[-3000:]


def test_torch_device_frame_gives_the_host_bits():
    _torch_worker("device_frame")


def test_front_end_orders_after_the_producer_stream():
    _torch_worker("producer_stream")


def test_other_labels_add_no_upload_and_empty_steps_no_call():
    cfg = ref.Config(prediction_horizon=4)
    f, _, _ = make(cfg)
    img, boxes = render([(3.0, 0.0, 0.5, 1.2, "person"), (1.5, 1.0, 1.0, 0.8, "car"), (1.2, -0.8, 0.6, 0.4, "car")])
    assert f.set_initial_tracking(img, to_2d(boxes)[0])
    person = [b for b in boxes if b[4] == "person"]
    f.get_tracking_ctrl(img, to_2d(person), T.Velocity2D())
    only = f.depth_last_upload()
    assert only == 2 * (person[0][2] + 1) * (person[0][3] + 1)
    calls = f.depth_calls()
    f.get_tracking_ctrl(img, to_2d(boxes), T.Velocity2D())
    assert f.depth_last_upload() == only and f.depth_calls() == calls + 1
    f.get_tracking_ctrl(img, [], T.Velocity2D())
    assert f.depth_calls() == calls + 1
    cars = [b for b in boxes if b[4] == "car"]
    res = f.get_tracking_ctrl(img, to_2d(cars), T.Velocity2D())  # detections, none of the label: no upload
    assert f.depth_calls() == calls + 2 and f.depth_last_upload() == 0 and res.is_found


class ArrayInterfaceFrame:
    """A host frame that is not an ndarray: its __array_interface__ hands out a fresh bytes object each time (as a
    PIL 'I;16' image does), so only the converted array holds the pixels."""

    def __init__(self, a):
        self.a = np.ascontiguousarray(a)

    @property
    def __array_interface__(self):
        return dict(shape=self.a.shape, typestr="<u2", data=self.a.tobytes(), version=3)


def test_array_interface_frame_gives_the_ndarray_result():
    cfg = ref.Config(prediction_horizon=6)
    frames = [render([(3.0 - 0.1 * k, 0.3, 0.5, 1.2, "person"), (4.5, -1.0, 0.4, 1.0, "person")],
                     np.random.default_rng(k)) for k in range(4)]
    outs = []
    for wrap in (False, True):
        f, _, _ = make(cfg)
        img0 = ArrayInterfaceFrame(frames[0][0]) if wrap else frames[0][0]
        assert f.set_initial_tracking(img0, to_2d(frames[0][1])[0])
        run = []
        for img, boxes in frames:
            res = f.get_tracking_ctrl(ArrayInterfaceFrame(img) if wrap else img, to_2d(boxes), T.Velocity2D())
            run.append((np.array(res.trajectory.velocities.vx), np.array(res.trajectory.velocities.omega),
                        f.get_tracked_state(), f.depth_last_upload()))
        outs.append(run)
    for a, b in zip(*outs):
        for x, y in zip(a[:3], b[:3]):
            np.testing.assert_array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
        assert a[3] == b[3] > 0


class FakeDeviceFrame:
    def __init__(self, ptr, shape, strides=None):
        self.__cuda_array_interface__ = dict(shape=shape, typestr="<u2", data=(ptr, False), strides=strides,
                                             version=3, stream=None)


def test_device_frames_that_are_not_device_memory_of_the_detector_are_refused():
    """Checked before any read (kc_depth.hip check_device_frame): a host address given as a device frame."""
    import kompass_hip as kh

    cfg = ref.Config(prediction_horizon=4)
    f, _, _ = make(cfg)
    img, boxes = render([(3.0, 0.0, 0.5, 1.2, "person")])
    assert f.set_initial_tracking(img, to_2d(boxes)[0])
    host = np.ascontiguousarray(img)
    with pytest.raises(ValueError, match="device"):
        f.get_tracking_ctrl(FakeDeviceFrame(host.ctypes.data, host.shape), to_2d(boxes), T.Velocity2D())
    ctx = kh.DepthContext(np.array(DEPTH_RANGE, np.float32), *MOUNT, FOCAL, PRINCIPAL, 1e-3)
    with pytest.raises(ValueError, match="device"):
        ctx.box_stats(None, [(0, 0, 10, 10)], device_ptr=host.ctypes.data, shape=host.shape, strides=(W, 1))
    # and the follower goes on with host frames
    assert f.get_tracking_ctrl(img, to_2d(boxes), T.Velocity2D()).is_found


def test_device_frames_larger_than_their_buffer_are_refused():
    """A device buffer (a torch tensor) described with more rows, or with strides that walk past its end."""
    _torch_worker("oversized")
