"""The torch checks of test_vision_follower_gpu.py, run in a fresh process by it: torch is imported BEFORE
kompass_cpp, so that the process has one HIP runtime (torch's).  Not collected by pytest."""
import sys
from pathlib import Path

import torch  # noqa: I001  (first: see above)

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kompass-core_amd"), str(Path(__file__).resolve().parent)]

import numpy as np  # noqa: E402

import rgbd_follower_ref as ref  # noqa: E402
import pytest  # noqa: E402
from test_vision_follower_gpu import FOCAL, H, PRINCIPAL, T, W, FakeDeviceFrame, make, render, to_2d  # noqa: E402


def _run(f, frames, as_device):
    out = []
    for img, boxes in frames:
        frame = torch.from_numpy(img).cuda() if as_device else img
        if as_device:
            torch.cuda.synchronize()
        res = f.get_tracking_ctrl(frame, to_2d(boxes), T.Velocity2D())
        out.append((res.is_found, np.array(res.trajectory.velocities.vx), np.array(res.trajectory.velocities.omega),
                    f.get_tracked_state(), f.depth_last_upload()))
    return out


def device_frame():
    cfg = ref.Config(prediction_horizon=6)
    frames = []
    for k in range(8):
        frames.append(render([(3.0 - 0.1 * k, 0.3, 0.5, 1.2, "person"), (5.0, -1.0, 0.4, 1.0, "person"),
                              (2.0, 1.5, 0.8, 0.5, "cup")], np.random.default_rng(k)))
    outs = []
    for as_device in (False, True):
        f, _, _ = make(cfg)
        assert f.set_initial_tracking(frames[0][0], to_2d(frames[0][1])[0])
        outs.append(_run(f, frames, as_device))
    for h, d in zip(*outs):
        assert h[0] == d[0]
        for a, b in zip(h[1:4], d[1:4]):
            np.testing.assert_array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
        assert h[4] > 0 and d[4] == 0
    # a strided (transposed-view) device frame, and one written on a side stream through the front end
    img, boxes = frames[3]
    f1, _, _ = make(cfg)
    f2, _, _ = make(cfg)
    for f in (f1, f2):
        assert f.set_initial_tracking(frames[0][0], to_2d(frames[0][1])[0])
    host = f1.get_tracking_ctrl(img, to_2d(boxes), T.Velocity2D())
    t = torch.from_numpy(np.ascontiguousarray(img.T)).cuda().t()
    assert not t.is_contiguous()
    torch.cuda.synchronize()
    dev = f2.get_tracking_ctrl(t, to_2d(boxes), T.Velocity2D())
    np.testing.assert_array_equal(np.array(host.trajectory.velocities.vx), np.array(dev.trajectory.velocities.vx))
    assert f2.depth_last_upload() == 0


def producer_stream():
    from kompass_core.control import VisionRGBDFollower, VisionRGBDFollowerConfig
    from kompass_core.models import AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits, RobotGeometry, \
        RobotType

    robot = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER,
                  geometry_params=np.array([0.3, 0.6]))
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=3.0, max_decel=3.0),
                          omega_limits=AngularCtrlLimits(max_vel=2.0, max_acc=3.0, max_decel=3.0, max_steer=np.pi))
    img, boxes = render([(2.5, 0.2, 0.5, 1.2, "person"), (4.0, -1.0, 0.6, 0.6, "cup")])
    results = []
    for device in (False, True):
        c = VisionRGBDFollower(robot, lim, VisionRGBDFollowerConfig(target_distance=0.5),
                               camera_focal_length=list(FOCAL), camera_principal_point=list(PRINCIPAL))
        assert c.set_initial_tracking_2d_target(None, to_2d(boxes)[0], img)
        if device:
            side = torch.cuda.Stream()
            pinned = torch.from_numpy(img).pin_memory()
            with torch.cuda.stream(side):
                frame = torch.zeros((H, W), dtype=torch.int32, device="cuda")  # queued work ahead of the frame
                for _ in range(20):
                    frame = frame + 1
                dev = pinned.to("cuda", non_blocking=True)  # the frame, written on the side stream
                assert c.loop_step(detections_2d=to_2d(boxes), depth_image=dev)
                assert c.planner.depth_last_upload() == 0
        else:
            assert c.loop_step(detections_2d=to_2d(boxes), depth_image=img)
        results.append((np.array(c.linear_x_control), np.array(c.angular_control), c.dist_error))
    torch.cuda.synchronize()
    for a, b in zip(*results):
        np.testing.assert_array_equal(a, b)



def oversized():
    cfg = ref.Config(prediction_horizon=4)
    f, _, _ = make(cfg)
    img, boxes = render([(3.0, 0.0, 0.5, 1.2, "person")])
    assert f.set_initial_tracking(img, to_2d(boxes)[0])
    dev = torch.from_numpy(img[: H // 2]).cuda()
    torch.cuda.synchronize()
    p = dev.data_ptr()
    for shape, strides in [((H * 1000, W), None), ((H // 2, W), (2 * W * 4000, 2))]:
        with pytest.raises(ValueError, match="outside"):
            f.get_tracking_ctrl(FakeDeviceFrame(p, shape, strides), to_2d(boxes), T.Velocity2D())
    # the buffer itself, described as it is, is read in place
    res = f.get_tracking_ctrl(FakeDeviceFrame(p, (H // 2, W)), to_2d(boxes), T.Velocity2D())
    assert res.is_found and f.depth_last_upload() == 0
    assert f.get_tracking_ctrl(img, to_2d(boxes), T.Velocity2D()).is_found


if __name__ == "__main__":
    {"device_frame": device_frame, "producer_stream": producer_stream, "oversized": oversized}[sys.argv[1]]()
    torch.cuda.synchronize()
    print("ok")
