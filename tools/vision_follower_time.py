"""VisionRGBDFollower.loop_step on the MI355X at 1, 8 and 32 detections per frame (640 x 480): with the frame on
the host, with the frame already on the device (a torch tensor), and the reference-shaped restatement in Python
(tests/rgbd_follower_ref.py with tests/depth_detector_ref.py for the pixels).  Half of the extra detections share
the target's label, half do not.  Prints one JSON line per size (median microseconds)."""
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "kompass-core_amd"), str(ROOT / "tests")]

import rgbd_follower_ref as ref  # noqa: E402
import torch  # noqa: E402
from depth_detector_ref import Detector  # noqa: E402
from kompass_core.control import VisionRGBDFollower, VisionRGBDFollowerConfig  # noqa: E402
from kompass_core.datatypes import Bbox2D  # noqa: E402
from kompass_core.models import (AngularCtrlLimits, LinearCtrlLimits, Robot, RobotCtrlLimits,  # noqa: E402
                                 RobotGeometry, RobotType)

W, H, FOCAL, PRINCIPAL = 640, 480, (525.0, 525.0), (319.5, 239.5)


def median_us(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)) * 1e6, 1)


def frame(n, rng):
    img = np.full((H, W), 7000, np.uint16)
    boxes = [(290, 150, 60, 180, "person")]
    for i in range(n - 1):
        sx, sy = int(rng.integers(20, 90)), int(rng.integers(20, 150))
        tx, ty = int(rng.integers(0, W - sx)), int(rng.integers(0, H - sy))
        boxes.append((tx, ty, sx, sy, "person" if i % 2 == 0 else "chair"))
    for tx, ty, sx, sy, _ in reversed(boxes):
        img[ty:ty + sy + 1, tx:tx + sx + 1] = int(rng.integers(1500, 5000))
    img[150:331, 290:351] = 2500
    return img, boxes


def main():
    robot = Robot(robot_type=RobotType.DIFFERENTIAL_DRIVE, geometry_type=RobotGeometry.Type.CYLINDER,
                  geometry_params=np.array([0.3, 0.6]))
    lim = RobotCtrlLimits(vx_limits=LinearCtrlLimits(max_vel=1.0, max_acc=3.0, max_decel=3.0),
                          omega_limits=AngularCtrlLimits(max_vel=2.0, max_acc=3.0, max_decel=3.0, max_steer=np.pi))
    for n in (1, 8, 32):
        img, boxes = frame(n, np.random.default_rng(n))
        b2d = [Bbox2D([b[0], b[1]], [b[2], b[3]], 0.0, b[4]) for b in boxes]
        c = VisionRGBDFollower(robot, lim, VisionRGBDFollowerConfig(target_distance=0.5),
                               camera_focal_length=list(FOCAL), camera_principal_point=list(PRINCIPAL))
        assert c.set_initial_tracking_2d_target(None, b2d[0], img)
        dev = torch.from_numpy(img).cuda()
        torch.cuda.synchronize()
        host_step = lambda: c.loop_step(detections_2d=b2d, depth_image=img)  # noqa: E731
        dev_step = lambda: c.loop_step(detections_2d=b2d, depth_image=dev)  # noqa: E731
        cfg = ref.Config(target_distance=0.5, distance_tolerance=0.05, rotation_gain=0.5, enable_search=True)
        r = ref.Follower(cfg, 0.3, 1.0, 2.0)
        det = Detector(np.array([0.0, 1e3], np.float32), [0, 0, 0], [0, 0, 0, 1], FOCAL, PRINCIPAL, 1e-3)
        c0, s0, _ = det.boxes(img, [boxes[0][:4]])
        r.set_initial(ref.Box(c0[0], s0[0], "person"))

        def restated():
            same = [b for b in boxes if b[4] == "person"]
            cs, ss, idx = det.boxes(img, [b[:4] for b in same])
            r.step([ref.Box(cs[j], ss[j], "person") for j in range(len(idx))])

        for fn in (host_step, dev_step, restated):
            assert fn() is not False
        print(json.dumps({"boxes": n, "loop_step_host_frame_us": median_us(host_step, 300),
                          "loop_step_device_frame_us": median_us(dev_step, 300),
                          "restatement_us": median_us(restated, 5)}), flush=True)


if __name__ == "__main__":
    main()
