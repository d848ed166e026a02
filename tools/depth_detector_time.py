"""DepthDetector per-frame cost on the GPU, on the reference's real 1280x720 depth frame (tests/golden): the
device-event time of the one depth_boxes_kernel launch and of the frame upload (kc_depth timing), the wall clock
of kompass_cpp.vision.DepthDetector.compute_3d_detections, and the numpy restatement (tests/depth_detector_ref.py)
for the same boxes.  Workloads: 1 / 8 / 64 boxes of 64^2, 256^2 and the full frame, each with the frame on the
host and on the device (a hipMalloc copy); the RGB-D follower's range (0 .. 1000 m, factor 1e-3: all 65536 raw values kept).

  python tools/depth_detector_time.py [--reps 30] [--runs 5] [--out depth_detector_time.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "kompass-core_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import kompass_hip as kh  # noqa: E402
from depth_detector_ref import Detector  # noqa: E402
from test_depth_detector_gpu import device_frame  # noqa: E402
from kompass_core.datatypes import Bbox2D  # noqa: E402
from kompass_core.vision import DepthDetector  # noqa: E402

RANGE, FACTOR = np.array([0.0, 1e3], np.float32), 1e-3
FOCAL, PRINCIPAL = [911.0, 910.5], [640.5, 360.25]


def boxes_of(side, n, h, w, rng):
    if side is None:
        return [(0, 0, w - 1, h - 1)] * n
    return [(int(rng.integers(0, w - side)), int(rng.integers(0, h - side)), side - 1, side - 1) for _ in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--ref-reps", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    img = np.load(ROOT / "tests" / "golden" / "bag_image_depth.npz")["depth"]
    h, w = img.shape
    dev, dev_frame = device_frame(img)   # (dev keeps the device copy alive)
    args = (RANGE, [0, 0, 0], [0, 0, 0, 1], FOCAL, PRINCIPAL, FACTOR)
    ctx, ref, det = kh.DepthContext(*args), Detector(*args), DepthDetector(*args)
    ctx.timing_enable(True)
    rng = np.random.default_rng(0)
    rows = []
    for side in (64, 256, None):
        for n in (1, 8, 64):
            boxes = boxes_of(side, n, h, w, rng)
            b2 = [Bbox2D(top_left_corner=[b[0], b[1]], size=[b[2] + 1, b[3] + 1]) for b in boxes]
            for b, bb in zip(b2, boxes):
                b.size = np.array([bb[2], bb[3]], np.int32)
            for where in ("host", "device"):
                frame = dev_frame if where == "device" else {}
                src = None if where == "device" else img
                kern, up, call, e2e = [], [], [], []
                for _ in range(a.runs):
                    k_run, u_run, c_run = [], [], []
                    for _ in range(a.reps):
                        t0 = time.perf_counter()
                        ctx.boxes(src, boxes, state=(0.0, 0.0, 0.0), **frame)
                        c_run.append((time.perf_counter() - t0) * 1e6)
                        t = dict(ctx.timings())
                        k_run.append(t["depth_boxes_kernel"] * 1e3)
                        u_run.append(t.get("upload", 0.0) * 1e3)
                    kern.append(statistics.median(k_run))
                    up.append(statistics.median(u_run))
                    call.append(statistics.median(c_run))
                    if where == "host":
                        e_run = []
                        for _ in range(a.reps):
                            t0 = time.perf_counter()
                            det.compute_3d_detections(img, b2, 0.0, 0.0, 0.0, 0.0)
                            e_run.append((time.perf_counter() - t0) * 1e6)
                        e2e.append(statistics.median(e_run))
                upload_bytes = ctx.last_upload()
                t0 = time.perf_counter()
                for _ in range(a.ref_reps):
                    ref.boxes(img, boxes, state=(0.0, 0.0, 0.0))
                ref_us = (time.perf_counter() - t0) / a.ref_reps * 1e6
                med = lambda v: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]  # noqa: E731
                row = dict(box="full" if side is None else f"{side}^2", boxes=n, frame=where,
                           kernel_us=med(kern), upload_us=med(up), call_us=med(call),
                           compute_3d_detections_us=med(e2e) if e2e else None, upload_bytes=upload_bytes,
                           numpy_restatement_us=round(ref_us, 1))
                rows.append(row)
                print(json.dumps(row), flush=True)
    if a.out:
        Path(a.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
