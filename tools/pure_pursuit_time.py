"""PurePursuit per-step cost on the GPU: kompass_cpp.control.PurePursuit.execute(dt, scan) and
execute(dt, points) (wall clock per call), the device-event time of the one pp_search_kernel launch behind it
(the same candidate list through a kc_dwa context with timing on), and the CPU restatement
(tests/pure_pursuit_ref.py: oracle CollisionChecker, one pose at a time) for the same step.

Scenes: "blocked" -- the robot inside a closed ring, every candidate collides (the whole list is searched) -- for
max_search_candidates M in {10, 1000} and prediction_horizon H in {10, 100}; "clear" -- the nominal command is clear.

  python tools/pure_pursuit_time.py [--reps 50] [--out pure_pursuit_time.json]
"""
import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "kompass-core_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import kompass_cpp  # noqa: E402
import kompass_hip as kh  # noqa: E402
import pure_pursuit_ref as ref  # noqa: E402
from oracle import ko  # noqa: E402

DT = 0.1
DIMS = [0.1, 0.4]


def scene(kind):
    """blocked: a closed ring 0.45 m around the robot; clear: a corridor 1.2 m wide along the path (+x)."""
    ang = np.linspace(-math.pi, math.pi, 720, endpoint=False)
    if kind == "blocked":
        r = np.full(720, 0.45)
    else:
        with np.errstate(divide="ignore"):
            r = np.minimum(np.abs(0.6 / np.sin(ang)), 8.0)
    pts = np.stack([r * np.cos(ang), r * np.sin(ang), np.zeros(720)], 1).astype(np.float32)
    return r.astype(np.float64), ang, pts


def controller(M, H):
    cfg = kompass_cpp.control.PurePursuitConfig()
    # omega offsets up to 2 rad/s (a robot spinning on the spot inside the ring would be clear)
    cfg.from_dict({"max_search_candidates": M, "prediction_horizon": H, "path_search_step": 2.0 / M})
    lim = kompass_cpp.control.ControlLimitsParams(
        vel_x_ctr_params=kompass_cpp.control.LinearVelocityControlParams(1.0, 2.0, 2.0),
        vel_y_ctr_params=kompass_cpp.control.LinearVelocityControlParams(1.0, 2.0, 2.0),
        omega_ctr_params=kompass_cpp.control.AngularVelocityControlParams(0.7, 1.0, 2.0, 2.0))
    pp = kompass_cpp.control.PurePursuit(
        control_type=kompass_cpp.control.ControlType.DIFFERENTIAL_DRIVE, control_limits=lim,
        robot_shape_type=kompass_cpp.types.RobotGeometry.CYLINDER, robot_dimensions=DIMS,
        sensor_position_robot=[0.0, 0.0, 0.0], sensor_rotation_robot=[0, 0, 0, 1], octree_res=0.1, config=cfg)
    path = kompass_cpp.types.Path(points=np.float32([[x, 0.0, 0.0] for x in np.arange(0.0, 10.01, 0.5)]))
    pp.set_current_path(path)
    pp.set_current_state(0.0, 0.0, 0.0, 0.0)
    pp.set_current_velocity(kompass_cpp.types.Velocity2D(vx=0.5, vy=0.0, omega=0.0))
    return pp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rows = []
    for kind, MH in (("blocked", [(10, 10), (10, 100), (1000, 10), (1000, 100)]), ("clear", [(10, 10), (1000, 100)])):
        ranges, ang, pts = scene(kind)
        for M, H in MH:
            pp = controller(M, H)
            row = dict(scene=kind, M=M, H=H)
            for sensor, arg in (("scan", kompass_cpp.types.LaserScan(ranges=ranges, angles=ang)), ("points", pts)):
                res = pp.execute(DT, arg)
                for _ in range(3):
                    pp.execute(DT, arg)
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    res = pp.execute(DT, arg)
                row[f"{sensor}_call_us"] = (time.perf_counter() - t0) / a.reps * 1e6
                row[f"{sensor}_cmd"] = [res.velocity_command.vx, res.velocity_command.vy, res.velocity_command.omega]
            # the step's candidate list, nominal first: through a context with event timing, and the restatement
            nominal = pp.execute(DT)
            cands = pp.search_candidates(nominal.velocity_command)
            vx = np.array([c.vx for c in cands])
            vy = np.array([c.vy for c in cands])
            om = np.array([c.omega for c in cands])
            row["candidates"] = len(cands)
            ctx = kh.DwaContext(kh.CYLINDER, DIMS, octree_res=0.1, max_samples=4, max_points=4)
            ctx.set_points((0.0, 0.0, 0.0, 0.0), pts)
            ctx.timing_enable(True)
            ms = []
            for _ in range(a.reps):
                first = ctx.first_clear_command((0.0, 0.0, 0.0), vx, vy, om, H, DT)
                ms += [t for n, t in ctx.timings() if n == "pp_search_kernel"]
            ctx.close()
            row["first_clear"] = first
            assert len(ms) == a.reps
            row["kernel_us_median"] = float(np.median(ms)) * 1e3
            coll = ko.Collision(kh.CYLINDER, DIMS, res=0.1)
            coll.update_state(0.0, 0.0, 0.0)
            coll.update_points(pts, True)
            reps = max(1, min(a.reps, 5 if kind == "blocked" else a.reps))
            t0 = time.perf_counter()
            for _ in range(reps):
                want = ref.first_clear(coll, (0.0, 0.0, 0.0), list(zip(vx, vy, om)), H, DT)
            row["cpu_restatement_us"] = (time.perf_counter() - t0) / reps * 1e6
            assert want == first, (want, first)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()
