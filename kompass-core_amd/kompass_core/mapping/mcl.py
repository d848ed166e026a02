"""Monte-Carlo localisation front end: a particle filter over a `WorldMap`, the particles on the device
(`kompass_cpp.mapping.MCL`, DESIGN.md 4.11 rules 28 to 41).

Not in the reference, which leaves localisation, like the world-frame map, to its ROS side.  `WorldMap.match` corrects
a pose that is already within a few cells, from a whole local grid, and returns one winner.  This takes a raw laser
scan, keeps N hypotheses and reports their spread; seeded over the free cells (`init_global`) it needs no guess.  Every
step ray-casts the map in place for every particle and beam, so the map may change between steps."""
from __future__ import annotations

from typing import Tuple

import numpy as np

import kompass_cpp

from .world_map import cpp_world_map


class MCLEstimate:
    """What `MCL.step` returns: the pose `x, y, yaw` (metres, radians; the weighted mean about the best particle),
    `n_eff` (the effective particle count W1^2 / W2), `resampled` (whether the step ended with a resample),
    `best_cost` (the smallest accumulated penalty), `spread` (the weighted standard deviation of position in metres,
    formed in doubles from a read-back of the particles, not from the device's exact sums) and `record`, those sums.
    It has `x`, `y` and `yaw`, so `WorldMap.update`, `match`, `scan` and `points` take it as a robot state.

    `fit` says how well the particles fit the scan in absolute terms (DESIGN.md 4.11 rules 59 and 60): the step's mean
    penalty a contributing beam over ALL particles, in 1 / 256 of a penalty unit, or -1 when no beam contributed.
    `n_eff`, `spread` and `best_cost` are relative to the particle set, so a filter that is confidently wrong looks the
    same in them as one that is right; in `fit` it does not.  Use it to gate `WorldMap.integrate_scan` / `update`:
    writing the map from a wrong pose damages it.  No threshold is shipped: a good value depends on the tables and
    the map, and none has been measured; `fit_slow` and `fit_fast`, its two running averages (rule 61), show what is
    usual for the run so far.  `injected` is the number of slots the step's resample drew anew over the map's free
    cells (0 with recovery off); `cost_min` and `cost_best` are the smallest step cost and the best particle's,
    `beams_used` the beams that contributed."""

    def __init__(self, inner):
        self._e = inner

    def __getattr__(self, name):
        if name in ("x", "y", "yaw", "n_eff", "resampled", "best_cost", "spread", "record", "txe", "tye", "fit", "fit_slow",
                    "fit_fast", "injected", "cost_min", "cost_best", "beams_used"):
            return getattr(self._e, name)
        raise AttributeError(name)

    def __iter__(self):
        return iter((self.x, self.y, self.yaw))

    def __repr__(self):
        return (f"MCLEstimate(x={self.x:.3f}, y={self.y:.3f}, yaw={self.yaw:.4f}, n_eff={self.n_eff:.1f}, "
                f"spread={self.spread:.3f}, resampled={self.resampled}, best_cost={self.best_cost}, fit={self.fit}, "
                f"injected={self.injected})")


def _pose(robot_state) -> Tuple[float, float, float]:
    if hasattr(robot_state, "yaw"):
        return float(robot_state.x), float(robot_state.y), float(robot_state.yaw)
    x, y, yaw = robot_state
    return float(x), float(y), float(yaw)


class MCL:
    def __init__(self, world_map, n_particles: int, angles, range_max: float, sigma_hit: float = 0.1, seed: int = 0,
                 motion_noise: Tuple[float, float, float] = (0.02, 0.01, 0.01), resample_ratio: Tuple[int, int] = (1, 2),
                 unknown_blocks: bool = False, skip_no_return: bool = False, spread: bool = True, model: str = "beam",
                 recovery=None, **model_args):
        """world_map: a `WorldMap` (kept alive).  angles: the beams in the scan frame, radians; a sensor's yaw offset is
        folded in here, a translated mount is out of scope.  range_max: metres; a measured range that is not finite or
        not below it is a beam without a return: it counts as range_max, or not at all with skip_no_return.
        sigma_hit and **model (err_shift, n_pen, floor, pen_scale, w_shift, n_w, wtab0, temperature): the sensor model
        the integer penalty and weight tables are built from; its defaults are judgement, not measurement.
        motion_noise: sigmas a step adds, (forward m, lateral m, yaw rad).  resample_ratio (num, den): resample when
        n_eff < N num / den.  spread=False saves the read-back of the particles a step.
        model: "beam" (every step ray-casts the map for every particle and beam) or "field", the likelihood-field model
        (DESIGN.md 4.11 rules 44 and 45): a beam costs one lookup of the map's distance field at its endpoint, beams
        without a return say nothing; **model_args are then reach (cells, default ceil(3 sigma_hit / resolution) within
        1 .. 63), floor, pen_scale, w_shift, n_w, wtab0, temperature.  It enables the map's distance field itself when
        that is off or shorter (unknown_blocks decides what blocks there).
        recovery: None (off), True (the defaults) or (a_slow, a_fast, (num, den)): see `set_recovery`."""
        if model not in ("beam", "field"):
            raise ValueError('model must be "beam" or "field"')
        inner = cpp_world_map(world_map)
        if inner is None:
            raise TypeError("expected a WorldMap")
        self._map = world_map
        a = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
        self._mcl = kompass_cpp.mapping.MCL(inner, int(n_particles), a, float(range_max), int(seed))
        self._mcl.set_flags(bool(unknown_blocks), bool(skip_no_return))
        if model == "field":
            self._mcl.set_field_model(sigma_hit=float(sigma_hit), **model_args)
        else:
            self._mcl.set_model(sigma_hit=float(sigma_hit), **model_args)
        self.model = model
        self._mcl.set_motion_noise(*(float(v) for v in motion_noise))
        self._mcl.set_resample_ratio(int(resample_ratio[0]), int(resample_ratio[1]))
        self._mcl.set_spread(bool(spread))
        self.set_recovery(recovery)

    def set_recovery(self, recovery=True) -> None:
        """Recovery from a lost filter by injected particles (DESIGN.md 4.11 rules 61 to 63).  The fit of every step feeds
        a slow and a fast average, slow += (m - slow) >> a_slow and fast alike; while fast lies above slow, the scans fit
        worse than they used to, and the step ends with a resample in which min(N num / den, N (fast - slow) / fast)
        slots, spread evenly, are drawn anew over the map's free cells as `init_global` draws them.  None: off (the
        averages still run and `MCLEstimate.fit` is still reported); True: a_slow 4, a_fast 1, at most 1 / 4 of the
        particles, which are judgement, not measurement; or (a_slow, a_fast, (num, den)).  The injecting resample reads the
        map on the device, and `step` waits for it: the map may be written (`integrate_scan`, `update`, `shift`) as soon
        as `step` has returned."""
        if recovery is None or recovery is False:
            self._mcl.clear_recovery()
        elif recovery is True:
            self._mcl.set_recovery()
        else:
            a_slow, a_fast, (num, den) = recovery
            self._mcl.set_recovery(int(a_slow), int(a_fast), int(num), int(den))

    def init(self, robot_state, sigma_xy: float, sigma_yaw: float) -> None:
        """Gaussian around robot_state (x, y, yaw), sigmas in metres and radians."""
        self._mcl.init(*_pose(robot_state), float(sigma_xy), float(sigma_yaw))

    def init_global(self) -> int:
        """Uniform over the map's empty cells, any heading -> the number of those cells."""
        return self._mcl.init_global()

    def step(self, odom_from, odom_to, ranges) -> MCLEstimate:
        """odom_from, odom_to: the odometry's pose before and after (robot states or (x, y, yaw), in any common frame:
        only their difference counts).  ranges: float [B] in metres, or a `LaserScanData` of the same beams."""
        r = getattr(ranges, "ranges", ranges)
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(-1)
        return MCLEstimate(self._mcl.step(_pose(odom_from), _pose(odom_to), r))

    def resample(self) -> None:
        self._mcl.resample()

    def particles(self):
        """(x float64 [N], y, yaw, acc uint32 [N]) in metres and radians, copied from the device."""
        tx, ty, h, acc = self._mcl.particles()
        meta = self._map.map_meta_data
        res = float(np.float32(meta["resolution"]))
        return (meta["origin_x"] + tx / 65536.0 * res, meta["origin_y"] + ty / 65536.0 * res, h * (2.0 * np.pi / 65536.0), acc)

    @property
    def n_particles(self) -> int:
        return self._mcl.size
