"""World map front end: a world-frame occupancy map that stays on the device, fused from the `LocalMapper`'s
egocentric grids (`kompass_cpp.mapping.WorldMap`).

Not in the reference, which leaves the world-frame map to its ROS side.  The `LocalMapper`'s grid turns with the
robot and forgets what leaves its window; `GridPlanner.replan` wants a world-frame map that changes.  This is the
map between the two: seeded from a prior (the PCD grid), updated from each local grid where that grid lies, and
handed to the planner in place (`setup_problem(None, ..., grid=world_map)`, `replan(map=world_map)`)."""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np

import kompass_cpp

from .movers import MoverDetection


class WorldMapMatch:
    """What `WorldMap.match` found (DESIGN.md 4.11 rules 9 to 15): the winner (k, u, v) of the window in yaw steps and
    cells, its `score`, the guess's `score_guess`, the `points` (occupied local cells) that were matched, the
    corrected pose `x, y, yaw`, and `ratio = score / (3 * points)`: 1.0 when every point sits on an occupied cell
    of the map, 0.0 without points.  `scores()` is the whole table, uint32 [2 n_yaw + 1, 2 reach + 1, 2 reach + 1]
    indexed [k + n_yaw, v + reach, u + reach], for whoever wants a covariance; it is the map's last table, so it
    raises once the map has made another match.  `applied`: set by `update(match=True)`, whether the update fused
    at the corrected pose."""

    def __init__(self, record):
        self._record = record
        self.applied: Optional[bool] = None

    def __getattr__(self, name):
        if name in ("k", "u", "v", "score", "score_guess", "points", "x", "y", "yaw", "pose"):
            return getattr(self._record, name)
        raise AttributeError(name)

    @property
    def ratio(self) -> float:
        return self.score / (3.0 * self.points) if self.points else 0.0

    def scores(self) -> np.ndarray:
        return self._record.scores()

    def __repr__(self):
        return (f"WorldMapMatch(k={self.k}, u={self.u}, v={self.v}, score={self.score}, score_guess={self.score_guess}, "
                f"points={self.points}, ratio={self.ratio:.3f}, applied={self.applied})")


def cpp_world_map(obj):
    """The `kompass_cpp.mapping.WorldMap` behind `obj` (this module's `WorldMap`, or the class itself), else None: what
    the controllers' `loop_step(local_map=...)` looks for."""
    inner = getattr(obj, "_map", obj)
    return inner if isinstance(inner, kompass_cpp.mapping.WorldMap) else None


class WorldMap:
    def __init__(self, width: int, height: int, resolution: float, origin: Tuple[float, float] = (0.0, 0.0), hit: int = 3,
                 miss: int = 1, e_min: int = -8, e_max: int = 14, occ_thr: int = 1):
        """width x height cells of `resolution` metres, `origin` the world position of cell (0, 0)'s centre.
        hit / miss: the evidence an occupied / empty observation adds / takes away, kept within e_min .. e_max; a
        cell is occupied from occ_thr up.  hit = miss = 127, e_min = -126, e_max = 127: every observation decides the
        class (with e_min = -127 a hit on a cell at -127 lands on 0, below occ_thr = 1: DESIGN.md 4.11)."""
        self._map = kompass_cpp.mapping.WorldMap(width=int(width), height=int(height), resolution=float(resolution),
                                                 origin_x=float(origin[0]), origin_y=float(origin[1]))
        if (hit, miss, e_min, e_max, occ_thr) != (3, 1, -8, 14, 1):
            self._map.set_model(hit=int(hit), miss=int(miss), e_min=int(e_min), e_max=int(e_max), occ_thr=int(occ_thr))
        self.last_match: Optional[WorldMapMatch] = None  # of the last update(match=True)

    def set_model(self, hit: int = 3, miss: int = 1, e_min: int = -8, e_max: int = 14, occ_thr: int = 1) -> None:
        """Another update model; clears the map (evidence counted by one model means nothing under another)."""
        self._map.set_model(hit=int(hit), miss=int(miss), e_min=int(e_min), e_max=int(e_max), occ_thr=int(occ_thr))

    def set_prior(self, grid) -> None:
        """grid[I, J]: an int8 / int32 (width, height) array (`points_to_occupancy_grid` gives one), or a device array
        with `__cuda_array_interface__` in column-major strides.  100 -> occupied at e_max, 0 -> empty at e_min,
        anything else never observed.  Replaces the whole state."""
        self._map.set_prior(grid)

    @staticmethod
    def _local(local_map):
        mapper = local_map
        if hasattr(local_map, "_mapper"):  # the front end's LocalMapper holds the class once it has mapped a scan
            mapper = local_map._mapper
            if mapper is None:
                raise ValueError("the LocalMapper has no grid yet: update it from a scan first")
        if not isinstance(mapper, kompass_cpp.mapping.LocalMapper):
            mapper = np.asarray(mapper)
        return mapper

    def match(self, robot_state, local_map, n_yaw: int = 10, yaw_step: float = math.radians(0.5), reach: int = 10) -> WorldMapMatch:
        """Check a pose against the map: of the poses within `n_yaw` steps of `yaw_step` radians each side of
        robot_state's yaw and `reach` cells each side of its position, the one that puts the occupied cells of
        local_map (anything `update` accepts) onto the occupied cells of the map best.  Whole cells and whole yaw
        steps only; n_yaw and reach are at most 31.  The map is not modified.  -> WorldMapMatch."""
        return WorldMapMatch(self._map.match(self._local(local_map), float(robot_state.x), float(robot_state.y),
                                             float(robot_state.yaw), int(n_yaw), float(yaw_step), int(reach)))

    def shift(self, di: int, dj: int) -> None:
        """Move the window by whole cells on the device (DESIGN.md 4.11 rules 46 to 48), a positive di towards +x: what
        leaves the window is forgotten, what enters it is never observed, evidence and class move together.  The origin
        (`map_meta_data`) follows; `changed` is 0 afterwards; the distance field, when enabled, is recomputed by its next
        reader; `device_grid` keeps its address.  An `MCL` over this map moves its particles by itself (rule 50); a
        `GridPlanner` solves in full on its next `replan(map=world_map)` (rule 51)."""
        self._map.shift(int(di), int(dj))

    def recentre(self, robot_state, margin: int, stride: int) -> Tuple[int, int]:
        """Rule 49: no shift while the robot's cell is `margin` cells or more from every border; otherwise the whole
        multiple of `stride` cells, per axis, that brings it nearest the window's centre.  -> (di, dj), the shift made."""
        x, y, _ = self._pose(robot_state)
        return self._map.recentre(x, y, int(margin), int(stride))

    @property
    def offset(self) -> Tuple[int, int]:
        """(OI, OJ): the cells the window has moved since the map was created."""
        return self._map.offset()

    def update(self, robot_state, local_map, match: bool = False, min_ratio: float = 0.6, min_points: int = 30,
               follow: Optional[Tuple[int, int]] = None, **window) -> int:
        """Fuse one local grid; robot_state (x, y, yaw): the robot's pose in the world.  local_map: the front end's
        `LocalMapper` or a `kompass_cpp.mapping.LocalMapper` (its last grid where it lies on the device, no host
        round trip), or an int32 (grid_height, grid_width) array as `LocalMapper.occupancy`.  -> cells whose class
        changed.

        match=True: `match(robot_state, local_map, **window)` first, and fuse at the corrected pose when the match
        is trusted: ratio >= min_ratio, points >= min_points and score > score_guess; at the given pose otherwise.
        `last_match` holds the WorldMapMatch, its `applied` the decision.  The defaults of min_ratio and min_points
        are judgement, not measurement: nobody has tuned them on a robot.

        follow=(margin, stride): `recentre(robot_state, margin, stride)` before anything else, so the window rolls with the
        robot and the grid is fused into the shifted map."""
        mapper = self._local(local_map)
        if follow is not None:
            self.recentre(robot_state, int(follow[0]), int(follow[1]))
        if not match:
            if window:
                raise TypeError(f"unexpected arguments without match=True: {sorted(window)}")
            return self._map.update(mapper, float(robot_state.x), float(robot_state.y), float(robot_state.yaw))
        m = self.match(robot_state, mapper, **window)
        m.applied = bool(m.ratio >= min_ratio and m.points >= min_points and m.score > m.score_guess)
        self.last_match = m
        if m.applied:
            return self._map.update_at(mapper, m.pose)
        return self._map.update(mapper, float(robot_state.x), float(robot_state.y), float(robot_state.yaw))

    @staticmethod
    def _scan_args(scan, angles, range_max, range_min):
        """A `LaserScanData` or ranges plus angles -> (angles float64 [B], ranges float64 [B], range_max, range_min)"""
        ranges = getattr(scan, "ranges", scan)
        if hasattr(scan, "ranges"):
            angles = scan.angles if angles is None else angles
            range_max = scan.range_max if range_max is None else range_max
            range_min = scan.range_min if not range_min else range_min
        if angles is None or range_max is None:
            raise TypeError("an array of ranges needs angles and range_max")
        a = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
        r = np.ascontiguousarray(ranges, dtype=np.float64).reshape(-1)
        return a, r, float(range_max), float(range_min)

    def detect_movers(self, robot_state, scan, angles=None, range_max: Optional[float] = None, range_min: float = 0.0,
                      **config) -> "MoverDetection":
        """Moving obstacles in one raw laser scan (DESIGN.md 4.11 rules 64 to 69): the returns that end in cells the map has
        seen empty, more than sqrt(m2) cells from anything occupied, grouped into runs of neighbouring beams.  Arguments as
        `integrate_scan`'s; config: m2, gap, join_q (2^-16 cells^2), min_beams, whose defaults (4, 2, 9 << 16, 3) are
        judgement, not measurement.  The map is not modified; its distance field must be enabled.  Two launches on the
        device.  -> MoverDetection: `clusters` (x, y, radius in world metres), `labels` (int32 a beam) and `record`.
        Hand it to a `MoverTracker`, and `MoverTracker.skip_mask(detection)` to `integrate_scan(skip=...)` so that a
        mover's returns never reach the map."""
        a, r, range_max, range_min = self._scan_args(scan, angles, range_max, range_min)
        cfg = kompass_cpp.mapping.MoverDetectConfig(**{k: int(v) for k, v in config.items()})
        return MoverDetection(self._map.detect_movers(*self._pose(robot_state), a, r, range_max, range_min, cfg),
                              float(self._map.resolution))

    def integrate_scan(self, robot_state, scan, angles=None, range_max: Optional[float] = None, range_min: float = 0.0,
                       clear_no_return: bool = False, follow: Optional[Tuple[int, int]] = None, skip=None) -> int:
        """Fuse one raw laser scan by an inverse ray cast on the device (DESIGN.md 4.11 rules 52 to 58), no `LocalMapper`
        in between; robot_state (x, y, yaw): the scan frame's pose in the world (a robot state, an `MCL` estimate or a
        tuple).  scan: a `LaserScanData` (its angles, ranges, range_min and range_max; the arguments, where given, take
        their place), or an array of ranges in metres together with `angles`.  A beam's range ends in an occupied cell and
        crosses empty ones, a hit beating a miss where beams disagree; NaN, a negative range or one below range_min says
        nothing; inf or a range >= range_max is a beam without a return, which clears what it crosses up to range_max
        with clear_no_return and says nothing without.  A sensor's yaw offset is folded into `angles`; a translated mount
        is out of scope.  follow=(margin, stride): `recentre` first, as in `update`.  skip: a mask a beam, true where the
        beam is to say nothing whatever its range (`MoverTracker.skip_mask`); the free space along a skipped beam is not
        cleared either.  -> cells whose class changed."""
        a, r, range_max, range_min = self._scan_args(scan, angles, range_max, range_min)
        if follow is not None:
            self.recentre(robot_state, int(follow[0]), int(follow[1]))
        if skip is None:
            return self._map.integrate_scan(*self._pose(robot_state), a, r, range_max, range_min, bool(clear_no_return))
        mask = np.ascontiguousarray(np.asarray(skip).astype(bool), dtype=np.uint8).reshape(-1)
        return self._map.integrate_scan(*self._pose(robot_state), a, r, range_max, range_min, bool(clear_no_return), mask)

    def clear(self) -> None:
        self._map.clear()

    def points(self, robot_state, max_range: float) -> np.ndarray:
        """The occupied cells within max_range metres of robot_state's position as world-frame points, float32 [n, 3]
        with z = 0, in no particular order (DESIGN.md 4.11 rules 16 to 19): a cloud to show or to hand to a consumer of
        point clouds.  `DWA.loop_step(local_map=world_map)` and `PurePursuit.loop_step(local_map=world_map)` take the
        map itself and extract the same list on the device."""
        return self._map.points(float(robot_state.x), float(robot_state.y), float(max_range))

    @staticmethod
    def _pose(robot_state) -> Tuple[float, float, float]:
        if hasattr(robot_state, "yaw"):
            return float(robot_state.x), float(robot_state.y), float(robot_state.yaw)
        x, y, yaw = robot_state
        return float(x), float(y), float(yaw)

    def scan(self, robot_state, angles, range_max: float, unknown_blocks: bool = False, return_cells: bool = False):
        """The map's virtual laser scan (DESIGN.md 4.11 rules 20 to 27): what a lidar whose frame is at robot_state
        (x, y, yaw) would range along the beam `angles` (radians, in that frame), by the map's memory -> float64 [B]: the
        distance to the first occupied cell within range_max, else range_max.  unknown_blocks: a never-observed cell
        ends a beam as well.  return_cells: -> (ranges, int32 [B] of the hit cells I + J * width, -1 without a hit).
        One launch on the device."""
        a = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
        return self._map.scan(*self._pose(robot_state), a, float(range_max), bool(unknown_blocks), bool(return_cells))

    def scans(self, poses, angles, range_max: float, unknown_blocks: bool = False) -> np.ndarray:
        """The same for M poses (robot states or (x, y, yaw)) in one launch -> float64 [M, B]."""
        a = np.ascontiguousarray(angles, dtype=np.float64).reshape(-1)
        return self._map.scans([self._pose(p) for p in poses], a, float(range_max), bool(unknown_blocks))

    def laser_scan(self, robot_state, angles=None, range_max: float = 20.0, unknown_blocks: bool = False):
        """`scan` as a `LaserScanData`; angles: default 360 beams over [0, 2 pi)."""
        from ..datatypes.laserscan import LaserScanData

        a = np.arange(360) * (2 * math.pi / 360) if angles is None else np.asarray(angles, dtype=float).reshape(-1)
        inc = float(a[1] - a[0]) if a.size > 1 else 0.0
        return LaserScanData(angle_min=float(a[0]), angle_max=float(a[-1]), angle_increment=inc, range_max=float(range_max),
                             ranges=self.scan(robot_state, a, range_max, unknown_blocks), angles=a)

    @staticmethod
    def merge_scan(present, from_map) -> np.ndarray:
        """Rule 27: per beam the present range where it is finite and below the map's, else the map's."""
        q, v = np.asarray(present, dtype=np.float64), np.asarray(from_map, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            return np.where(np.isfinite(q) & (q < v), q, v)

    def enable_distance(self, reach_m: Optional[float] = None, reach_cells: Optional[int] = None, unknown_blocks: bool = False) -> int:
        """Keep a distance field over the map (DESIGN.md 4.11 rules 42 and 43): per cell the squared distance in cells to
        the nearest occupied cell (with unknown_blocks also a never-observed one) within the reach.  reach_m metres
        (rounded up to whole cells) or reach_cells, 1 .. 254; reach_cells=0 switches it off.  Kept lazily: an update
        costs nothing more, a reader refreshes the changed box first.  -> the reach in cells."""
        if (reach_m is None) == (reach_cells is None):
            raise TypeError("give reach_m or reach_cells")
        reach = int(reach_cells) if reach_m is None else int(math.ceil(float(reach_m) / float(np.float32(self._map.resolution))))
        if reach_m is not None and reach < 1:
            raise ValueError("reach_m must be positive")
        self._map.enable_distance(reach, bool(unknown_blocks))
        return reach

    def distance_field(self, metres: bool = False) -> np.ndarray:
        """A refreshed host copy of the distance plane: uint16 [width, height] squared cells, 0xFFFF beyond the reach; or
        with metres=True float32 metres, inf beyond the reach."""
        d = self._map.distance_field()
        if not metres:
            return d
        out = np.sqrt(d.astype(np.float32)) * np.float32(self._map.resolution)
        out[d == 0xFFFF] = np.inf
        return out

    def distance_at(self, x: float, y: float) -> float:
        """Metres from the cell that holds world point (x, y) to the nearest blocking cell; inf beyond the reach or
        outside the map.  Reads the whole plane back: for a look, not for a loop."""
        res = float(np.float32(self._map.resolution))
        ox, oy = self._map.origin
        i, j = int(math.floor((float(x) - ox) / res + 0.5)), int(math.floor((float(y) - oy) / res + 0.5))
        if not (0 <= i < self._map.width and 0 <= j < self._map.height):
            return math.inf
        d = int(self._map.distance_field()[i, j])
        return math.inf if d == 0xFFFF else math.sqrt(float(d)) * res

    @property
    def occupancy(self) -> np.ndarray:
        """A host copy of the class plane, int8 [width, height]: -1 unexplored, 0 empty, 100 occupied."""
        return self._map.get_cls()

    @property
    def evidence(self) -> np.ndarray:
        """A host copy of the evidence plane, int8 [width, height]: -128 never observed."""
        return self._map.get_evidence()

    @property
    def device_grid(self):
        """The class plane on the device (`__cuda_array_interface__`, int8 (width, height), column-major)."""
        return self._map.device_grid()

    @property
    def changed(self) -> int:
        return self._map.get_changed()

    @property
    def changed_box(self) -> Tuple[int, int, int, int]:
        """(i_min, j_min, i_max, j_max) of the cells the last update changed, all -1 when none."""
        return self._map.get_changed_box()

    @property
    def map_meta_data(self) -> Dict:
        """The dict `GridPlanner.setup_problem` takes."""
        ox, oy = self._map.origin
        return {"origin_x": ox, "origin_y": oy, "width": self._map.width, "height": self._map.height,
                "resolution": self._map.resolution}
