"""Grid planning front end: an occupancy grid on the host or on the device -> a collision-free
`kompass_cpp.types.Path` for the followers (`kompass_cpp.planning.GridPlanner`).

Not the reference's `OMPLGeometric` (`kompass_core/third_party/ompl/planner.py`, an OMPL wrapper and out of
scope): a deterministic, exact 8-connected shortest path on the grid.  `setup_problem` is shaped like
`OMPLGeometric.setup_problem` (:168-212), with the grid as one more argument.  The robot is a disc of its
circumscribed horizontal radius (the cylinder's or sphere's radius, half the box's diagonal): yaw-free and
conservative.  A clearance cost (`clearance_reach`, `clearance_weight`) makes the path trade length for distance
from obstacles: the counterpart, on the grid, of the `max_min_clearance` objective of the reference's OMPL front end
(`third_party/ompl/config.py:120-123`) and of `PathGeometric::clearance`.  `any_angle=True` hands out the any-angle
path over the same solve (line-of-sight shortcuts between its cells): the counterpart of the `simplifySolution()` the
reference's wrapper runs on every solve (`src/planning/ompl.cpp:61`).  An 8-connected path is at most 8 % longer than
the any-angle optimum, so what the shortcut buys is few waypoints and steady headings, not length.
`footprint="oriented"` (BOX robots) replaces the disc by the box itself over four heading classes (multiples of 45
degrees, the headings an 8-connected path can have): the robot moves along its own length axis wherever the oriented
box fits and turns in place only where the whole turning disc fits, so a long box is handed a path through a corridor
it can take lengthwise.  That is the restricted, deterministic counterpart of the reference's SE(2) planning against
the real shape.  `goal_yaw` stays unused on purpose: every heading class the box fits in at the goal cell ends the
path.
`find_frontiers` / `explore` ask the map for the goal instead of the caller: the frontiers of the known map (free cells
beside unexplored ones) that the robot's disc can reach without crossing an unexplored cell, as 8-connected components,
nearest first by travel cost, each with its nearest cell, its centroid and the path to it.  The reference leaves
frontier detection to its ROS side, as it does the world map; here it runs on the map where it lies on the device.
Not combined with a clearance cost or the oriented footprint: a frontier is ranked by plain travel cost to a cell.
`motion="car"` (rules 27 to 36) plans for a car-like (Ackermann) robot: the state is (cell, one of eight directed
headings), the transitions are one straight step and 45-degree arcs whose legs follow from `min_turning_radius`, reverse
is optional and comes at a price, there is no turn in place, and `goal_yaw` is honoured.  That is the restricted,
deterministic counterpart of the reference's SE(2) planning for its Ackermann users.  The planned polyline has
n = ceil(min_turning_radius / resolution * tan(pi / 8)) cells of tangent on either side of every 45-degree corner, so a
circular fillet of at least the turning radius fits; it leaves the polyline by at most 0.199 n cells: allow for that in
`margin`.  The polyline is what is planned and checked, not the fillet."""
import math
from typing import Dict, List, NamedTuple, Optional, Tuple

import kompass_cpp

from .mapping.world_map import WorldMap
from .models import Robot, RobotGeometry


class Frontier(NamedTuple):
    """One reachable frontier of `GridPlanner.find_frontiers`."""
    entry: Tuple[float, float]        # its nearest cell by travel cost, (x, y) in the map's frame
    entry_cell: Tuple[int, int]       # that cell's (i, j)
    centroid: Tuple[float, float]     # the mean of its cells, (x, y)
    cost: float                       # metres of path from the robot to the entry cell
    size: int                         # cells
    root: int                         # its label: the smallest flat index i + j * width among its cells


class GridPlanner:
    def __init__(self, robot: Robot, allow_unknown: bool = True, margin: float = 0.0, simplify: bool = False,
                 clearance_reach: float = 0.0, clearance_weight: float = 0.0, any_angle: bool = False,
                 max_span: int = 128, footprint: str = "disc", turn_cost: float = 1.0, motion: str = "grid",
                 min_turning_radius: float = 0.0, allow_reverse: bool = False, reverse_weight: int = 2,
                 goal_heading: str = "yaw"):
        """allow_unknown: UNEXPLORED cells can be crossed (default) or block like OCCUPIED ones.
        margin: metres added to the robot's radius.  simplify: drop the interior points of straight runs.
        clearance_reach, clearance_weight: see set_clearance_cost; the defaults leave it off.
        any_angle: solve() returns the any-angle path: from each kept cell the farthest of the next `max_span` cells
        (1 .. 1024) of the 8-connected path in line of sight, and with a clearance cost no closer to a blocking cell
        than that path came.  `simplify` is then ignored: collinear runs within the span are subsumed.
        footprint: "disc" (default) or "oriented": the box's own footprint over four heading classes, BOX robots only,
        not together with a clearance cost or `any_angle`.  turn_cost: straight-cell lengths a turn of 45 degrees
        costs (0.1 .. 1000); `get_cost()` includes the turns.
        motion: "grid" (default) or "car": (cell, eight headings) states, a straight step and 45-degree arcs of
        `min_turning_radius` metres (at most 8 turn cells at the map's resolution), no turn in place; with
        `allow_reverse` also backward at `reverse_weight` (1 .. 16) times the forward cost.  goal_heading: "yaw" ends
        the path in setup_problem's goal_yaw (to the nearest 45 degrees), "any" in whatever heading is cheapest.  With
        footprint="oriented" the box is tested by heading and `turn_cost` plays no part.  Not together with a
        clearance cost, `any_angle` or find_frontiers / explore; replan() is then a full solve."""
        if motion not in ("grid", "car"):
            raise ValueError(f"motion must be 'grid' or 'car', got {motion!r}")
        if goal_heading not in ("yaw", "any"):
            raise ValueError(f"goal_heading must be 'yaw' or 'any', got {goal_heading!r}")
        self.motion = motion
        if motion == "car":
            if clearance_reach > 0.0 and clearance_weight > 0.0:
                raise ValueError("car motion cannot be combined with a clearance cost")
            if any_angle:
                raise ValueError("car motion has no any-angle path: a segment at an arbitrary angle is no primitive")
            if not (math.isfinite(min_turning_radius) and min_turning_radius > 0.0):
                raise ValueError(f"car motion needs a positive min_turning_radius, got {min_turning_radius}")
            if allow_reverse and not 1 <= int(reverse_weight) <= 16:
                raise ValueError(f"reverse_weight must be in 1 .. 16, got {reverse_weight}")
        if footprint not in ("disc", "oriented"):
            raise ValueError(f"footprint must be 'disc' or 'oriented', got {footprint!r}")
        self.footprint = footprint
        if footprint == "oriented":
            if robot.geometry_type != RobotGeometry.Type.BOX:
                raise ValueError(f"the oriented footprint needs a BOX robot, got {robot.geometry_type}")
            if clearance_reach > 0.0 and clearance_weight > 0.0:
                raise ValueError("the oriented footprint cannot be combined with a clearance cost")
            if any_angle:
                raise ValueError("the oriented footprint has no any-angle path: a segment at an arbitrary angle has "
                                 "no heading class")
            if not (math.isfinite(turn_cost) and 1 <= math.floor(float(turn_cost) * 10.0 + 0.5) <= 10000):  # lround(turn_cost * 10)
                raise ValueError(f"turn_cost must be in 0.1 .. 1000 straight-cell lengths, got {turn_cost}")
        if not RobotGeometry.is_valid_parameters(robot.geometry_type, robot.geometry_params):
            raise ValueError(f"invalid geometry parameters {robot.geometry_params} for {robot.geometry_type}")
        self._planner = kompass_cpp.planning.GridPlanner(
            robot_shape=RobotGeometry.Type.to_kompass_cpp_lib(robot.geometry_type),
            robot_dimensions=[float(v) for v in robot.geometry_params], allow_unknown=bool(allow_unknown),
            margin=float(margin))
        self.simplify = bool(simplify)
        self.any_angle = bool(any_angle)
        self.max_span = int(max_span)
        if self.any_angle and not 1 <= self.max_span <= 1024:
            raise ValueError(f"max_span must be in 1 .. 1024, got {max_span}")
        self.solution = None
        self.frontiers: List[Frontier] = []   # of the last find_frontiers()
        self._problem = None   # the last setup_problem's (start_x, start_y, start_yaw, goal_x, goal_y, goal_yaw)
        self._map_source = None   # (the kompass_cpp WorldMap the grid was last read from, its offset then), else None
        if clearance_reach > 0.0 and clearance_weight > 0.0:
            self.set_clearance_cost(clearance_reach, clearance_weight)
        if footprint == "oriented":
            self._planner.set_oriented_footprint(True, float(turn_cost))
        if motion == "car":
            self._planner.set_car_motion(True, float(min_turning_radius), bool(allow_reverse), int(reverse_weight),
                                         goal_heading == "yaw")

    def set_clearance_cost(self, reach: float, weight: float):
        """Surcharge the cells within `reach` metres beyond the footprint (radius + margin): `weight` straight-cell
        lengths at the footprint's edge, falling linearly in the squared distance to 0 at the reach.  The path
        then minimises length plus surcharge.  reach <= 0 or weight <= 0 switches it off.  Raises with the oriented
        footprint on."""
        self._planner.set_clearance_cost(float(reach), float(weight))
        self.solution = None

    def setup_problem(self, map_meta_data: Dict, start_x: float, start_y: float, start_yaw: float, goal_x: float,
                      goal_y: float, goal_yaw: float, grid=None):
        """map_meta_data: origin_x, origin_y, width, height, resolution; cell (i, j) of the (width, height) grid
        sits at (origin_x + i * resolution, origin_y + j * resolution).
        grid: an int32 / int8 numpy array grid[i, j]; a device array with `__cuda_array_interface__` in
        column-major strides (read in place); a `kompass_cpp.mapping.LocalMapper` or the front end's
        `kompass_core.mapping.LocalMapper` (its last grid on the device; map_meta_data may then be None); a
        `kompass_core.mapping.WorldMap` (its class plane on the device and its metadata; map_meta_data may be None);
        or None to keep the grid of the last call."""
        self._set_map(map_meta_data, grid)
        self._planner.setup_problem(start_x=start_x, start_y=start_y, start_yaw=start_yaw, goal_x=goal_x,
                                    goal_y=goal_y, goal_yaw=goal_yaw)
        self._problem = (start_x, start_y, start_yaw, goal_x, goal_y, goal_yaw)
        self.solution = None

    def _set_map(self, map_meta_data, grid):
        """The bounds and the grid as setup_problem takes them."""
        if grid is not None:
            self._map_source = (grid._map, tuple(grid.offset)) if isinstance(grid, WorldMap) else None
        if isinstance(grid, WorldMap):
            map_meta_data, grid = grid.map_meta_data, grid.device_grid
        mapper = grid
        if hasattr(grid, "_mapper"):  # the front end's LocalMapper holds the class once it has mapped a scan
            mapper = grid._mapper
            if mapper is None:
                raise ValueError("the LocalMapper has no grid yet: update it from a scan first")
        if isinstance(mapper, kompass_cpp.mapping.LocalMapper):
            self._planner.set_grid_from_mapper(mapper)
        else:
            if map_meta_data is None:
                raise ValueError("map_meta_data is needed unless the grid is a LocalMapper")
            missing = [k for k in ("origin_x", "origin_y", "width", "height", "resolution") if k not in map_meta_data]
            if missing:
                raise ValueError(f"map_meta_data lacks {missing}")
            self._planner.set_space_bounds_from_map(
                origin_x=map_meta_data["origin_x"], origin_y=map_meta_data["origin_y"], width=map_meta_data["width"],
                height=map_meta_data["height"], resolution=map_meta_data["resolution"])
            if grid is not None:
                self._planner.set_grid(grid)

    def solve(self) -> Optional["kompass_cpp.types.Path"]:
        """The path, or None when the start or goal is outside the grid, invalid, or the goal out of reach."""
        return self._solution(self._planner.solve())

    def replan(self, map=None, start=None) -> Optional["kompass_cpp.types.Path"]:
        """solve() for the goal of the last setup_problem from the cost field the planner kept: the same path, at the
        cost of what changed.  map: the map's next state, a grid as setup_problem takes it (same shape and
        metadata), or None for the grid as it is.  start: the robot's new (x, y) or (x, y, yaw), or None.  With only a
        new start no pass runs; with a new map the passes run over the part of the field a changed cell can reach.
        Falls back to a full solve by itself where nothing can be kept (`replanned` says which it was).  A WorldMap's
        metadata is read again: when its window has been shifted since the bounds were taken, the bounds and the
        problem's cells are set again and the solve is a full one (DESIGN.md 4.11 rule 51)."""
        if self._problem is None:
            raise RuntimeError("replan needs a setup_problem first: it keeps that goal")
        moved = False
        if isinstance(map, WorldMap):
            moved = self._planner.set_grid_from_world_map(map._map)
            self._map_source = (map._map, tuple(map.offset))
        elif map is not None:
            self._map_source = None
            mapper = map._mapper if hasattr(map, "_mapper") else map
            if mapper is None:
                raise ValueError("the LocalMapper has no grid yet: update it from a scan first")
            if isinstance(mapper, kompass_cpp.mapping.LocalMapper):
                self._planner.set_grid_from_mapper(mapper)
            else:
                self._planner.set_grid(mapper)
        if start is not None:
            yaw = float(start[2]) if len(start) > 2 else self._problem[2]
            p = self._problem = (float(start[0]), float(start[1]), yaw) + self._problem[3:]
            self._planner.setup_problem(start_x=p[0], start_y=p[1], start_yaw=p[2], goal_x=p[3], goal_y=p[4], goal_yaw=p[5])
        return self._solution(self._planner.solve() if moved else self._planner.replan())

    def find_frontiers(self, robot_x: float, robot_y: float, map=None, map_meta_data: Optional[Dict] = None,
                       min_size: int = 8, min_distance: float = 0.0) -> List[Frontier]:
        """The frontiers of the known map the robot can reach from (robot_x, robot_y), nearest first.  A frontier
        cell is a cell the robot's disc fits on (only occupied cells inflate; unexplored cells are never crossed,
        whatever `allow_unknown` says), at `min_distance` metres of path or more, beside an unexplored cell; a
        frontier is an 8-connected group of at least `min_size` of them.  map: anything setup_problem(grid=...) takes,
        a WorldMap or a LocalMapper read in place, or None for the grid and bounds as they are.  An empty list when
        there is none, or the robot's cell is outside the map or not free for the disc (`status` says which).
        A solve-type call: `solution`, get_cost and path_cells describe nothing until the next solve().  The problem
        of the last setup_problem stays: the next solve() or replan() plans from its start to its goal, not from
        (robot_x, robot_y).  A map or metadata given here replaces the grid and the bounds as setup_problem's would, and
        that problem's start and goal are then taken into the new bounds' cells again."""
        if self.motion == "car":
            raise ValueError("exploration is not combined with car motion: a frontier is ranked by the disc's travel "
                             "cost to a cell, and the car's field is one of (cell, heading) states")
        if self.footprint == "oriented":
            raise ValueError("exploration is not combined with the oriented footprint: a frontier is ranked by the "
                             "disc's travel cost to a cell, and the oriented field is one of (cell, heading) states")
        if self._planner.get_clearance_weight10() > 0:
            raise ValueError("exploration is not combined with a clearance cost: a frontier is ranked by plain travel "
                             "cost, and min_distance is a length")
        if int(min_size) < 1:
            raise ValueError(f"min_size must be at least 1, got {min_size}")
        if not (math.isfinite(min_distance) and min_distance >= 0.0):
            raise ValueError(f"min_distance must be finite and >= 0, got {min_distance}")
        if map is not None or map_meta_data is not None:
            self._set_map(map_meta_data, map)
            if self._problem is not None:   # its cells were those of the bounds before
                p = self._problem
                self._planner.setup_problem(start_x=p[0], start_y=p[1], start_yaw=p[2], goal_x=p[3], goal_y=p[4], goal_yaw=p[5])
        self.solution = None
        self._planner.explore(robot_x=float(robot_x), robot_y=float(robot_y), min_distance=float(min_distance),
                              min_size=int(min_size))
        self.frontiers = [Frontier(**f) for f in self._planner.get_frontiers()]
        return self.frontiers

    def explore(self, robot_x: float, robot_y: float, map=None, map_meta_data: Optional[Dict] = None, min_size: int = 8,
                min_distance: float = 0.0) -> Optional["kompass_cpp.types.Path"]:
        """find_frontiers, then the path to the nearest one (robot first, its entry cell last), or None without one."""
        found = self.find_frontiers(robot_x, robot_y, map=map, map_meta_data=map_meta_data, min_size=min_size,
                                    min_distance=min_distance)
        return self.frontier_path(0) if found else None

    def frontier_path(self, k: int) -> "kompass_cpp.types.Path":
        """The path to frontier k of the last find_frontiers() list; IndexError outside it."""
        if not 0 <= int(k) < len(self.frontiers):
            raise IndexError(f"frontier {k} of {len(self.frontiers)}")
        return self._planner.get_frontier_solution(int(k))

    def frontier_path_cells(self, k: int):
        if not 0 <= int(k) < len(self.frontiers):
            raise IndexError(f"frontier {k} of {len(self.frontiers)}")
        return self._planner.get_frontier_path_cells(int(k))

    @property
    def components(self) -> int:
        """The frontiers of the last find_frontiers(), kept or not."""
        return self._planner.get_components()

    def frontier_labels(self):
        """uint32 [width, height]: the label of every frontier cell of the last find_frontiers(), 0xFFFFFFFF elsewhere."""
        return self._planner.get_frontier_labels()

    def reads(self, world_map) -> bool:
        """The grid was last read from this WorldMap (the front end's or the kompass_cpp class), at the window offset the
        map has now: what a reader of the kept cost field in the map's cell frame has to know (DESIGN.md 4.12 rule 24)."""
        inner = getattr(world_map, "_map", world_map)
        return (self._map_source is not None and self._map_source[0] is inner
                and tuple(self._map_source[1]) == tuple(inner.offset()))

    @property
    def footprint_r2(self) -> int:
        """The disc's squared radius in cells: a cell is valid when no blocking cell lies within it."""
        return int(self._planner.get_footprint_r2())

    @property
    def replanned(self) -> bool:
        """The last replan() kept a field; False after a solve() and after a replan() that had to solve in full."""
        return self._planner.replanned()

    def _solution(self, found):
        if not found:
            self.solution = None
        elif self.any_angle:
            self.solution = self._planner.get_any_angle_solution(self.max_span)
        else:
            self.solution = self._planner.get_solution(self.simplify)
        return self.solution

    def get_cost(self) -> float:
        """Metres of path, plus the surcharges of the cells it leaves while a clearance cost is set."""
        return self._planner.get_cost()

    @property
    def path_length(self) -> float:
        """Metres along the path's steps alone."""
        return self._planner.get_path_length()

    @property
    def min_clearance(self) -> float:
        """Metres from the path's cells to the nearest blocking cell, inf when none is within the clearance reach
        (needs a clearance cost)."""
        return self._planner.get_path_min_clearance()

    def clearance_field(self):
        """(clear2 uint16, penalty uint32) [width, height] of the last solve: squared cells to the nearest blocking
        cell (0xFFFF beyond the reach) and the surcharge per cell (needs a clearance cost)."""
        return self._planner.get_clearance()

    @property
    def status(self) -> int:
        return self._planner.get_status()

    @property
    def passes(self) -> int:
        return self._planner.get_passes()

    @property
    def path_cells(self):
        if self.any_angle:
            return self._planner.get_any_angle_cells(self.max_span)
        return self._planner.get_path_cells(self.simplify)

    def get_path_states(self):
        """(n, 3) int32 states (i, j, k) of the oriented path: cell and heading class, k = 0 .. 3 for the box's length
        axis along (1, 0), (1, 1), (0, 1), (-1, 1); a turn repeats its cell.  With motion="car": (i, j, h), h = 0 .. 7
        the heading E, NE, N, NW, W, SW, S, SE, one row per primitive boundary.  Empty without a path or with
        footprint="disc" and motion="grid"."""
        return self._planner.get_path_states()

    def get_path_moves(self):
        """(n - 1,) int32 primitive ids between the rows of get_path_states() with motion="car": 0 S (a step ahead),
        1 L / 2 R (a 45-degree arc ahead), 3 B, 4 BL, 5 BR (the same backward).  Empty otherwise."""
        return self._planner.get_path_moves()

    @property
    def turn_cells(self) -> int:
        """The legs of a 45-degree arc in cells at the map's resolution; 0 with motion="grid"."""
        return self._planner.get_car_turn_cells()

    @property
    def any_angle_length(self) -> float:
        """Metres along the any-angle path of `max_span` (path_length and get_cost keep describing the 8-connected
        path under it)."""
        return self._planner.get_any_angle_length(self.max_span)

    @property
    def any_angle_min_clearance(self) -> float:
        """Metres from the cells the any-angle path touches to the nearest blocking cell: never below min_clearance;
        inf without a clearance cost."""
        return self._planner.get_any_angle_min_clearance(self.max_span)
