"""MPPI front-end (not in the reference): a sampling model-predictive follower over the world map's
distance plane.  The planner is `kompass_cpp.control.MPPI`; every step is two launches on the MI355X and one read-back.
Unlike the reference's controllers it plans a whole sequence inside its horizon: slow down, turn into the door, speed
up.

It is also the one controller here whose roll-out carries a time index, so it can cost moving obstacles at each step's own
time (rules 13 to 18): `loop_step(..., moving_obstacles=[(x, y, vx, vy, radius), ...])`, discs in the world with a
constant velocity.  Where they come from, a tracker for instance, is the caller's.

`MPPIConfig(acceleration_limits=True)` rolls every sample out under the control limits' accelerations, from the velocity
the controller commanded last (rules 25 to 29): what the robot is told is then the first step of a roll-out that was
costed.  Off by default.

`MPPIConfig(footprint="box")` gives the roll-out the robot's shape (rules 30 to 36): a BOX robot's length x width is covered
by up to eight equal discs along its length, and a state is a hit when any of them is, at the state's own heading.  The
default, "disc", is the one disc of `hit_radius` at the pose."""
from __future__ import annotations

import logging
import math
from typing import List, Optional

import numpy as np

from attrs import define, field, validators

import kompass_cpp
from ..mapping.world_map import cpp_world_map
from ..models import Robot, RobotCtrlLimits, RobotGeometry, RobotState, RobotType
from ._base_ import FollowerConfig, FollowerTemplate


def _rng(lo, hi):
    return [validators.ge(lo), validators.le(hi)]


@define
class MPPIConfig(FollowerConfig):
    """The defaults are those of the closed-loop scene of DESIGN.md 4.12: judgement, not measurement; nobody has tuned
    them on a robot.  Lengths are in cells of the map, a step is the control time step."""
    samples: int = field(default=1024, validator=_rng(1, 65536))
    horizon: int = field(default=32, validator=_rng(1, 64))
    window: int = field(default=96, validator=_rng(1, 256))                 # path points the cost looks at
    control_horizon: int = field(default=2, validator=_rng(1, 64))         # controls the getters return
    sigma_forward: float = field(default=0.5, validator=_rng(0.0, 64.0))    # cells a step
    sigma_lateral: float = field(default=0.5, validator=_rng(0.0, 64.0))    # cells a step, OMNI only
    sigma_turn: float = field(default=500.0 / 65536.0 * 2.0 * math.pi, validator=_rng(0.0, math.pi))  # radians a step
    temperature: float = field(default=64.0, validator=_rng(1e-3, 1e9))     # lambda: w = exp(-(S - S_min) / lambda)
    weight_shift: int = field(default=2, validator=_rng(0, 30))
    weight_entries: int = field(default=256, validator=_rng(1, 4096))
    hit_radius: float = field(default=3.0, validator=_rng(0.0, 63.0))       # cells: closer to an obstacle is a hit
    clearance: float = field(default=7.0, validator=_rng(1.0, 63.0))        # cells: the penalty fades out here
    clearance_weight: float = field(default=60.0, validator=_rng(0.0, 65535.0))
    far_penalty: int = field(default=0, validator=_rng(0, 65535))
    hit_penalty: int = field(default=4000, validator=_rng(0, 1 << 20))
    path_weight: int = field(default=8, validator=_rng(0, 1 << 16))
    goal_weight: int = field(default=20, validator=_rng(0, 1 << 20))
    path_cap: float = field(default=20.0, validator=_rng(0.0, 1024.0))      # cells: farther from the path costs no more
    distance_reach: int = field(default=8, validator=_rng(1, 254))          # the plane's reach when it has to be enabled
    allow_reverse: bool = field(default=False)
    min_turning_radius: float = field(default=0.5, validator=_rng(1e-3, 1e3))  # metres, ACKERMANN only
    seed: int = field(default=0)
    # Moving obstacles: judgement too, tried on the crossing scene of DESIGN.md 4.12 alone.  A mover is hit inside
    # hit_radius + its radius; the ramp begins mover_margin cells farther out and is mover_weight at its top
    mover_margin: float = field(default=4.0, validator=_rng(0.0, 1024.0))    # cells
    mover_weight: float = field(default=200.0, validator=_rng(0.0, 1048576.0))
    mover_hit_penalty: int = field(default=4000, validator=_rng(0, 1 << 20))
    # The grid planner's cost field (loop_step(cost_field=...), rules 19 to 21; the field counts 10 a straight cell):
    # every state a sample reaches adds (min(field, field_cap) * field_run_weight) >> 8, the last one field_goal_weight
    # times its capped field.  Judgement, not tuning: the values the two scenes of DESIGN.md 4.12 were tried with
    field_run_weight: int = field(default=32, validator=_rng(0, 1 << 12))
    field_goal_weight: int = field(default=2, validator=_rng(0, 64))
    field_cap: int = field(default=1 << 20, validator=_rng(1, 1 << 24))
    # Rules 25 to 29: the roll-out obeys max_acc / max_decel of the control limits, from the velocity commanded last, and
    # the command is the first applied control of the new sequence.  Off: the step of rules 1 to 24, whose first control
    # is passed through the limits after the step
    acceleration_limits: bool = field(default=False)
    # Rules 30 to 36: "box" takes (length, width) from a BOX robot's geometry_params and covers it with up to eight discs
    # along its length; their r2 stands in the place of hit_radius'.  footprint_margin (cells) is rule 36's: sqrt(2)
    # rounded up to half a cell, derived in DESIGN.md 4.12, not tuned.  "disc": the step of rules 1 to 29
    footprint: str = field(default="disc", validator=validators.in_(("disc", "box")))
    footprint_margin: float = field(default=1.5, validator=_rng(0.0, 63.0))

    def to_kompass_cpp(self) -> "kompass_cpp.control.MPPIConfig":
        c = kompass_cpp.control.MPPIConfig()
        c.samples, c.horizon, c.window = int(self.samples), int(self.horizon), int(self.window)
        c.sigma_forward, c.sigma_lateral, c.sigma_turn = float(self.sigma_forward), float(self.sigma_lateral), float(self.sigma_turn)
        c.lambda_, c.w_shift, c.n_w = float(self.temperature), int(self.weight_shift), int(self.weight_entries)
        c.hit_radius, c.clearance, c.clearance_weight = float(self.hit_radius), float(self.clearance), float(self.clearance_weight)
        c.pen_far, c.pen_hit, c.w_path, c.w_goal = int(self.far_penalty), int(self.hit_penalty), int(self.path_weight), int(self.goal_weight)
        c.path_cap, c.reach = float(self.path_cap), int(self.distance_reach)
        c.allow_reverse, c.min_turning_radius = bool(self.allow_reverse), float(self.min_turning_radius)
        c.seed = int(self.seed) & (2 ** 64 - 1)
        c.mover_margin, c.mover_weight, c.mover_hit_penalty = float(self.mover_margin), float(self.mover_weight), int(self.mover_hit_penalty)
        c.field_run_weight, c.field_goal_weight, c.field_cap = int(self.field_run_weight), int(self.field_goal_weight), int(self.field_cap)
        c.acceleration_limits = bool(self.acceleration_limits)
        c.footprint_margin = float(self.footprint_margin)
        return c


def _moving_obstacles(given) -> list:
    """A sequence of (x, y, vx, vy, radius), an (n, 5) array, or objects with those attributes -> [MovingObstacle]."""
    if given is None:
        return []
    if isinstance(given, np.ndarray):
        if given.size == 0:
            return []
        if given.ndim != 2 or given.shape[1] != 5:
            raise ValueError(f"moving_obstacles as an array is (n, 5): x, y, vx, vy, radius; got {given.shape}")
    out = []
    for o in given:
        if isinstance(o, kompass_cpp.control.MovingObstacle):
            out.append(o)
        elif all(hasattr(o, k) for k in ("x", "y", "vx", "vy", "radius")):
            out.append(kompass_cpp.control.MovingObstacle(float(o.x), float(o.y), float(o.vx), float(o.vy), float(o.radius)))
        else:
            v = [float(a) for a in o]
            if len(v) != 5:
                raise ValueError(f"a moving obstacle is (x, y, vx, vy, radius), got {len(v)} values")
            out.append(kompass_cpp.control.MovingObstacle(*v))
    return out


class MPPI(FollowerTemplate):
    def __init__(self, robot: Robot, ctrl_limits: RobotCtrlLimits, config: Optional[MPPIConfig] = None,
                 config_file: Optional[str] = None, config_root_name: Optional[str] = None, control_time_step: float = 0.1, **_):
        if config_file:
            raise NotImplementedError("config files are not read by this build; pass an MPPIConfig")
        self._robot = robot
        self._config = config or MPPIConfig()
        self._control_time_step = float(control_time_step)
        self._got_path = False
        self._planner = kompass_cpp.control.MPPI(control_type=RobotType.to_kompass_cpp_lib(robot.robot_type),
                                                 control_limits=ctrl_limits.to_kompass_cpp_lib(),
                                                 time_step=self._control_time_step, config=self._config.to_kompass_cpp())
        if self._config.footprint == "box":
            if robot.geometry_type != RobotGeometry.Type.BOX:
                raise ValueError(f'MPPIConfig(footprint="box") needs a BOX robot, got {robot.geometry_type}')
            length, width = (float(v) for v in np.asarray(robot.geometry_params, dtype=float).reshape(-1)[:2])
            self._planner.set_box_footprint(length, width)
        self._params = kompass_cpp.control.FollowerParameters()
        self._params.from_dict({k: float(getattr(self._config, k)) for k in (
            "max_point_interpolation_distance", "lookahead_distance", "goal_dist_tolerance", "goal_orientation_tolerance",
            "path_segment_length", "loosing_goal_distance")})
        self._planner.set_follower_params(self._params)
        self._result = None
        self._warned_r2 = False
        self._cost_field = None
        logging.info("MPPI CONTROLLER IS READY")

    @property
    def planner(self) -> "kompass_cpp.control.MPPI":
        return self._planner

    def loop_step(self, *, current_state: RobotState, local_map=None, moving_obstacles=None, cost_field=None, **_) -> bool:
        """One control step over `local_map`, a WorldMap (kompass_core.mapping.WorldMap or the kompass_cpp class); its
        distance plane is enabled when it is off.  Nothing else can serve: the controller reads the plane on the device.

        moving_obstacles: discs in the world frame at the time of `current_state`, metres and m/s: a sequence of (x, y,
        vx, vy, radius), an (n, 5) array, or objects with those attributes.  They hold for this step only: None or an
        empty sequence clears the list.  More than 64: the 64 nearest to the robot are taken.

        cost_field: a `kompass_core.planning.GridPlanner` that has solved (or replanned) on `local_map`; for this step
        the controller steers by its kept cost-to-go field, read where it lies on the device, instead of the path (rules
        19 to 24): no path need be set, and the goal is the planner's.  None: the path mode.  ValueError when the
        planner's grid was not read from this map, or the map's window has moved since (`WorldMap.shift` / `recentre`)
        and the planner has not read it again through `replan(map=world_map)`.  `field_at_robot` tells afterwards
        whether the robot stands where the field has a value; the controller itself does not refuse."""
        world_map = cpp_world_map(local_map)
        if world_map is None:
            raise TypeError("MPPI.loop_step needs local_map=<WorldMap>: it costs its samples against the world map's "
                            f"distance plane on the device, got {type(local_map).__name__}")
        if cost_field is None:
            if self._planner.has_cost_field:
                self._planner.clear_cost_field()
        else:
            if not hasattr(cost_field, "reads") or not hasattr(cost_field, "_planner"):
                raise TypeError(f"cost_field is a kompass_core.planning.GridPlanner, got {type(cost_field).__name__}")
            if not cost_field.reads(world_map):
                raise ValueError("cost_field: the planner's grid was not read from this WorldMap at its present window "
                                 "offset; plan on it (setup_problem(grid=world_map) / replan(map=world_map)) first")
            hit_r2 = int(round(float(self._config.hit_radius) ** 2))
            if cost_field.footprint_r2 < hit_r2 and not self._warned_r2:
                logging.warning("MPPI: the planner's footprint r2 = %d is below the controller's hit r2 = %d: a cell the "
                                "field holds valid can be a hit", cost_field.footprint_r2, hit_r2)
                self._warned_r2 = True
            self._planner.set_cost_field(cost_field._planner)
        self._cost_field = cost_field   # kept alive while attached
        self._planner.set_moving_obstacles(_moving_obstacles(moving_obstacles))
        self._result = self._planner.execute(
            world_map, kompass_cpp.types.State(current_state.x, current_state.y, current_state.yaw, current_state.speed))
        return self._result.status in (kompass_cpp.control.FollowingStatus.COMMAND_FOUND,
                                       kompass_cpp.control.FollowingStatus.GOAL_REACHED)

    def logging_info(self) -> str:
        if self._result:
            v = self._result.velocity_command
            return f"MPPI status: {self._result.status}, Cmd: vx={v.vx:.2f}, vy={v.vy:.2f}, w={v.omega:.2f}"
        return "MPPI not started"

    def _controls(self, k) -> List[float]:
        """The first control_horizon entries of the new sequence; the first is the command the acceleration limits let
        through."""
        if not self._result or self._result.status != kompass_cpp.control.FollowingStatus.COMMAND_FOUND:
            return [0.0]
        v = self._result.velocity_command
        first = (v.vx, v.vy, v.omega)[k]
        return [first] + [c[k] for c in self._planner.controls(int(self._config.control_horizon))[1:]]

    @property
    def linear_x_control(self) -> List[float]:
        return self._controls(0)

    @property
    def linear_y_control(self) -> List[float]:
        return self._controls(1)

    @property
    def angular_control(self) -> List[float]:
        return self._controls(2)

    def predicted_path(self):
        """The new sequence rolled out on the host by rule 4: [(x, y, yaw)] in the world, one a step."""
        return [tuple(p) for p in self._planner.predicted_path()]

    @property
    def record(self):
        """(s_min, k_best, s_0, den, n_hit, step) of the last step."""
        return tuple(self._planner.last_record)

    @property
    def field_at_robot(self) -> int:
        """The cost field at the robot's cell in the last step with a cost_field, in the planner's units (10 a straight
        cell); 0xFFFFFFFF when the robot stands in an invalid or cut-off cell or outside the map."""
        return int(self._planner.field_at_robot)

    @property
    def last_velocity(self):
        """(F, L, H) in the roll-out's integers that the last command was formed from, and the next step's start velocity
        (rule 28); zero before a step with acceleration_limits, after a reset and when the map's resolution changes."""
        return tuple(int(v) for v in self._planner.last_velocity)

    @property
    def footprint(self):
        """(the disc offsets along the heading in cells, r2) the last step ran with: one offset 0.0 and hit_radius' r2 in
        "disc" mode; None before a step."""
        if self._result is None:
            return None
        i = self._planner.last_inputs
        return ([o / 65536.0 for o in i["offsets"]] or [0.0]), int(i["r2"])

    @property
    def n_hit_moving(self) -> int:
        """The samples of the last step that a moving obstacle ended (they are among the record's n_hit)."""
        return int(self._planner.last_n_hit_moving)
