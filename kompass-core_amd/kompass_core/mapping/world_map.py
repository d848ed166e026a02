"""World map front end: a world-frame occupancy map that stays on the device, fused from the `LocalMapper`'s
egocentric grids (`kompass_cpp.mapping.WorldMap`).

Not in the reference, which leaves the world-frame map to its ROS side.  The `LocalMapper`'s grid turns with the
robot and forgets what leaves its window; `GridPlanner.replan` wants a world-frame map that changes.  This is the
map between the two: seeded from a prior (the PCD grid), updated from each local grid where that grid lies, and
handed to the planner in place (`setup_problem(None, ..., grid=world_map)`, `replan(map=world_map)`)."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

import kompass_cpp


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

    def set_model(self, hit: int = 3, miss: int = 1, e_min: int = -8, e_max: int = 14, occ_thr: int = 1) -> None:
        """Another update model; clears the map (evidence counted by one model means nothing under another)."""
        self._map.set_model(hit=int(hit), miss=int(miss), e_min=int(e_min), e_max=int(e_max), occ_thr=int(occ_thr))

    def set_prior(self, grid) -> None:
        """grid[I, J]: an int8 / int32 (width, height) array (`points_to_occupancy_grid` gives one), or a device array
        with `__cuda_array_interface__` in column-major strides.  100 -> occupied at e_max, 0 -> empty at e_min,
        anything else never observed.  Replaces the whole state."""
        self._map.set_prior(grid)

    def update(self, robot_state, local_map) -> int:
        """Fuse one local grid; robot_state (x, y, yaw): the robot's pose in the world.  local_map: the front end's
        `LocalMapper` or a `kompass_cpp.mapping.LocalMapper` (its last grid where it lies on the device, no host
        round trip), or an int32 (grid_height, grid_width) array as `LocalMapper.occupancy`.  -> cells whose class
        changed."""
        mapper = local_map
        if hasattr(local_map, "_mapper"):  # the front end's LocalMapper holds the class once it has mapped a scan
            mapper = local_map._mapper
            if mapper is None:
                raise ValueError("the LocalMapper has no grid yet: update it from a scan first")
        if not isinstance(mapper, kompass_cpp.mapping.LocalMapper):
            mapper = np.asarray(mapper)
        return self._map.update(mapper, float(robot_state.x), float(robot_state.y), float(robot_state.yaw))

    def clear(self) -> None:
        self._map.clear()

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
