"""Moving obstacles from raw laser scans: what `WorldMap.detect_movers` finds (DESIGN.md 4.11 rules 64 to 69) and the
tracker that turns it, scan after scan, into the list `MPPI.loop_step(moving_obstacles=...)` takes.

The loop on raw scans: localise, `world_map.detect_movers(state, scan)`, `tracker.update(detection, dt)`,
`world_map.integrate_scan(state, scan, skip=tracker.skip_mask(detection))`, plan,
`mppi.loop_step(..., moving_obstacles=tracker.moving_obstacles())`.

Not built: a circular scan seam (a mover across the first and last beam gives two clusters); settling a long-stationary
track into the map (it stays a zero-velocity mover, which MPPI avoids and the planner does not see); clearing the free
space along a skipped beam; movers closer than sqrt(m2) cells to a wall; association better than greedy nearest
neighbour; accelerating movers; movers for DWA, PurePursuit or DVZ."""
from __future__ import annotations

from typing import Optional

import numpy as np

import kompass_cpp


class MoverDetection:
    """`clusters`: float64 [n, 3] of (x, y, radius) in world metres; `labels`: int32 a beam, the kept cluster's number,
    -1 for a beam that is not dynamic, -2 for a dynamic beam of a dropped run; `record`: (n_dynamic, n_runs, n_kept,
    n_returned); `raw`: rule 68's integers a cluster; `resolution`: the map's."""

    def __init__(self, detection, resolution: float):
        self._detection = detection
        self.resolution = float(resolution)
        self.clusters = np.array([(c.x, c.y, c.radius) for c in detection.clusters], np.float64).reshape(-1, 3)
        self.labels = np.asarray(detection.labels)
        self.record = tuple(detection.record)
        self.raw = [c.raw for c in detection.clusters]

    def __len__(self):
        return len(self.clusters)

    def __repr__(self):
        return f"MoverDetection(clusters={len(self)}, record={self.record})"


class MoverTracker:
    def __init__(self, alpha: float = 0.5, beta: float = 0.3, max_misses: int = 3, gate: Optional[float] = None,
                 gate_cells: float = 6.0):
        """An alpha-beta track a mover with a two-point start, greedy nearest-neighbour association in track order; host
        only.  gate: the furthest a cluster may lie from a track's prediction, in metres; None: gate_cells times the
        resolution of the first detection.  alpha = 0.5, beta = 0.3, max_misses = 3 and a gate of 6 cells are the
        prototype's values: judgement, not measurement."""
        self._cfg = (float(alpha), float(beta), int(max_misses))
        self._gate = None if gate is None else float(gate)
        self._gate_cells = float(gate_cells)
        self._tracker = None if gate is None else kompass_cpp.mapping.MoverTracker(*self._cfg, self._gate)

    def update(self, detection, dt: float) -> None:
        """One scan's `MoverDetection` (or an (n, 3) array of x, y, radius), dt seconds after the last."""
        if isinstance(detection, MoverDetection):
            if self._tracker is None:
                self._tracker = kompass_cpp.mapping.MoverTracker(*self._cfg, self._gate_cells * detection.resolution)
            self._tracker.update(detection._detection, float(dt))
            return
        if self._tracker is None:
            raise ValueError("clusters as an array need the gate in metres: MoverTracker(gate=...)")
        rows = np.asarray(detection, dtype=np.float64).reshape(-1, 3)
        self._tracker.update([kompass_cpp.mapping.MoverCluster(float(x), float(y), float(r)) for x, y, r in rows], float(dt))

    @property
    def tracks(self):
        """The live tracks in creation order: id, x, y, vx, vy, radius, hits, misses"""
        return [] if self._tracker is None else list(self._tracker.tracks)

    def moving_obstacles(self) -> np.ndarray:
        """float64 [n, 5] of (x, y, vx, vy, radius), a row a live track: what `MPPI.loop_step(moving_obstacles=...)` takes"""
        return np.array([(t.x, t.y, t.vx, t.vy, t.radius) for t in self.tracks], np.float64).reshape(-1, 5)

    @staticmethod
    def skip_mask(detection) -> np.ndarray:
        """bool a beam: the member beams of every kept cluster, for `WorldMap.integrate_scan(skip=...)`"""
        labels = detection.labels if hasattr(detection, "labels") else detection
        return np.asarray(labels) >= 0

    def clear(self) -> None:
        if self._tracker is not None:
            self._tracker.clear()
