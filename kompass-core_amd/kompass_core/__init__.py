"""kompass_core front-end subset for the MI355X build.

Mirrors the Python layer of the reference that sits on the accelerated hot path
(`kompass_core.control.DWA` / `PurePursuit` / `Stanley` / `DVZ` / `VisionRGBFollower` /
`VisionRGBDFollower`, `kompass_core.mapping.LocalMapper`, `kompass_core.vision.DepthDetector`, the grid planner
`kompass_core.planning.GridPlanner`
and the model / datatype helpers their harness uses); everything else of kompass_core
(PID, OMPL, calibration ...) is out of scope.
"""
import kompass_cpp  # noqa: F401  (the compiled module; fails loudly if not built)

from . import algorithms, control, datatypes, mapping, models, planning, vision  # noqa: F401
