from .local_mapper import LocalMapper, MapConfig, ScanModelConfig  # noqa: F401
from .mcl import MCL, MCLEstimate  # noqa: F401
from .movers import MoverDetection, MoverTracker  # noqa: F401
from .world_map import WorldMap, WorldMapMatch  # noqa: F401
