from .laserscan import LaserScanData  # noqa: F401
from kompass_cpp.types import Bbox2D, Bbox3D, PointsOfInterest  # noqa: F401
