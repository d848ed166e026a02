from .laserscan import LaserScanData  # noqa: F401
from .pointcloud import PointCloudData, get_occupancy_grid_from_pcd, get_points_from_pcd  # noqa: F401
from kompass_cpp.types import Bbox2D, Bbox3D, PointsOfInterest  # noqa: F401
