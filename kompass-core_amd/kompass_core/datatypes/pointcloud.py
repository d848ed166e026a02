"""PCD maps and the PointCloudData record (src/kompass_core/datatypes/pointcloud.py): the reader is host code,
the cloud -> occupancy grid runs on the device (kompass_cpp.utils.read_pcd_to_occupancy_grid)."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
from attrs import define, field, validators
from kompass_cpp.utils import read_pcd, read_pcd_to_occupancy_grid


def get_points_from_pcd(file_path: str) -> np.ndarray:
    """The points of a PCD file as an (N, 3) float32 array."""
    return read_pcd(file_path)


def get_occupancy_grid_from_pcd(file_path: str, grid_resolution: float, z_ground_limit: float,
                                robot_height: float) -> Tuple[np.ndarray, list]:
    """(grid, origin) of a PCD file: grid an int8 (cells_x, cells_y) array of -1 / 0 / 100 (no point or only
    points above robot_height / ground up to z_ground_limit / an obstacle up to robot_height), origin
    [min_x, min_y, 0]."""
    return read_pcd_to_occupancy_grid(file_path, grid_resolution, z_ground_limit, robot_height)


@define
class PointCloudData:
    """PointCloud data class: a PointCloud2-style byte buffer and its layout"""

    data: np.ndarray = field()
    point_step: int = field(validator=validators.gt(0))
    row_step: int = field(validator=validators.gt(0))
    height: int = field(validator=validators.gt(0))
    width: int = field(validator=validators.gt(0))
    x_offset: Optional[int] = field(default=None)
    y_offset: Optional[int] = field(default=None)
    z_offset: Optional[int] = field(default=None)
