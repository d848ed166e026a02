from ._trajectory_ import TrajectoryCostsWeights  # noqa: F401
from ._base_ import FollowerConfig, FollowerTemplate  # noqa: F401
from .dwa import DWA, DWAConfig  # noqa: F401
from .pure_pursuit import PurePursuit, PurePursuitConfig  # noqa: F401
from .stanley import Stanley, StanleyConfig  # noqa: F401
from .dvz import DVZ, DVZConfig  # noqa: F401
from .mppi import MPPI, MPPIConfig  # noqa: F401
from .rgb_follower import VisionRGBFollower, VisionRGBFollowerConfig  # noqa: F401
from .rgbd_follower import VisionRGBDFollower, VisionRGBDFollowerConfig  # noqa: F401
from kompass_cpp.types import PathInterpolationType  # noqa: F401
