from .linear import Linear  # noqa: F401
from .pose_estimation import PoseEstimationModel  # noqa: F401
