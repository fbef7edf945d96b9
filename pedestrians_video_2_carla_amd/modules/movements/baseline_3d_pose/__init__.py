from .baseline_3d_pose import Baseline3DPose, Baseline3DPoseRot  # noqa: F401
