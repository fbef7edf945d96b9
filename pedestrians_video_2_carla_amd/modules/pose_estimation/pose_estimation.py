"""Base of the pose-estimation models (reference modules/pose_estimation/pose_estimation.py:5-12): frames in, heatmaps out."""
from pedestrians_video_2_carla_amd.modules.flow.output_types import PoseEstimationModelOutputType
from pedestrians_video_2_carla_amd.modules.movements.movements import MovementsModel


class PoseEstimationModel(MovementsModel):
    @property
    def output_type(self) -> PoseEstimationModelOutputType:
        return PoseEstimationModelOutputType.heatmaps

    @property
    def needs_heatmaps(self) -> bool:
        return self.output_type == PoseEstimationModelOutputType.heatmaps
