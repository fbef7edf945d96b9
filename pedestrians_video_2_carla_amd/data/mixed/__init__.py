from pedestrians_video_2_carla_amd.data.mixed.mixed_dataset import MixedDataset  # noqa: F401
from pedestrians_video_2_carla_amd.data.mixed.mixed_datamodule import (  # noqa: F401
    CarlaRecAMASSDataModule, JAADCarlaRecAMASSDataModule, JAADCarlaRecBenchmarkDataModule, JAADCarlaRecDataModule,
    MixedDataModule)
from pedestrians_video_2_carla_amd.data.mixed.pipeline import MixedProjection2DPipeline  # noqa: F401
from pedestrians_video_2_carla_amd.data.mixed.loader import MixedDeviceLoader  # noqa: F401
