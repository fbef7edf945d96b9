from pedestrians_video_2_carla_amd.data.smpl.skeleton import SMPL_SKELETON  # noqa: F401
