"""``python -m pedestrians_video_2_carla_amd ...``: the launcher (modeling.py)."""
from pedestrians_video_2_carla_amd.modeling import run

if __name__ == '__main__':
    run()
