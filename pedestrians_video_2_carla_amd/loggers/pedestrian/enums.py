"""The logger's enums (reference loggers/pedestrian/enums.py:4-24): the same members and values, so command lines and saved
hyper-parameters carry over. The renderers that need a CARLA server, source videos or a body model keep their names and are
dropped by ``PedestrianLogger`` with a warning."""
from enum import Enum


class PedestrianRenderers(Enum):
    none = 0                  # rendering is off when this is the only renderer
    source_videos = 1         # not built here
    source_carla = 2          # not built here
    target_points = 3         # the original data
    input_points = 4          # what the model sees (after noise / missing joints)
    projection_points = 5     # what the model projects
    carla = 6                 # not built here
    smpl = 7                  # not built here
    zeros = 100               # a black panel


class MergingMethod(Enum):
    vertical = 0
    horizontal = 1
    square = 2
