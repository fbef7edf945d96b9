from .disabled_pedestrian_writer import DisabledPedestrianWriter
from .enums import MergingMethod, PedestrianRenderers
from .pedestrian_logger import PedestrianLogger
from .pedestrian_writer import PedestrianWriter

__all__ = ['DisabledPedestrianWriter', 'MergingMethod', 'PedestrianLogger', 'PedestrianRenderers', 'PedestrianWriter']
