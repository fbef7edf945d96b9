"""``PedestrianLogger``: the video logger a ``Trainer`` carries in ``loggers`` (reference loggers/pedestrian/pedestrian_logger.py:
26-113, restated without Lightning's logger base). It decides once, in the reference's order, which renderers survive and whether
anything is written at all; the writer is built on first use."""
import os
import warnings
from typing import List, Union

from .disabled_pedestrian_writer import DisabledPedestrianWriter
from .enums import MergingMethod, PedestrianRenderers
from .pedestrian_writer import PedestrianWriter


class PedestrianLogger(object):
    def __init__(self,
                 save_dir: str,
                 name: str,
                 version: Union[int, str] = 0,
                 log_every_n_steps: int = 50,
                 video_saving_frequency_reduction: int = 10,
                 renderers: List[PedestrianRenderers] = None,
                 **kwargs):
        """``log_every_n_steps`` should be the trainer's; clips are written every ``log_every_n_steps *
        video_saving_frequency_reduction`` steps. ``kwargs`` go to the writer: ``input_nodes``, ``output_nodes``, ``max_videos``,
        ``merging_method``, ``fps``, ``image_size``, ``radius``, ``line_width``, ``video_writer`` and the accepted, unused
        ``source_videos_*`` / ``body_model_dir``."""
        self._save_dir = save_dir
        self._name = name
        self._version = version
        self._kwargs = kwargs
        self._experiment = None
        self._writer_cls = PedestrianWriter

        self._video_saving_frequency_reduction = video_saving_frequency_reduction
        self._log_every_n_steps = log_every_n_steps
        self._reduced_log_every_n_steps = log_every_n_steps * video_saving_frequency_reduction

        if self._reduced_log_every_n_steps <= 1:
            warnings.warn('Video logging interval set to 0. Disabling video output.')
            self._writer_cls = DisabledPedestrianWriter

        self._renderers = list(renderers) if renderers else []

        def drop(renderer, message):
            if renderer in self._renderers:
                self._renderers = [r for r in self._renderers if r != renderer]
                if message:
                    warnings.warn(message)

        # no CARLA client, no body model and no source-video reader are built here: not a question of what is installed
        if PedestrianRenderers.carla in self._renderers or PedestrianRenderers.source_carla in self._renderers:
            warnings.warn('CARLA renderers not available. Disabling CARLA renderers.')
            drop(PedestrianRenderers.carla, None)
            drop(PedestrianRenderers.source_carla, None)
        drop(PedestrianRenderers.smpl, 'SMPL renderer not available. Disabling SMPL renderer.')
        drop(PedestrianRenderers.none, None)
        drop(PedestrianRenderers.source_videos, 'Source videos renderer not available. Disabling source videos renderer.')
        if kwargs.get('output_nodes', None) is None:
            drop(PedestrianRenderers.projection_points, 'No output_nodes was specified. Disabling projection_points renderer.')

        if len(self._renderers) == 0:
            warnings.warn('No renderers specified. Disabling video output.')
            self._writer_cls = DisabledPedestrianWriter

    @staticmethod
    def add_logger_specific_args(parent_parser):
        parser = parent_parser.add_argument_group('Pedestrian Logger')
        parser.add_argument('--video_saving_frequency_reduction', dest='video_saving_frequency_reduction', metavar='REDUCTION',
                            default=10, type=lambda x: max(int(x), 0),
                            help='Save videos every REDUCTION * log_every_n_steps. If 0 or less disables saving videos.')
        parser.add_argument('--max_videos', dest='max_videos', default=10, type=int,
                            help='Maximum number of videos to save from each batch; -1 saves all. Default: 10')
        parser.add_argument('--renderers', dest='renderers', metavar='RENDERER', default=[], choices=list(PedestrianRenderers),
                            nargs='+', action='extend', type=PedestrianRenderers.__getitem__,
                            help="Renderers to use for video output; to disable rendering pass 'none' as the only renderer. "
                                 'Choices: {}.'.format(set(PedestrianRenderers.__members__.keys())))
        parser.add_argument('--merging_method', dest='merging_method', metavar='METHOD', default=MergingMethod.square,
                            choices=list(MergingMethod), type=MergingMethod.__getitem__,
                            help="How to merge multiple videos into one. Choices: {}. Default: 'square'".format(
                                set(MergingMethod.__members__.keys())))
        # accepted for command-line compatibility; the source videos renderer is not built
        parser.add_argument('--source_videos_dir', dest='source_videos_dir', default=None)
        parser.add_argument('--source_videos_overlay_skeletons', dest='source_videos_overlay_skeletons', default=False,
                            action='store_true')
        parser.add_argument('--source_videos_overlay_bboxes', dest='source_videos_overlay_bboxes', default=False, action='store_true')
        parser.add_argument('--source_videos_overlay_classes', dest='source_videos_overlay_classes', default=False,
                            action='store_true')
        return parent_parser

    @property
    def name(self) -> str:
        return self._name

    @property
    def version(self) -> Union[int, str]:
        return self._version

    @property
    def save_dir(self) -> str:
        return self._save_dir

    @property
    def log_dir(self) -> str:
        return os.path.join(self._save_dir, self._name, str(self._version))

    @property
    def renderers(self) -> List[PedestrianRenderers]:
        return list(self._renderers)

    @property
    def reduced_log_every_n_steps(self) -> int:
        return self._reduced_log_every_n_steps

    @property
    def disabled(self) -> bool:
        return self._writer_cls is DisabledPedestrianWriter

    @property
    def experiment(self):
        if self._experiment is None:
            self._experiment = self._writer_cls(log_dir=self.log_dir, renderers=self._renderers,
                                                reduced_log_every_n_steps=self._reduced_log_every_n_steps, **self._kwargs)
        return self._experiment

    def log_hyperparams(self, params):
        pass

    def log_metrics(self, metrics, step):
        pass
