"""Heatmap targets for loaders (reference data/base/mixins/dataset/video_mixin.py:186-225, ``_add_heatmaps_to_targets``).

The reference's video datasets build ``targets['heatmaps']`` per clip on DataLoader workers, at the clip's full resolution, in a
Python loop over frames and joints. ``HeatmapTargets`` is the batched replacement a loader calls once per batch: on the device it
is one K28a launch that writes the maps already pooled to the model's output resolution (``ops.heatmap_targets``); on the host,
the tensor restatement of the same. ``pool=None`` reproduces the reference's full-resolution maps bit for bit.
"""
from typing import Dict, Optional, Tuple

from torch import Tensor


class HeatmapTargets:
    def __init__(self, sigma: int = 1, clip_size: Tuple[int, int] = (368, 368), pool: Optional[Tuple[int, int, int]] = (9, 8, 1)):
        self.sigma, self.clip_size, self.pool = sigma, (int(clip_size[0]), int(clip_size[1])), pool

    @staticmethod
    def add_cli_args(parser):
        parser.add_argument('--heatmaps_sigma', type=int, default=1,
                            help='Standard deviation, in pixels of the clip, of the Gaussian target heatmaps.')
        return parser

    def __call__(self, projection_2d: Tensor, shifts: Tensor, original_size: Tuple[int, int]) -> Tensor:
        """``projection_2d`` (B,T,J,>=2) in pixels of the original frame, ``shifts`` (B,T,2) the crop's offset,
        ``original_size`` = (height, width) the crop was resized from -> (B,T,J+1,oh,ow)."""
        from pedestrians_video_2_carla_amd import ops
        (ch, cw), (oh, ow) = self.clip_size, original_size
        return ops.heatmap_targets(projection_2d, shifts, (cw / float(ow), ch / float(oh)), self.clip_size, self.sigma, self.pool)

    def add_to_targets(self, targets: Dict[str, Tensor], shifts: Tensor, original_size: Tuple[int, int]) -> Dict[str, Tensor]:
        targets['heatmaps'] = self(targets['projection_2d'], shifts, original_size)
        return targets
