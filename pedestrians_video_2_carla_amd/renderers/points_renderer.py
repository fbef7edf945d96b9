"""The renderers of the video logger that need nothing but the key points.

The reference takes ``Renderer`` and ``PointsRenderer`` from the external ``pedestrians_scenarios`` package
(pedestrian_writer.py:8-10), which draws each frame with PIL on the host and hands back images. Here a renderer hands back a
*panel description* for ``ops.render_points`` -- ``(points, colors, edges)``, or None for a black panel -- so that one launch (K34)
draws every panel, video and frame of a logged batch. That package is not available: pixel parity with its drawing is unpinned, the
rules in include/p2c.h (K34) are the definition."""
from typing import Optional, Tuple, Type

import torch
from torch import Tensor

from pedestrians_video_2_carla_amd.data.base.skeleton import Skeleton


class Renderer(object):
    """The zeros renderer: a black panel of ``image_size = (width, height)``."""

    def __init__(self, image_size: Tuple[int, int] = (800, 600), **kwargs) -> None:
        self._image_size = (int(image_size[0]), int(image_size[1]))

    @property
    def image_size(self) -> Tuple[int, int]:
        return self._image_size

    def render(self, frames: Optional[Tensor] = None, **kwargs):
        return None


class PointsRenderer(Renderer):
    """Key points as discs of ``radius`` in the skeleton's colours (``input_nodes.get_colors()``, RGB only), bones of
    ``line_width`` pixels between ``input_nodes.get_edges()`` when ``line_width`` > 0."""

    def __init__(self, input_nodes: Type[Skeleton], image_size: Tuple[int, int] = (800, 600), radius: int = 2, line_width: int = 0,
                 **kwargs) -> None:
        super().__init__(image_size=image_size)
        self._input_nodes = input_nodes
        self.radius, self.line_width = int(radius), int(line_width)
        colors = input_nodes.get_colors()
        self._colors = torch.tensor([tuple(colors[k])[:3] for k in input_nodes], dtype=torch.uint8)
        edges = [(a.value, b.value) for a, b in input_nodes.get_edges()] if self.line_width > 0 else []
        self._edges = torch.tensor(edges, dtype=torch.int64).reshape(-1, 2)
        self._on = {}

    def render(self, frames: Tensor, **kwargs):
        """``frames`` (V,T,J,C>=2) in pixels -> ``(points, colors, edges)`` on the frames' device (the tables are moved there once)."""
        if frames.ndim != 4 or frames.shape[2] != len(self._colors):
            raise RuntimeError(f'PointsRenderer({self._input_nodes.__name__}): points (V,T,{len(self._colors)},C) expected, '
                               f'got {tuple(frames.shape)}')
        if frames.device not in self._on:
            self._on[frames.device] = (self._colors.to(frames.device), self._edges.to(frames.device))
        return (frames, *self._on[frames.device])
