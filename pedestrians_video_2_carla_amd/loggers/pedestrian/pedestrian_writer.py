"""``PedestrianWriter``: which clips of a batch are drawn, how their panels merge, where the files go (reference
loggers/pedestrian/pedestrian_writer.py:27-307, restated).

The policy is the reference's. The pixels are not drawn per frame with PIL on the host: every used renderer hands back a panel
description and ONE ``ops.render_points`` call (K34 on the device) draws all panels, videos and frames of the logged batch, already
merged; one copy brings them to the host. The renderers that need a CARLA server, source videos or a body model are not built:
``PedestrianLogger`` drops them, and one that reaches the writer anyway is a black panel."""
import math
import os
from typing import Any, Callable, Dict, List, Optional, Tuple, Type

import torch
from torch import Tensor

from pedestrians_video_2_carla_amd.data.base.skeleton import Skeleton
from pedestrians_video_2_carla_amd.renderers.points_renderer import PointsRenderer, Renderer
from pedestrians_video_2_carla_amd.transforms.pose.normalization.hips_neck_extractor import HipsNeckExtractor
from pedestrians_video_2_carla_amd.transforms.pose.normalization.reference_skeletons_denormalizer import \
    ReferenceSkeletonsDeNormalizer

from .enums import MergingMethod, PedestrianRenderers


def npz_video_writer(path: str, frames: Tensor, fps: float) -> str:
    """``frames`` uint8 (T,H,W,3) -> ``path + '.npz'`` holding ``frames`` and ``fps`` (no codec needed)."""
    import numpy as np
    np.savez_compressed(path + '.npz', frames=frames.numpy(), fps=np.float64(fps))
    return path + '.npz'


def default_video_writer() -> Callable[[str, Tensor, float], Any]:
    """``torchvision.io.write_video`` to ``path + '.mp4'`` as the reference does when torchvision is installed, else the .npz writer."""
    try:
        import torchvision.io
    except ImportError:
        return npz_video_writer

    def mp4_video_writer(path: str, frames: Tensor, fps: float) -> str:
        torchvision.io.write_video(path + '.mp4', frames, fps=fps)
        return path + '.mp4'
    return mp4_video_writer


def grid_layout(n: int, merging_method: MergingMethod) -> Tuple[MergingMethod, int, int]:
    """(method used, rows, cols) for ``n`` renderers (pedestrian_writer.py:55-73): fewer than three under ``square`` lie side by
    side; ``square`` is ceil(sqrt(n)) columns and as many rows as they need; ``vertical`` is one column."""
    if n < 3 and merging_method == MergingMethod.square:
        merging_method = MergingMethod.horizontal
    if merging_method == MergingMethod.square:
        cols = int(math.ceil(math.sqrt(n)))
        return merging_method, int(math.ceil(n / cols)), cols
    if merging_method == MergingMethod.vertical:
        return merging_method, n, 1
    return merging_method, 1, n


class _HostHipsNeck(object):
    """The hips-neck normaliser and de-normaliser on tensor ops, for host tensors (the project's normaliser is a device kernel):
    shift = mean of the hips joints, scale = |mean of the neck joints - shift| (reference extractor.py:23-36,
    normalizer.py:21-43)."""

    def __init__(self, nodes: Type[Skeleton], near_zero: float = 1e-5) -> None:
        self._hips, self._neck = HipsNeckExtractor(nodes).points()
        self._near_zero = near_zero

    def shift_scale(self, sample: Tensor) -> Tuple[Tensor, Tensor]:
        shift = sample[..., list(self._hips), :].mean(-2)
        return shift, torch.linalg.norm(sample[..., list(self._neck), :].mean(-2) - shift, dim=-1)

    def normalize(self, sample: Tensor) -> Tensor:
        shift, scale = self.shift_scale(sample[..., :2])
        out = sample.clone()
        out[..., :2] = torch.nan_to_num((sample[..., :2] - shift[..., None, :]) / scale[..., None, None], nan=0.0, posinf=0.0, neginf=0.0)
        if sample.shape[-1] > 2:
            out[..., :2] = out[..., :2].where(out[..., 2:3] >= self._near_zero, out.new_zeros(()))
        return out

    def from_projection(self, frames: Tensor, meta: Dict[str, List[Any]], autonormalize: bool = False) -> Tensor:
        from pedestrians_video_2_carla_amd.data.carla import reference as ref
        if autonormalize:
            frames = self.normalize(frames)
        types = ref.skeleton_types_from_meta(meta, batch_size=len(frames), device=frames.device).long()
        shift, scale = self.shift_scale(ref.get_projections(frames.device)[types][..., :2])      # (V,2), (V)
        head = frames[..., :2] * scale[:, None, None, None] + shift[:, None, None, :]
        return head if frames.shape[-1] == 2 else torch.cat((head, frames[..., 2:]), dim=-1)


class PedestrianWriter(object):
    def __init__(self,
                 log_dir: str,
                 renderers: List[PedestrianRenderers],
                 input_nodes: Type[Skeleton],
                 output_nodes: Type[Skeleton] = None,
                 reduced_log_every_n_steps: int = 500,
                 fps: float = 30.0,
                 max_videos: int = 10,
                 merging_method: MergingMethod = MergingMethod.square,
                 image_size: Tuple[int, int] = (800, 600),
                 radius: int = 2,
                 line_width: int = 0,
                 video_writer: Optional[Callable[[str, Tensor, float], Any]] = None,
                 **kwargs) -> None:
        self._log_dir = log_dir
        self._reduced_log_every_n_steps = reduced_log_every_n_steps
        self._fps = fps
        self._max_videos = max_videos
        self._videos_slice = slice(0, max_videos) if max_videos > 0 else slice(None)

        self._used_renderers: List[PedestrianRenderers] = list(renderers)
        self._merging_method, self._video_rows, self._video_columns = grid_layout(len(self._used_renderers), merging_method)
        # a square that the renderers do not fill is padded with black panels
        self._used_renderers += [PedestrianRenderers.zeros] * (self._video_rows * self._video_columns - len(self._used_renderers))

        self._input_nodes = input_nodes
        self._output_nodes = output_nodes
        self._image_size = (int(image_size[0]), int(image_size[1]))          # (width, height)
        self._radius, self._line_width = int(radius), int(line_width)
        self._video_writer = video_writer if video_writer is not None else default_video_writer()

        points = dict(image_size=self._image_size, radius=self._radius, line_width=self._line_width)
        zeros = Renderer(image_size=self._image_size)
        used = self._used_renderers
        self._renderers: Dict[PedestrianRenderers, Renderer] = {r: zeros for r in PedestrianRenderers}
        if PedestrianRenderers.input_points in used:
            self._renderers[PedestrianRenderers.input_points] = PointsRenderer(input_nodes=input_nodes, **points)
        if PedestrianRenderers.target_points in used:
            self._renderers[PedestrianRenderers.target_points] = PointsRenderer(input_nodes=input_nodes, **points)
        if PedestrianRenderers.projection_points in used and output_nodes is not None:
            self._renderers[PedestrianRenderers.projection_points] = PointsRenderer(input_nodes=output_nodes, **points)
        self._denormalizers = {}

    # ---- policy ---------------------------------------------------------------------------------------------------------------
    reduced_log_every_n_steps = property(lambda self: self._reduced_log_every_n_steps)
    used_renderers = property(lambda self: list(self._used_renderers))
    layout = property(lambda self: (self._video_rows, self._video_columns))
    merging_method = property(lambda self: self._merging_method)

    def wants(self, step: int, force: bool = False) -> bool:
        """The interval gate of ``log_videos`` (pedestrian_writer.py:140): step 0 and every multiple of the reduced interval."""
        return bool(force) or step % self._reduced_log_every_n_steps == 0

    def _from_projection(self, nodes, frames: Tensor, meta, autonormalize: bool = False) -> Tensor:
        """``ReferenceSkeletonsDeNormalizer(HipsNeckExtractor(nodes)).from_projection`` -- its kernels on the device, the same rules
        on tensor ops for host tensors."""
        key = (nodes, frames.is_cuda)
        if key not in self._denormalizers:
            self._denormalizers[key] = (ReferenceSkeletonsDeNormalizer(extractor=HipsNeckExtractor(input_nodes=nodes))
                                        if frames.is_cuda else _HostHipsNeck(nodes))
        return self._denormalizers[key].from_projection(frames, meta, autonormalize=autonormalize)

    # ---- the call -------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def log_videos(self,
                   meta: Dict[str, Any],
                   step: int,
                   batch_idx: int,
                   stage: str,
                   vid_callback: Callable = None,
                   force: bool = False,
                   inputs: Tensor = None,
                   targets: Dict[str, Tensor] = None,
                   projection_2d: Tensor = None,
                   projection_2d_transformed: Tensor = None,
                   **kwargs) -> None:
        if not self.wants(step, force):
            return
        s = self._videos_slice
        videos = self._render(inputs[s], {k: v[s] for k, v in targets.items()}, {k: v[s] for k, v in meta.items()},
                              projection_2d[s] if projection_2d is not None else None,
                              projection_2d_transformed[s] if projection_2d_transformed is not None else None, batch_idx)
        for vid_idx, (vid, vid_meta) in enumerate(videos):
            video_dir = os.path.join(self._log_dir, stage, vid_meta.get('set_name', None) or '', vid_meta['video_id'])
            os.makedirs(video_dir, exist_ok=True)
            name = '{pedestrian_id}-{clip_id:0>2d}-step={step:0>4d}'.format(
                pedestrian_id=vid_meta['pedestrian_id'], clip_id=int(vid_meta['clip_id']), step=step)
            self._video_writer(os.path.join(video_dir, name), vid, self._fps)
            if vid_callback is not None:
                vid_callback(vid, vid_idx, self._fps, stage, vid_meta)

    def _panels(self, frames: Tensor, targets: Dict[str, Tensor], meta, projection_2d, projection_2d_transformed) -> list:
        """One panel description per used renderer (pedestrian_writer.py:215-233, 257-265)."""
        used = self._used_renderers
        transformed = 'projection_2d_transformed' in targets
        points = {}
        if PedestrianRenderers.input_points in used:
            points[PedestrianRenderers.input_points] = self._from_projection(self._input_nodes, frames, meta,
                                                                             autonormalize=not transformed)
        if PedestrianRenderers.target_points in used:
            points[PedestrianRenderers.target_points] = self._from_projection(
                self._input_nodes, targets['projection_2d_transformed' if transformed else 'projection_2d'], meta,
                autonormalize=not transformed)
        if PedestrianRenderers.projection_points in used and self._output_nodes is not None:
            if projection_2d_transformed is not None:
                points[PedestrianRenderers.projection_points] = self._from_projection(self._output_nodes, projection_2d_transformed, meta)
            elif projection_2d is not None:
                points[PedestrianRenderers.projection_points] = self._from_projection(self._output_nodes, projection_2d, meta,
                                                                                      autonormalize=True)
        return [self._renderers[r].render(points[r]) if r in points else None for r in used]

    def _render(self, frames, targets, meta, projection_2d, projection_2d_transformed, batch_idx):
        """[(uint8 host clip (T, rows H, cols W, 3), its meta)] for the sliced batch: one launch, one copy."""
        from pedestrians_video_2_carla_amd import ops
        panels = self._panels(frames, targets, meta, projection_2d, projection_2d_transformed)
        if all(p is None for p in panels):
            return []
        width, height = self._image_size
        merged = ops.render_points(panels, size=(height, width), layout=(self._video_rows, self._video_columns),
                                   radius=self._radius, line_width=self._line_width)
        merged = merged.cpu()
        out = []
        for vid_idx in range(merged.shape[0]):
            vid_meta = {
                'video_id': 'video_{:0>2d}_{:0>2d}'.format(batch_idx, vid_idx),
                'pedestrian_id': '{}_{}'.format(meta['age'][vid_idx] if 'age' in meta else 'adult',
                                                meta['gender'][vid_idx] if 'gender' in meta else 'female'),
                'clip_id': 0,
            }
            vid_meta.update({k: v[vid_idx] for k, v in meta.items() if k != 'skeletons'})
            out.append((merged[vid_idx], vid_meta))
        return out
