"""``LitPoseEstimationFlow``: frames -> model -> heatmaps -> 2-D keypoints (reference modules/flow/pose_estimation.py:17-134).

The step restates the reference's ``_get_sliced_data``: ``heatmaps`` (the model output, what ``LossModes.heatmaps`` reads),
``projection_2d_confidence`` / ``projection_2d`` decoded from them in pixel space, ``projection_2d_transformed`` when the data
module has a transform, ``inputs`` and ``targets`` with ``targets['heatmaps']`` at the output's resolution. The three pieces the
reference runs as Python loops are one launch each here (K28, csrc/p2c_heatmaps.hip):

  targets   ``targets['heatmaps']`` already at the output's resolution is used as supplied; a full-resolution one is pooled
            ``avg_pool2d(9, 8, 1)`` as in the reference; when the key is absent the pooled maps are written straight from
            ``targets['projection_2d']`` (pixels of the original frame), ``targets['heatmaps_shift']`` (B,T,2; zeros if absent)
            and ``meta['original_size']`` = (height, width) of the original frame (the frames' own size if absent) by K28a
            (``ops.heatmap_targets``) -- the full-resolution maps the reference's datasets build on the host never exist.
  decode    ``ops.heatmap_keypoints`` (K28c) instead of a triple loop with a host sync per map. It serves logging and metrics
            only, so training steps under ``lean_train_outputs`` (default) skip it.
  loss      ``HeatmapsLoss`` -> ``ops.heatmaps_loss`` (K28b).

Models: ``Linear`` only. ``UniPoseLSTM``, ``P0`` and ``AvPedestrianPoseTransformer`` need third-party sources and downloaded
ResNet weights; they are neither built nor registered, so the default model is ``Linear`` where the reference has
``UniPoseLSTM``. A model whose output type is not ``heatmaps`` takes the autoencoder flow's step.
"""
from typing import Dict

import torch

from pedestrians_video_2_carla_amd.modules.flow.autoencoder import LitAutoencoderFlow
from pedestrians_video_2_carla_amd.modules.flow.output_types import PoseEstimationModelOutputType
from pedestrians_video_2_carla_amd.modules.pose_estimation.linear import Linear


class LitPoseEstimationFlow(LitAutoencoderFlow):
    def __init__(self, *args, heatmaps_sigma: int = 1, lean_train_outputs: bool = True, **kwargs):
        super().__init__(*args, **kwargs)
        self.heatmaps_sigma = heatmaps_sigma
        self.lean_train_outputs = lean_train_outputs
        self._datamodule = None
        self._meta = None

    @classmethod
    def get_available_models(cls) -> Dict[str, Dict[str, torch.nn.Module]]:
        return {'movements': {m.__name__: m for m in [Linear]}}

    @classmethod
    def get_default_models(cls) -> Dict[str, torch.nn.Module]:
        return {'movements': Linear}

    @staticmethod
    def add_model_specific_args(parent_parser):
        parent_parser = LitAutoencoderFlow.add_model_specific_args(parent_parser)
        from pedestrians_video_2_carla_amd.data.base.heatmaps import HeatmapTargets
        return HeatmapTargets.add_cli_args(parent_parser)

    def get_initial_metrics(self):
        return {}

    def _calculate_initial_metrics(self):
        return {}

    def attach_datamodule(self, datamodule):
        self._datamodule = datamodule

    def _transform_callable(self):
        dm = self._datamodule
        if dm is None and getattr(self, 'trainer', None) is not None:
            dm = getattr(self.trainer, 'datamodule', None)
        return getattr(dm, 'transform_callable', None)

    def _unwrap_batch(self, batch):
        unwrapped = super()._unwrap_batch(batch)
        self._meta = unwrapped[2]                # the original frame size the targets' keypoints are in
        return unwrapped

    def _target_heatmaps(self, targets, frames, heatmaps):
        """``targets['heatmaps']`` at the resolution of the model's output (no gradient flows into it)."""
        from pedestrians_video_2_carla_amd import ops
        with torch.no_grad():
            given = targets.get('heatmaps')
            if given is not None:
                if given.shape[-2:] == heatmaps.shape[-2:]:
                    return given
                k, s, p = ops.HEATMAPS_POOL           # the reference's resize (pose_estimation.py:96-107)
                pooled = torch.nn.functional.avg_pool2d(given.flatten(0, 1), kernel_size=k, stride=s, padding=p)
                return pooled.unflatten(0, given.shape[:2])
            kp = targets['projection_2d']
            shift = targets.get('heatmaps_shift')
            if shift is None:
                shift = kp.new_zeros((*kp.shape[:2], 2))
            H, W = frames.shape[-2:]
            oh, ow = (self._meta or {}).get('original_size', (H, W)) if isinstance(self._meta, dict) else (H, W)
            return ops.heatmap_targets(kp, shift, (W / float(ow), H / float(oh)), (H, W), self.heatmaps_sigma, ops.HEATMAPS_POOL)

    def _inner_step(self, frames, targets, edge_index=None, batch_vector=None, stage='train'):
        model = self.movements_model
        if model.output_type != PoseEstimationModelOutputType.heatmaps:
            return super()._inner_step(frames, targets, edge_index, batch_vector, stage=stage)
        from pedestrians_video_2_carla_amd import ops
        heatmaps = model(frames, targets=targets if self.training and model.needs_targets else None,
                         edge_index=None, batch_vector=None)
        eval_slice = (slice(None), model.eval_slice)
        sliced = {'heatmaps': heatmaps[eval_slice]}
        if not (self.lean_train_outputs and stage == 'train'):
            # the model's output is in pixel space; the reference hands frames.shape[-2:] over as (bbox_width, bbox_height)
            keypoints = ops.heatmap_keypoints(heatmaps.detach(), tuple(frames.shape[-2:]))
            sliced['projection_2d_confidence'] = keypoints[eval_slice]
            sliced['projection_2d'] = keypoints[..., :2][eval_slice]
            transform = self._transform_callable()
            if transform is not None:
                sliced['projection_2d_transformed'] = transform(keypoints[..., :2])[eval_slice]
        sliced['inputs'] = frames[eval_slice]
        sliced['targets'] = {k: v[eval_slice[:v.ndim]] for k, v in targets.items()}
        sliced['targets']['heatmaps'] = self._target_heatmaps(sliced['targets'], sliced['inputs'], sliced['heatmaps'])
        return sliced
