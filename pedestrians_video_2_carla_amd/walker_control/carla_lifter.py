"""2-D keypoint clips -> the rows a CARLA walker consumes, behind a trained movements model.

``CarlaLifter(flow_or_model).lift(frames, meta)`` is ``export_clips(flow.predict_step(batch))`` without the tensors in between:
for a ``LinearAE`` with the 6-D rotation output on 26 input joints it is ONE launch (K32, ``ops.lift_to_carla``) on fp32 device
tensors -- no (B,T,26,6) model output, no forward kinematics, no projection, no (B,T,26,3,3) rotations in HBM. ``push`` /
``reset`` stream a video clip by clip: the last relative rotation of a clip is where the next one starts, so the rows do not
depend on where the video was cut (the reference restarts every clip from the reference pose, projection.py:170-195).
Any other movements model with a rotation output runs the composed path (model -> pose head -> export), with one warning.
"""
import warnings
from typing import Optional, Tuple

import torch
from torch import Tensor

from pedestrians_video_2_carla_amd import ops
from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType
from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
from pedestrians_video_2_carla_amd.walker_control.carla_pose import skel_type_of

_KINDS = {MovementsModelOutputType.pose_changes: 'pose_changes', MovementsModelOutputType.relative_rot: 'relative_rot'}


class CarlaLifter:
    def __init__(self, flow_or_model, device=None):
        self.flow = flow_or_model if hasattr(flow_or_model, 'movements_model') else None
        self.model = self.flow.movements_model if self.flow is not None else flow_or_model
        self.device = torch.device(device) if device is not None else None
        self._image: Optional[Tensor] = None
        self._image_key = None
        self._carry: Optional[Tensor] = None
        self._warned = False
        self.packs = 0          # how often this lifter packed the weight image
        self._hook = self.model.register_load_state_dict_post_hook(lambda module, keys: self._invalidate())

    # ---- what runs ---------------------------------------------------------------------------------------------------
    @property
    def kind(self) -> Optional[str]:
        """'pose_changes' / 'relative_rot', or None for a model whose output holds no relative rotations."""
        return _KINDS.get(getattr(self.model, 'output_type', None))

    def _linear_ae(self):
        """(weights, biases, dims) of a LinearAE the one-launch path can take, else None."""
        model = self.model
        if type(model) is not LinearAE or self.kind is None or not model.fused_mlp or model.mlp_precision != 'fp32':
            return None
        layers = model._linears()
        dims = [layers[0].in_features] + [m.out_features for m in layers]
        if not ops.lift_supported(dims):
            return None
        return [m.weight for m in layers], [m.bias for m in layers], dims

    @property
    def supported(self) -> bool:
        return self._linear_ae() is not None

    def _invalidate(self):
        self._image_key = None

    def _packed_image(self, weights, biases, dims, device) -> Tensor:
        """The packed weight image for ``device``, current: the model's own when an optimizer keeps it so, else this lifter's,
        packed once and again when a parameter's ``_version`` moved or a state dict was loaded. (An edit through ``.data``
        moves no version: call ``reset_image()`` after one.)"""
        model = self.model
        if model._image_managed and model._image is not None and model._image.device == device:
            return model._image
        key = (device, tuple(p._version for p in weights + biases), tuple(p.data_ptr() for p in weights + biases))
        if self._image is None or self._image.device != device:
            self._image = torch.empty(ops.mlp_image_layout(dims)[0], dtype=torch.float32, device=device)
            self._image_key = None
        if key != self._image_key:
            ops.mlp_pack(weights, biases, self._image)
            self._image_key = key
            self.packs += 1
        return self._image

    def reset_image(self):
        self._invalidate()

    def close(self):
        """Take the load_state_dict hook off the model (a lifter made for one loop)."""
        self._hook.remove()

    # ---- public ------------------------------------------------------------------------------------------------------
    def lift(self, frames: Tensor, meta_or_skel_type, world_loc: Optional[Tensor] = None,
             world_rot: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """``frames`` (B,T,26,2), the batch's ``meta`` (its 'age' / 'gender' lists or 'skel_type') or a (B) skeleton-type
        tensor -> ``bones`` (B,T',26,6), ``root`` (B,T',6) over the frames of the model's ``eval_slice``. Stateless: every clip
        starts from the reference pose. ``world_loc`` (B,T,3) / ``world_rot`` (B,T,3,3): the world transform of each frame;
        without them the root rows are the identity world's (a flow with ``ZeroTrajectory``)."""
        bones, root, _ = self._run(frames, meta_or_skel_type, world_loc, world_rot, None)
        return bones, root

    def push(self, frames: Tensor, meta_or_skel_type, world_loc: Optional[Tensor] = None,
             world_rot: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """The next clip of a video: as ``lift``, but the pose continues where the previous ``push`` left it (pose_changes
        models; a relative_rot model has nothing to carry). The same clips, B and order of clips in every call."""
        bones, root, final = self._run(frames, meta_or_skel_type, world_loc, world_rot, self._carry)
        self._carry = final
        return bones, root

    def reset(self):
        """The next ``push`` starts from the reference pose again."""
        self._carry = None

    # ---- the work ----------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _run(self, frames, meta_or_skel_type, world_loc, world_rot, initial):
        if self.device is not None:
            frames = frames.to(self.device)
            world_loc = world_loc.to(self.device) if world_loc is not None else None
            world_rot = world_rot.to(self.device) if world_rot is not None else None
        if self.flow is not None and world_loc is None and not bool(getattr(self.flow.trajectory_model, 'is_identity', False)):
            raise RuntimeError('CarlaLifter: the flow has a trajectory model; pass the world_loc / world_rot of each frame')
        B = frames.shape[0]
        if initial is not None and initial.shape[0] != B:
            raise RuntimeError(f'CarlaLifter.push: {B} clips after {initial.shape[0]}; reset() starts another video')
        skel_type = skel_type_of(meta_or_skel_type, B, frames.device, strict=True)
        plan = self._linear_ae()
        if plan is not None:
            weights, biases, dims = plan
            image = None
            if frames.is_cuda and frames.dtype == torch.float32 and all(p.device == frames.device for p in weights):
                image = self._packed_image(weights, biases, dims, frames.device)
            bones, root, final, _ = ops.lift_to_carla(frames, weights, biases, skel_type, self.kind + '_6d', image=image,
                                                      image_is_current=image is not None, world_loc=world_loc,
                                                      world_rot=world_rot, initial_rel_rot=initial)
        else:
            if not self._warned:
                self._warned = True
                warnings.warn(f'CarlaLifter: {type(self.model).__name__} is not the 52-26-13-6-39-78-156 LinearAE with a rotation '
                              'output that the one-launch path (K32) covers; running model -> pose head -> export')
            was_training = self.model.training
            self.model.eval()
            try:
                y = self.model(frames)
            finally:
                self.model.train(was_training)
            if self.kind is None or isinstance(y, tuple):
                raise KeyError('relative_pose_loc / relative_pose_rot are missing: a movements model that outputs absolute '
                               'locations has no bone rotations to export')
            kind = self.kind + ('_6d' if y.ndim == 4 and y.shape[-1] == 6 else '')
            bones, root, final, _ = ops.pose_to_carla_rows(y, skel_type, kind, world_loc, world_rot, initial)
        sl = getattr(self.model, 'eval_slice', slice(None))
        return bones[:, sl], root[:, sl], final
