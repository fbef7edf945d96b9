"""Poses as CARLA consumes them: ``{bone name: Transform}`` in ``CARLA_SKELETON`` order, plus a root ``Transform`` per frame.

``CarlaPose.tensors_to_pose`` / ``pose_to_tensors`` / ``empty`` carry the names of the reference's ``P3dPose``
(walker_control/p3d_pose.py:34-96) so its users find them; the arithmetic is ``ops.carla_pose_export`` /
``ops.carla_pose_import`` (K30 on the device, the tensor definitions on the host), and ``clips_to_transforms`` converts a whole
``(B, T, ...)`` prediction with one call of it and one device-to-host copy instead of one of each per frame.
"""
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from pedestrians_video_2_carla_amd import ops
from pedestrians_video_2_carla_amd.carla_utils import mock_carla as carla
from pedestrians_video_2_carla_amd.data.carla import reference as ref
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON

BONE_NAMES = tuple(m.name for m in CARLA_SKELETON)


def transform_from_row(row) -> 'carla.Transform':
    """One exported row (x, y, z, pitch, yaw, roll) -> ``Transform``."""
    x, y, z, pitch, yaw, roll = (float(v) for v in row)
    return carla.Transform(location=carla.Location(x=x, y=y, z=z), rotation=carla.Rotation(pitch=pitch, yaw=yaw, roll=roll))


def export_clips(outputs, resample=None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """``outputs``: what ``flow.predict_step`` returns -- ``(sliced, meta)`` or ``sliced`` alone -- with ``relative_pose_loc``
    (B,T,J,3) and ``relative_pose_rot`` (B,T,J,3,3), and ``world_loc`` (B,T,3) / ``world_rot`` (B,T,3,3) when the flow has them.
    Returns host arrays ``bones`` (B,T,J,6) and ``root`` (B,T,6) or None: one ``carla_pose_export`` call, one copy.
    ``resample``: ``(bones, root) -> (bones, root)`` applied where the rows are, before the copy (``CarlaResampler.resample``)."""
    sliced = outputs[0] if isinstance(outputs, (tuple, list)) else outputs
    loc, rot = sliced.get('relative_pose_loc'), sliced.get('relative_pose_rot')
    if loc is None or rot is None:
        raise KeyError('relative_pose_loc / relative_pose_rot are missing: the flow did not materialise its poses '
                       '(a lean train step, or a movements model that outputs absolute locations)')
    wl, wr = sliced.get('world_loc'), sliced.get('world_rot')
    if wl is None or wr is None:
        wl = wr = None
    bones, root = ops.carla_pose_export(loc, rot, wl, wr)
    if resample is not None:
        bones, root = resample(bones, root)
    if root is None:
        return bones.cpu().numpy(), None
    rows = torch.cat((bones, root.unsqueeze(-2)), -2).cpu().numpy()          # bones and root travel together
    return rows[..., :-1, :], rows[..., -1, :]


def skel_type_of(meta_or_skel_type, B: int, device, strict: bool) -> Tensor:
    """The batch's ``meta`` ('age' / 'gender' lists or 'skel_type') or a (B) skeleton-type tensor -> int32 (B) on ``device``.
    Not ``strict``: (age, gender) go through the de-normaliser's substitutions -- ``neutral`` and missing values are the adult
    female skeleton, as the reference warns (smpl_dataset.py:31-33)."""
    if isinstance(meta_or_skel_type, Tensor):
        return meta_or_skel_type.to(device=device, dtype=torch.int32)
    return ref.skeleton_types_from_meta(meta_or_skel_type, batch_size=B, strict=strict, device=device)


class Retargeter:
    """Per-frame poses of another kind -> CARLA poses through one ``ops`` converter, named by the subclass (``_op``), whose
    ``retarget`` / ``export`` (under ``no_grad``) turn their arguments into ``(x, skel_type, world_loc, world_rot, lead)``."""
    _op: str

    def __init__(self, device=None):
        self.device = torch.device(device) if device is not None else None

    def _retarget(self, x, skel_type, world_loc, world_rot, lead) -> Dict[str, Tensor]:
        out = getattr(ops, self._op)(x, skel_type)
        ref_loc, _ = ref.get_relative_tensors(x.device, dtype=x.dtype)
        return {'relative_pose_loc': ref_loc[ref.frame_types(skel_type, lead)], **out, 'world_loc': world_loc, 'world_rot': world_rot}

    def _export(self, x, skel_type, world_loc, world_rot, lead) -> Tuple[Tensor, Tensor]:
        out = getattr(ops, self._op)(x, skel_type, world_loc, world_rot, want=('bones', 'root'))
        return out['bones'], out['root']


class CarlaPose:
    def __init__(self, device=None):
        self._device = device

    @property
    def empty(self) -> 'OrderedDict[str, carla.Transform]':
        """Every bone at the identity transform, keys in ``CARLA_SKELETON`` order."""
        return OrderedDict((name, carla.Transform()) for name in BONE_NAMES)

    def tensors_to_pose(self, locations: Tensor, rotations: Tensor) -> 'OrderedDict[str, carla.Transform]':
        """``locations`` (J,3) and ``rotations`` (J,3,3) of one frame, relative or absolute, in the order of ``empty`` ->
        ``{bone name: Transform}`` (the result is relative or absolute as the tensors are)."""
        if locations.ndim != 2 or len(locations) != len(BONE_NAMES):
            raise ValueError(f'tensors_to_pose: ({len(BONE_NAMES)},3) locations of one frame expected, got {tuple(locations.shape)}')
        bones, _ = ops.carla_pose_export(locations, rotations)
        return OrderedDict(zip(BONE_NAMES, (transform_from_row(r) for r in bones.cpu().numpy())))

    def pose_to_tensors(self, pose) -> Tuple[Tensor, Tensor]:
        """``{bone name: Transform}`` (read in its own order, as the reference does) -> fp32 ``(locations (J,3),
        rotations (J,3,3))`` on this pose's device."""
        rows = [(p.location.x, p.location.y, p.location.z, p.rotation.pitch, p.rotation.yaw, p.rotation.roll)
                for p in pose.values()]
        return ops.carla_pose_import(torch.tensor(rows, dtype=torch.float32, device=self._device))

    def clips_to_transforms(self, outputs) -> Tuple[List[List['OrderedDict']], Optional[List[List['carla.Transform']]]]:
        """A whole prediction (see ``export_clips``) -> ``poses[b][t]`` = ``{bone name: Transform}`` and ``roots[b][t]`` = the
        frame's root ``Transform`` (None when the flow has no world tensors)."""
        bones, root = export_clips(outputs)
        if bones.shape[-2] != len(BONE_NAMES):
            raise ValueError(f'clips_to_transforms: {bones.shape[-2]} bones, {len(BONE_NAMES)} expected')
        poses = [[OrderedDict(zip(BONE_NAMES, (transform_from_row(r) for r in frame))) for frame in clip] for clip in bones]
        roots = [[transform_from_row(r) for r in clip] for clip in root] if root is not None else None
        return poses, roots
