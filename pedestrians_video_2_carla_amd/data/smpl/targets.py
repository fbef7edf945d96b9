"""``SmplCarlaTargets``: CARLA-space 3-D ground truth for AMASS clips, added to the batches of any source.

The stored AMASS subsets carry each clip's SMPL body pose under ``targets/amass_body_pose``; the reference's (commented-out) call
site of ``convert_smpl_to_carla`` (data/smpl/smpl_dataset.py:59-75) names what it becomes: ``carla_relative_pose_rot``,
``carla_absolute_pose_rot`` and ``carla_absolute_pose_loc`` ("starting points"). Here that is one ``ops.smpl_to_carla`` call per
batch (K35 on device batches). In a mixed batch the clips of other sources have NaN body poses, so their new targets are NaN, as
every target a source lacks is.
"""
from typing import Iterator

import torch

from pedestrians_video_2_carla_amd.data.carla import reference as ref

BODY_POSE_KEY = 'amass_body_pose'
TARGET_KEYS = {'relative_pose_rot': 'carla_relative_pose_rot', 'absolute_pose_rot': 'carla_absolute_pose_rot',
               'absolute_pose_loc': 'carla_absolute_pose_loc'}


def add_smpl_carla_targets(batch):
    """``(frames, targets, meta)`` -> the same batch object when ``targets`` hold no body pose, else a batch whose targets also
    hold the three CARLA pose tensors (B,T,26,3,3) / (B,T,26,3,3) / (B,T,26,3)."""
    from pedestrians_video_2_carla_amd import ops
    frames, targets, meta = batch
    pose = targets.get(BODY_POSE_KEY) if hasattr(targets, 'get') else None
    if pose is None:
        return batch
    if not pose.is_floating_point():
        pose = pose.float()
    skel_type = ref.skeleton_types_from_meta(meta, batch_size=pose.shape[0], strict=False, device=pose.device)
    out = ops.smpl_to_carla(pose, skel_type, want=tuple(TARGET_KEYS))
    return frames, {**targets, **{TARGET_KEYS[k]: v for k, v in out.items()}}, meta


class SmplCarlaTargets:
    """A re-iterable over ``batches`` (a ``DeviceLoader``, a list, any iterable of ``(frames, targets, meta)``) that yields
    ``add_smpl_carla_targets(batch)``. ``len`` (when the source has one) and ``epoch``, which the epoch loop reads and sets, are
    the source's own."""

    def __new__(cls, batches):
        if cls is SmplCarlaTargets and hasattr(batches, '__len__'):
            cls = _SizedSmplCarlaTargets
        return super().__new__(cls)

    def __init__(self, batches):
        self.batches = batches

    def __iter__(self) -> Iterator:
        for batch in self.batches:
            yield add_smpl_carla_targets(batch)

    @property
    def epoch(self):
        return self.batches.epoch            # AttributeError when the source has none: hasattr() answers for the source

    @epoch.setter
    def epoch(self, value):
        self.batches.epoch = value


class _SizedSmplCarlaTargets(SmplCarlaTargets):
    def __len__(self) -> int:
        return len(self.batches)


def wrap_smpl_carla_targets(batches, enabled: bool):
    """The launcher's ``--smpl_carla_targets``: off, or no batches of its own (the synthetic training stream) -> unchanged."""
    return SmplCarlaTargets(batches) if enabled and batches is not None else batches
