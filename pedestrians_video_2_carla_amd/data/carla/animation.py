"""Predictions as a CARLA animation file: what a player script feeds to a walker, frame by frame.

One ``.npz`` with ``bones`` (N,T,J,6) and ``root`` (N,T,6) -- rows of (x, y, z, pitch, yaw, roll), metres and degrees, CARLA's
axes, see ``ops.carla_pose_export`` -- ``bone_names`` (J), ``age`` / ``gender`` (N: which walker blueprint a clip belongs to)
and ``fps``. Playing it needs a CARLA server and is not part of this package. Four writers, one file format: predictions
(``save_carla_animation``), keypoint clips through a LinearAE flow (``lift_carla_animation``, K32), mocap clips
(``retarget_carla_animation``, K35) and keypoint clips through a flow that predicts 3-D locations (``ik_carla_animation``, K36).
"""
from typing import Dict

import numpy as np

from pedestrians_video_2_carla_amd.walker_control.carla_pose import BONE_NAMES, export_clips


def save_carla_animation(path: str, outputs, fps: float = 30.0) -> str:
    """``outputs``: the list ``Trainer.predict`` returns, ``(sliced, meta)`` per batch. Every batch is converted with one
    ``carla_pose_export`` call and copied to the host once. Returns the path written (``.npz`` appended when missing)."""
    outputs = list(outputs)
    if not outputs:
        raise ValueError('no predictions to save')
    rows = []
    for sliced, meta in outputs:
        b, r = export_clips(sliced)
        if r is None:
            raise KeyError('world_loc / world_rot are missing from the predictions: no root transform to store')
        rows.append((b, r, meta))
    return _write(path, rows, fps)


def lift_carla_animation(path: str, flow, batches, fps: float = 30.0) -> str:
    """The file ``save_carla_animation(path, trainer.predict(flow, batches), fps)`` writes, from ``Trainer.predict_carla``:
    a LinearAE flow takes one launch per batch (K32) and no pose tensor is materialised; bones and root travel to the host
    together, one copy per batch. ``batches``: ``(frames, targets, meta)`` as for ``predict``."""
    from pedestrians_video_2_carla_amd.trainer import Trainer
    return _write_device_rows(path, Trainer().predict_carla(flow, batches), fps, 'no predictions to save')


def retarget_carla_animation(path: str, batches, fps: float = 30.0, device=None) -> str:
    """Mocap clips as the file ``save_carla_animation`` writes: ``batches`` of ``(frames, targets, meta)`` whose targets hold
    ``amass_body_pose`` (B,T,66) -- the stored AMASS subsets, a mixture's AMASS clips -- and ``world_rot`` (B,T,3,3) where the
    subset has it (the identity otherwise; the root location of a body pose is zero). One ``ops.smpl_to_carla`` call per batch
    (K35 on device tensors: one launch) and one copy to the host: bones and root travel together."""
    from pedestrians_video_2_carla_amd.walker_control.smpl_retargeter import SmplRetargeter
    retargeter = SmplRetargeter(device)

    def clips():
        for _, targets, meta in batches:
            if 'amass_body_pose' not in targets:
                raise KeyError('amass_body_pose is missing from the targets: not a batch of AMASS clips')
            yield (*retargeter.export(targets['amass_body_pose'], meta, targets.get('world_rot')), meta)
    return _write_device_rows(path, clips(), fps, 'no clips to save')


def ik_carla_animation(path: str, flow, batches, fps: float = 30.0) -> str:
    """The file of ``save_carla_animation`` from a flow whose movements model outputs absolute locations (PoseFormer,
    Baseline3DPose, ``--movements_output_type absolute_loc``): ``Trainer.predict_carla(flow, batches, ik=True)`` fits the bone
    rotations to the predicted locations with one launch of K36 per batch; bones and root travel to the host together, one copy
    per batch. ``batches``: ``(frames, targets, meta)`` as for ``predict``."""
    from pedestrians_video_2_carla_amd.trainer import Trainer
    return _write_device_rows(path, Trainer().predict_carla(flow, batches, ik=True), fps, 'no predictions to save')


def _write_device_rows(path: str, batches, fps: float, when_empty: str) -> str:
    """``batches`` of (bones (n,T,J,6), root (n,T,6), meta) on the device: bones and root travel to the host together, one copy
    per batch."""
    import torch
    rows = []
    for bones, root, meta in batches:
        both = torch.cat((bones, root.unsqueeze(-2)), -2).cpu().numpy()
        rows.append((both[..., :-1, :], both[..., -1, :], meta))
    if not rows:
        raise ValueError(when_empty)
    return _write(path, rows, fps)


def _write(path: str, rows, fps: float) -> str:
    """``rows``: per batch (bones (n,T,J,6), root (n,T,6), meta) on the host."""
    bones, roots, ages, genders = [], [], [], []
    for b, r, meta in rows:
        n = len(b)
        bones.append(b)
        roots.append(r)
        ages.extend(str(a) for a in meta.get('age', ['adult'] * n))
        genders.extend(str(g) for g in meta.get('gender', ['female'] * n))
    bones, roots = np.concatenate(bones, 0), np.concatenate(roots, 0)
    if bones.shape[-2] != len(BONE_NAMES):
        raise ValueError(f'save_carla_animation: {bones.shape[-2]} bones, {len(BONE_NAMES)} expected')
    if not str(path).endswith('.npz'):
        path = str(path) + '.npz'
    np.savez(path, bones=bones.astype(np.float32), root=roots.astype(np.float32), bone_names=np.array(BONE_NAMES),
             age=np.array(ages), gender=np.array(genders), fps=np.float64(fps))
    return str(path)


def load_carla_animation(path: str) -> Dict[str, object]:
    """The file back: arrays ``bones`` / ``root``, lists ``bone_names`` / ``age`` / ``gender``, float ``fps``."""
    with np.load(path, allow_pickle=False) as f:
        return {'bones': f['bones'], 'root': f['root'], 'bone_names': [str(s) for s in f['bone_names']],
                'age': [str(s) for s in f['age']], 'gender': [str(s) for s in f['gender']], 'fps': float(f['fps'])}
