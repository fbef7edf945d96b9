"""Predictions as a CARLA animation file: what a player script feeds to a walker, frame by frame.

One ``.npz`` with ``bones`` (N,T,J,6) and ``root`` (N,T,6) -- rows of (x, y, z, pitch, yaw, roll), metres and degrees, CARLA's
axes, see ``ops.carla_pose_export`` -- ``bone_names`` (J), ``age`` / ``gender`` (N: which walker blueprint a clip belongs to)
and ``fps``. Playing it needs a CARLA server and is not part of this package. ``resample_carla_animation`` rewrites a file at
another rate (K37), ``smooth_carla_animation`` smoothed along time (K39), ``root_motion_carla_animation`` with the root motion of
its planted feet (K40), ``loop_carla_animation`` as a loop of any length (K41). Four writers, one file format: predictions
(``save_carla_animation``), keypoint clips through a LinearAE flow (``lift_carla_animation``, K32), mocap clips
(``retarget_carla_animation``, K35) and keypoint clips through a flow that predicts 3-D locations (``ik_carla_animation``, K36).
"""
from typing import Dict

import numpy as np

from pedestrians_video_2_carla_amd.walker_control.carla_pose import BONE_NAMES, export_clips


def save_carla_animation(path: str, outputs, fps: float = 30.0, out_fps=None, smooth=None, root_motion=None, loop=None) -> str:
    """``outputs``: the list ``Trainer.predict`` returns, ``(sliced, meta)`` per batch. Every batch is converted with one
    ``carla_pose_export`` call and copied to the host once. Returns the path written (``.npz`` appended when missing).
    ``out_fps`` (here and in the other writers): every clip is resampled from ``fps`` to that rate where its rows are, before the
    copy (``ops.resample_carla_rows``, K37 on the device), and the file's ``fps`` is ``out_fps``. ``smooth`` (here and in the other
    writers): a ``CarlaSmoother`` or a dict of its arguments (``mode`` among them; ``one_euro`` takes ``fps`` from here when it has
    none); every clip is smoothed as a video of its own where its rows are (K39 on the device), at the source rate and before
    the resampling. None: the file is what it is without the argument. ``root_motion`` (here and in the other writers): True, a
    ``CarlaRootMotion`` or a dict of its arguments (``ground``); every clip, a video of its own, gets root rows that keep its
    supporting foot planted (K40 on the device), after the smoothing and before the resampling. None: the bytes of before.
    ``loop`` (here and in the other writers): a ``CarlaLooper`` that knows its ``frames`` or a dict of its arguments (``blend``,
    ``min_period``, ``frames``, ...); every clip, a video of its own, becomes ``frames`` frames of the cycle that closes best (K41
    on the device; NaN rows where a clip has none), after the root motion and before the resampling. None: the bytes of before."""
    outputs = list(outputs)
    if not outputs:
        raise ValueError('no predictions to save')
    resample = _stages(fps, out_fps, smooth, root_motion, loop)
    rows = []
    for sliced, meta in outputs:
        b, r = export_clips(sliced, resample)
        if r is None:
            raise KeyError('world_loc / world_rot are missing from the predictions: no root transform to store')
        rows.append((b, r, meta))
    return _write(path, rows, fps if out_fps is None else out_fps)


def _resampler(fps, out_fps):
    """None without ``out_fps``, else ``(bones, root) -> (bones, root)`` at ``out_fps``: stateless, every clip its own video."""
    if out_fps is None:
        return None
    from pedestrians_video_2_carla_amd.walker_control.resample import CarlaResampler
    return CarlaResampler(fps, out_fps).resample


def _stages(fps, out_fps, smooth, root_motion=None, loop=None):
    """What happens to a batch's rows where they are: smoothing at the source rate, then the root motion of the planted feet,
    then the loop, then resampling; None when none of them is asked."""
    from pedestrians_video_2_carla_amd.walker_control.smooth import as_smoother
    smoother, resample = as_smoother(smooth, fps), _resampler(fps, out_fps)
    stages = [smoother.smooth] if smoother is not None else []
    if root_motion is not None:
        from pedestrians_video_2_carla_amd.walker_control.root_motion import as_root_motion
        mover = as_root_motion(root_motion)
        if mover is not None:
            stages.append(mover.apply)
    if loop is not None:
        from pedestrians_video_2_carla_amd.walker_control.loop import as_looper
        stages.append(as_looper(loop).loop)
    if resample is not None:
        stages.append(resample)
    if not stages:
        return None
    if len(stages) == 1:
        return stages[0]

    def run(bones, root):
        for stage in stages:
            bones, root = stage(bones, root)
        return bones, root
    return run


def lift_carla_animation(path: str, flow, batches, fps: float = 30.0, out_fps=None, smooth=None, root_motion=None,
                         loop=None) -> str:
    """The file ``save_carla_animation(path, trainer.predict(flow, batches), fps)`` writes, from ``Trainer.predict_carla``:
    a LinearAE flow takes one launch per batch (K32) and no pose tensor is materialised; bones and root travel to the host
    together, one copy per batch. ``batches``: ``(frames, targets, meta)`` as for ``predict``."""
    from pedestrians_video_2_carla_amd.trainer import Trainer
    return _write_device_rows(path, Trainer().predict_carla(flow, batches), fps, 'no predictions to save', out_fps, smooth, root_motion,
                              loop)


def retarget_carla_animation(path: str, batches, fps: float = 30.0, device=None, out_fps=None, smooth=None, root_motion=None,
                             loop=None) -> str:
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
    return _write_device_rows(path, clips(), fps, 'no clips to save', out_fps, smooth, root_motion, loop)


def ik_carla_animation(path: str, flow, batches, fps: float = 30.0, out_fps=None, smooth=None, root_motion=None,
                       loop=None) -> str:
    """The file of ``save_carla_animation`` from a flow whose movements model outputs absolute locations (PoseFormer,
    Baseline3DPose, ``--movements_output_type absolute_loc``): ``Trainer.predict_carla(flow, batches, ik=True)`` fits the bone
    rotations to the predicted locations with one launch of K36 per batch; bones and root travel to the host together, one copy
    per batch. ``batches``: ``(frames, targets, meta)`` as for ``predict``."""
    from pedestrians_video_2_carla_amd.trainer import Trainer
    return _write_device_rows(path, Trainer().predict_carla(flow, batches, ik=True), fps, 'no predictions to save', out_fps, smooth,
                              root_motion, loop)


def _write_device_rows(path: str, batches, fps: float, when_empty: str, out_fps=None, smooth=None, root_motion=None,
                       loop=None) -> str:
    """``batches`` of (bones (n,T,J,6), root (n,T,6), meta) on the device: bones and root travel to the host together, one copy
    per batch, smoothed (``smooth``), given root motion (``root_motion``) and then resampled to ``out_fps`` before it when those
    are given."""
    import torch
    resample = _stages(fps, out_fps, smooth, root_motion, loop)
    rows = []
    for bones, root, meta in batches:
        if resample is not None:
            bones, root = resample(bones, root)
        both = torch.cat((bones, root.unsqueeze(-2)), -2).cpu().numpy()
        rows.append((both[..., :-1, :], both[..., -1, :], meta))
    if not rows:
        raise ValueError(when_empty)
    return _write(path, rows, fps if out_fps is None else out_fps)


def _write(path: str, rows, fps: float, **more) -> str:
    """``rows``: per batch (bones (n,T,J,6), root (n,T,6), meta) on the host; ``more``: further arrays of the file."""
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
             age=np.array(ages), gender=np.array(genders), fps=np.float64(fps), **more)
    return str(path)


def resample_carla_animation(src_path: str, dst_path: str, fps: float, mode: str = 'slerp', device=None, chunk=None) -> str:
    """The file at ``src_path`` at ``fps`` frames per second: every clip resampled from the stored rate (``CarlaResampler``; on
    ``device``, K37 there for a GPU), everything else as stored. ``chunk``: the clips stream through ``push`` in pieces of that
    many frames, as a video that arrives clip by clip would. Returns the path written."""
    import torch
    from pedestrians_video_2_carla_amd.walker_control.resample import CarlaResampler
    src = load_carla_animation(src_path)
    resampler = CarlaResampler(src['fps'], fps, mode)
    bones, root = (torch.from_numpy(src[k]).to(device) if device is not None else torch.from_numpy(src[k]) for k in ('bones', 'root'))
    if chunk is None:
        out_b, out_r = resampler.resample(bones, root)
    else:
        if int(chunk) < 1:
            raise ValueError(f'resample_carla_animation: chunk = {chunk}; at least one frame expected')
        pieces = [resampler.push(bones[:, t:t + int(chunk)], root[:, t:t + int(chunk)]) for t in range(0, bones.shape[1], int(chunk))]
        out_b, out_r = torch.cat([p[0] for p in pieces], 1), torch.cat([p[1] for p in pieces], 1)
    both = torch.cat((out_b, out_r.unsqueeze(-2)), -2).cpu().numpy()
    return _write(dst_path, [(both[..., :-1, :], both[..., -1, :], {'age': src['age'], 'gender': src['gender']})], fps)


def smooth_carla_animation(src_path: str, dst_path: str, mode: str = 'gaussian', chunk=None, device=None, **params) -> str:
    """The file at ``src_path`` smoothed along time: every clip through ``CarlaSmoother(mode, **params)`` (on ``device``, K39
    there for a GPU; ``one_euro`` takes the stored ``fps`` when none is given), everything else as stored. ``chunk``: the clips
    stream through ``push`` in pieces of that many frames and ``flush``, as a video that arrives piece by piece would; the
    file is the same. Returns the path written."""
    import torch
    from pedestrians_video_2_carla_amd.walker_control.smooth import as_smoother
    src = load_carla_animation(src_path)
    smoother = as_smoother(dict(mode=mode, **params), src['fps'])
    bones, root = (torch.from_numpy(src[k]).to(device) if device is not None else torch.from_numpy(src[k]) for k in ('bones', 'root'))
    if chunk is None:
        out_b, out_r = smoother.smooth(bones, root)
    else:
        if int(chunk) < 1:
            raise ValueError(f'smooth_carla_animation: chunk = {chunk}; at least one frame expected')
        pieces = [smoother.push(bones[:, t:t + int(chunk)], root[:, t:t + int(chunk)]) for t in range(0, bones.shape[1], int(chunk))]
        pieces.append(smoother.flush())
        out_b, out_r = torch.cat([p[0] for p in pieces], 1), torch.cat([p[1] for p in pieces], 1)
    both = torch.cat((out_b, out_r.unsqueeze(-2)), -2).cpu().numpy()
    return _write(dst_path, [(both[..., :-1, :], both[..., -1, :], {'age': src['age'], 'gender': src['gender']})], src['fps'])


def root_motion_carla_animation(src_path: str, dst_path: str, ground=None, chunk=None, device=None) -> str:
    """The file at ``src_path`` with root rows that keep every clip's supporting foot planted (``CarlaRootMotion(ground)``; on
    ``device``, K40 there for a GPU), everything else as stored; a stored root that already moves is honoured. ``chunk``: the
    clips stream through ``push`` in pieces of that many frames, as a video that arrives piece by piece would; the file is
    the same. Returns the path written."""
    import torch
    from pedestrians_video_2_carla_amd.walker_control.root_motion import CarlaRootMotion
    src = load_carla_animation(src_path)
    mover = CarlaRootMotion(ground)
    bones, root = (torch.from_numpy(src[k]).to(device) if device is not None else torch.from_numpy(src[k]) for k in ('bones', 'root'))
    if chunk is None:
        out_r = mover.apply(bones, root)[1]
    else:
        if int(chunk) < 1:
            raise ValueError(f'root_motion_carla_animation: chunk = {chunk}; at least one frame expected')
        out_r = torch.cat([mover.push(bones[:, t:t + int(chunk)], root[:, t:t + int(chunk)])[1]
                           for t in range(0, bones.shape[1], int(chunk))], 1)
    both = torch.cat((bones, out_r.unsqueeze(-2)), -2).cpu().numpy()
    return _write(dst_path, [(both[..., :-1, :], both[..., -1, :], {'age': src['age'], 'gender': src['gender']})], src['fps'])


def loop_carla_animation(src_path: str, dst_path: str, frames: int, blend: int, min_period: int, max_period=None,
                         device=None) -> str:
    """The file at ``src_path`` as ``frames`` frames of a loop: every stored clip, a video of its own, is searched for the cycle
    that closes best and that cycle is played (``CarlaLooper(blend, min_period, max_period)``; on ``device``, K41 there for a
    GPU), everything else as stored. The file also holds ``loop_start`` / ``loop_end`` (N) int64 and ``loop_cost`` (N): the
    cycle of each clip in the source's frames; a clip without one has -1, -1 and NaN, and NaN rows. Returns the path written."""
    import torch
    from pedestrians_video_2_carla_amd.walker_control.loop import CarlaLooper
    src = load_carla_animation(src_path)
    looper = CarlaLooper(blend, min_period, max_period, frames=frames)
    bones, root = (torch.from_numpy(src[k]).to(device) if device is not None else torch.from_numpy(src[k]) for k in ('bones', 'root'))
    found = looper.find(bones)
    out_b, out_r = looper.play(bones, root, looper.frames, found['loop'])
    both = torch.cat((out_b, out_r.unsqueeze(-2)), -2).cpu().numpy()
    pairs = found['loop'].cpu().numpy()
    return _write(dst_path, [(both[..., :-1, :], both[..., -1, :], {'age': src['age'], 'gender': src['gender']})], src['fps'],
                  loop_start=pairs[:, 0].astype(np.int64), loop_end=pairs[:, 1].astype(np.int64),
                  loop_cost=found['loop_cost'].cpu().numpy().astype(np.float32))


def load_carla_animation(path: str) -> Dict[str, object]:
    """The file back: arrays ``bones`` / ``root``, lists ``bone_names`` / ``age`` / ``gender``, float ``fps``, and the arrays
    ``loop_start`` / ``loop_end`` / ``loop_cost`` of a file ``loop_carla_animation`` wrote."""
    with np.load(path, allow_pickle=False) as f:
        out = {'bones': f['bones'], 'root': f['root'], 'bone_names': [str(s) for s in f['bone_names']],
               'age': [str(s) for s in f['age']], 'gender': [str(s) for s in f['gender']], 'fps': float(f['fps'])}
        out.update({k: f[k] for k in ('loop_start', 'loop_end', 'loop_cost') if k in f.files})
        return out
