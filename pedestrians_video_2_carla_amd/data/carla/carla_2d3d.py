"""``Carla2D3DDataModule``: the reference's infinite synthetic training set, generated on the device (K38).

Reference: data/carla/datamodules/carla_2d3d_datamodule.py + ``Carla2D3DIterableDataset.generate_batch``
(data/carla/datasets/carla_2d3d_dataset.py:145-210). Same constructor keywords, flags, defaults and bounds; same batch
``(frames, targets, meta)`` with the projection layer's outputs, ``pose_changes`` / ``world_loc_changes`` / ``world_rot_changes`` and
the Projection2D targets. What differs:

  * the random numbers are counter based (``generator.py``): training step i of rank r is clips [i B, (i + 1) B) of stream r, so a
    resumed run draws what the uninterrupted one would and nothing goes into a checkpoint;
  * validation and test are ``val_set_size`` / ``test_set_size`` clips of two reserved streams, generated once per device in batches of
    ``batch_size`` (the last one short) and kept -- there is no HDF5 subset to prepare;
  * CARLA skeleton in and out, noise 'zero' / 'uniform', no augmentation: the whole batch is ONE launch (``ops.generate_carla_batch``);
    gaussian noise, ``augment_flip`` / ``augment_rotate`` or another input skeleton: the kernel makes the raw part and
    ``DeviceProjection2DPipeline`` (K11, its own torch-generator draws) the tail.
"""
import argparse
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from pedestrians_video_2_carla_amd import ops
from pedestrians_video_2_carla_amd.data.base.base_datamodule import BaseDataModule
from pedestrians_video_2_carla_amd.data.base.base_transforms import BaseTransforms
from pedestrians_video_2_carla_amd.data.carla import generator
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON

Batch = Tuple[torch.Tensor, Dict[str, torch.Tensor], Dict[str, List]]

_POSE_KEYS = ('pose_changes', 'relative_pose_loc', 'relative_pose_rot', 'absolute_pose_loc', 'absolute_pose_rot', 'world_loc',
              'world_rot', 'world_loc_changes', 'world_rot_changes')
_TRANSFORM_KEYS = ('projection_2d_transformed', 'projection_2d_shift', 'projection_2d_scale')


def _bounded_int(minimum: int, maximum: int):
    """``type=int`` with the reference's ``MinMaxAction`` bounds (utils/argparse.py)."""
    def parse(text: str) -> int:
        value = int(text)
        if not minimum <= value <= maximum:
            raise argparse.ArgumentTypeError(f'{value} is outside [{minimum}, {maximum}]')
        return value
    parse.__name__ = 'int'
    return parse


class Carla2D3DDataModule(BaseDataModule):
    STREAMS = {'val': generator.VAL_STREAM, 'test': generator.TEST_STREAM}

    def __init__(self,
                 val_set_size: Optional[int] = 8192,
                 test_set_size: Optional[int] = 8192,
                 random_changes_each_frame: Optional[int] = 3,
                 max_change_in_deg: Optional[float] = 5,
                 max_world_rot_change_in_deg: Optional[float] = 0,
                 max_initial_world_rot_change_in_deg: Optional[float] = 0,
                 clip_length: Optional[int] = 30,
                 batch_size: Optional[int] = 64,
                 transform: Union[BaseTransforms, str, None] = BaseTransforms.hips_neck_bbox,
                 input_nodes=None,
                 seed: Optional[int] = 22742,
                 noise: Optional[str] = 'zero',
                 noise_param: float = 1.0,
                 augment_flip: Union[bool, float] = False,
                 augment_rotate: Union[bool, float] = False,
                 missing_joint_probabilities: Union[float, Sequence[float]] = (),
                 needs_confidence: bool = False,
                 **kwargs):
        if transform is None:
            transform = BaseTransforms.none
        super().__init__(data_nodes=CARLA_SKELETON, input_nodes=input_nodes, clip_length=clip_length, batch_size=batch_size,
                         transform=transform, **kwargs)
        if self.transform == BaseTransforms.user_defined:
            raise NotImplementedError('the device generator runs the built-in normalisers only')
        if not 0 <= int(random_changes_each_frame) <= len(CARLA_SKELETON):
            raise ValueError(f'random_changes_each_frame must lie in [0, {len(CARLA_SKELETON)}], got {random_changes_each_frame}')
        if noise not in (None, 'zero', 'gaussian', 'uniform'):
            raise ValueError('Unknown noise type: {}'.format(noise))
        self.val_set_size, self.test_set_size = int(val_set_size), int(test_set_size)
        self.random_changes_each_frame = int(random_changes_each_frame)
        self.max_change_in_deg = max_change_in_deg
        self.max_world_rot_change_in_deg = max_world_rot_change_in_deg
        self.max_initial_world_rot_change_in_deg = max_initial_world_rot_change_in_deg
        self.seed = 22742 if seed is None else seed
        self.noise, self.noise_param = noise or 'zero', noise_param
        if isinstance(missing_joint_probabilities, (int, float)):
            missing_joint_probabilities = (missing_joint_probabilities,)
        self.missing_joint_probabilities = ops.generate_miss_prob(missing_joint_probabilities)
        self.augment_flip, self.augment_rotate = augment_flip, augment_rotate
        self.needs_confidence = needs_confidence
        self._pipelines: Dict[bool, object] = {}
        self._eval_cache: Dict[tuple, List[Batch]] = {}

    # ---- the reference's class interface --------------------------------------------------------------------------------------
    @classmethod
    def uses_infinite_train_set(cls) -> bool:
        return True

    @staticmethod
    def add_data_specific_args(parent_parser):
        parser = parent_parser.add_argument_group('Carla2D3D DataModule')
        parser.add_argument('--random_changes_each_frame', type=int, default=3, metavar='NUM_NODES',
                            help='Number of nodes that will be randomly changed in each frame.')
        parser.add_argument('--max_change_in_deg', type=_bounded_int(0, 15), default=5, metavar='DEGREES',
                            help='Max random [+/-] change in degrees.')
        parser.add_argument('--max_world_rot_change_in_deg', type=_bounded_int(0, 15), default=0, metavar='DEGREES',
                            help='Max random [+/-] world rotation yaw change in each frame in degrees.')
        parser.add_argument('--max_initial_world_rot_change_in_deg', type=_bounded_int(0, 180), default=0, metavar='DEGREES',
                            help="Max random [+/-] 'world' rotation yaw change in degrees applied to first frame.")
        parser.add_argument('--val_set_size', type=int, default=8192, metavar='NUM_SAMPLES',
                            help='Number of samples (clips) to use for validation.')
        parser.add_argument('--test_set_size', type=int, default=8192, metavar='NUM_SAMPLES',
                            help='Number of samples (clips) to use for testing.')
        return parent_parser

    @property
    def settings(self) -> Dict:
        return {**self.hparams, 'random_changes_each_frame': self.random_changes_each_frame,
                'max_change_in_deg': self.max_change_in_deg, 'max_world_rot_change_in_deg': self.max_world_rot_change_in_deg,
                'max_initial_world_rot_change_in_deg': self.max_initial_world_rot_change_in_deg,
                'val_set_size': self.val_set_size, 'test_set_size': self.test_set_size}

    # ---- which path a batch takes -----------------------------------------------------------------------------------------------
    @property
    def needs_deform(self) -> bool:
        return self.missing_joint_probabilities is not None and any(self.missing_joint_probabilities) or self.noise != 'zero'

    def fused(self, is_training: bool) -> bool:
        """The whole batch in one launch: CARLA skeleton in and out, noise 'zero' / 'uniform', no augmentation."""
        augmented = is_training and bool(self.augment_flip or self.augment_rotate)
        return self.input_nodes is self.data_nodes and self.noise in ('zero', 'uniform') and not augmented

    def target_keys(self, is_training: bool = True) -> Tuple[str, ...]:
        keys = ('projection_2d',) + _POSE_KEYS
        if self.needs_deform:
            keys += ('projection_2d_deformed',)
        if self.transform != BaseTransforms.none:
            keys += _TRANSFORM_KEYS
        return keys

    def clip_range(self, stage: str, index: int, rank: int = 0) -> Tuple[int, int, int]:
        """(stream, first_clip, clips) of batch ``index`` of ``stage``: training step i of rank r is clips [i B, (i + 1) B) of
        stream r; validation / test batch i is clips [i B, min((i + 1) B, set size)) of the stage's reserved stream."""
        B = self.batch_size
        if stage == 'train':
            return int(rank), index * B, B
        size = self.val_set_size if stage == 'val' else self.test_set_size
        return self.STREAMS[stage], index * B, max(min(B, size - index * B), 0)

    def draws(self, stage: str, index: int, rank: int = 0):
        """The definition's draws of that batch (host tensors)."""
        stream, first, B = self.clip_range(stage, index, rank)
        return generator.draws(self.seed, stream, first, B, self.clip_length, **self._draw_kwargs(fused=True))

    def _draw_kwargs(self, fused: bool) -> Dict:
        return dict(random_changes_each_frame=self.random_changes_each_frame, max_change_in_deg=self.max_change_in_deg,
                    max_world_rot_change_in_deg=self.max_world_rot_change_in_deg,
                    max_initial_world_rot_change_in_deg=self.max_initial_world_rot_change_in_deg,
                    noise=self.noise if fused else 'zero', noise_param=self.noise_param)

    def _pipeline(self, is_training: bool):
        if is_training not in self._pipelines:
            from pedestrians_video_2_carla_amd.data.base.projection_2d_pipeline import DeviceProjection2DPipeline
            self._pipelines[is_training] = DeviceProjection2DPipeline(
                self.data_nodes, self.input_nodes, transform=self.transform, noise=self.noise, noise_param=self.noise_param,
                augment_flip=self.augment_flip, augment_rotate=self.augment_rotate,
                missing_joint_probabilities=self.missing_joint_probabilities or (), needs_confidence=self.needs_confidence,
                is_training=is_training, seed=self.seed)
        return self._pipelines[is_training]

    # ---- batches ------------------------------------------------------------------------------------------------------------------
    def generate_batch(self, device, batch_size: int = None, seed_offset: int = 0, *, stream: int = 0,
                       first_clip: Optional[int] = None, is_training: bool = True) -> Batch:
        """Clips [first_clip, first_clip + B) of ``stream``; ``seed_offset`` = the batch's index in the stream (first_clip =
        seed_offset B) for callers of the synthetic module's signature."""
        B, T = batch_size or self.batch_size, self.clip_length
        if seed_offset < 0:
            raise ValueError('a batch index cannot be negative: validation and test have streams of their own')
        first_clip = seed_offset * B if first_clip is None else first_clip
        fused = self.fused(is_training)
        if self.needs_confidence and fused:      # what ops.collate raises for a two-channel pose (confidence_mixin.py:17-18)
            raise RuntimeError('Tensors must have same number of dimensions: got 3 and 2')
        transform = self.transform.name
        if fused:
            want = ('frames', 'skel_type') + self.target_keys(is_training)
        else:
            want = ('skel_type', 'projection_2d') + _POSE_KEYS
        out = ops.generate_carla_batch(B, T, seed=self.seed, stream=stream, first_clip=first_clip, device=device,
                                       transform=transform if fused else 'none',
                                       miss_prob=self.missing_joint_probabilities if fused and self.needs_deform else None,
                                       want=want, **self._draw_kwargs(fused))
        skel_type = out.pop('skel_type')
        if fused:
            frames = out.pop('frames')
            targets = out
        else:
            raw = out.pop('projection_2d')
            frames, projection_targets = self._pipeline(is_training)(raw)
            targets = {**projection_targets, **out}
        age, gender = generator.age_gender(generator.skeleton_types(self.seed, stream, first_clip, B))
        return frames, targets, {'age': age, 'gender': gender, 'skel_type': skel_type}

    def train_batches(self, device, steps: int, rank: int = 0, first_step: int = 0):
        for i in range(first_step, first_step + steps):
            stream, first, B = self.clip_range('train', i, rank)
            yield self.generate_batch(device, batch_size=B, stream=stream, first_clip=first)

    def _eval_batches(self, device, stage: str) -> List[Batch]:
        key = (stage, str(device))
        if key not in self._eval_cache:
            size = self.val_set_size if stage == 'val' else self.test_set_size
            batches = []
            for i in range(-(-max(size, 0) // self.batch_size)):
                stream, first, B = self.clip_range(stage, i)
                batches.append(self.generate_batch(device, batch_size=B, stream=stream, first_clip=first, is_training=False))
            self._eval_cache[key] = batches
        return self._eval_cache[key]

    def val_batches(self, device) -> List[Batch]:
        return self._eval_batches(device, 'val')

    def test_batches(self, device) -> List[Batch]:
        return self._eval_batches(device, 'test')
