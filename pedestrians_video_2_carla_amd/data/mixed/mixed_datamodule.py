"""``MixedDataModule`` and the reference's four mixtures (reference data/mixed/mixed_datamodule.py and
jaad_carlarec_datamodule.py, carlarec_amass_datamodule.py, jaad_carlarec_amass_datamodule.py,
jaad_carlarec_benchmark_datamodule.py).

A mixed data module holds one data module per source, built from the common keywords overridden by that source's own
(``data_modules_kwargs``), mixes their stored subsets by the requested proportions (``MixedDataset``) and hands out a
``MixedDeviceLoader`` whose batches went through K26. Out of scope, as for ``BaseDataModule`` here: dataset ingestion
(csv / xml / AMASS files) -- a source is a stored subset --, ``class_counts`` merging and the initial-metrics pass.
"""
import logging
from typing import Any, Dict, List, Optional, Sequence, Type

import numpy as np

from pedestrians_video_2_carla_amd.data.base.base_datamodule import BaseDataModule
from pedestrians_video_2_carla_amd.data.base.skeleton import Skeleton, get_common_indices
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
from pedestrians_video_2_carla_amd.data.mixed.mixed_dataset import MixedDataset, validate_proportions
from pedestrians_video_2_carla_amd.data.openpose.skeleton import BODY_25_SKELETON
from pedestrians_video_2_carla_amd.data.smpl.skeleton import SMPL_SKELETON

_PIPELINE_KEYS = ('noise', 'noise_param', 'missing_joint_probabilities', 'augment_flip', 'augment_rotate', 'needs_confidence')


# The source data modules of the reference's mixtures. Their ingestion is out of scope; what the mixtures need of them is
# the class (as the key of the per-source kwargs and the name in hparams) and the BaseDataModule behaviour.
class JAADOpenPoseDataModule(BaseDataModule):
    pass


class JAADBenchmarkDataModule(JAADOpenPoseDataModule):
    pass


class CarlaRecordedDataModule(BaseDataModule):
    pass


class CarlaBenchmarkDataModule(CarlaRecordedDataModule):
    pass


class AMASSDataModule(BaseDataModule):
    pass


def flat_args_as_list_arg(kwargs: Dict, name: str, pop: bool = False) -> List:
    """``name`` as a list, given either as such or as ``name_0, name_1, ...`` (reference utils/argparse.py:64-81; with
    ``pop`` the flat ones are removed -- the reference's version raises NameError when ``name`` itself is present)."""
    flat = sorted((kw for kw in kwargs if kw.startswith(f'{name}_') and kw[len(name) + 1:].isdigit()),
                  key=lambda x: int(x[len(name) + 1:]))
    values = list(kwargs[name]) if name in kwargs else [kwargs[kw] for kw in flat if kwargs[kw] is not None]
    if pop:
        for kw in flat:
            kwargs.pop(kw)
    return values


class MixedDataModule(object):
    data_modules: List[Type[BaseDataModule]] = []

    # default mixing proportions; overridden by subclasses
    train_proportions: Sequence[float] = []
    val_proportions: Sequence[float] = []
    test_proportions: Sequence[float] = []

    def __init__(self,
                 data_modules_kwargs: Dict[Type[BaseDataModule], Dict[str, Any]],
                 data_modules: Optional[List[Type[BaseDataModule]]] = None,
                 train_proportions: Optional[List[float]] = None,
                 val_proportions: Optional[List[float]] = None,
                 test_proportions: Optional[List[float]] = None,
                 mappings: Optional[Dict[str, str]] = None,
                 **kwargs):
        all_data_modules = list(self.data_modules) + list(data_modules or [])
        assert len(all_data_modules) > 1, 'At least 2 data modules are required'
        self._skip_metadata = kwargs.get('skip_metadata', False)
        self._mappings = mappings
        kwargs.setdefault('input_nodes', CARLA_SKELETON)               # mixed_datamodule.py:203-206
        self._source_kwargs = [{**kwargs, **data_modules_kwargs.get(dm_cls, {})} for dm_cls in all_data_modules]
        self._data_modules: List[BaseDataModule] = [dm_cls(**kw) for dm_cls, kw in zip(all_data_modules, self._source_kwargs)]
        if len({dm.input_nodes for dm in self._data_modules}) != 1:
            raise ValueError('all sources must map onto one input skeleton')
        self.input_nodes = self._data_modules[0].input_nodes
        self.batch_size = self._data_modules[0].batch_size

        self.hparams: Dict[str, Any] = {}
        for dm in self._data_modules:
            self.hparams.update(dm.hparams)
        self.requested_train_proportions = self._validate_proportions(train_proportions or self.train_proportions)
        self.requested_val_proportions = self._validate_proportions(val_proportions or self.val_proportions)
        self.requested_test_proportions = self._validate_proportions(test_proportions or self.test_proportions)
        self.hparams['train_proportions'] = self.requested_train_proportions
        self.hparams['val_proportions'] = self.requested_val_proportions
        self.hparams['test_proportions'] = self.requested_test_proportions
        self.hparams['mixed_datasets'] = [dm.__class__.__name__ for dm in self._data_modules]
        self.hparams['data_module_name'] = self.__class__.__name__     # explicitly set this to avoid confusion
        self.hparams['data_nodes'] = 'Mixed'

    @staticmethod
    def _map_missing_joint_probabilities(probabilities: List, input_nodes: Type[Skeleton],
                                         output_nodes: Type[Skeleton]) -> List:
        """Missing-joint probabilities given for ``input_nodes``, for ``output_nodes``: common joints keep theirs, the rest
        take the mean (mixed_datamodule.py:102-130)."""
        if len(probabilities) > 1:
            missing_joint_probabilities = np.array(probabilities)
            mean_missing_joint_probability = np.mean(missing_joint_probabilities)
            output_indices, input_indices = get_common_indices(input_nodes, output_nodes)
            mapped = np.ones(len(output_nodes)) * mean_missing_joint_probability
            mapped[output_indices] = missing_joint_probabilities[input_indices]
            return mapped.tolist()
        return probabilities[:]

    def _validate_proportions(self, proportions):
        return validate_proportions(proportions, len(self._data_modules))

    @classmethod
    def uses_infinite_train_set(cls):
        return False                    # mixing infinite datasets is not supported

    def proportions(self, stage: str) -> Sequence[float]:
        return {'train': self.requested_train_proportions, 'val': self.requested_val_proportions,
                'test': self.requested_test_proportions, 'predict': self.requested_test_proportions}[stage]

    def get_dataset(self, subsets: Sequence, stage: str = 'train', seed: int = 22742) -> MixedDataset:
        """``subsets``: per data module, the path of a stored subset or its (projection_2d, targets, meta) host arrays."""
        from pedestrians_video_2_carla_amd.data.base.subset_io import load_subset
        assert len(subsets) == len(self._data_modules), 'one stored subset per data module'
        loaded = [load_subset(s) if isinstance(s, str) else s for s in subsets]
        dataset = MixedDataset(loaded, skip_metadata=self._skip_metadata, proportions=self.proportions(stage),
                               mappings=self._mappings, seed=seed)
        self.hparams[f'{stage}_set_sizes'] = tuple(np.diff(dataset.cumulative_sizes, prepend=0).tolist())
        return dataset

    def get_dataloader(self, subsets: Sequence, device, stage: str = 'train', shuffle: Optional[bool] = None,
                       drop_last: bool = True, is_training: Optional[bool] = None, rank: int = 0, world_size: int = 1,
                       seed: int = 22742, **pipeline_kwargs):
        """A ``MixedDeviceLoader`` over the mixture of ``subsets`` for ``stage``; ``pipeline_kwargs`` override the
        ``Projection2DMixin`` keywords of every source (those given at construction apply per source)."""
        from pedestrians_video_2_carla_amd.data.mixed.loader import MixedDeviceLoader
        from pedestrians_video_2_carla_amd.data.mixed.pipeline import MixedProjection2DPipeline
        shuffle = (stage == 'train') if shuffle is None else shuffle
        dataset = self.get_dataset(subsets, stage, seed)
        settings = []
        for i in dataset.sources:
            dm, kw = self._data_modules[i], self._source_kwargs[i]
            settings.append({'data_nodes': dm.data_nodes, 'transform': dm.transform,
                             **{k: kw[k] for k in _PIPELINE_KEYS if k in kw}, **pipeline_kwargs})
        pipeline = MixedProjection2DPipeline(settings, self.input_nodes, seed=seed,
                                             is_training=shuffle if is_training is None else is_training)
        return MixedDeviceLoader(dataset, pipeline, self.batch_size, device, shuffle=shuffle, drop_last=drop_last,
                                 seed=seed, rank=rank, world_size=world_size)

    def save_predictions(self, *args, **kwargs) -> str:
        # assumption: data was converted to the same format as the first data module
        return self._data_modules[0].save_predictions(*args, **kwargs)


def _off_jaad(kwargs: Dict, others: Sequence[Type[Skeleton]]):
    """The mixtures with JAAD: probabilities / noise are given for BODY_25 and mapped to the other skeletons; with
    ``strong_points`` < 1 they are meant to deform the datasets OTHER than JAAD, whose detections are already imperfect
    (jaad_carlarec_datamodule.py:21-40)."""
    jaad_probabilities = flat_args_as_list_arg(kwargs, 'missing_joint_probabilities', True)
    kwargs.pop('missing_joint_probabilities', None)
    strong_points = kwargs.get('strong_points', 0)
    jaad_noise = kwargs.get('noise', 'zero')
    other_noise = jaad_noise
    mapped = [MixedDataModule._map_missing_joint_probabilities(jaad_probabilities, BODY_25_SKELETON, nodes) for nodes in others]
    if (len(jaad_probabilities) or jaad_noise != 'zero') and strong_points < 1:
        logging.getLogger(__name__).warning(
            'Strong points is less than 1, but JAAD missing joint probabilities and/or noise are set. Assuming that the '
            'artificial missing joints and noise are meant for the datasets OTHER than JAAD.')
        jaad_probabilities, jaad_noise = [], 'zero'
    return jaad_probabilities, jaad_noise, mapped, other_noise


_CROSSING = {'frame.pedestrian.is_crossing': 'crossing'}


def _jaad(probabilities, noise):
    return {'data_nodes': BODY_25_SKELETON, 'input_nodes': CARLA_SKELETON, 'missing_joint_probabilities': probabilities,
            'noise': noise, 'classification_targets_key': 'crossing'}


def _carla(probabilities, noise=None):
    kw = {'data_nodes': CARLA_SKELETON, 'input_nodes': CARLA_SKELETON, 'missing_joint_probabilities': probabilities,
          'classification_targets_key': 'frame.pedestrian.is_crossing'}
    return kw if noise is None else {**kw, 'noise': noise}


class JAADCarlaRecDataModule(MixedDataModule):
    data_modules = [JAADOpenPoseDataModule, CarlaRecordedDataModule]
    train_proportions = [0.2, 0.8]
    val_proportions = [0, -1]
    test_proportions = [0, -1]

    def __init__(self, **kwargs):
        jaad_p, jaad_noise, (carla_p,), carla_noise = _off_jaad(kwargs, [CARLA_SKELETON])
        super().__init__(data_modules_kwargs={self.data_modules[0]: _jaad(jaad_p, jaad_noise),
                                              self.data_modules[1]: _carla(carla_p, carla_noise)},
                         mappings=dict(_CROSSING), **kwargs)


class JAADCarlaRecBenchmarkDataModule(JAADCarlaRecDataModule):
    data_modules = [JAADBenchmarkDataModule, CarlaBenchmarkDataModule]


class CarlaRecAMASSDataModule(MixedDataModule):
    data_modules = [CarlaRecordedDataModule, AMASSDataModule]
    train_proportions = [0.5, 0.5]
    val_proportions = [0.5, 0.5]
    test_proportions = [0.5, 0.5]

    def __init__(self, **kwargs):
        carla_p = flat_args_as_list_arg(kwargs, 'missing_joint_probabilities', True)
        kwargs.pop('missing_joint_probabilities', None)
        amass_p = MixedDataModule._map_missing_joint_probabilities(carla_p, CARLA_SKELETON, SMPL_SKELETON)
        super().__init__({CarlaRecordedDataModule: _carla(carla_p),
                          AMASSDataModule: {'data_nodes': SMPL_SKELETON, 'input_nodes': CARLA_SKELETON,
                                            'missing_joint_probabilities': amass_p}}, **kwargs)


class JAADCarlaRecAMASSDataModule(MixedDataModule):
    data_modules = [JAADOpenPoseDataModule, CarlaRecordedDataModule, AMASSDataModule]
    train_proportions = [0.1, 0.4, 0.5]
    val_proportions = [0, 0, -1]
    test_proportions = [0, 0, -1]

    def __init__(self, **kwargs):
        jaad_p, jaad_noise, (carla_p, amass_p), other_noise = _off_jaad(kwargs, [CARLA_SKELETON, SMPL_SKELETON])
        super().__init__({JAADOpenPoseDataModule: _jaad(jaad_p, jaad_noise),
                          CarlaRecordedDataModule: _carla(carla_p, other_noise),
                          AMASSDataModule: {'data_nodes': SMPL_SKELETON, 'input_nodes': CARLA_SKELETON,
                                            'missing_joint_probabilities': amass_p, 'noise': other_noise}}, **kwargs)
