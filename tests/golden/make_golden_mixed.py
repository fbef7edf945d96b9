#!/usr/bin/env python3
"""Generate tests/golden/mixed.npz by running the reference's own ``MixedDataset``, ``MixedDataModule.
_map_missing_joint_probabilities``, ``SMPL_SKELETON`` and ``get_common_indices`` (build container only).

Stand-ins as in make_golden.py, plus ``numpy.find_common_type`` (removed in numpy 2; ``result_type`` is what it computed
for array dtypes), an empty ``LightningDataModule`` and an empty ``h5py``. The toy datasets are this file's, in memory:
JAAD-like clips with a ``crossing`` target, CARLA-like clips with ``frame.pedestrian.is_crossing`` and an extra float
target, string and numeric meta of which each side lacks one. Only data is stored: sizes, templates (as names of dtypes),
filled items.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402

LENGTHS = (50, 400)
MAPPINGS = {'frame.pedestrian.is_crossing': 'crossing'}


def toy_subset(which: int, n: int, T: int = 4):
    """Host arrays of one toy source, in the stored-subset form (projection_2d, targets, meta). Shared with the tests."""
    g = np.random.default_rng(100 + which)
    if which == 0:      # JAAD-like: BODY_25 with confidence, boxes, int64 class target under its own name
        proj = g.random((n, T, 25, 3), dtype=np.float32)
        targets = {'bboxes': g.random((n, T, 2, 2), dtype=np.float32), 'crossing': g.integers(0, 2, (n,)).astype(np.int64)}
        meta = {'video_id': [f'video_{i % 7:04d}' for i in range(n)], 'clip_id': np.arange(n, dtype=np.int64),
                'clip_width': np.full(n, 1920.0)}
    else:               # CARLA-like: 26 joints, float32 world targets, the class target under the CARLA name
        proj = g.random((n, T, 26, 2), dtype=np.float32)
        targets = {'world_loc': g.random((n, T, 3), dtype=np.float32),
                   'frame.pedestrian.is_crossing': g.integers(0, 2, (n,)).astype(np.int64)}
        meta = {'video_id': [f'rec_{i % 5}' for i in range(n)], 'clip_id': np.arange(n, dtype=np.int64) + 1000,
                'age': ['adult' if i % 2 else 'child' for i in range(n)], 'speed': g.random(n)}
    return proj, targets, meta


class ToyDataset(torch.utils.data.Dataset):
    def __init__(self, subset):
        self.proj, self.targets, self.meta = subset

    def __len__(self):
        return len(self.proj)

    def __getitem__(self, i):
        meta = {k: (v[i] if isinstance(v, list) else v[i].item()) for k, v in self.meta.items()}
        return torch.from_numpy(self.proj[i]), {k: torch.from_numpy(np.asarray(v[i])) for k, v in self.targets.items()}, meta


def main():
    if not os.path.isdir(MG.REF_SRC):
        sys.exit('reference tree not present: the committed .npz files are the artefact to use')
    MG.install_standins()
    if not hasattr(np, 'find_common_type'):
        np.find_common_type = lambda array_types, scalar_types: np.result_type(*array_types, *scalar_types)
    sys.modules['pytorch_lightning'].LightningDataModule = object
    MG._module('h5py')                       # imported by the reference's base data module, never called here
    sys.path.insert(0, MG.REF_SRC)
    from pedestrians_video_2_carla.data.base.skeleton import get_common_indices
    from pedestrians_video_2_carla.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla.data.mixed.mixed_dataset import MixedDataset
    from pedestrians_video_2_carla.data.openpose.skeleton import BODY_25_SKELETON
    from pedestrians_video_2_carla.data.smpl.skeleton import SMPL_SKELETON

    out = {}
    datasets = [ToyDataset(toy_subset(i, n)) for i, n in enumerate(LENGTHS)]
    for name, proportions in (('p2080', [0.2, 0.8]), ('p0all', [0, -1]), ('pnone', None)):
        np.random.seed(5)
        ds = MixedDataset(datasets, proportions=proportions, mappings=MAPPINGS)
        out[f'{name}/sizes'] = np.diff(ds.cumulative_sizes, prepend=0)
        keys = sorted(ds._targets_template)
        out[f'{name}/target_keys'] = np.array(keys)
        out[f'{name}/target_dtypes'] = np.array([np.dtype(ds._targets_template[k][0]).name for k in keys])
        for k in keys:
            out[f'{name}/target_shape/{k}'] = np.array(ds._targets_template[k][1], dtype=np.int64)
        mkeys = sorted(ds._meta_template)
        out[f'{name}/meta_keys'] = np.array(mkeys)
        out[f'{name}/meta_kinds'] = np.array([np.dtype(ds._meta_template[k]).kind for k in mkeys])
        for end, index in (('first', 0), ('last', len(ds) - 1)):
            # where the item came from (the reference's ConcatDataset / Subset bookkeeping), then the filled item
            which = int(np.searchsorted(ds.cumulative_sizes, index, side='right'))
            inner = index - (ds.cumulative_sizes[which - 1] if which else 0)
            sub = ds.datasets[which]
            out[f'{name}/{end}/row'] = np.int64(sub.indices[inner] if hasattr(sub, 'indices') else inner)
            out[f'{name}/{end}/dataset'] = np.int64(datasets.index(sub.dataset if hasattr(sub, 'indices') else sub))
            _, targets, meta = ds[index]
            for k, v in targets.items():
                out[f'{name}/{end}/targets/{k}'] = v.numpy()
            for k, v in meta.items():
                out[f'{name}/{end}/meta/{k}'] = np.array(v)

    from pedestrians_video_2_carla.data.mixed.mixed_datamodule import MixedDataModule
    mapper = MixedDataModule._map_missing_joint_probabilities
    probs = (np.arange(25) / 50.0).tolist()
    out['miss/body25'] = np.array(probs)
    out['miss/body25_to_carla'] = np.array(mapper(probs, BODY_25_SKELETON, CARLA_SKELETON))
    out['miss/body25_to_smpl'] = np.array(mapper(probs, BODY_25_SKELETON, SMPL_SKELETON))
    out['miss/single'] = np.array(mapper([0.25], BODY_25_SKELETON, SMPL_SKELETON))
    out['miss/empty_len'] = np.int64(len(mapper([], BODY_25_SKELETON, SMPL_SKELETON)))

    out['smpl/names'] = np.array([m.name for m in SMPL_SKELETON])
    out['smpl/flip_mask'] = np.array(SMPL_SKELETON.get_flip_mask(), dtype=np.int64)
    out['smpl/hips'] = np.int64(SMPL_SKELETON.get_hips_point().value)
    out['smpl/neck'] = np.int64(SMPL_SKELETON.get_neck_point().value)
    for a, b, sa, sb in (('smpl', 'carla', SMPL_SKELETON, CARLA_SKELETON), ('carla', 'smpl', CARLA_SKELETON, SMPL_SKELETON),
                         ('smpl', 'body25', SMPL_SKELETON, BODY_25_SKELETON), ('body25', 'smpl', BODY_25_SKELETON, SMPL_SKELETON)):
        o, i = get_common_indices(input_nodes=sa, output_nodes=sb)
        out[f'smpl/in_{a}__out_{b}__out_idx'] = np.array(o, dtype=np.int64)
        out[f'smpl/in_{a}__out_{b}__in_idx'] = np.array(i, dtype=np.int64)
    MG.npz('mixed', **out)


if __name__ == '__main__':
    main()
