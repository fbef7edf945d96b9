"""``MixedDataset`` over stored subsets (reference data/mixed/mixed_dataset.py:7-107).

The reference concatenates ``torch.utils.data`` datasets (optionally random ``Subset``s of them, sized by the requested
proportions) and fills, item by item, the targets and meta a source lacks. Here a source is a stored subset -- the host
arrays ``(projection_2d, targets, meta)`` of ``load_subset`` -- and the same bookkeeping is kept as index arrays, so that a
loader can gather whole batches: ``source_of`` / ``row_of`` over the concatenated index space, ``gather_targets`` /
``gather_meta`` for a batch of indices, ``__getitem__`` for one (the reference's item, minus the pose processing that K26
does per batch).

Stated deviation: the rows of a proportioned source are drawn without replacement from ``numpy.random.default_rng(seed)``;
the reference draws from numpy's global state. And where the reference would ``numpy.full(shape, nan, dtype=<integer>)``
for a key a source lacks -- undefined, and a warning on current numpy -- this raises ``ValueError`` naming the key.
"""
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

Subset = Tuple[np.ndarray, Dict[str, np.ndarray], Dict[str, Iterable]]


def validate_proportions(proportions: Sequence[float], n: int) -> Sequence[float]:
    """``MixedDataModule._validate_proportions`` (mixed_datamodule.py:163-168)."""
    assert len(proportions) == n, 'Proportions must be specified for each data module.'
    assert (all(0 <= p <= 1 for p in proportions) and sum(proportions) == 1) or all((p == 0 or p == -1) for p in proportions)
    return proportions


def _meta_item(v, i):
    x = v[i]
    return x.item() if isinstance(x, np.generic) else x


class MixedDataset:
    def __init__(self, datasets: Sequence[Subset], skip_metadata: bool = False,
                 proportions: Optional[Iterable[float]] = None, mappings: Optional[Dict[str, str]] = None,
                 seed: int = 22742, **kwargs):
        datasets = list(datasets)
        lengths = [len(d[0]) for d in datasets]
        if len({d[0].shape[1] for d in datasets}) > 1:
            raise ValueError(f'all sources must share the clip length, got {[d[0].shape[1] for d in datasets]}')
        proportions = None if proportions is None else list(proportions)
        if proportions is None:                                        # use all available data
            used = [(i, np.arange(n)) for i, n in enumerate(lengths)]
        elif all((p == 0 or p == -1) for p in proportions):            # use whole dataset or none
            used = [(i, np.arange(lengths[i])) for i, p in enumerate(proportions) if p != 0]
        else:                                                          # use a subset of the dataset
            rng = np.random.default_rng(seed)
            possible_total = min(lengths[i] / p if p != 0 else float('inf') for i, p in enumerate(proportions))
            used = [(i, rng.choice(lengths[i], int(possible_total * p), replace=False))
                    for i, p in enumerate(proportions) if p != 0]
        self.datasets = datasets
        self.sources: List[int] = [i for i, _ in used]                 # which of `datasets` each used source is
        self.indices: List[np.ndarray] = [np.asarray(rows, dtype=np.int64) for _, rows in used]
        self.cumulative_sizes = np.cumsum([len(r) for r in self.indices]).tolist()
        # the concatenated index space: position -> (used source, row in that source's arrays)
        self.source_of = np.concatenate([np.full(len(r), k, dtype=np.int64) for k, r in enumerate(self.indices)]
                                        or [np.zeros(0, dtype=np.int64)])
        self.row_of = np.concatenate(self.indices or [np.zeros(0, dtype=np.int64)])

        self._mappings = mappings
        self._inverse_mappings = {v: k for k, v in mappings.items()} if mappings else None
        mappings_keys = tuple(mappings.keys()) if mappings else tuple()

        # common targets: over ALL given datasets, as the reference (:49-61)
        self._targets_template: Dict[str, Tuple[np.dtype, Tuple[int, ...]]] = {}
        all_keys = {k for _, t, _ in datasets for k in t if k not in mappings_keys}
        for key in sorted(all_keys):
            having = [np.asarray(t[key]) for _, t, _ in datasets if key in t]
            shapes = [tuple(a.shape[1:]) for a in having]
            assert all(s == shapes[0] for s in shapes), \
                f'{key} has different shapes in different datasets: {str(list(shapes))}'
            self._targets_template[key] = (np.result_type(*[a.dtype for a in having]), shapes[0])
        for key, (dtype, _) in self._targets_template.items():
            if dtype.kind in 'iub' and any(self._target_source_key(key, datasets[i][1]) is None for i in self.sources):
                raise ValueError(f'target {key!r} is {dtype.name} and a source lacks it: there is no integer NaN to fill it with')

        # common meta: over the USED sources (:64-72); pandas' column dtypes restated: strings stay strings, a numeric
        # column that some source lacks holds NaN and is therefore float64
        self._meta_template: Optional[Dict[str, np.dtype]] = None
        if not skip_metadata:
            self._meta_template = {}
            metas = [datasets[i][2] for i in self.sources]
            for key in dict.fromkeys(k for m in metas for k in m):
                if key in mappings_keys:
                    continue
                firsts = [np.asarray(_meta_item(m[key], 0)) for m in metas if key in m and len(m[key])]
                if any(a.dtype.kind in 'USO' for a in firsts):
                    self._meta_template[key] = np.dtype('str')
                elif len(firsts) < len(metas):
                    self._meta_template[key] = np.dtype('float64')
                else:
                    self._meta_template[key] = np.result_type(*[a.dtype for a in firsts])

    def __len__(self) -> int:
        return int(self.source_of.shape[0])

    def _target_source_key(self, key: str, targets: Dict) -> Optional[str]:
        if key in targets:
            return key
        mapped = self._inverse_mappings.get(key) if self._inverse_mappings else None
        return mapped if mapped in targets else None

    @property
    def targets_template(self):
        return self._targets_template

    @property
    def meta_template(self):
        return self._meta_template

    # ---- batches ---------------------------------------------------------------------------------------------------------
    def gather_targets(self, index: np.ndarray) -> Dict[str, np.ndarray]:
        """Common targets of the items ``index`` (concatenated index space), in that order (:77-90)."""
        index = np.asarray(index, dtype=np.int64)
        src, row = self.source_of[index], self.row_of[index]
        out = {}
        for key, (dtype, shape) in self._targets_template.items():
            buf = np.full((len(index),) + shape, np.nan if dtype.kind not in 'iub' else 0, dtype=dtype)
            for k, i in enumerate(self.sources):
                name = self._target_source_key(key, self.datasets[i][1])
                sel = src == k
                if name is not None and sel.any():
                    buf[sel] = self.datasets[i][1][name][row[sel]]
            out[key] = buf
        return out

    def gather_meta(self, index: np.ndarray) -> Dict[str, list]:
        """Common meta of the items ``index`` as lists (:92-105): a missing string is 'nan', a missing number NaN."""
        if self._meta_template is None:
            return {}
        index = np.asarray(index, dtype=np.int64)
        src, row = self.source_of[index], self.row_of[index]
        out = {}
        for key, dtype in self._meta_template.items():
            col = []
            for k, r in zip(src, row):
                meta = self.datasets[self.sources[k]][2]
                mapped = self._inverse_mappings.get(key) if self._inverse_mappings else None
                name = key if key in meta else (mapped if mapped in meta else None)
                value = _meta_item(meta[name], r) if name is not None else np.nan
                col.append(np.array([value], dtype=dtype).item())
            out[key] = col
        return out

    def __getitem__(self, index: int):
        """(projection_2d as stored, common targets, common meta) of one item."""
        if index < 0:
            index += len(self)
        i = np.array([index])
        proj = self.datasets[self.sources[self.source_of[index]]][0][self.row_of[index]]
        return proj, {k: v[0] for k, v in self.gather_targets(i).items()}, {k: v[0] for k, v in self.gather_meta(i).items()}
