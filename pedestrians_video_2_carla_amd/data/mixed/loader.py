"""``MixedDeviceLoader``: ``DeviceLoader`` over a ``MixedDataset`` (several stored subsets with different skeletons).

Same batch contract ``(frames, targets, meta)``, same shuffle / ``drop_last`` / rank-striding rules (they are
``DeviceLoader``'s own methods) and the same double-buffered pinned staging. The epoch order runs over the concatenated
index space of the dataset; the raw poses of a batch are staged per source (their shapes differ), packed in batch order,
together with ``source[n]`` and ``row[n]`` = clip n's position in its source's staged rows; targets are assembled in batch
order from the dataset's common template (NaN where a source lacks a key). ``source`` / ``row`` are checked here, on the
host, where they are built; the kernel only clamps. ``skel_type`` is provided only when every source has ``age`` and
``gender``.
"""
from typing import Dict, Iterable, Iterator, Tuple

import numpy as np
import torch

from pedestrians_video_2_carla_amd import ops
from pedestrians_video_2_carla_amd.data.base.loader import DeviceLoader
from pedestrians_video_2_carla_amd.data.carla import reference as ref
from pedestrians_video_2_carla_amd.data.mixed.mixed_dataset import MixedDataset


class MixedDeviceLoader(DeviceLoader):
    def __init__(self, dataset: MixedDataset, pipeline, batch_size: int, device, shuffle: bool = False,
                 drop_last: bool = True, seed: int = 22742, rank: int = 0, world_size: int = 1):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('MixedDeviceLoader feeds the HIP input pipeline: it needs a GPU device')
        if pipeline.num_sources != len(dataset.sources):
            raise RuntimeError(f'{pipeline.num_sources} pipeline settings for {len(dataset.sources)} used sources')
        self.dataset, self.pipeline = dataset, pipeline
        self.batch_size, self.shuffle, self.drop_last = int(batch_size), shuffle, drop_last
        self.rank, self.world_size, self.seed, self.epoch = rank, world_size, seed, 0
        self.n = len(dataset)
        used = [dataset.datasets[i] for i in dataset.sources]
        self._raw = [torch.from_numpy(np.ascontiguousarray(d[0], dtype=np.float32)) for d in used]
        self._has_bboxes = ['bboxes' in d[1] for d in used]
        self._skel_type = None
        if all('age' in d[2] and 'gender' in d[2] for d in used):    # per-clip reference skeleton (projection.py:52-71)
            self._skel_type = [ref.skeleton_types_from_meta({'age': list(d[2]['age']), 'gender': list(d[2]['gender'])},
                                                            batch_size=len(d[0]), strict=True).to(torch.int32).numpy()
                               for d in used]
        B = self.batch_size
        shapes = {f'raw/{k}': ((B,) + tuple(r.shape[1:]), torch.float32) for k, r in enumerate(self._raw)}
        shapes['source'], shapes['row'] = ((B,), torch.uint8), ((B,), torch.int32)
        for k, (dtype, shape) in dataset.targets_template.items():
            shapes['targets/' + k] = ((B,) + shape, torch.float32 if dtype.kind == 'f' else torch.from_numpy(np.zeros(0, dtype)).dtype)
        if self._skel_type is not None:
            shapes['meta/skel_type'] = ((B,), torch.int32)
        self._pinned = [{k: torch.empty(s, dtype=t).pin_memory() for k, (s, t) in shapes.items()} for _ in range(2)]
        self._copy_stream = torch.cuda.Stream(device=self.device)
        self._slot_events = [None, None]

    def _stage(self, idx: torch.Tensor, slot: int):
        index = idx.numpy()
        src, row = self.dataset.source_of[index], self.dataset.row_of[index]
        ops.check_mixed_index(src, row, [r.shape[0] for r in self._raw])
        host: Dict[str, Tuple[torch.Tensor, int]] = {}
        packed = np.zeros(len(index), dtype=np.int32)
        prev = self._slot_events[slot]
        if prev is not None:
            prev.synchronize()          # the DMA engine has finished reading this pinned set (issued two batches ago)
        pins = self._pinned[slot]
        counts = []
        for k, raw in enumerate(self._raw):
            sel = np.flatnonzero(src == k)
            packed[sel] = np.arange(len(sel), dtype=np.int32)
            counts.append(len(sel))
            torch.index_select(raw, 0, torch.from_numpy(row[sel]), out=pins[f'raw/{k}'][:len(sel)])
            host[f'raw/{k}'] = len(sel)
        ops.check_mixed_index(src, packed, counts)
        n = len(index)
        pins['source'][:n] = torch.from_numpy(src.astype(np.uint8))
        pins['row'][:n] = torch.from_numpy(packed)
        for k, v in self.dataset.gather_targets(index).items():
            pins['targets/' + k][:n] = torch.from_numpy(v)
        if self._skel_type is not None:
            st = np.zeros(n, dtype=np.int32)
            for k, table in enumerate(self._skel_type):
                st[src == k] = table[row[src == k]]
            pins['meta/skel_type'][:n] = torch.from_numpy(st)
        out = {}
        with torch.cuda.stream(self._copy_stream):
            for k, pin in pins.items():
                out[k] = pin[:host.get(k, n)].to(self.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._copy_stream)
        self._slot_events[slot] = ev
        return out, ev, idx

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, Dict[str, torch.Tensor], Dict[str, Iterable]]]:
        order = self._order()
        self.epoch += 1
        chunks = list(order.split(self.batch_size))
        if chunks and self.drop_last and chunks[-1].numel() < self.batch_size:
            chunks.pop()
        staged = self._stage(chunks[0], 0) if chunks else None
        for i in range(len(chunks)):
            tensors, ev, idx = staged
            staged = self._stage(chunks[i + 1], (i + 1) & 1) if i + 1 < len(chunks) else None
            stream = torch.cuda.current_stream(self.device)
            stream.wait_event(ev)
            for t in tensors.values():
                t.record_stream(stream)
            raws = [tensors.pop(f'raw/{k}') for k in range(len(self._raw))]
            source, row = tensors.pop('source'), tensors.pop('row')
            targets = {k[8:]: v for k, v in tensors.items() if k.startswith('targets/')}
            meta = self.dataset.gather_meta(idx.numpy())
            if 'meta/skel_type' in tensors:
                meta['skel_type'] = tensors['meta/skel_type']
            frames, projection_targets = self.pipeline(raws, source, row, targets, meta, has_bboxes=self._has_bboxes)
            yield frames, {**targets, **projection_targets}, meta
