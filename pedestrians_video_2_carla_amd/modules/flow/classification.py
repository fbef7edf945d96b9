"""``LitClassificationFlow``: (B, T, J, 2) keypoint clips -> classifier -> logits, CrossEntropyLoss / BCEWithLogitsLoss
(reference modules/flow/classification.py:41-596).

Constructor, outputs key (``<targets_key>_logits``), criterion choice (BCE only for ``num_classes == 2`` with a binary-output
model), ``_unwrap_batch``, ``_inner_step`` (target squeezed when ``out.ndim - 1 != target.ndim``), the three steps' return value
``{'loss', 'preds', 'targets'}`` and the logged names ``{stage}_loss/primary`` / ``{stage}_loss/<CriterionName>`` are the
reference's. On the device the loss, its gradient, the predicted class and the confusion counts of a batch are ONE launch
(K24, ``ops.classification_loss``); the reference's per-step ``torch.isnan(loss)`` host sync is replaced by ``check_finite``.

Metrics. The reference updates eight torchmetrics objects per batch. Here every train and eval step adds its batch to one
device (C, C) int32 matrix ``confusion[target, predicted]`` inside the loss launch, and ``compute_metrics`` (end of an epoch)
all-reduces it over the ranks, derives on the host, and resets it:

  ConfusionMatrix   the matrix itself (rows: target, columns: prediction)
  per class c       tp = M[c, c], fp = column sum - tp, fn = row sum - tp, support = row sum
                    precision = tp / (tp + fp), recall = tp / (tp + fn), F1 = harmonic mean of the two; a 0 / 0 gives 0
  'macro'           unweighted mean over the C classes          'weighted'   mean weighted by support
  'micro'           the counts pooled over the classes          'none'       the per-class values
  Accuracy          per class it is the recall: 'micro' = trace / total, 'macro' = mean per-class recall
  'none' with num_classes == 2 reports the positive class (index 1), as the reference's ``_unwrap_nested_metrics`` does;
  ``classification_average='benchmark'`` = Accuracy 'micro', Precision / Recall / F1Score 'none'.

AUROC, ROCCurve, PRCurve (torchmetrics' definitions, which the reference registers) need every score of the epoch, ranked per
class, so they cannot come from the matrix. ``validation_step`` and ``test_step`` -- the reference updates its metrics in
``_eval_step_end`` only -- append their batch's fp32 softmax (binary: sigmoid) scores and int32 targets to a device epoch buffer
(``ops.rank_scores``, one launch; the buffer doubles when full, is no module buffer and is not in ``state_dict``), and
``compute_metrics`` ranks it on the device (K25, ``ops.rank_curves``): per class, one-vs-rest, the distinct scores in descending
order with the positives ``tps`` and negatives ``fps`` at or above each (scikit-learn's ``_binary_clf_curve``). From those, on
the host in fp64, with P = tps[-1] and Q = fps[-1]:

  AUROC     sum_k (fps[k] - fps[k-1]) (tps[k] + tps[k-1]) / (2 P Q), the sum in integers; NaN for a class with P == 0 or Q == 0;
            reported: the unweighted mean over the classes (torchmetrics' default 'macro', whatever ``classification_average``
            is; NaN if any class is NaN), the one value for the binary form
  ROCCurve  (fpr, tpr, thresholds) = ([0, fps / Q], [0, tps / P], [thresholds[0] + 1, thresholds...])
  PRCurve   precision = tps / (tps + fps), recall = tps / P, both cut after the first point of full recall, reversed, with
            (1, 0) appended; thresholds = the cut piece reversed
  a curve is a tuple of three numpy arrays (binary form) or of three per-class lists of arrays; rows whose target lies outside
  [0, C) or that hold a NaN score are dropped. ``classification_rank_metrics=False`` turns all of this off.

Not registered: the initial-metrics pass, W&B tables and video logging (``sample_curve`` gives the 20 points per curve that the
reference's ``_log_curve`` would log). The graph classifiers and torch_geometric batches are out of scope, and so
is HIP-graph capture of this flow (``Trainer(use_graph=False)``).
"""
import platform
from typing import Any, Dict, Union

import numpy as np
import torch
import torch.distributed as dist

from pedestrians_video_2_carla_amd.modules.classification import GRU, LSTM
from pedestrians_video_2_carla_amd.modules.flow.lightning_shim import LightningModuleBase
from pedestrians_video_2_carla_amd.modules.flow.output_types import ClassificationModelOutputType

AVERAGES = ('micro', 'macro', 'weighted', 'none')
BENCHMARK_AVERAGE = {'Accuracy': 'micro', 'Precision': 'none', 'Recall': 'none', 'F1Score': 'none'}


def _ratio(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.divide(a, b, out=np.zeros(np.broadcast(a, b).shape), where=b != 0)


def classification_metrics(matrix, average: Dict[str, str]) -> Dict[str, Any]:
    """Accuracy / Precision / Recall / F1Score of a (C, C) ``confusion[target, predicted]`` matrix under ``average`` (one of
    ``AVERAGES`` per metric; definitions in the module docstring). Scalars are floats, 'none' gives a (C,) array -- for C == 2
    the positive class's value."""
    m = np.asarray(matrix, dtype=np.float64)
    C = m.shape[0]
    tp, support, predicted = np.diag(m), m.sum(axis=1), m.sum(axis=0)
    per_class = {'Precision': _ratio(tp, predicted), 'Recall': _ratio(tp, support)}
    per_class['F1Score'] = _ratio(2 * per_class['Precision'] * per_class['Recall'], per_class['Precision'] + per_class['Recall'])
    per_class['Accuracy'] = per_class['Recall']
    micro = float(_ratio(tp.sum(), m.sum()))         # pooled: sum tp / sum (tp + fp) = sum tp / sum (tp + fn) = trace / total
    out = {}
    for name in ('Accuracy', 'Precision', 'Recall', 'F1Score'):
        avg, v = average[name], per_class[name]
        if avg == 'micro':
            out[name] = micro
        elif avg == 'macro':
            out[name] = float(v.mean())
        elif avg == 'weighted':
            out[name] = float(_ratio((v * support).sum(), support.sum()))
        elif avg == 'none':
            out[name] = float(v[1]) if C == 2 else v
        else:
            raise ValueError(f'unknown average {avg!r} for {name}')
    return out


def rank_metrics(curves: Dict[str, Any], binary: bool) -> Dict[str, Any]:
    """'AUROC', 'ROCCurve', 'PRCurve' (module docstring) from the output of ``ops.rank_curves``."""
    auroc = curves['auroc'].cpu().numpy().astype(np.float64)
    roc, pr = ([], [], []), ([], [], [])
    with np.errstate(divide='ignore', invalid='ignore'):
        for th, tps, fps in zip(curves['thresholds'], curves['tps'], curves['fps']):
            th = th.cpu().numpy().astype(np.float64)
            tps, fps = tps.cpu().numpy().astype(np.float64), fps.cpu().numpy().astype(np.float64)
            if len(th) == 0:
                empty = np.zeros(0)
                for dst, v in zip(roc + pr, (empty,) * 6):
                    dst.append(v)
                continue
            P, Q = tps[-1], fps[-1]
            roc[0].append(np.concatenate([[0.0], fps / Q]))
            roc[1].append(np.concatenate([[0.0], tps / P]))
            roc[2].append(np.concatenate([[th[0] + 1.0], th]))
            cut = int(np.argmax(tps == P)) + 1                           # up to the first point of full recall
            pr[0].append(np.concatenate([(tps / (tps + fps))[:cut][::-1], [1.0]]))
            pr[1].append(np.concatenate([(tps / P)[:cut][::-1], [0.0]]))
            pr[2].append(th[:cut][::-1].copy())
    if binary:
        return {'AUROC': float(auroc[0]), 'ROCCurve': tuple(v[0] for v in roc), 'PRCurve': tuple(v[0] for v in pr)}
    return {'AUROC': float(auroc.mean()), 'ROCCurve': roc, 'PRCurve': pr}


def sample_curve(x, y, samples: int = 20):
    """The points of one class's curve that the reference logs (``_log_curve``): ``x[int(len * k / samples)]`` for k < samples,
    samples = min(samples, len(y)); two lists of floats."""
    n = min(samples, len(y))
    return ([float(x[int(len(x) * k / n)]) for k in range(n)], [float(y[int(len(y) * k / n)]) for k in range(n)])


class LitClassificationFlow(LightningModuleBase):
    rank_initial_capacity = 4096       # rows of the epoch score buffer when it is first allocated; it doubles when full

    def __init__(self, classification_model, classification_targets_key: str,
                 classification_average: Union[str, Dict[str, str]] = 'macro', num_classes: int = 2,
                 classification_rank_metrics: bool = True, **kwargs: Any):
        super().__init__()
        self.classification_model = classification_model
        self._targets_key = classification_targets_key
        self._outputs_key = classification_targets_key + '_logits'
        self._num_classes = num_classes
        if isinstance(classification_average, str):
            self._average = dict(BENCHMARK_AVERAGE) if classification_average == 'benchmark' else {
                k: classification_average for k in BENCHMARK_AVERAGE}
        else:
            self._average = dict(classification_average)
        for k in BENCHMARK_AVERAGE:
            if self._average.get(k) not in AVERAGES:
                raise ValueError(f'classification_average: {k} needs one of {AVERAGES}, got {self._average.get(k)!r}')
        self._binary = (num_classes == 2 and classification_model.output_type == ClassificationModelOutputType.binary)
        self.criterion = torch.nn.BCEWithLogitsLoss() if self._binary else torch.nn.CrossEntropyLoss()
        # confusion[target, predicted] of the running epoch, added to by every step's loss launch (K24)
        self.register_buffer('confusion', torch.zeros(num_classes, num_classes, dtype=torch.int32), persistent=False)
        # scores and targets of the running evaluation epoch (AUROC and the curves): plain attributes, not in state_dict
        self._rank_on = bool(classification_rank_metrics)
        self._rank_scores = self._rank_targets = None
        self._rank_rows = 0
        self.save_hyperparameters({'host': platform.node(), 'classification_average': self._average,
                                   **self.classification_model.hparams})

    # ---- registry / introspection ----------------------------------------------------------------------------------
    outputs_key = property(lambda self: self._outputs_key)
    needs_graph = property(lambda self: self.classification_model.needs_graph)
    needs_heatmaps = property(lambda self: False)
    needs_confidence = property(lambda self: self.classification_model.needs_confidence)

    @classmethod
    def get_available_models(cls) -> Dict[str, Dict[str, torch.nn.Module]]:
        return {'classification': {'LSTM': LSTM, 'GRU': GRU}}

    @classmethod
    def get_default_models(cls) -> Dict[str, torch.nn.Module]:
        return {'classification': LSTM}

    @staticmethod
    def add_model_specific_args(parent_parser):
        parser = parent_parser.add_argument_group('Classification Module')
        parser.add_argument('--classification_average', type=str, choices=list(AVERAGES) + ['benchmark'], default='macro')
        return parent_parser

    def configure_optimizers(self):
        """The model's own configuration (reference classification.py:221-222), as the one-element list the trainer takes."""
        return [self.classification_model.configure_optimizers()]

    def get_initial_metrics(self):
        return {}

    def get_metrics(self):
        """Names of the registered metrics and their averages (the values come from ``compute_metrics``)."""
        rank = {'AUROC': 'macro', 'ROCCurve': None, 'PRCurve': None} if self._rank_on else {}
        return {'ConfusionMatrix': None, **self._average, **rank}

    sample_curve = staticmethod(sample_curve)

    # ---- hooks the trainer calls -----------------------------------------------------------------------------------
    def on_train_batch_start(self, batch, batch_idx, *args, **kwargs):
        pass

    def on_validation_batch_start(self, batch, batch_idx, *args, **kwargs):
        pass

    def on_test_batch_start(self, batch, batch_idx, *args, **kwargs):
        pass

    def training_step(self, batch, batch_idx):
        return self._step(batch, batch_idx, 'train')

    def validation_step(self, batch, batch_idx):
        return self._rank_accumulate(self._step(batch, batch_idx, 'val'))

    def test_step(self, batch, batch_idx):
        return self._rank_accumulate(self._step(batch, batch_idx, 'test'))

    def _rank_accumulate(self, outputs):
        """Append an evaluation step's scores and targets to the epoch buffer (one launch; no host sync)."""
        if not self._rank_on:
            return outputs
        from pedestrians_video_2_carla_amd import ops
        logits = outputs['preds'][self._outputs_key]
        target = torch.atleast_1d(outputs['targets'][self._targets_key]).reshape(-1)
        B, C = target.shape[0], 1 if self._binary else logits.shape[-1]
        if B == 0:
            return outputs
        need = self._rank_rows + B
        if self._rank_scores is None or self._rank_scores.device != logits.device or self._rank_scores.shape[1] != C:
            cap = max(int(self.rank_initial_capacity), 1)
            while cap < B:
                cap *= 2
            self._rank_scores = torch.empty(cap, C, dtype=torch.float32, device=logits.device)
            self._rank_targets = torch.empty(cap, dtype=torch.int32, device=logits.device)
            self._rank_rows, need = 0, B
        elif need > self._rank_targets.shape[0]:
            cap = self._rank_targets.shape[0]
            while cap < need:
                cap *= 2
            scores = torch.empty(cap, C, dtype=torch.float32, device=logits.device)
            targets = torch.empty(cap, dtype=torch.int32, device=logits.device)
            scores[:self._rank_rows] = self._rank_scores[:self._rank_rows]
            targets[:self._rank_rows] = self._rank_targets[:self._rank_rows]
            self._rank_scores, self._rank_targets = scores, targets
        ops.rank_scores(logits, target, self._rank_scores, self._rank_targets, self._rank_rows, binary=self._binary)
        self._rank_rows = need
        return outputs

    def _rank_gather(self, sync: bool):
        """The epoch's (scores, targets), of all ranks when ``sync``: the ranks hold different numbers of rows, so the counts
        are gathered first, then the rows padded to the largest count, and the padding trimmed. None when nobody has a row."""
        rows = self._rank_rows
        C = 1 if self._binary else self._num_classes
        dev = self._rank_scores.device if self._rank_scores is not None else self.confusion.device
        scores = self._rank_scores[:rows] if rows else torch.empty(0, C, dtype=torch.float32, device=dev)
        targets = self._rank_targets[:rows] if rows else torch.empty(0, dtype=torch.int32, device=dev)
        if sync and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            world = dist.get_world_size()
            counts = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world)]
            dist.all_gather(counts, torch.tensor([rows], dtype=torch.int64, device=dev))
            counts = [int(c) for c in counts]
            most = max(counts)
            if most == 0:
                return None
            ps, pt = torch.zeros(most, C, dtype=torch.float32, device=dev), torch.full((most,), -1, dtype=torch.int32, device=dev)
            ps[:rows], pt[:rows] = scores, targets
            all_s, all_t = [torch.empty_like(ps) for _ in range(world)], [torch.empty_like(pt) for _ in range(world)]
            dist.all_gather(all_s, ps)
            dist.all_gather(all_t, pt)
            scores = torch.cat([v[:n] for v, n in zip(all_s, counts)])
            targets = torch.cat([v[:n] for v, n in zip(all_t, counts)])
        return (scores, targets) if targets.shape[0] else None

    def compute_metrics(self, reset: bool = True, sync: bool = True) -> Dict[str, Any]:
        """End of an epoch: the metrics of everything counted since the last reset (module docstring); ``sync`` all-reduces the
        matrix over the ranks first. Arrays ('none' with more than two classes, the matrix) come back as lists. When evaluation
        steps accumulated scores, 'AUROC' (a float), 'ROCCurve' and 'PRCurve' (tuples of numpy arrays -- a curve has up to one
        point per row) are added; ``sync`` gathers the ranks' rows first, ``reset`` empties the epoch buffer."""
        if sync and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.confusion, op=dist.ReduceOp.SUM)
        matrix = self.confusion.cpu().numpy().astype(np.int64)
        if reset:
            self.confusion.zero_()
        out = {'ConfusionMatrix': matrix.tolist()}
        for k, v in classification_metrics(matrix, self._average).items():
            out[k] = v.tolist() if isinstance(v, np.ndarray) else v
        if self._rank_on:
            from pedestrians_video_2_carla_amd import ops
            epoch = self._rank_gather(sync)
            if reset:
                self._rank_rows = 0
            if epoch is not None:
                out.update(rank_metrics(ops.rank_curves(*epoch), self._binary))
        return out

    def check_finite(self, stage: str = 'train'):
        """Deferred NaN guard: one host sync for all logged losses of ``stage``; raises like the reference would."""
        bad = [k for k, v in getattr(self, 'logged', {}).items()
               if k.startswith(stage + '_loss/') and isinstance(v, torch.Tensor) and not bool(torch.isfinite(v))]
        if bad:
            raise RuntimeError("Couldn't calculate any loss. Non-finite: {}".format(bad))

    # ---- the step ---------------------------------------------------------------------------------------------------
    def _unwrap_batch(self, batch):
        if isinstance(batch, (tuple, list)):
            return (*batch, None, None)
        raise TypeError('graph batches (torch_geometric) are outside this flow')

    def forward(self, batch, *args, **kwargs):
        (frames, targets, meta, edge_index, batch_vector) = self._unwrap_batch(batch)
        return self._inner_step(frames, targets, edge_index, batch_vector), meta

    def _step(self, batch, batch_idx, stage):
        (frames, targets, meta, edge_index, batch_vector) = self._unwrap_batch(batch)
        sliced = self._inner_step(frames, targets, edge_index, batch_vector)
        loss_dict = self._calculate_lossess(stage, len(frames), sliced, meta)
        return self._get_outputs(stage, len(frames), sliced, meta, loss_dict)

    def _inner_step(self, frames, targets, edge_index=None, batch_vector=None):
        out = self.classification_model(frames, edge_index, batch_vector)
        target = targets[self._targets_key]
        if out.ndim - 1 != target.ndim:
            target = target.squeeze(-1)
        return {'inputs': frames, self._outputs_key: out, 'targets': {**targets, self._targets_key: target}}

    def _calculate_lossess(self, stage, batch_size, sliced, meta):
        from pedestrians_video_2_carla_amd import ops
        logits, target = sliced[self._outputs_key], torch.atleast_1d(sliced['targets'][self._targets_key])
        loss = ops.classification_loss(logits, target, confusion=self.confusion, binary=self._binary)
        loss_dict = {self.criterion.__class__.__name__: loss}
        for k, v in loss_dict.items():
            self.log('{}_loss/{}'.format(stage, k), v, batch_size=batch_size)
        return loss_dict

    def _get_outputs(self, stage, batch_size, sliced, meta, loss_dict):
        name = self.criterion.__class__.__name__
        if name in loss_dict:
            loss = loss_dict[name]
            self.log('{}_loss/primary'.format(stage), loss, batch_size=batch_size)
            return {'loss': loss, 'preds': {self._outputs_key: sliced[self._outputs_key].detach()}, 'targets': sliced['targets']}
        raise RuntimeError("Couldn't calculate any loss.")
