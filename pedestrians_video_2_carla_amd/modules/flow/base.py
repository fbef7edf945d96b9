"""``LitBaseFlow``: loss-mode resolution and the train/val/test step control flow.

Mirrors reference modules/flow/base.py:33-510 for the parts on the hot path:
  __init__ (43-110)           loss_modes -> ordered ``_losses_to_calculate`` (requirements first), outputs key
  _unwrap_batch (231-246)     (frames, targets, meta) -> + (None, None)
  _step (397-410)             _inner_step -> _calculate_lossess -> detach -> _get_outputs
  _calculate_lossess (440-469), _get_outputs (415-438), configure_optimizers (153-163), Lightning hook names.

Differences, all about host synchronisation:
  * the reference tests ``torch.isnan(loss)`` after every loss (base.py:461) -- three device->host syncs per step.
    Here a NaN/inf loss is dropped only when ``strict_nan_check=True`` (reference behaviour, syncs); by default the value
    is kept on device and ``check_finite()`` can be called every N steps.
  * ``self.log`` receives device tensors; nothing calls ``.item()`` inside the step.
W&B is out of scope; validation metrics are device metrics (``get_metrics``). ``_log_videos`` forwards the
validation / test tensors to the trainer's ``PedestrianLogger`` (loggers/pedestrian) and does nothing without one.
"""
import platform
from types import FunctionType
from typing import Any, Dict, List, Tuple, Union

import torch
from torch import Tensor

from pedestrians_video_2_carla_amd.data.base.base_transforms import BaseTransforms
from pedestrians_video_2_carla_amd.loss import LossModes
from pedestrians_video_2_carla_amd.modules.flow.lightning_shim import LightningModuleBase
from pedestrians_video_2_carla_amd.modules.flow.output_types import (MovementsModelOutputType,
                                                                   TrajectoryModelOutputType)
from pedestrians_video_2_carla_amd.modules.movements.zero import ZeroMovements
from pedestrians_video_2_carla_amd.modules.trajectory.zero import ZeroTrajectory


class LitBaseFlow(LightningModuleBase):
    def __init__(self,
                 movements_model=None,
                 trajectory_model=None,
                 loss_modes: List[Union[LossModes, str]] = None,
                 loss_weights: Dict[str, Tensor] = None,
                 mask_missing_joints: bool = True,
                 strict_nan_check: bool = False,
                 **kwargs):
        super().__init__()
        self.movements_model = movements_model if movements_model is not None else ZeroMovements(**kwargs)
        self.trajectory_model = trajectory_model if trajectory_model is not None else ZeroTrajectory(**kwargs)
        self.mask_missing_joints = mask_missing_joints
        self.strict_nan_check = strict_nan_check
        self.loss_weights = loss_weights if loss_weights is not None else {}

        if loss_modes is None or len(loss_modes) == 0:
            loss_modes = [LossModes.loc_2d]
        self._loss_modes = [LossModes[lm] if isinstance(lm, str) else lm for lm in loss_modes]

        ordered = []
        for mode in self._loss_modes:            # requirements first, then the mode itself (base.py:76-81)
            if len(mode.value) > 2:
                ordered.extend(LossModes[k] for k in mode.value[2])
            ordered.append(mode)
        self._losses_to_calculate = []
        for mode in dict.fromkeys(ordered):
            fn, criterion, *rest = mode.value
            reqs = rest[0] if rest else tuple()
            if isinstance(fn, FunctionType):
                self._losses_to_calculate.append((mode.name, fn, criterion, reqs))
            else:                                # class-style loss: instantiate once (base.py:85-91)
                self._losses_to_calculate.append((mode.name, fn(
                    criterion=criterion, input_nodes=self.movements_model.input_nodes,
                    output_nodes=self.movements_model.output_nodes, mask_missing_joints=self.mask_missing_joints,
                    loss_params=kwargs.get('loss_params', [])), None, reqs))

        transform = kwargs.get('transform', BaseTransforms.hips_neck)
        if isinstance(transform, str):
            transform = BaseTransforms[transform.lower()]
        self._outputs_key = 'projection_2d_transformed' if transform != BaseTransforms.none else 'projection_2d'
        self._crucial_keys = self._get_crucial_keys()

        self.save_hyperparameters({
            'host': platform.node(),
            'loss_modes': [mode.name for mode in self._loss_modes],
            'loss_weights': self.loss_weights,
            **self.movements_model.hparams,
            **self.trajectory_model.hparams,
        })

    # ---- registry / introspection ----------------------------------------------------------------------------------
    def _get_crucial_keys(self):
        return [self._outputs_key]

    @property
    def outputs_key(self) -> str:
        return self._outputs_key

    @property
    def crucial_keys(self) -> List[str]:
        return self._crucial_keys.copy()

    @classmethod
    def get_available_models(cls) -> Dict[str, Dict[str, torch.nn.Module]]:
        return {}

    @classmethod
    def get_default_models(cls) -> Dict[str, torch.nn.Module]:
        return {}

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path: str, map_location=None, **kwargs):
        """Lightning's ``load_from_checkpoint``: the flow of the file's ``hyper_parameters`` (keyword arguments win) with its
        ``state_dict`` loaded; see ``checkpoint.load_from_checkpoint``."""
        from pedestrians_video_2_carla_amd import checkpoint
        return checkpoint.load_from_checkpoint(cls, checkpoint_path, map_location=map_location, **kwargs)

    def get_metrics(self):
        """Metrics updated on every validation / test batch (reference base.py:146-151). The flows return device metrics
        (``pedestrians_video_2_carla_amd.metrics``): one HIP launch per update, host sync only in ``compute()``."""
        return {}

    @property
    def metrics(self):
        if getattr(self, '_metrics', None) is None:
            self._metrics = dict(self.get_metrics())
        return self._metrics

    def _update_metrics(self, outputs):
        """base.py:472-473 ``self.metrics(outputs['preds'], outputs['targets'])`` -- update only, nothing is read back."""
        preds = {k: v for k, v in outputs['preds'].items() if v is not None}
        for metric in self.metrics.values():
            metric.update(preds, outputs['targets'])

    def compute_metrics(self, reset: bool = True, sync: bool = True):
        """End of a validation / test epoch: {name: value}; ``sync`` all-reduces the device states over the ranks first."""
        out = {}
        for name, metric in self.metrics.items():
            if sync:
                metric.sync()
            if metric._state is not None and float(metric._state.abs().sum()) > 0:
                out[name] = float(metric.compute())
            if reset:
                metric.reset()
        return out

    def get_initial_metrics(self):
        return {}

    needs_graph = property(lambda self: self.movements_model.needs_graph)
    needs_heatmaps = property(lambda self: getattr(self.movements_model, 'needs_heatmaps', False))
    needs_confidence = property(lambda self: getattr(self.movements_model, 'needs_confidence', False))

    def configure_optimizers(self):
        configs = [self.movements_model.configure_optimizers(), self.trajectory_model.configure_optimizers()]
        return [c for c in configs if 'optimizer' in c]

    @staticmethod
    def add_model_specific_args(parent_parser):
        group = parent_parser.add_argument_group('BaseFlow Module')
        group.add_argument('--mask_missing_joints', type=lambda v: str(v).lower() in ('1', 'true', 'yes'), default=True)
        group.add_argument('--loss_modes', metavar='MODE', default=[], choices=list(LossModes), nargs='+',
                           action='extend', type=LossModes.__getitem__,
                           help='Loss modes in preferred order; choices: {}'.format(set(LossModes.__members__)))
        return parent_parser

    # ---- hooks ------------------------------------------------------------------------------------------------------
    def _on_batch_start(self, batch, batch_idx):
        pass

    def on_train_batch_start(self, batch, batch_idx, *args, **kwargs):
        self._on_batch_start(batch, batch_idx)

    def on_validation_batch_start(self, batch, batch_idx, *args, **kwargs):
        self._on_batch_start(batch, batch_idx)

    def on_test_batch_start(self, batch, batch_idx, *args, **kwargs):
        self._on_batch_start(batch, batch_idx)

    def predict_step(self, batch, batch_idx):
        self._on_batch_start(batch, batch_idx)
        return self(batch)

    def training_step(self, batch, batch_idx):
        return self._step(batch, batch_idx, 'train')

    def validation_step(self, batch, batch_idx):
        out = self._step(batch, batch_idx, 'val')
        self._update_metrics(out)
        return out

    def test_step(self, batch, batch_idx):
        out = self._step(batch, batch_idx, 'test')
        self._update_metrics(out)
        return out

    # ---- the step ---------------------------------------------------------------------------------------------------
    def _unwrap_batch(self, batch):
        if isinstance(batch, (tuple, list)):
            return (*batch, None, None)
        raise TypeError('graph batches (torch_geometric) are outside the hot path')

    def forward(self, batch, *args, **kwargs) -> Any:
        (frames, targets, meta, edge_index, batch_vector) = self._unwrap_batch(batch)
        return self._inner_step(frames, targets, edge_index, batch_vector, stage='predict'), meta

    def _step(self, batch, batch_idx, stage):
        (frames, targets, meta, edge_index, batch_vector) = self._unwrap_batch(batch)
        sliced = self._inner_step(frames, targets, edge_index, batch_vector, stage=stage)
        loss_dict = self._calculate_lossess(stage, len(frames), sliced, meta)
        # nothing below needs gradients (base.py:403-406)
        sliced = {k: v.detach() if isinstance(v, torch.Tensor) else v for k, v in sliced.items()}
        self._log_videos(meta=meta, batch_idx=batch_idx, stage=stage, **sliced)
        return self._get_outputs(stage, len(frames), sliced, loss_dict)

    def _inner_step(self, frames, targets, edge_index, batch_vector, stage='train'):
        raise NotImplementedError()

    def _loss_is_usable(self, loss) -> bool:
        if loss is None:
            return False
        if self.strict_nan_check:
            return not bool(torch.isnan(loss))     # host sync, reference behaviour (base.py:461)
        return True

    def _calculate_lossess(self, stage, batch_size, sliced, meta):
        loss_dict = {}
        for (name, loss_fn, criterion, reqs) in self._losses_to_calculate:
            loss = loss_fn(
                criterion=criterion,
                input_nodes=self.movements_model.input_nodes,
                output_nodes=self.movements_model.output_nodes,
                mask_missing_joints=self.mask_missing_joints,
                requirements={k: v for k, v in loss_dict.items() if k in reqs},
                loss_weights=self.loss_weights,
                **sliced)
            if self._loss_is_usable(loss):
                loss_dict[name] = loss
                if LossModes[name] in self._loss_modes:
                    break            # stop after the first requested loss that could be calculated (base.py:464-465)
        for k, v in loss_dict.items():
            self.log('{}_loss/{}'.format(stage, k), v, batch_size=batch_size)
        return loss_dict

    def _get_outputs(self, stage, batch_size, sliced, loss_dict):
        for mode in self._loss_modes:
            if mode.name in loss_dict:
                self.log('{}_loss/primary'.format(stage), loss_dict[mode.name], batch_size=batch_size)
                mt, tt = self.movements_model.output_type, self.trajectory_model.output_type
                changes = tt == TrajectoryModelOutputType.changes
                return {
                    'loss': loss_dict[mode.name],
                    'preds': {
                        'pose_changes': sliced.get('pose_inputs') if mt == MovementsModelOutputType.pose_changes else None,
                        'world_rot_changes': sliced.get('world_rot_inputs') if changes else None,
                        'world_loc_changes': sliced.get('world_loc_inputs') if changes else None,
                        **{k: sliced.get(k) for k in self._crucial_keys},
                    },
                    'targets': sliced['targets'],
                }
        raise RuntimeError("Couldn't calculate any loss.")

    def check_finite(self, stage: str = 'train'):
        """Deferred NaN guard: one host sync for all logged losses of ``stage``; raises like the reference would."""
        bad = [k for k, v in getattr(self, 'logged', {}).items()
               if k.startswith(stage + '_loss/') and isinstance(v, torch.Tensor) and not bool(torch.isfinite(v))]
        if bad:
            raise RuntimeError("Couldn't calculate any loss. Non-finite: {}".format(bad))

    def _log_videos(self, meta=None, batch_idx=0, stage='train', **sliced):
        """Validation and test steps hand their (already materialised) tensors to every ``PedestrianLogger`` of the trainer; the
        writer's interval gate decides. Stage ``train`` stays a no-op here: the lean train step returns no projection and a
        replayed graph runs no Python -- ``Trainer.fit`` logs training clips from one extra eval-mode forward instead."""
        if stage not in ('val', 'test'):
            return
        trainer = getattr(self, 'trainer', None)
        loggers = getattr(trainer, 'loggers', None)
        if not loggers:
            return
        from pedestrians_video_2_carla_amd.loggers.pedestrian import PedestrianLogger
        for logger in loggers:
            if isinstance(logger, PedestrianLogger):
                logger.experiment.log_videos(meta=meta, step=trainer.global_step, batch_idx=batch_idx, stage=stage,
                                             inputs=sliced.get('inputs'), targets=sliced.get('targets'),
                                             projection_2d=sliced.get('projection_2d'),
                                             projection_2d_transformed=sliced.get('projection_2d_transformed'))
