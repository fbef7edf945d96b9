"""``ModelCheckpoint``: keep the best ``save_top_k`` checkpoints by a monitored validation value (the reference builds Lightning's
with ``monitor='val_loss/primary', mode='min', save_top_k=1``, modeling.py:240-245).

A callback of ``Trainer`` is any object with optional ``on_validation_end(trainer, flow, monitors)`` and
``on_fit_end(trainer, flow)``; nothing wider. The trainer calls ``on_validation_end`` after the epoch's validation AND after the
epoch-interval LR schedulers stepped, so a file written here holds the scheduler state the next epoch starts from.
"""
import math
import os
from typing import Any, Dict, Optional


class ModelCheckpoint:
    def __init__(self, dirpath: str, monitor: Optional[str] = 'val_loss/primary', mode: str = 'min', save_top_k: int = 1,
                 save_last: bool = False, filename: str = 'epoch={epoch}-step={step}'):
        if mode not in ('min', 'max'):
            raise ValueError(f"mode must be 'min' or 'max', not {mode!r}")
        if save_top_k < -1:
            raise ValueError(f'save_top_k must be -1 (all), 0 (none) or positive, not {save_top_k!r}')
        self.dirpath, self.monitor, self.mode = dirpath, monitor, mode
        self.save_top_k, self.save_last, self.filename = int(save_top_k), bool(save_last), filename
        self.best_k_models: Dict[str, float] = {}
        self.kth_best_model_path = ''
        self.best_model_path = ''
        self.best_model_score: Optional[float] = None
        self.last_model_path = ''

    # ---- bookkeeping ---------------------------------------------------------------------------------------------------------
    def _better(self, a: float, b: float) -> bool:
        return a < b if self.mode == 'min' else a > b

    def _worst(self) -> str:
        pick = max if self.mode == 'min' else min
        return pick(self.best_k_models, key=self.best_k_models.get)      # ties: the one that came first

    def _best(self) -> str:
        pick = min if self.mode == 'min' else max
        return pick(self.best_k_models, key=self.best_k_models.get)

    def check_monitor_top_k(self, current: float) -> bool:
        """Would a checkpoint with this score be kept? A tie with the worst kept one is NOT better: the older file stays."""
        if self.save_top_k == 0:
            return False
        if self.save_top_k == -1 or len(self.best_k_models) < self.save_top_k:
            return True
        return self._better(current, self.best_k_models[self._worst()])

    def format_path(self, epoch: int, step: int) -> str:
        base = os.path.join(self.dirpath, self.filename.format(epoch=epoch, step=step))
        path, version = base + '.ckpt', 0
        while path in self.best_k_models or (os.path.exists(path) and path != self.last_model_path):
            version += 1
            path = f'{base}-v{version}.ckpt'
        return path

    def update(self, current: float, path: str) -> Optional[str]:
        """Book ``path`` with score ``current``; returns the path that dropped out of the top k (to be deleted), if any."""
        dropped = None
        if self.save_top_k > 0 and len(self.best_k_models) >= self.save_top_k:
            dropped = self._worst()
            del self.best_k_models[dropped]
        self.best_k_models[path] = current
        self.kth_best_model_path = self._worst()
        self.best_model_path = self._best()
        self.best_model_score = self.best_k_models[self.best_model_path]
        return dropped

    # ---- hooks ---------------------------------------------------------------------------------------------------------------
    def on_validation_end(self, trainer, flow, monitors: Dict[str, float]) -> None:
        if self.monitor is not None and self.monitor not in monitors:
            raise KeyError(f'ModelCheckpoint(monitor={self.monitor!r}): not among the validation monitors {sorted(monitors)}')
        epoch, step = trainer.current_epoch - 1, trainer.global_step         # the epoch that just ended, counted from 0
        current = float(monitors[self.monitor]) if self.monitor is not None else float(step)
        if math.isfinite(current) and self.check_monitor_top_k(current):
            path = self.format_path(epoch, step)
            dropped = self.update(current, path)
            trainer.save_checkpoint(path)                  # (holds this callback's state: booked first)
            if dropped is not None and dropped != path:
                self._remove(dropped)
        if self.save_last:
            last = os.path.join(self.dirpath, 'last.ckpt')
            self.last_model_path = last
            trainer.save_checkpoint(last)

    @staticmethod
    def _remove(path: str) -> None:
        from pedestrians_video_2_carla_amd.checkpoint import _rank
        if _rank() == 0 and os.path.exists(path):
            os.remove(path)

    # ---- state, under the ``callbacks`` key of a checkpoint ---------------------------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        return {'monitor': self.monitor, 'best_model_score': self.best_model_score, 'best_model_path': self.best_model_path,
                'best_k_models': dict(self.best_k_models), 'kth_best_model_path': self.kth_best_model_path,
                'last_model_path': self.last_model_path, 'dirpath': self.dirpath}

    def load_state_dict(self, state: Dict[str, Any]) -> None:
        self.best_model_score = state.get('best_model_score')
        self.best_model_path = state.get('best_model_path', '')
        self.last_model_path = state.get('last_model_path', '')
        if state.get('dirpath') == self.dirpath:          # (another directory: its files are not this callback's to delete)
            self.best_k_models = dict(state.get('best_k_models', {}))
            self.kth_best_model_path = state.get('kth_best_model_path', '')
