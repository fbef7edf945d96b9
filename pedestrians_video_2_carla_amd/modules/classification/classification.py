"""``ClassificationModel``: the plugin base of the classification flow (reference modules/classification/classification.py:5-19)
and the recurrent classifier LSTM and GRU share (reference modules/classification/lstm.py, gru.py).

Both classifiers are Linear (optional embedding) -> recurrent stack (batch_first) -> Linear on the LAST time step. Submodule
names (``linear_1``, ``lstm_1`` / ``gru_1``, ``linear_2``, ``dropout``) match the reference's, so its state_dicts load with
identical keys; without ``embeddings_size`` ``linear_1`` is an ``nn.Identity`` (the reference's ``lambda x: x``).

Dropout applies NOTHING: the reference calls ``self.dropout(x)`` twice and discards the result both times (lstm.py:89,92), so
``p_dropout`` never changes an output. The module and the hyper-parameter are kept (checkpoints, CLI); the discarded calls --
and the random numbers they would draw -- are not reproduced, so train() and eval() outputs are equal.

Only ``out[:, -1, :]`` is returned, so ``linear_2`` runs on the last step's (B, H) alone, i.e. on ``hT`` of the top layer, and
the top layer's recurrence receives ``g_hT`` and no ``g_out`` in the backward.

On the GPU in fp32 (outside autocast) the linears run as the build's dense kernels (K16 / K12) and the layers as
``ops.lstm_layer`` (K7b / K18, through Seq2Seq's ``_run_stack``) or ``ops.gru_layer`` (K23). Host tensors, other dtypes, autocast
and ``P2C_CLS_FRAMEWORK=1`` run the ``nn`` modules; so does a hidden size above 1024, with a once-per-shape RuntimeWarning.
"""
import warnings

import torch
from torch import nn

from pedestrians_video_2_carla_amd.modules.flow.base_model import BaseModel
from pedestrians_video_2_carla_amd.modules.flow.output_types import ClassificationModelOutputType


class ClassificationModel(BaseModel):
    def __init__(self, num_classes: int = 2, **kwargs):
        self.num_classes = num_classes
        super().__init__(prefix='classification', **kwargs)

    @property
    def output_type(self):
        return ClassificationModelOutputType.multiclass

    @staticmethod
    def add_model_specific_args(parent_parser):
        return BaseModel.add_model_specific_args(parent_parser, prefix='classification')


class RecurrentClassifier(ClassificationModel):
    """Linear + ``rnn_type`` stack + Linear on the last step; ``rnn_name`` is the attribute the stack is registered under."""
    rnn_type = None
    rnn_name = None

    def __init__(self, hidden_size: int = 64, num_layers: int = 2, embeddings_size: int = None, p_dropout: float = 0.25,
                 input_features: int = 2, **kwargs):
        super().__init__(**kwargs)
        if self.input_nodes is None:                                        # (the reference's GRU defaults to the CARLA skeleton)
            from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
            self.input_nodes = CARLA_SKELETON
        self._input_size = len(self.input_nodes) * input_features          # (x, y) points
        self._embeddings_size = embeddings_size if embeddings_size else self._input_size
        self.linear_1 = nn.Linear(self._input_size, embeddings_size) if embeddings_size else nn.Identity()
        setattr(self, self.rnn_name, self.rnn_type(input_size=self._embeddings_size, hidden_size=hidden_size,
                                                   num_layers=num_layers, batch_first=True))
        self.linear_2 = nn.Linear(hidden_size, self.num_classes)
        self.dropout = nn.Dropout(p_dropout)                                # kept, never applied (module docstring)
        self._hparams.update({'hidden_size': hidden_size, 'num_layers': num_layers, 'embeddings_size': embeddings_size,
                              'p_dropout': p_dropout})

    @classmethod
    def add_model_specific_args(cls, parent_parser):
        ClassificationModel.add_model_specific_args(parent_parser)
        parser = parent_parser.add_argument_group(f'{cls.__name__} Classification Model')
        parser.add_argument('--embeddings_size', default=None, type=int)
        parser.add_argument('--num_layers', default=2, type=int)
        parser.add_argument('--hidden_size', default=64, type=int)
        parser.add_argument('--p_dropout', default=0.25, type=float)
        return parent_parser

    @property
    def rnn(self):
        return getattr(self, self.rnn_name)

    def _hip_path(self, x: torch.Tensor) -> bool:
        from pedestrians_video_2_carla_amd import ops
        from pedestrians_video_2_carla_amd.modules.movements.seq2seq import seq2seq as s2s
        if not (x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled()) or ops.cls_framework():
            return False
        H = self.rnn.hidden_size
        if 1 <= H <= 1024:
            return True
        key = ('classification', type(self).__name__, H)
        if key not in s2s._WARNED:
            s2s._WARNED.add(key)
            warnings.warn(f'classification {type(self).__name__}: nn.{self.rnn_type.__name__}(hidden_size={H}) is outside the HIP '
                          f'recurrence (any hidden size up to 1024): this stack runs on the framework RNN path, roughly an '
                          f'order of magnitude slower per step', RuntimeWarning, stacklevel=3)
        return False

    def _last_hidden(self, x: torch.Tensor) -> torch.Tensor:
        """x (T, B, E) time-major on the device -> hT (B, H) of the top layer, on the HIP recurrences."""
        raise NotImplementedError()

    def forward(self, x, *args, **kwargs):
        B, T = x.shape[0:2]
        x = x.reshape(B, T, self._input_size)
        if self._hip_path(x):
            from pedestrians_video_2_carla_amd import ops
            xt = x.transpose(0, 1).reshape(T * B, self._input_size)             # time-major rows
            if isinstance(self.linear_1, nn.Linear):
                xt = ops.dense(xt, self.linear_1.weight, self.linear_1.bias)
            last = self._last_hidden(xt.view(T, B, self._embeddings_size))
            return ops.dense(last, self.linear_2.weight, self.linear_2.bias)
        x = self.linear_1(x)
        x, _ = self.rnn(x)
        return self.linear_2(x[:, -1, :])
