"""LSTM movements model (reference modules/movements/lstm.py:5-83): Linear (optional embedding) + nn.LSTM(batch_first) + Linear.

Submodule names (``linear_1``, ``lstm_1``, ``linear_2``) match the reference's, so its state_dicts load with identical keys;
without ``embeddings_size`` ``linear_1`` is an ``nn.Identity`` (the reference's ``lambda x: x``: no parameters either way).

On the GPU in fp32 (outside autocast) the two linears run as the build's dense kernels (K16 / K12) and every LSTM layer as
``ops.lstm_layer`` through Seq2Seq's layer loop ``_run_stack``: the recurrence is K7b in one launch for hidden sizes 16 / 32 / 48 /
64 / 96 / 128 and K18 (one launch per time step) for any other width up to 1024. Wider stacks, host tensors, other dtypes and
autocast run ``self.lstm_1`` itself (wider stacks with a once-per-shape RuntimeWarning).
"""
import torch
from torch import nn

from pedestrians_video_2_carla_amd.modules.movements.movements import MovementsModel, MovementsModelOutputTypeMixin


class LSTM(MovementsModelOutputTypeMixin, MovementsModel):
    """Very basic Linear + LSTM + Linear model."""

    def __init__(self, hidden_size: int = 64, num_layers: int = 2, embeddings_size: int = None, **kwargs):
        super().__init__(**kwargs)
        self._input_size = len(self.input_nodes) * 2          # (x, y) points
        self._output_nodes_len = len(self.output_nodes)
        self._output_size = self._output_nodes_len * self.output_features
        self._embeddings_size = embeddings_size if embeddings_size else self._input_size
        self.linear_1 = nn.Linear(self._input_size, embeddings_size) if embeddings_size else nn.Identity()
        self.lstm_1 = nn.LSTM(input_size=self._embeddings_size, hidden_size=hidden_size, num_layers=num_layers, batch_first=True)
        self.linear_2 = nn.Linear(hidden_size, self._output_size)
        self._hparams.update({'hidden_size': hidden_size, 'num_layers': num_layers, 'embeddings_size': embeddings_size})

    @staticmethod
    def add_model_specific_args(parent_parser):
        parent_parser = MovementsModel.add_model_specific_args(parent_parser)
        parser = parent_parser.add_argument_group('LSTM Movements Model')
        parser = MovementsModelOutputTypeMixin.add_cli_args(parser)
        parser.add_argument('--embeddings_size', default=None, type=int)
        parser.add_argument('--num_layers', default=2, type=int)
        parser.add_argument('--hidden_size', default=64, type=int)
        return parent_parser

    def _hip_path(self, x: torch.Tensor) -> bool:
        from pedestrians_video_2_carla_amd import ops
        from pedestrians_video_2_carla_amd.modules.movements.seq2seq.seq2seq import _warn_fallback
        if not (x.is_cuda and x.dtype == torch.float32 and not torch.is_autocast_enabled()):
            return False
        H = self.lstm_1.hidden_size
        if ops.lstm_supported(H) or ops.lstm_steps_supported(H):
            return True
        _warn_fallback(self.lstm_1, who='LSTM', covers='any hidden size up to 1024')
        return False

    def forward(self, x, *args, **kwargs):
        original_shape = x.shape
        B, T = original_shape[0:2]
        x = x.reshape(B, T, self._input_size)
        if self._hip_path(x):
            from pedestrians_video_2_carla_amd import ops
            from pedestrians_video_2_carla_amd.modules.movements.seq2seq.seq2seq import _run_stack
            xt = x.transpose(0, 1).reshape(T * B, self._input_size)             # time-major rows
            if isinstance(self.linear_1, nn.Linear):
                xt = ops.dense(xt, self.linear_1.weight, self.linear_1.bias)
            y, _, _ = _run_stack(self.lstm_1, xt.view(T, B, self._embeddings_size))
            out = ops.dense(y.reshape(T * B, -1), self.linear_2.weight, self.linear_2.bias).view(T, B, self._output_size)
            out = out.transpose(0, 1)
        else:
            x = self.linear_1(x)
            x, _ = self.lstm_1(x)
            out = self.linear_2(x)
        out = out.reshape(B, T, self._output_nodes_len, self.output_features)
        return self._format_output(out)
