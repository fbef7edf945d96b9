"""GRU classifier (reference modules/classification/gru.py:9-95): Linear + nn.GRU(batch_first) + Linear on the last step.
See ``classification.py`` for the layout, the dropout that applies nothing and the device path."""
from torch import nn

from pedestrians_video_2_carla_amd.modules.classification.classification import RecurrentClassifier


class GRU(RecurrentClassifier):
    """Very basic Linear + GRU + Linear model."""
    rnn_type = nn.GRU
    rnn_name = 'gru_1'

    def _last_hidden(self, x):
        from pedestrians_video_2_carla_amd import ops
        rnn, hT = self.gru_1, None
        for k in range(rnn.num_layers):                  # nn.GRU's layer loop on K23 (zero initial state, no inter-layer dropout)
            x, hT = ops.gru_layer(x, None, getattr(rnn, f'weight_ih_l{k}'), getattr(rnn, f'weight_hh_l{k}'),
                                  getattr(rnn, f'bias_ih_l{k}', None) if rnn.bias else None,
                                  getattr(rnn, f'bias_hh_l{k}', None) if rnn.bias else None)
        return hT
