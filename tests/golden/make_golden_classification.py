#!/usr/bin/env python3
"""Generate tests/golden/model_cls_*.npz by RUNNING THE REFERENCE's own LSTM and GRU classifiers (build container only).

The reference imports under the third-party stand-ins of make_golden.py (``install_standins``); its
modules/classification/lstm.py and gru.py run unmodified. Each fixture holds the input frames, the state_dict (``sd__*``), the
output (B, num_classes), a fixed random ``g_out`` and the parameter gradients (``grad__*``, in ``<name>_grads.npz``) of
``(out * g_out).sum()``:

  model_cls_gru_default.npz     GRU defaults: H = 64, L = 2, CARLA, num_classes = 2, B = 4, T = 16
  model_cls_gru_body25_emb.npz  GRU, BODY_25 input, embeddings_size = 32, H = 100, L = 3, num_classes = 5, B = 4, T = 4
  model_cls_gru_h191.npz        GRU, H = 191, L = 1, B = 4, T = 15
  model_cls_lstm_default.npz    LSTM defaults: H = 64, L = 2, CARLA, num_classes = 2, B = 4, T = 16

The models train() with p_dropout = 0.25: the reference discards what its dropout returns, so the outputs do not depend on it.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF_SRC, install_standins, npz  # noqa: E402


def main():
    if not os.path.isdir(REF_SRC):
        sys.exit('reference tree not present: the committed .npz files are the artefact to use')
    install_standins()
    sys.path.insert(0, REF_SRC)
    from pedestrians_video_2_carla.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla.data.openpose.skeleton import BODY_25_SKELETON
    from pedestrians_video_2_carla.modules.classification.gru import GRU
    from pedestrians_video_2_carla.modules.classification.lstm import LSTM
    for name, cls, nodes, B, T, kw in (
            ('model_cls_gru_default', GRU, CARLA_SKELETON, 4, 16, {}),
            ('model_cls_gru_body25_emb', GRU, BODY_25_SKELETON, 4, 4, dict(hidden_size=100, num_layers=3, embeddings_size=32,
                                                                           num_classes=5)),
            ('model_cls_gru_h191', GRU, CARLA_SKELETON, 4, 15, dict(hidden_size=191, num_layers=1)),
            ('model_cls_lstm_default', LSTM, CARLA_SKELETON, 4, 16, {}),
    ):
        g = torch.Generator().manual_seed(31)
        torch.manual_seed(22742)
        model = cls(input_nodes=nodes, **kw).train()
        frames = torch.randn(B, T, len(nodes), 2, generator=g)
        out = model(frames)
        g_out = torch.randn(out.shape, generator=g)
        (out * g_out).sum().backward()
        sd = {('sd__' + k): v for k, v in model.state_dict().items()}
        grads = {('grad__' + k): p.grad for k, p in model.named_parameters()}
        # (the gradients go to a companion file: state_dict and gradients together would pass the 1 MiB limit of a committed file)
        npz(name, frames=frames, out=out, g_out=g_out, n_params=sum(p.numel() for p in model.parameters()), **sd)
        npz(name + '_grads', **grads)


if __name__ == '__main__':
    main()
