#!/usr/bin/env python3
"""Generate tests/golden/model_lstm_*.npz by RUNNING THE REFERENCE's own LSTM movements model (build container only).

The reference imports under the third-party stand-ins of make_golden.py (``install_standins``); its
modules/movements/lstm.py runs unmodified. Each fixture holds the input frames, the state_dict (``sd__*``), the output and
the parameter gradients (``grad__*``, in ``<name>_grads.npz``) of ``(out * g_out).sum()`` for a fixed random ``g_out``:

  model_lstm_pose_changes.npz     defaults: H = 64, L = 2, CARLA, B = 4, T = 16, output (B,T,26,3,3)
  model_lstm_h191_pose_2d.npz     H = 191 (the reference's retrain sweep), L = 1, B = 4, T = 15, pose_2d
  model_lstm_body25_emb.npz       BODY_25 input, embeddings_size = 32, H = 100, L = 3, B = 4, T = 4, pose_2d
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
    from pedestrians_video_2_carla.modules.flow.output_types import MovementsModelOutputType as MT
    from pedestrians_video_2_carla.modules.movements.lstm import LSTM
    for name, nodes, B, T, kw in (
            ('model_lstm_pose_changes', CARLA_SKELETON, 4, 16, {}),
            ('model_lstm_h191_pose_2d', CARLA_SKELETON, 4, 15, dict(hidden_size=191, num_layers=1, movements_output_type=MT.pose_2d)),
            ('model_lstm_body25_emb', BODY_25_SKELETON, 4, 4, dict(hidden_size=100, num_layers=3, embeddings_size=32,
                                                                    movements_output_type=MT.pose_2d)),
    ):
        g = torch.Generator().manual_seed(31)
        torch.manual_seed(22742)
        model = LSTM(input_nodes=nodes, **kw).train()
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
