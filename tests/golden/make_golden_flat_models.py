#!/usr/bin/env python3
"""Generate tests/golden/model_{seq2seq_flat_embeddings,linear_ae_2d,linear}_*.npz by RUNNING THE REFERENCE's own
Seq2SeqFlatEmbeddings, LinearAE2D and Linear movements models (build container only).

The reference imports under the third-party stand-ins of make_golden.py (``install_standins``); its model files run unmodified.
Each fixture holds the input frames, the state_dict (``sd__*``), the train-mode output, ``n_params`` and the parameter gradients
(``grad__*``) of ``(out * g_out).sum()`` for a fixed random ``g_out``; the Seq2Seq fixtures keep their gradients in a
``<name>_grads.npz`` companion (state_dict and gradients together would pass the size limit of a committed file) and use
``p_dropout=0`` so that the train-mode gradients are reproducible. Model seed 22742, data seed 31.

  model_seq2seq_flat_embeddings_pose_2d     CLI defaults (52 -> 128 -> 64, H = 64, L = 2), pose_2d, CARLA, B = 4, T = 15
  model_seq2seq_flat_embeddings_inv_body25  BODY_25 input, embeddings_size=[96], invert_sequence, hidden_size=32, B = 3, T = 4
  model_linear_ae_2d                        defaults (f = 8), CARLA, B = 4, T = 16
  model_linear_ae_2d_f16_body25             f = 16, BODY_25, B = 3, T = 5
  model_linear_pose_changes                 Linear, pose_changes (output (B,T,26,3,3)), B = 3, T = 5
  model_linear_conf_pose_2d                 Linear, needs_confidence (frames (B,T,26,3)), pose_2d, B = 3, T = 5
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
    from pedestrians_video_2_carla.modules.movements.linear import Linear
    from pedestrians_video_2_carla.modules.movements.linear_ae.linear_ae_2d import LinearAE2D
    from pedestrians_video_2_carla.modules.movements.seq2seq.seq2seq_flat_embeddings import Seq2SeqFlatEmbeddings
    for name, cls, nodes, B, T, C, split, kw in (
            ('model_seq2seq_flat_embeddings_pose_2d', Seq2SeqFlatEmbeddings, CARLA_SKELETON, 4, 15, 2, True,
             dict(embeddings_size_0=128, embeddings_size_1=64, embeddings_size_2=None, embeddings_size_3=None,
                  embeddings_size_4=None, movements_output_type=MT.pose_2d, p_dropout=0.0)),
            ('model_seq2seq_flat_embeddings_inv_body25', Seq2SeqFlatEmbeddings, BODY_25_SKELETON, 3, 4, 2, True,
             dict(embeddings_size=[96], invert_sequence=True, hidden_size=32, movements_output_type=MT.pose_2d, p_dropout=0.0)),
            ('model_linear_ae_2d', LinearAE2D, CARLA_SKELETON, 4, 16, 2, False, {}),
            ('model_linear_ae_2d_f16_body25', LinearAE2D, BODY_25_SKELETON, 3, 5, 2, False, dict(model_scaling_factor=16)),
            ('model_linear_pose_changes', Linear, CARLA_SKELETON, 3, 5, 2, False, dict(movements_output_type=MT.pose_changes)),
            ('model_linear_conf_pose_2d', Linear, CARLA_SKELETON, 3, 5, 3, False,
             dict(needs_confidence=True, movements_output_type=MT.pose_2d)),
    ):
        g = torch.Generator().manual_seed(31)
        torch.manual_seed(22742)
        model = cls(input_nodes=nodes, **kw).train()
        frames = torch.randn(B, T, len(nodes), C, generator=g)
        out = model(frames)
        g_out = torch.randn(out.shape, generator=g)
        (out * g_out).sum().backward()
        sd = {('sd__' + k): v for k, v in model.state_dict().items()}
        grads = {('grad__' + k): p.grad for k, p in model.named_parameters()}
        base = dict(frames=frames, out=out, g_out=g_out, n_params=sum(p.numel() for p in model.parameters()), **sd)
        if split:
            npz(name, **base)
            npz(name + '_grads', **grads)
        else:
            npz(name, **base, **grads)


if __name__ == '__main__':
    main()
