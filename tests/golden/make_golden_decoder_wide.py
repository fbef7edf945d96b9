#!/usr/bin/env python3
"""Generate tests/golden/model_seq2seq_embeddings_h64_pose_changes{,_grads}.npz by RUNNING THE REFERENCE's own
Seq2SeqEmbeddings(hidden_size=64, single_joint_embeddings_size=8, pose_changes) (build container only).

The reference imports under the third-party stand-ins of make_golden.py (``install_standins``); its model files run unmodified.
hidden_size 64 with the pose_changes output (26 x 6 = 156 features per frame, seq2seq.py:245-288) is the shape whose decoder
loop K7c runs in one launch (csrc/p2c_s2s_wide.h). single_joint_embeddings_size=8 keeps the files small, as in
model_seq2seq_embeddings_h128_pose_changes. Model seed 22742, data seed 43, 4 clips of 16 frames.

  model_seq2seq_embeddings_h64_pose_changes        eval mode: frames, the state_dict (``sd__*``), out, n_params
  model_seq2seq_embeddings_h64_pose_changes_grads  the same weights built with p_dropout=0, train mode: g_out (fixed random) and the
                                                   parameter gradients (``grad__*``) of ``(out * g_out).sum()``
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF_SRC, install_standins, npz  # noqa: E402

NAME = 'model_seq2seq_embeddings_h64_pose_changes'


def main():
    if not os.path.isdir(REF_SRC):
        sys.exit('reference tree not present: the committed .npz files are the artefact to use')
    install_standins()
    sys.path.insert(0, REF_SRC)
    from pedestrians_video_2_carla.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla.modules.flow.output_types import MovementsModelOutputType as MT
    from pedestrians_video_2_carla.modules.movements.seq2seq.seq2seq_embeddings import Seq2SeqEmbeddings
    g = torch.Generator().manual_seed(43)
    frames = torch.randn(4, 16, 26, 2, generator=g)
    kw = dict(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, movements_output_type=MT.pose_changes, hidden_size=64,
              single_joint_embeddings_size=8)
    torch.manual_seed(22742)
    model = Seq2SeqEmbeddings(**kw).eval()
    with torch.no_grad():
        out = model(frames)
    sd = {('sd__' + k): v for k, v in model.state_dict().items()}
    npz(NAME, frames=frames, out=out, n_params=sum(p.numel() for p in model.parameters()), **sd)

    train = Seq2SeqEmbeddings(p_dropout=0.0, **kw)
    train.load_state_dict(model.state_dict())
    train.train()
    g_out = torch.randn(out.shape, generator=g)
    (train(frames) * g_out).sum().backward()
    npz(NAME + '_grads', g_out=g_out, **{('grad__' + k): p.grad for k, p in train.named_parameters()})


if __name__ == '__main__':
    main()
