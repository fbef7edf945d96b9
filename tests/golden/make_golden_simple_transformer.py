#!/usr/bin/env python3
"""Generate tests/golden/model_simple_transformer_*.npz by RUNNING THE REFERENCE's own SimpleTransformer (build container only).

The reference imports under the third-party stand-ins of make_golden.py (``install_standins``); its
modules/movements/transformers.py runs unmodified. Forward and backward run in ``.eval()`` (no dropout); the gradients are those
of ``(out * g_out).sum()`` for a fixed random ``g_out``. A full state_dict at d = 52 is 6.3 MB, so only the tiny case keeps all
of it:

  model_simple_transformer_tiny_{0,1}.npz   a 4-joint skeleton (d = 8, 2 heads), each of the six layers perturbed by seeded
                                            noise after construction (a layer-indexing bug cannot pass on six identical layers);
                                            the state_dict split over two files (``sd__*``), frames / out / g_out in _0
  model_simple_transformer_tiny_grads.npz   its parameter gradients (``grad__*``; the unused template has none)
  model_simple_transformer_carla.npz        CARLA (d = 52, 4 heads), seed 22742: the template layer's parameters (``tpl__*``:
                                            all six layers start as copies of it), frames / out / g_out, and per parameter the
                                            gradient's sum and norm (``gsum__*``, ``gnorm__*``)
  model_simple_transformer_body25.npz       BODY_25 (d = 50, 5 heads), seed 1234, the same reduced form
"""
import enum
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF_SRC, install_standins, npz  # noqa: E402


class TINY_SKELETON(enum.Enum):
    hips = 0
    neck = 1
    head = 2
    foot = 3


def main():
    if not os.path.isdir(REF_SRC):
        sys.exit('reference tree not present: the committed .npz files are the artefact to use')
    install_standins()
    sys.path.insert(0, REF_SRC)
    from pedestrians_video_2_carla.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla.data.openpose.skeleton import BODY_25_SKELETON
    from pedestrians_video_2_carla.modules.flow.output_types import MovementsModelOutputType as MT
    from pedestrians_video_2_carla.modules.movements.transformers import SimpleTransformer

    def run(model, nodes, B, T, g):
        frames = torch.randn(B, T, len(nodes), 2, generator=g)
        out = model(frames)
        g_out = torch.randn(out.shape, generator=g)
        (out * g_out).sum().backward()
        return frames, out, g_out

    # (a) tiny skeleton, every layer different
    g = torch.Generator().manual_seed(31)
    torch.manual_seed(7)
    model = SimpleTransformer(input_nodes=TINY_SKELETON, n_heads=2, movements_output_type=MT.pose_2d)
    with torch.no_grad():
        for layer in model.encoder.layers:
            for p in layer.parameters():
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    model.eval()
    frames, out, g_out = run(model, TINY_SKELETON, 3, 7, g)
    sd = {('sd__' + k): v for k, v in model.state_dict().items()}
    keys = sorted(sd)
    half = [k for k in keys if k.startswith('sd__encoder_layer.') or any(k.startswith(f'sd__encoder.layers.{i}.') for i in (0, 1, 2))]
    npz('model_simple_transformer_tiny_0', frames=frames, out=out, g_out=g_out, n_params=sum(p.numel() for p in model.parameters()),
        **{k: sd[k] for k in half})
    npz('model_simple_transformer_tiny_1', **{k: sd[k] for k in keys if k not in half})
    npz('model_simple_transformer_tiny_grads', **{('grad__' + k): p.grad for k, p in model.named_parameters() if p.grad is not None})

    # (b), (c) the seeded initial model, reduced
    for name, nodes, heads, seed, B, T in (('model_simple_transformer_carla', CARLA_SKELETON, 4, 22742, 2, 16),
                                           ('model_simple_transformer_body25', BODY_25_SKELETON, 5, 1234, 2, 30)):
        g = torch.Generator().manual_seed(5)
        torch.manual_seed(seed)
        model = SimpleTransformer(input_nodes=nodes, n_heads=heads, movements_output_type=MT.pose_2d).eval()
        frames, out, g_out = run(model, nodes, B, T, g)
        arrays = dict(frames=frames, out=out, g_out=g_out, n_params=sum(p.numel() for p in model.parameters()),
                      keys=sorted(model.state_dict().keys()))
        arrays.update({('tpl__' + k): v for k, v in model.encoder_layer.state_dict().items()})
        for k, p in model.named_parameters():
            if p.grad is not None:
                arrays['gsum__' + k] = p.grad.double().sum()
                arrays['gnorm__' + k] = p.grad.double().norm()
        npz(name, **arrays)


if __name__ == '__main__':
    main()
