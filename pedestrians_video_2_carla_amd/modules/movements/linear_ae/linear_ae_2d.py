"""LinearAE2D movements model (reference modules/movements/linear_ae/linear_ae_2d.py:8-79): the autoencoder flow's per-frame
2-D pose autoencoder 2J -> 1024/f -> 512/f -> 256/f -> 128/f -> 256/f -> 512/f -> 1024/f -> 2J with
``model_scaling_factor`` f = 8 by default and output type ``pose_2d``.

The reference's encoder ENDS in a Linear and its decoder STARTS with one: there is no ReLU at the 128/f bottleneck (nor after
the last layer), ReLU everywhere else. K8 (``ops.fused_mlp``) applies a ReLU between all of its layers, so it does not compute
this function; on the GPU in fp32 the eight layers are the K16 composition ``ops.dense_chain`` for every f -- eight GEMMs forward
with the ReLUs in their epilogues, seven input-gradient GEMMs with the ReLU masks in theirs, and K12 / K16-TN weight gradients
(added straight into the flat gradient buffer inside the trainer's step). ``torch.nn.functional.linear`` is never entered on the
device. Host tensors, other dtypes and autocast take the plain ``nn.Sequential`` pair.

Attribute names are kept (``__encoder`` / ``__decoder`` inside class ``LinearAE2D``) so state_dict keys
(``_LinearAE2D__encoder.0.weight`` ...) match reference checkpoints.
"""
import torch
from torch import nn

from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType
from pedestrians_video_2_carla_amd.modules.movements.movements import MovementsModel


def _half(sizes):
    """Linear layers over ``sizes`` with ReLU between them and none at the end."""
    layers = []
    for i, (a, b) in enumerate(zip(sizes[:-1], sizes[1:])):
        layers.append(nn.Linear(a, b))
        if i < len(sizes) - 2:
            layers.append(nn.ReLU(True))
    return nn.Sequential(*layers)


class LinearAE2D(MovementsModel):
    """Autoencoder of linear layers and ReLU for 2-D poses; every frame is encoded on its own."""

    def __init__(self, model_scaling_factor: int = 8, **kwargs):
        super().__init__(**kwargs)
        f = model_scaling_factor
        self.__n_out = len(self.output_nodes)
        self.__in = len(self.input_nodes) * 2                  # (x, y) per joint
        self.__encoder = _half([self.__in, 1024 // f, 512 // f, 256 // f, 128 // f])
        self.__decoder = _half([128 // f, 256 // f, 512 // f, 1024 // f, self.__n_out * 2])
        self.hip_path = True       # False: framework ops on the device too (tools/bench_flat_models.py)
        self._hparams.update({'model_scaling_factor': model_scaling_factor})

    @property
    def output_type(self) -> MovementsModelOutputType:
        return MovementsModelOutputType.pose_2d

    @staticmethod
    def add_model_specific_args(parent_parser):
        parent_parser = MovementsModel.add_model_specific_args(parent_parser)
        group = parent_parser.add_argument_group('LinearAE2D Movements Model')
        group.add_argument('--model_scaling_factor', default=8, type=int)
        return parent_parser

    def _chain(self):
        """(Linear layers, ReLU-after-layer flags) of encoder + decoder in order."""
        mods = list(self.__encoder) + list(self.__decoder)
        layers, relus = [], []
        for i, m in enumerate(mods):
            if isinstance(m, nn.Linear):
                layers.append(m)
                relus.append(i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU))
        return layers, relus

    def forward(self, x, *args, **kwargs):
        lead = x.shape[0:2]
        flat = x.reshape((-1, self.__in))
        if self.hip_path and flat.is_cuda and flat.dtype == torch.float32 and not torch.is_autocast_enabled():
            from pedestrians_video_2_carla_amd import ops
            layers, relus = self._chain()
            out = ops.dense_chain(flat, [m.weight for m in layers], [m.bias for m in layers], relus)
        else:
            out = self.__decoder(self.__encoder(flat))
        return out.view(*lead, self.__n_out, 2)
