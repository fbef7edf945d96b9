"""Seq2SeqFlatEmbeddings: a Linear + ReLU stack over the whole flattened frame in front of the Seq2Seq encoder
(reference modules/movements/seq2seq/seq2seq_flat_embeddings.py:7-73; default 2J -> 128 -> 64).

Unlike Seq2SeqEmbeddings the stack ends in a ReLU, so it cannot be folded into the encoder's input projection. On the GPU in
fp32 ``_format_input`` is ONE launch (K21, ``ops.relu_stack`` -> ``p2c_relu_stack_fwd``) that writes the sequence-first
(T,B,E) tensor the encoder LSTM consumes, time-reversed when ``invert_sequence`` -- no permute copy, no flip copy -- and two
launches backward (the hidden activations are recomputed; inside the flat trainer's step the gradients are added straight into
the flat gradient buffer). Widths outside K21 (``ops.relu_stack_supported``: the weight images no longer fit the LDS, e.g.
512 -> 256) are a chain of K16 GEMMs with the ReLU in their epilogues (``ops.dense_chain``) and one permuting copy. Host
tensors, other dtypes and autocast (the CPU parity pipeline) take the plain ``nn.Sequential``.

Parameters live in ``embeddings = nn.Sequential(Linear, ReLU, ...)`` (keys ``embeddings.0.*``, ``embeddings.2.*``, ...) so
reference checkpoints load unchanged. ``embeddings_size`` is a list, or the sweep-friendly flat ``embeddings_size_0..4`` kwargs
(``None`` entries dropped, the rest in index order; reference utils/argparse.py:47-81).
"""
import torch
from torch import nn

from .seq2seq import Seq2Seq

MAX_EMBEDDING_LAYERS = 5
DEFAULT_EMBEDDINGS_SIZE = (128, 64)


def flat_args_as_list_arg(kwargs, name):
    """``kwargs[name]`` if present, else the non-None ``name_<i>`` values ordered by i."""
    if name in kwargs:
        return list(kwargs[name])
    flat = sorted((k for k in kwargs if k.startswith(f'{name}_') and k[len(name) + 1:].isdigit()),
                  key=lambda k: int(k[len(name) + 1:]))
    return [kwargs[k] for k in flat if kwargs[k] is not None]


def list_arg_as_flat_args(parser, name, max_length, defaults=None, value_type=float):
    """``--name_0 .. --name_<max_length-1>`` instead of a sweep-incompatible ``nargs='+'``."""
    for i in range(max_length):
        parser.add_argument(f'--{name}_{i}', default=defaults[i] if (defaults is not None and i < len(defaults)) else None,
                            type=value_type)
    return parser


class Seq2SeqFlatEmbeddings(Seq2Seq):
    def __init__(self, input_features: int = 2, **kwargs):
        self.embeddings_size = flat_args_as_list_arg(kwargs, 'embeddings_size') or list(DEFAULT_EMBEDDINGS_SIZE)
        super().__init__(**{**kwargs, 'input_features': None, 'input_size': self.embeddings_size[-1]})
        sizes = [input_features * len(self.input_nodes)] + self.embeddings_size
        self.embeddings = nn.Sequential(*[m for a, b in zip(sizes[:-1], sizes[1:]) for m in (nn.Linear(a, b), nn.ReLU())])
        self.hip_path = True       # False: the stack runs as framework ops on the device too (tools/bench_flat_models.py)
        self._hparams.update({'embeddings_size': self.embeddings_size})

    @staticmethod
    def add_model_specific_args(parent_parser):
        parent_parser = Seq2Seq.add_model_specific_args(parent_parser)
        group = parent_parser.add_argument_group('Seq2SeqFlatEmbeddings Movements Module')
        list_arg_as_flat_args(group, 'embeddings_size', MAX_EMBEDDING_LAYERS, list(DEFAULT_EMBEDDINGS_SIZE), int)
        return parent_parser

    def _linears(self):
        return [m for m in self.embeddings if isinstance(m, nn.Linear)]

    def _format_input(self, x):
        B, T = x.shape[:2]
        flat = x.reshape(B, T, -1)
        if self.hip_path and flat.is_cuda and flat.dtype == torch.float32 and not torch.is_autocast_enabled():
            from pedestrians_video_2_carla_amd import ops
            layers = self._linears()
            ws, bs = [m.weight for m in layers], [m.bias for m in layers]
            dims = [flat.shape[-1]] + [m.out_features for m in layers]
            if not flat.requires_grad and ops.relu_stack_supported(dims):
                return ops.relu_stack(flat, ws, bs, flip=self.invert_sequence)                   # (T,B,E), one launch (K21)
            emb = ops.dense_chain(flat.reshape(B * T, -1), ws, bs, [True] * len(layers)).view(B, T, -1)
            if self.invert_sequence:          # one gather: sequence-first and time-reversed
                rows = (torch.arange(B, device=x.device) * T).unsqueeze(0) + torch.arange(T - 1, -1, -1, device=x.device).unsqueeze(1)
                return emb.reshape(B * T, -1).index_select(0, rows.reshape(-1)).view(T, B, -1)
            return emb.permute(1, 0, 2).contiguous()
        emb = self.embeddings(flat.reshape(B * T, -1)).view(B, T, -1).permute(1, 0, 2)           # sequence first
        return emb.flip(0) if self.invert_sequence else emb
