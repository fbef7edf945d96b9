"""Linear movements model (reference modules/movements/linear.py:6-58): one dense layer per frame, the flows' debug model.

``needs_confidence`` makes the input (x, y, confidence) per joint; every ``movements_output_type`` is supported through
``_format_output``. On the GPU in fp32 the layer is K16 forward and K12 for the weight gradient (``ops.dense``); host tensors,
other dtypes and autocast take ``nn.Linear``. The ``linear`` submodule name matches the reference's state_dict.
"""
from torch import nn

from pedestrians_video_2_carla_amd.modules.movements.movements import MovementsModel, MovementsModelOutputTypeMixin


def boolean(v) -> bool:
    s = str(v).strip().lower()
    if s in ('y', 'yes', 't', 'true', 'on', '1'):
        return True
    if s in ('n', 'no', 'f', 'false', 'off', '0'):
        return False
    raise ValueError(f'invalid truth value {v!r}')


class Linear(MovementsModelOutputTypeMixin, MovementsModel):
    """The simplest dummy model used to debug the flow."""

    def __init__(self, needs_confidence: bool = False, **kwargs):
        super().__init__(**kwargs)
        self.__needs_confidence = needs_confidence
        self.__n_out = len(self.output_nodes)
        self.__in = len(self.input_nodes) * (3 if needs_confidence else 2)
        self.linear = nn.Linear(self.__in, self.__n_out * self.output_features)
        self.hip_path = True       # False: nn.Linear on the device too (tools/bench_flat_models.py)

    @property
    def needs_confidence(self) -> bool:
        return self.__needs_confidence

    @staticmethod
    def add_model_specific_args(parent_parser):
        parent_parser = MovementsModel.add_model_specific_args(parent_parser)
        group = parent_parser.add_argument_group('Linear Model')
        MovementsModelOutputTypeMixin.add_cli_args(group)
        group.add_argument('--needs_confidence', dest='needs_confidence', type=boolean, default=False)
        return parent_parser

    def forward(self, x, *args, **kwargs):
        from pedestrians_video_2_carla_amd import ops
        lead = x.shape[0:2]
        flat = x.reshape((-1, self.__in))
        # (K16 / K12; ops.dense itself hands host tensors to the framework)
        out = ops.dense(flat, self.linear.weight, self.linear.bias) if self.hip_path else self.linear(flat)
        return self._format_output(out.view(*lead, self.__n_out, self.output_features))
