"""Baseline3DPose / Baseline3DPoseRot: the pose-lifting baseline of Martinez et al. (ICCV 2017) as a movements model
(reference modules/movements/baseline_3d_pose/baseline_3d_pose.py, baseline_3d_pose_rot.py).

The wrapper builds ``LinearModel(linear_size, num_stage, p_dropout)`` as ``baseline``, replaces its ``w1`` / ``w2`` with layers
sized for the skeletons (2 J_in inputs, F J_out outputs: F = 3 locations, or 3 + a 6-D rotation for the Rot variant), and only
then re-initialises the weight of every nn.Linear with kaiming_normal_ -- the reference's order, so one seed gives the reference's
initial parameters. Frames are independent rows: (B, T, J, 2) -> (B T, 2 J) -> MLP -> (B, T, J_out, F). Baseline3DPose feeds the
``absolute_loc`` pose head; Baseline3DPoseRot returns (locations, rotation_6d_to_matrix of the rest) for ``absolute_loc_rot``.
"""
import torch
from torch import nn

from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType
from pedestrians_video_2_carla_amd.modules.movements.baseline_3d_pose.linear_model import LinearModel
from pedestrians_video_2_carla_amd.modules.movements.movements import MovementsModel
from pedestrians_video_2_carla_amd.transforms.rotation_conversions import rotation_6d_to_matrix


class Baseline3DPose(MovementsModel):
    """Based on the PyTorch implementation (3d_pose_baseline_pytorch) of the 3D pose baseline of Martinez et al., ICCV 2017."""
    _output_features = 3            # (x, y, z) joint locations

    def __init__(self, linear_size=1024, num_stage=2, p_dropout=0.5, **kwargs):
        super().__init__(**kwargs)
        self._input_size = len(self.input_nodes) * 2          # (x, y) points
        self._output_nodes_len = len(self.output_nodes)
        self._output_size = self._output_nodes_len * self._output_features
        self.baseline = LinearModel(linear_size=linear_size, num_stage=num_stage, p_dropout=p_dropout)
        self.baseline.w1 = nn.Linear(self._input_size, linear_size)
        self.baseline.w2 = nn.Linear(linear_size, self._output_size)
        self._hparams.update({'linear_size': linear_size, 'num_stage': num_stage, 'p_dropout': p_dropout})
        self.apply(self.init_weights)

    @property
    def output_type(self) -> MovementsModelOutputType:
        return MovementsModelOutputType.absolute_loc

    def init_weights(self, m):
        if type(m) == nn.Linear:
            torch.nn.init.kaiming_normal_(m.weight)

    @staticmethod
    def add_model_specific_args(parent_parser):
        parent_parser = MovementsModel.add_model_specific_args(parent_parser)
        parser = parent_parser.add_argument_group('Baseline3DPose Lightning Module')
        parser.add_argument('--num_stage', default=2, type=int)
        parser.add_argument('--linear_size', default=1024, type=int)
        parser.add_argument('--p_dropout', default=0.5, type=float)
        return parent_parser

    def _run(self, x):
        original_shape = x.shape
        x = self.baseline(x.reshape(-1, self._input_size))
        return x.view(*original_shape[0:2], self._output_nodes_len, self._output_features)

    def forward(self, x, *args, **kwargs):
        return self._run(x)


class Baseline3DPoseRot(Baseline3DPose):
    """Baseline3DPose with a 6-D rotation per joint beside its location."""
    _output_features = 9            # (x, y, z) + rotation 6-D vector

    @property
    def output_type(self) -> MovementsModelOutputType:
        return MovementsModelOutputType.absolute_loc_rot

    @staticmethod
    def add_model_specific_args(parent_parser):
        parent_parser = MovementsModel.add_model_specific_args(parent_parser)
        parser = parent_parser.add_argument_group('Baseline3DPoseRot Movements Module')
        parser.add_argument('--num_stage', default=2, type=int)
        parser.add_argument('--linear_size', default=1024, type=int)
        parser.add_argument('--p_dropout', default=0.5, type=float)
        return parent_parser

    def forward(self, x, *args, **kwargs):
        x = self._run(x)
        return x[..., :3], rotation_6d_to_matrix(x[..., 3:])
