"""The MLP of Martinez et al., "A simple yet effective baseline for 3d human pose estimation" (ICCV 2017), as published with
its PyTorch port (3d_pose_baseline_pytorch, src/model.py): the model the reference's Baseline3DPose(Rot) wrap
(reference modules/movements/baseline_3d_pose/*.py import it from third_party/baseline_3d_pose, an empty submodule there).

Restated from the published layer list, with its submodule names and registration order, so that state_dict keys match:
  w1 -> batch_norm1 -> ReLU -> Dropout, then num_stage x ``Linear`` (y = drop(relu(bn2(w2(drop(relu(bn1(w1(x)))))))); x + y),
  then w2. Every BatchNorm1d has the defaults (eps 1e-5, momentum 0.1, affine, running statistics).

On the GPU in fp32 (outside autocast) every Linear is ``ops.dense`` (K16 forward and input gradient, K12 / K16 weight gradient)
and every BatchNorm + ReLU + Dropout (+ the residual add of a block) is one ``ops.batch_norm_act`` (K19). The dropout masks
come from one in-kernel stream per model (``ops.dropout_state``; site 0 = ``batch_norm1``, 1 + 2 i / 2 + 2 i = the two layers of
stage i). Host tensors, other dtypes and autocast run the nn modules below as they are.
"""
import torch
from torch import nn


class Linear(nn.Module):
    """One residual stage: two (Linear, BatchNorm1d, ReLU, Dropout) layers and the skip connection."""

    def __init__(self, linear_size: int, p_dropout: float = 0.5):
        super().__init__()
        self.l_size = linear_size
        self.relu = nn.ReLU(inplace=True)
        self.dropout = nn.Dropout(p_dropout)
        self.w1 = nn.Linear(self.l_size, self.l_size)
        self.batch_norm1 = nn.BatchNorm1d(self.l_size)
        self.w2 = nn.Linear(self.l_size, self.l_size)
        self.batch_norm2 = nn.BatchNorm1d(self.l_size)

    def forward(self, x):
        y = self.dropout(self.relu(self.batch_norm1(self.w1(x))))
        y = self.dropout(self.relu(self.batch_norm2(self.w2(y))))
        return x + y


class LinearModel(nn.Module):
    def __init__(self, linear_size: int = 1024, num_stage: int = 2, p_dropout: float = 0.5):
        super().__init__()
        self.linear_size = linear_size
        self.p_dropout = p_dropout
        self.num_stage = num_stage
        self.input_size = 16 * 2          # the published model's 16 joints (the wrappers replace w1 / w2 for their skeletons)
        self.output_size = 16 * 3
        self.w1 = nn.Linear(self.input_size, self.linear_size)
        self.batch_norm1 = nn.BatchNorm1d(self.linear_size)
        self.linear_stages = nn.ModuleList([Linear(self.linear_size, self.p_dropout) for _ in range(num_stage)])
        self.w2 = nn.Linear(self.linear_size, self.output_size)
        self.relu = nn.ReLU(inplace=True)
        self.dropout = nn.Dropout(self.p_dropout)

    def _device_path(self, x: torch.Tensor) -> bool:
        return bool(x.is_cuda and x.dtype == torch.float32 and x.ndim == 2 and not torch.is_autocast_enabled()
                    and self.w1.weight.is_cuda and self.w1.weight.dtype == torch.float32)

    def _kernel_drop_state(self, device):
        """The state of this model's in-kernel dropout stream (``ops.dropout_state``), or None when the framework's dropout is
        asked for (P2C_TORCH_DROPOUT=1)."""
        from pedestrians_video_2_carla_amd import ops
        if not ops.kernel_dropout_enabled():
            return None
        st = getattr(self, '_drop_state', None)
        if st is None or st.device != device:
            st = self._drop_state = ops.dropout_state(device)
        return st

    def _device_forward(self, x: torch.Tensor) -> torch.Tensor:
        from pedestrians_video_2_carla_amd import ops
        drops = [self.dropout.p] + [s.dropout.p for s in self.linear_stages]
        st = self._kernel_drop_state(x.device) if (self.training and max(drops) > 0) else None
        y = ops.dense(x.contiguous(), self.w1.weight, self.w1.bias)
        y = ops.batch_norm_act(y, self.batch_norm1, self.dropout.p, st, 0)
        for i, stage in enumerate(self.linear_stages):
            h = ops.dense(y, stage.w1.weight, stage.w1.bias)
            h = ops.batch_norm_act(h, stage.batch_norm1, stage.dropout.p, st, 1 + 2 * i)
            h = ops.dense(h, stage.w2.weight, stage.w2.bias)
            y = ops.batch_norm_act(h, stage.batch_norm2, stage.dropout.p, st, 2 + 2 * i, residual=y)
        return ops.dense(y, self.w2.weight, self.w2.bias)

    def forward(self, x):
        if self._device_path(x):
            return self._device_forward(x)
        y = self.dropout(self.relu(self.batch_norm1(self.w1(x))))
        for i in range(self.num_stage):
            y = self.linear_stages[i](y)
        return self.w2(y)
