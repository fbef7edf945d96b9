"""Base of the class-style pose losses (reference loss/base_pose_loss.py:13-110).

The reference gathers the common joints, builds a boolean mask and boolean-indexes both tensors (dynamic shapes, two
copies) before MSELoss. On device that is one masked-MSE kernel (p2c_loss2d_*), or nothing at all when the fused pose
head already produced the value (``_fused`` in the sliced dict).
"""
from typing import Type

from torch import Tensor
from torch.nn.modules import loss

from pedestrians_video_2_carla_amd.data.base.skeleton import Skeleton, get_common_indices


def index_list(idx, n):
    return list(range(n)) if isinstance(idx, slice) else list(idx)


class BasePoseLoss(object):
    fused_name = None

    def __init__(self, criterion: loss._Loss, input_nodes: Type[Skeleton], output_nodes: Type[Skeleton],
                 mask_missing_joints: bool = True, sum_per_joint: bool = False, sum_per_frame: bool = False,
                 **kwargs) -> None:
        assert not (sum_per_joint and sum_per_frame), 'sum_per_joint and sum_per_frame are mutually exclusive'
        self._sum_per_joint, self._sum_per_frame = sum_per_joint, sum_per_frame
        self._criterion = criterion
        self._input_nodes, self._output_nodes = input_nodes, output_nodes
        self._output_indices, self._input_indices = get_common_indices(input_nodes, output_nodes)
        self._mask_missing_joints = mask_missing_joints
        hips = input_nodes.get_hips_point() if input_nodes is not None else None
        self._input_hips = None if isinstance(hips, (list, tuple)) else hips

    def hips_column(self, n_gt_joints: int) -> int:
        """Position of the input skeleton's hips joint in the common-joint list (utils/tensors.py:33-38)."""
        if self._input_hips is None:
            return -1
        if isinstance(self._input_indices, slice):
            return self._input_hips.value
        return list(self._input_indices).index(self._input_hips.value)

    def __call__(self, **kwargs) -> Tensor:
        fused = kwargs.get('_fused')
        grouped = self._sum_per_joint or self._sum_per_frame      # the fused pose head forms the plain masked mean only
        if fused is not None and self.fused_name and not grouped:
            value = fused.get(self.fused_name, self._input_nodes, self._output_nodes, self._mask_missing_joints)
            if value is not None:
                return value
        from pedestrians_video_2_carla_amd import ops
        gt = self._extract_gt_targets(**kwargs)
        pred = self._extract_predicted_targets(**kwargs)
        n_common = min(pred.shape[-2], gt.shape[-2])
        if grouped:
            return self._grouped(pred, gt, index_list(self._output_indices, n_common), index_list(self._input_indices, n_common))
        return ops.loss_loc_2d(pred, gt, index_list(self._output_indices, n_common),
                               index_list(self._input_indices, n_common), self.hips_column(gt.shape[-2]),
                               self._mask_missing_joints)

    def _grouped(self, pred: Tensor, gt: Tensor, pred_idx, gt_idx) -> Tensor:
        """sum_per_joint / sum_per_frame (reference base_pose_loss.py:68-104: a Python loop over the groups with boolean-mask
        gathers and an isnan host sync each) as tensor ops of fixed shape: the criterion per (B,T,K) row, unselected rows and
        skipped groups zeroed, no gather, no sync. Every group skipped: 0, where the reference raises on an empty stack."""
        import torch
        from pedestrians_video_2_carla_amd import ops
        common_pred, common_gt = pred[..., pred_idx, :], gt[..., gt_idx, :].to(pred.dtype)
        mask = None
        if self._mask_missing_joints:
            mask = torch.all(common_gt != 0, dim=-1)               # missing joints are 'perfect' zeros (utils/tensors.py:29)
            hips = self.hips_column(gt.shape[-2])
            if hips >= 0:
                mask[..., hips] = True
        return ops.grouped_loss_tensor(common_pred, common_gt, mask, self._criterion, -2 if self._sum_per_joint else 1)[0]

    def _extract_gt_targets(self, **kwargs) -> Tensor:
        raise NotImplementedError

    def _extract_predicted_targets(self, **kwargs) -> Tensor:
        raise NotImplementedError
