"""pose_changes: the criterion between the predicted pose changes and the target pose changes, frame by frame
(reference loss/pose_changes.py:7-28: ``criterion(pose_inputs, targets['pose_changes'])``; registered with
``nn.MSELoss(reduction='sum')``).

fp32 device tensors with an ``nn.MSELoss`` take one HIP launch each way (K27, ``ops.pose_change_loss``: the direct form of the
kernel behind cum_pose_changes); host tensors, fp64 and other criteria run the reference's tensor expression."""
from typing import Dict

from torch import Tensor
from torch.nn.modules import loss


def calculate_loss_pose_changes(criterion: loss._Loss, pose_inputs: Tensor = None,
                                targets: Dict[str, Tensor] = None, **kwargs) -> Tensor:
    if pose_inputs is None or isinstance(pose_inputs, tuple) or targets is None or 'pose_changes' not in targets:
        return None
    six_d = pose_inputs.ndim == 4 and pose_inputs.shape[-1] == 6    # raw 6-D network output (the reference's mixin has
    if not six_d and pose_inputs.ndim != 5:                         # already converted it, movements.py:105-118)
        return None                       # location outputs carry no rotation changes to compare
    from pedestrians_video_2_carla_amd import ops
    if ops.pose_change_loss_supported(pose_inputs, targets['pose_changes'], criterion):
        return ops.pose_change_loss(pose_inputs, targets['pose_changes'], cumulative=False, reduction=criterion.reduction)
    if six_d:
        from pedestrians_video_2_carla_amd.transforms.rotation_conversions import rotation_6d_to_matrix
        pose_inputs = rotation_6d_to_matrix(pose_inputs)
    return criterion(pose_inputs, targets['pose_changes'])
