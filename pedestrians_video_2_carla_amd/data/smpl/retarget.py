"""SMPL body poses (AMASS ``targets/amass_body_pose``) -> CARLA poses: the tensor definition of K35.

Restates reference data/smpl/smpl_dataset.py:103-142 (``SMPLDataset.convert_smpl_to_carla``) with data/smpl/utils.py:53-58
(the axes convention) for any leading dimensions and any floating dtype. Per frame with skeleton type t:

1. p (22,3): the 66 values in original SMPL joint order -> ``SMPL_SKELETON`` order, times (-1, 1, 1);
2. M[s] = euler_angles_to_matrix(p[s], 'XYZ') = Rx Ry Rz;
3. C = identity for the 26 CARLA bones, C[ci] = M[si] for the 21 common pairs, C[spine01] = M[Spine3] @ M[Spine2];
4. L[j] = abs_ref_rot[t][j] @ K, K = [[1,0,0],[0,0,-1],[0,1,0]]; local[j] = L[j]^T C[j] L[j]  (L is a rotation: the reference's
   ``linalg.solve(L, C)`` is L^T C);
5. relative_pose_rot[j] = local[j] @ ref_rel_rot[t][j] (for the five bones without an SMPL joint C = I, local = I and the row is
   ref_rel_rot[t][j] itself); absolute_pose_loc / absolute_pose_rot = forward kinematics of
   (ref_rel_loc[t], relative_pose_rot) in the row-vector convention of ``data/carla/reference.forward_kinematics``.

Every frame starts from the reference pose; nothing is masked: a non-finite joint gives NaN in its bone and the bone's descendants.
"""
from typing import Dict, Optional, Sequence

import torch
from torch import Tensor

from pedestrians_video_2_carla_amd.data.base.skeleton import get_common_indices
from pedestrians_video_2_carla_amd.data.carla import reference as ref
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON, PARENTS
from pedestrians_video_2_carla_amd.data.smpl.skeleton import SMPL_SKELETON, map_from_original
from pedestrians_video_2_carla_amd.transforms.rotation_conversions import euler_angles_to_matrix

POSE_KEYS, ROW_KEYS = ref.POSE_KEYS, ref.ROW_KEYS
J = len(CARLA_SKELETON)

# CARLA bone j <- SMPL_SKELETON joint SMPL_OF_BONE[j] (-1: the bone keeps the reference pose)
_CI, _SI = get_common_indices(SMPL_SKELETON)
SMPL_OF_BONE = tuple(dict(zip(_CI, _SI)).get(j, -1) for j in range(J))
SPINE01 = CARLA_SKELETON.crl_spine01__C.value


def conventions_rot(dtype=torch.float32, device=None) -> Tensor:
    """K: SMPL's axes seen from CARLA's (a quarter turn about X)."""
    return torch.tensor(((1.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0)), dtype=dtype, device=device)


def check_shapes(body_pose: Tensor, skel_type: Tensor, world_loc: Optional[Tensor], world_rot: Optional[Tensor],
                 want: Sequence[str]):
    """-> the leading dimensions of ``body_pose`` ((..., 66) or (..., 22, 3)); raises on anything that does not fit them."""
    if body_pose.ndim >= 2 and tuple(body_pose.shape[-2:]) == (22, 3):
        lead = tuple(body_pose.shape[:-2])
    elif body_pose.ndim >= 1 and body_pose.shape[-1] == 66:
        lead = tuple(body_pose.shape[:-1])
    else:
        raise RuntimeError(f'smpl_to_carla: body_pose (..., 66) or (..., 22, 3) expected, got {tuple(body_pose.shape)}')
    return ref.check_shapes('smpl_to_carla', lead, skel_type, world_loc, world_rot, want)


@torch.no_grad()
def convert_smpl_to_carla(body_pose: Tensor, skel_type: Tensor, world_loc: Optional[Tensor] = None,
                          world_rot: Optional[Tensor] = None, want: Sequence[str] = POSE_KEYS) -> Dict[str, Tensor]:
    """``body_pose`` (..., 66) or (..., 22, 3), ``skel_type`` integer with a shape that is a prefix of the leading dimensions
    (rows of ``CARLA_REFERENCE_SKELETON_TYPES``) -> dict of the ``want``-ed among ``relative_pose_rot`` (..., 26, 3, 3),
    ``absolute_pose_loc`` (..., 26, 3), ``absolute_pose_rot`` (..., 26, 3, 3), ``bones`` (..., 26, 6) and ``root`` (..., 6) (the
    rows of ``ops.carla_pose_export``; ``root`` from ``world_loc`` / ``world_rot``). Tensor ops, the dtype of ``body_pose``."""
    want = tuple(want)
    lead = check_shapes(body_pose, skel_type, world_loc, world_rot, want)
    dtype, device = body_pose.dtype, body_pose.device
    p = map_from_original(body_pose) * torch.tensor((-1.0, 1.0, 1.0), dtype=dtype, device=device)
    m = euler_angles_to_matrix(p, 'XYZ')                                            # (..., 22, 3, 3)
    changes = torch.eye(3, dtype=dtype, device=device).expand(lead + (J, 3, 3)).clone()
    changes[..., _CI, :, :] = m[..., _SI, :, :]
    changes[..., SPINE01, :, :] = m[..., SMPL_SKELETON.Spine3.value, :, :] @ m[..., SMPL_SKELETON.Spine2.value, :, :]

    st = ref.frame_types(skel_type, lead, device)
    rel_loc, rel_rot = (t[st] for t in ref.get_relative_tensors(device, dtype=dtype))
    _, abs_rot = ref.get_absolute_tensors(device, dtype=dtype)
    local = abs_rot[st] @ conventions_rot(dtype, device)
    local_changes = (local.transpose(-1, -2) @ changes) @ local
    # a bone without an SMPL joint has C = I, so local = L^T L = I: it keeps the reference row itself, not its product with
    # the rounded L^T L
    mapped = torch.tensor([s >= 0 for s in SMPL_OF_BONE], device=device).reshape(J, 1, 1)
    relative_pose_rot = torch.where(mapped, local_changes @ rel_rot, rel_rot)

    out = {}
    if 'relative_pose_rot' in want:
        out['relative_pose_rot'] = relative_pose_rot
    if 'absolute_pose_loc' in want or 'absolute_pose_rot' in want:
        a_loc, a_rot = [None] * J, [None] * J
        for j, parent in enumerate(PARENTS):
            if parent < 0:
                a_loc[j], a_rot[j] = rel_loc[..., j, :], relative_pose_rot[..., j, :, :]
            else:
                a_loc[j] = (rel_loc[..., j, None, :] @ a_rot[parent])[..., 0, :] + a_loc[parent]
                a_rot[j] = relative_pose_rot[..., j, :, :] @ a_rot[parent]
        if 'absolute_pose_loc' in want:
            out['absolute_pose_loc'] = torch.stack(a_loc, -2)
        if 'absolute_pose_rot' in want:
            out['absolute_pose_rot'] = torch.stack(a_rot, -3)
    return {**out, **ref.carla_rows(want, rel_loc, relative_pose_rot, world_loc, world_rot)}
