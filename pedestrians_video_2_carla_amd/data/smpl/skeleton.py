"""SMPL skeleton (22 joints, in the order of the P3dPose representation, not of original SMPL) and its CARLA joint
correspondences.

Data restated from reference data/smpl/skeleton.py (enum members :37-63; hips / neck :97-103; flip mask :105-130;
CARLA pairs :159-181 (21 joints)). Needed as index tables for the collate kernels' flip permutation and node map.
"""
from pedestrians_video_2_carla_amd.data.base.skeleton import Skeleton, register_skeleton
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON as C

_SMPL = ('Pelvis Spine1 Spine2 Spine3 L_Collar L_Shoulder L_Elbow L_Wrist Neck Head R_Collar R_Shoulder R_Elbow R_Wrist '
         'R_Hip R_Knee R_Ankle R_Foot L_Hip L_Knee L_Ankle L_Foot').split()


class SMPL_SKELETON(Skeleton):
    _ignore_ = ['i', 'n']
    for i, n in enumerate(_SMPL):
        vars()[n] = i

    @classmethod
    def get_root_point(cls):
        return cls.Pelvis

    @classmethod
    def get_neck_point(cls):
        return cls.Neck

    @classmethod
    def get_hips_point(cls):
        return cls.Pelvis

    @classmethod
    def get_flip_mask(cls):
        swap = {'L': 'R', 'R': 'L'}
        return tuple(cls[swap[m.name[0]] + m.name[1:]].value if m.name[1] == '_' else m.value for m in cls)


_S = SMPL_SKELETON

# joint order of the original SMPL body model, which AMASS body poses are stored in (reference skeleton.py:9-34)
ORIGINAL_SMPL_JOINTS = ('Pelvis L_Hip R_Hip Spine1 L_Knee R_Knee Spine2 L_Ankle R_Ankle Spine3 L_Foot R_Foot Neck L_Collar '
                        'R_Collar Head L_Shoulder R_Shoulder L_Elbow R_Elbow L_Wrist R_Wrist').split()
FROM_ORIGINAL = tuple(ORIGINAL_SMPL_JOINTS.index(n) for n in _SMPL)       # SMPL_SKELETON joint s <- original joint [s]
TO_ORIGINAL = tuple(_SMPL.index(n) for n in ORIGINAL_SMPL_JOINTS)


def map_from_original(tensor):
    """(..., 66) or (..., 22, 3) in original SMPL joint order -> (..., 22, 3) in ``SMPL_SKELETON`` order (reference :132-142)."""
    if tensor.shape[-1] == len(_SMPL) * 3:
        tensor = tensor.reshape(tuple(tensor.shape[:-1]) + (len(_SMPL), 3))
    if tuple(tensor.shape[-2:]) != (len(_SMPL), 3):
        raise ValueError(f'map_from_original: (..., 66) or (..., 22, 3) expected, got {tuple(tensor.shape)}')
    return tensor[..., FROM_ORIGINAL, :]


def map_to_original(tensor, reshape=True):
    """The inverse: (..., 22, 3) in ``SMPL_SKELETON`` order -> original order, flattened to (..., 66) with ``reshape``
    (reference :144-156)."""
    if tuple(tensor.shape[-2:]) != (len(_SMPL), 3):
        raise ValueError(f'map_to_original: (..., 22, 3) expected, got {tuple(tensor.shape)}')
    mapped = tensor[..., TO_ORIGINAL, :]
    return mapped.reshape(tuple(mapped.shape[:-2]) + (len(_SMPL) * 3,)) if reshape else mapped


_S.map_from_original = staticmethod(map_from_original)       # where the reference's users look for them
_S.map_to_original = staticmethod(map_to_original)


register_skeleton('SMPL_SKELETON', _S, [
    (C.crl_hips__C, _S.Pelvis), (C.crl_spine__C, _S.Spine1), (C.crl_spine01__C, _S.Spine3),
    (C.crl_shoulder__L, _S.L_Collar), (C.crl_arm__L, _S.L_Shoulder), (C.crl_foreArm__L, _S.L_Elbow),
    (C.crl_hand__L, _S.L_Wrist), (C.crl_neck__C, _S.Neck), (C.crl_Head__C, _S.Head),
    (C.crl_shoulder__R, _S.R_Collar), (C.crl_arm__R, _S.R_Shoulder), (C.crl_foreArm__R, _S.R_Elbow),
    (C.crl_hand__R, _S.R_Wrist), (C.crl_thigh__R, _S.R_Hip), (C.crl_leg__R, _S.R_Knee), (C.crl_foot__R, _S.R_Ankle),
    (C.crl_toe__R, _S.R_Foot), (C.crl_thigh__L, _S.L_Hip), (C.crl_leg__L, _S.L_Knee), (C.crl_foot__L, _S.L_Ankle),
    (C.crl_toe__L, _S.L_Foot),
])
