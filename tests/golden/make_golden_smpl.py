#!/usr/bin/env python3
"""Generate tests/golden/smpl_to_carla.npz by RUNNING THE REFERENCE's own SMPLDataset.convert_smpl_to_carla
(data/smpl/smpl_dataset.py:103-142; build container only).

The stand-ins of make_golden.py are reused unchanged; h5py and human_body_prior (third-party, absent, not touched by the
conversion) get empty stand-in modules. The dataset object is made with ``object.__new__`` and given the four attributes
the conversion reads (its constructor wants a data file), then the reference's function runs unmodified.

Contents (data only: inputs and the reference's three fp32 outputs):
  a_*  the 68 poses of the reference's tests/data/smpl/test_amass_dataset.py:32-61 -- the zero pose, each of the 22 joints
       turned by 90 degrees about each axis, L_Shoulder + L_Elbow together -- for (adult, female) and (adult, male);
  b_*  16 random frames per skeleton type, angles uniform in +-3 rad, for all four types.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF_SRC, _module, install_standins, npz  # noqa: E402


def main():
    if not os.path.isdir(REF_SRC):
        sys.exit('reference tree not present: the committed .npz files are the artefact to use')
    install_standins()
    _module('h5py')
    _module('human_body_prior')
    try:
        import importlib_metadata  # noqa: F401
    except ImportError:
        _module('importlib_metadata', metadata=None)
    sys.path.insert(0, REF_SRC)
    from pedestrians_video_2_carla.data.carla import reference as ref_tables
    from pedestrians_video_2_carla.data.smpl.skeleton import _ORIG_SMPL_SKELETON
    from pedestrians_video_2_carla.data.smpl.smpl_dataset import SMPLDataset
    from pedestrians_video_2_carla.data.smpl.utils import get_conventions_rot

    ds = object.__new__(SMPLDataset)
    ds.device = torch.device('cpu')
    ds.nodes_len = 26
    ds.reference_axes_rot = get_conventions_rot()
    ds.reference_axes_dir = torch.tensor((-1, 1, 1))

    types_ = list(ref_tables.CARLA_REFERENCE_SKELETON_TYPES)

    def run(pose, skel_type):
        outs = [ds.convert_smpl_to_carla(pose[n:n + 1], *types_[int(t)]) for n, t in enumerate(skel_type)]
        return [torch.cat([o[i] for o in outs]) for i in range(3)]      # relative rot, absolute loc, absolute rot

    # (a) the reference's own test poses
    n_joints = len(_ORIG_SMPL_SKELETON)
    moves = torch.tensor(np.deg2rad(np.array(((0.0, 0.0, 90.0), (0.0, 90.0, 0.0), (90.0, 0.0, 0.0)))), dtype=torch.float32)
    n_a = n_joints * 3 + 2
    a_pose = torch.zeros(n_a, n_joints, 3)
    for i in range(n_joints):
        for a in range(3):
            a_pose[i * 3 + a + 1, i] = moves[a]
    a_pose[n_a - 1, _ORIG_SMPL_SKELETON.L_Shoulder.value] = moves[0]
    a_pose[n_a - 1, _ORIG_SMPL_SKELETON.L_Elbow.value] = moves[0]
    a_pose = a_pose.reshape(n_a, -1).repeat(2, 1)
    a_type = torch.tensor([0] * n_a + [1] * n_a, dtype=torch.int32)
    a_rel, a_loc, a_rot = run(a_pose, a_type)

    # (b) random frames
    g = torch.Generator().manual_seed(35)
    b_pose = (torch.rand(4 * 16, n_joints * 3, generator=g) * 2 - 1) * 3.0
    b_type = torch.arange(4, dtype=torch.int32).repeat_interleave(16)
    b_rel, b_loc, b_rot = run(b_pose, b_type)

    npz('smpl_to_carla',
        a_body_pose=a_pose, a_skel_type=a_type, a_relative_pose_rot=a_rel, a_absolute_pose_loc=a_loc, a_absolute_pose_rot=a_rot,
        b_body_pose=b_pose, b_skel_type=b_type, b_relative_pose_rot=b_rel, b_absolute_pose_loc=b_loc, b_absolute_pose_rot=b_rot)


if __name__ == '__main__':
    main()
