"""K36 (csrc/p2c_ik.hip, ``ops.locations_to_carla``, ``LocationRetargeter``) -- what runs without a GPU: the tensor definition
(walker_control/inverse_kinematics.py) pinned by its properties (the reference project has no such step, so there is no golden
file), a host run of the kernel's Procrustes step, the walker and trainer sides on host tensors, and the C-ABI surface.

Bounds. The definition is checked in fp64 to 1e-12: every step is a handful of products of unit vectors and rotations, eight
levels deep, so round-off is a few 1e-15 (measured: 1e-14 at most). ``e_ref[k]`` is the largest absolute difference, over the
round-trip inputs, between the definition run in fp32 and the same definition in fp64 on the same fp32 inputs: what one fp32
evaluation costs. It is measured here and must be finite and below 1e-4 (fp32 round-off 6e-8 through eight
levels of a few dozen operations on values <= 1.1 is 1e-5 at the very most); K36 -- in test_ik_gpu.py -- is allowed 4 * e_ref[k]
from fp64."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.data.carla import reference as ref
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON, PARENTS
from pedestrians_video_2_carla_amd.walker_control import inverse_kinematics as ik

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE_KEYS = ik.POSE_KEYS
MULTI = [j for j in range(26) if len(ik.CHILDREN[j]) > 1]
SINGLE = [j for j in range(26) if len(ik.CHILDREN[j]) == 1]
UNFITTED = [j for j in range(26) if not ik.CHILDREN[j]] + [CARLA_SKELETON.crl_root.value]      # the leaves and the root
EYE = torch.eye(3, dtype=torch.float64)


def rodrigues(axis, angle):
    """Unit ``axis`` (...,3), ``angle`` (...) -> the rotation matrices (...,3,3)."""
    K = torch.zeros(axis.shape[:-1] + (3, 3), dtype=axis.dtype)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -axis[..., 2], axis[..., 1], -axis[..., 0]
    K = K - K.transpose(-1, -2)
    s, c = torch.sin(angle)[..., None, None], torch.cos(angle)[..., None, None]
    return torch.eye(3, dtype=axis.dtype) + s * K + (1 - c) * (K @ K)


def fk(rel_loc, rel_rot):
    """``reference.forward_kinematics`` on tensors."""
    loc, rot = [None] * 26, [None] * 26
    for j, p in enumerate(PARENTS):
        if p < 0:
            loc[j], rot[j] = rel_loc[..., j, :], rel_rot[..., j, :, :]
        else:
            loc[j] = (rel_loc[..., j, None, :] @ rot[p])[..., 0, :] + loc[p]
            rot[j] = rel_rot[..., j, :, :] @ rot[p]
    return torch.stack(loc, -2), torch.stack(rot, -3)


def tables(skel_type):
    return tuple(t[skel_type.long()] for t in ref.get_relative_tensors(dtype=torch.float64))


@functools.lru_cache(maxsize=None)
def round_trip(scale=0.3, N=256, seed=36):
    """(skel_type (N,), relative rotations (N,26,3,3), their FK locations and absolute rotations), fp64: random rotations about
    random axes, angles ~ N(0, scale^2), on top of the reference pose, the four types cycling."""
    g = torch.Generator().manual_seed(seed)
    skel_type = (torch.arange(N) % 4).to(torch.int32)
    rel_loc, ref_rot = tables(skel_type)
    axis = torch.randn(N, 26, 3, generator=g, dtype=torch.float64)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    rot = rodrigues(axis, torch.randn(N, 26, generator=g, dtype=torch.float64) * scale) @ ref_rot
    loc, abs_rot = fk(rel_loc, rot)
    return skel_type, rot, loc, abs_rot


@functools.lru_cache(maxsize=None)
def fixture():
    """The round-trip locations as fp32 inputs: (loc (256,26,3) fp32, skel_type (256,) int32)."""
    skel_type, _, loc, _ = round_trip()
    return loc.float(), skel_type


@functools.lru_cache(maxsize=None)
def truth():
    """The fp64 definition on the fixture's fp32 inputs, and e_ref per pose output (fp32 definition against it)."""
    loc, skel_type = fixture()
    t64 = ik.fit_carla_rotations(loc.double(), skel_type)
    t32 = ik.fit_carla_rotations(loc, skel_type)
    return t64, {k: float((t32[k].double() - t64[k]).abs().max()) for k in POSE_KEYS}


# ---------------------------------------------------------------------------------------------------------- the definition
def test_tree_tables():
    assert [CARLA_SKELETON(j).name for j in MULTI] == ['crl_hips__C', 'crl_spine01__C', 'crl_Head__C']
    assert ik.CHILDREN[1] == (2, 16, 21) and ik.CHILDREN[3] == (4, 8, 12) and ik.CHILDREN[9] == (10, 11)
    assert all(ik.CHILDREN[j] == (j + 1,) for j in SINGLE)            # DFS order: a single child is the next bone
    assert len(SINGLE) + len(MULTI) + len(UNFITTED) - 1 == 26 and CARLA_SKELETON.crl_root.value in SINGLE
    rel_loc, _ = ref.get_relative_tensors(dtype=torch.float64)
    assert float(rel_loc[:, CARLA_SKELETON.crl_hips__C.value].abs().max()) == 0.0        # the root never has a usable child
    # the child sets of the Procrustes bones are far from collinear in every skeleton
    for j in MULTI:
        unit = rel_loc[:, list(ik.CHILDREN[j])]
        unit = unit / unit.norm(dim=-1, keepdim=True)
        assert float(torch.linalg.svdvals(unit)[:, 1].min()) >= 0.37, j


@pytest.mark.parametrize('scale', [0.3, 1.0, 3.0])
def test_fk_ik_fk_round_trip(scale):
    skel_type, _, loc, abs_rot = round_trip(scale)
    rel_loc, _ = tables(skel_type)
    out = ik.fit_carla_rotations(loc, skel_type)
    again, again_rot = fk(rel_loc, out['relative_pose_rot'])
    err = {'fk_of_fit': float((again - loc).abs().max()), 'absolute_pose_loc': float((out['absolute_pose_loc'] - loc).abs().max()),
           'fk_rot_of_fit': float((again_rot - out['absolute_pose_rot']).abs().max()),
           'procrustes_bones': float((out['absolute_pose_rot'][:, MULTI] - abs_rot[:, MULTI]).abs().max())}
    print(scale, err)
    assert all(e <= 1e-12 for e in err.values()), err
    if scale == 0.3:      # the shortest arc stays far from the half turn on these inputs
        for j in SINGLE[1:]:
            c = j + 1
            u = rel_loc[:, c, None, :] @ ref.get_relative_tensors(dtype=torch.float64)[1][skel_type.long()][:, j] @ out['absolute_pose_rot'][:, PARENTS[j]]
            u = u[:, 0] / u[:, 0].norm(dim=-1, keepdim=True)
            v = loc[:, c] - loc[:, j]
            v = v / v.norm(dim=-1, keepdim=True)
            assert float((u + v).norm(dim=-1).min()) >= 1.0, j
    # idempotent on its own re-targeted pose
    twice = ik.fit_carla_rotations(out['absolute_pose_loc'], skel_type)
    for k in POSE_KEYS:
        assert float((twice[k] - out[k]).abs().max()) <= 1e-12, k


def test_reference_pose_gives_the_reference_rotations():
    skel_type = torch.arange(4)
    rel_loc, ref_rot = tables(skel_type)
    abs_loc, abs_rot = (t.double() for t in ref.get_absolute_tensors(dtype=torch.float64))
    out = ik.fit_carla_rotations(abs_loc, skel_type)
    assert float((out['relative_pose_rot'] - ref_rot).abs().max()) <= 1e-12
    assert float((out['absolute_pose_rot'] - abs_rot).abs().max()) <= 1e-12
    assert float((out['absolute_pose_loc'] - abs_loc).abs().max()) <= 1e-12
    assert torch.equal(out['relative_pose_rot'][:, UNFITTED], ref_rot[:, UNFITTED])          # copied, not re-derived
    fitted = [j for j in range(26) if j not in UNFITTED]
    assert not torch.equal(out['relative_pose_rot'][:, fitted], ref_rot[:, fitted])          # ... which the others are


def test_all_zero_frame_is_the_reference_pose_bit_for_bit():
    for dtype in (torch.float64, torch.float32):
        skel_type = torch.tensor([0, 1, 2, 3, 1])
        _, ref_rot = (t[skel_type] for t in ref.get_relative_tensors(dtype=dtype))
        out = ik.fit_carla_rotations(torch.zeros(5, 26, 3, dtype=dtype), skel_type)
        assert torch.equal(out['relative_pose_rot'], ref_rot)
        # a frame whose joints coincide anywhere else is the same frame
        out = ik.fit_carla_rotations(torch.full((5, 26, 3), 2.5, dtype=dtype), skel_type)
        assert torch.equal(out['relative_pose_rot'], ref_rot)
    abs_loc, abs_rot = ref.get_absolute_tensors(dtype=torch.float64)
    out = ik.fit_carla_rotations(torch.zeros(4, 26, 3, dtype=torch.float64), torch.arange(4))
    assert float((out['absolute_pose_loc'] - abs_loc).abs().max()) <= 1e-12 and float((out['absolute_pose_rot'] - abs_rot).abs().max()) <= 1e-12


def test_translation_and_uniform_scale_do_not_matter():
    skel_type, _, loc, _ = round_trip()
    out = ik.fit_carla_rotations(loc, skel_type)
    moved = ik.fit_carla_rotations(1.7 * loc + torch.tensor([0.3, -1.1, 2.0], dtype=torch.float64), skel_type)
    for k in POSE_KEYS:
        assert float((moved[k] - out[k]).abs().max()) <= 1e-12, k
    # bone lengths that differ from the reference skeleton's: another type's locations give that pose on this type's bones
    other = ik.fit_carla_rotations(loc, (skel_type + 1) % 4, want=('absolute_pose_loc',))['absolute_pose_loc']
    back = ik.fit_carla_rotations(other, skel_type, want=('absolute_pose_loc',))['absolute_pose_loc']
    assert float((back - loc).abs().max()) <= 1e-12


def test_random_locations_give_finite_proper_rotations():
    g = torch.Generator().manual_seed(3)
    out = ik.fit_carla_rotations(torch.randn(512, 26, 3, generator=g, dtype=torch.float64), torch.arange(512) % 4)
    A = out['absolute_pose_rot']
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(out['relative_pose_rot']).all())
    assert float((A @ A.transpose(-1, -2) - EYE).abs().max()) <= 1e-12
    assert float(torch.linalg.det(A).min()) > 0.0


def test_antiparallel_bone_takes_the_half_turn_about_the_named_axis():
    g = torch.Generator().manual_seed(4)
    u = torch.randn(64, 3, generator=g, dtype=torch.float64)
    u[0], u[1], u[2], u[3] = torch.tensor([1.0, 0, 0]), torch.tensor([0, -1.0, 0]), torch.tensor([0.6, 0.6, 0.5]), torch.tensor([2.0, 1, 1])
    u = u / u.norm(dim=-1, keepdim=True)
    S = ik.shortest_arc(u, -u)
    assert float(((u.unsqueeze(-2) @ S)[:, 0] + u).abs().max()) <= 1e-12
    assert float((S @ S.transpose(-1, -2) - EYE).abs().max()) <= 1e-12 and float((torch.linalg.det(S) - 1).abs().max()) <= 1e-12
    mag = u.abs()
    k = [min(range(3), key=lambda i: (float(m[i]), i)) for m in mag]              # smallest |u_k|, lowest index on ties
    assert k[:4] == [1, 0, 2, 1]
    a = torch.linalg.cross(u, torch.eye(3, dtype=torch.float64)[k])
    a = a / a.norm(dim=-1, keepdim=True)
    assert float((S - (2 * a.unsqueeze(-1) * a.unsqueeze(-2) - EYE)).abs().max()) <= 1e-15
    assert float(((a.unsqueeze(-2) @ S)[:, 0] - a).abs().max()) <= 1e-12          # the axis stays
    # just above the threshold the half-vector form still turns u onto v
    # (|u + v| = 3e-6 is known to 1e-16: the half vector to 1e-10)
    v = (u.unsqueeze(-2) @ rodrigues(torch.linalg.cross(u, a), torch.full((64,), np.pi - 3e-6, dtype=torch.float64)))[:, 0]
    assert float(((u + v) ** 2).sum(-1).min()) > ik.ANTIPARALLEL_EPS
    near = ik.shortest_arc(u, v)
    assert float(((u.unsqueeze(-2) @ near)[:, 0] - v).abs().max()) <= 1e-9
    # through the fit: the left forearm folded back onto the arm exactly
    arm, forearm = CARLA_SKELETON.crl_arm__L.value, CARLA_SKELETON.crl_foreArm__L.value
    abs_loc, abs_rot = ref.get_absolute_tensors(dtype=torch.float64)
    loc = abs_loc.clone()
    loc[:, forearm] = abs_loc[:, arm] - (abs_loc[:, forearm] - abs_loc[:, arm])
    out = ik.fit_carla_rotations(loc, torch.arange(4), want=('absolute_pose_rot', 'absolute_pose_loc'))
    A = out['absolute_pose_rot'][:, arm]
    assert float((out['absolute_pose_loc'][:, forearm] - loc[:, forearm]).abs().max()) <= 1e-12
    assert float((A @ A.transpose(-1, -2) - EYE).abs().max()) <= 1e-12 and float((torch.linalg.det(A) - 1).abs().max()) <= 1e-12
    assert float((out['absolute_pose_rot'][:, :arm] - abs_rot[:, :arm]).abs().max()) <= 1e-12     # nothing above it moved


def child_correlations(loc, skel_type):
    """H (N,3,3,3) of the three Procrustes bones, as the definition forms it."""
    rel_loc, _ = tables(skel_type)
    out = []
    for j in MULTI:
        H = torch.zeros(loc.shape[0], 3, 3, dtype=torch.float64)
        for c in ik.CHILDREN[j]:
            r, _ = ik._unit(rel_loc[:, c])
            d, _ = ik._unit(loc[:, c] - loc[:, j])
            H = H + d.unsqueeze(-1) * r.unsqueeze(-2)
        out.append(H)
    return torch.stack(out, 1)


def test_host_run_of_the_kernels_procrustes_step_matches_the_svd(tmp_path):
    """p2c_procrustes::solve -- what the three Procrustes lanes of K36 call, unchanged -- compiled for the host, against the
    SVD of the definition on the three child sets of 64 frames (angle scale 1: well away from the reference pose)."""
    compiler = next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    assert compiler is not None, 'no host C++ compiler'
    exe = str(tmp_path / 'ik_procrustes_host')
    subprocess.run([compiler, '-O2', '-std=c++17', '-I', os.path.join(ROOT, 'pedestrians_video_2_carla_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'ik_procrustes_host.cpp'), '-o', exe], check=True)
    skel_type, _, loc, abs_rot = round_trip(1.0)
    H = child_correlations(loc[:64], skel_type[:64])
    H.numpy().tofile(str(tmp_path / 'h.bin'))
    subprocess.run([exe, str(tmp_path / 'h.bin'), str(tmp_path / 'r.bin')], check=True)
    R = torch.from_numpy(np.fromfile(str(tmp_path / 'r.bin'), dtype=np.float64).reshape(64, 3, 3, 3))
    want = ik.procrustes(H)
    err = float((R - want).abs().max())
    print(f'host solve against the SVD: {err:.3e}')
    assert err <= 1e-12 and float((R - abs_rot[:64, MULTI]).abs().max()) <= 1e-12


def test_procrustes_of_a_non_finite_matrix_is_nan_and_of_one_direction_a_proper_rotation():
    H = torch.zeros(3, 3, 3, dtype=torch.float64)
    H[0, 0, 0] = float('nan')
    H[1] = torch.tensor([0.0, 0.6, 0.8]).double().unsqueeze(-1) * torch.tensor([1.0, 0.0, 0.0]).double().unsqueeze(-2)
    H[2, 1, 2] = float('inf')
    R = ik.procrustes(H)
    assert bool(torch.isnan(R[0]).all()) and bool(torch.isnan(R[2]).all())
    assert bool(torch.isfinite(R[1]).all()) and float((R[1] @ R[1].T - EYE).abs().max()) <= 1e-12 and float(torch.linalg.det(R[1])) > 0


def nan_joint_cases():
    return [CARLA_SKELETON.crl_hips__C.value, CARLA_SKELETON.crl_spine01__C.value, CARLA_SKELETON.crl_foreArm__L.value,
            CARLA_SKELETON.crl_toeEnd__R.value]


def expected_nan(joint):
    """Which bones are NaN per pose output when ``joint`` alone is NaN in an ordinary frame (every child but the hips usable). A
    bone with several children is fitted without its parent: a NaN above it stops there for the absolute rotations, but not for
    the relative rotation (A[j] A[parent]^T) nor for the locations, which add up along the path."""
    nan_abs, nan_rel, nan_loc = ([False] * 26 for _ in range(3))
    for j, parent in enumerate(PARENTS):
        reads = [c for c in ik.CHILDREN[j] if j != CARLA_SKELETON.crl_root.value]
        own = bool(reads) and joint in [j] + reads
        above = parent >= 0 and nan_abs[parent]
        nan_abs[j] = own or (above and len(reads) <= 1)
        nan_rel[j] = bool(reads) and (nan_abs[j] or above)
        nan_loc[j] = parent >= 0 and (nan_loc[parent] or above)
    return torch.tensor(nan_abs), torch.tensor(nan_rel), torch.tensor(nan_loc)


@pytest.mark.parametrize('joint', nan_joint_cases())
def test_one_nan_joint_goes_where_the_arithmetic_takes_it(joint):
    """Nothing is masked: a NaN joint makes the fits that read it NaN -- its own bone's and its parent's -- and every prior
    below them, down to the next bone with several children."""
    loc, skel_type = fixture()
    loc = loc[:4].double().clone()
    clean = ik.fit_carla_rotations(loc, skel_type[:4])
    loc[1, joint] = float('nan')
    out = ik.fit_carla_rotations(loc, skel_type[:4])
    nan_abs, nan_rel, nan_loc = expected_nan(joint)
    assert int(nan_abs.sum()) == {1: 12, 3: 11, 6: 3, 20: 2}[joint]
    assert torch.equal(torch.isnan(out['absolute_pose_rot'][1]).all(-1).all(-1), nan_abs)
    assert torch.equal(torch.isnan(out['absolute_pose_rot'][1]).any(-1).any(-1), nan_abs)
    assert torch.equal(torch.isnan(out['relative_pose_rot'][1]).any(-1).any(-1), nan_rel)
    assert torch.equal(torch.isnan(out['absolute_pose_loc'][1]).any(-1), nan_loc)
    for k in POSE_KEYS:
        assert torch.equal(out[k][[0, 2, 3]], clean[k][[0, 2, 3]]), k
        keep = ~torch.isnan(out[k][1])
        assert torch.equal(out[k][1][keep], clean[k][1][keep]), k


def test_e_ref_of_an_fp32_evaluation():
    _, e_ref = truth()
    for k, e in e_ref.items():
        print(f'e_ref[{k}] = {e:.3e}')
        assert np.isfinite(e) and 0.0 < e < 1e-4, k


# ------------------------------------------------------------------------------------------------------------------- ops
def test_ops_dispatch_on_host_tensors_shapes_and_refusals():
    loc, skel_type = fixture()
    assert ops.IK_CARLA_OUTPUTS == ('relative_pose_rot', 'absolute_pose_loc', 'absolute_pose_rot', 'bones', 'root')
    clips, st = loc[:60].reshape(4, 15, 26, 3), torch.tensor([3, 0, 2, 1], dtype=torch.int32)
    flat = ops.locations_to_carla(clips.reshape(60, 26, 3), st.repeat_interleave(15))
    out = ops.locations_to_carla(clips, st)
    assert set(out) == set(POSE_KEYS) and out['absolute_pose_loc'].shape == (4, 15, 26, 3)
    for k in POSE_KEYS:
        assert out[k].dtype == torch.float32 and torch.equal(out[k].reshape(flat[k].shape), flat[k]), k
    # the rows are K30's, of the reference locations and the relative rotations
    wl, wr = torch.randn(4, 15, 3), out['absolute_pose_rot'][:, :, 5]
    rows = ops.locations_to_carla(clips, st, wl, wr, want=('bones', 'root'))
    ref_loc, _ = ref.get_relative_tensors()
    bones, root = ops.carla_pose_export(ref_loc[st.long()][:, None].expand(4, 15, 26, 3), out['relative_pose_rot'], wl, wr)
    assert set(rows) == {'bones', 'root'} and torch.equal(rows['bones'], bones) and torch.equal(rows['root'], root)
    assert ops.locations_to_carla(clips.double(), st)['relative_pose_rot'].dtype == torch.float64
    assert ops.locations_to_carla(clips[:0], st[:0])['absolute_pose_loc'].shape == (0, 15, 26, 3)
    assert not ops.locations_to_carla(clips.requires_grad_(True), st)['relative_pose_rot'].requires_grad
    clips = clips.detach()
    for bad in (lambda: ops.locations_to_carla(clips[..., :25, :], st), lambda: ops.locations_to_carla(clips, st[:3]),
                lambda: ops.locations_to_carla(clips[..., :2], st), lambda: ops.locations_to_carla(clips.long(), st),
                lambda: ops.locations_to_carla(clips, st, wl, None), lambda: ops.locations_to_carla(clips, st, want=('root',)),
                lambda: ops.locations_to_carla(clips, st, want=()), lambda: ops.locations_to_carla(clips, st, want=('pose',)),
                lambda: ops.locations_to_carla(clips, st.float()), lambda: ops.locations_to_carla(clips[0, 0], st[:0]),
                lambda: ops.locations_to_carla(clips, st, wl[:, :3], wr[:, :3], want=('root',))):
        with pytest.raises(RuntimeError):
            bad()


# ----------------------------------------------------------------------------------------------------- walker / trainer side
class LocationProjection(torch.nn.Module):
    """The stand-in of test_carla_pose.HostProjection for a model that outputs absolute locations: the build's pose head is a
    device kernel, so the host flow takes de-normalisation and projection from the oracle (fp32 in, fp32 out)."""

    def on_batch_start(self, batch, batch_idx):
        self._skel_type = ref.skeleton_types_from_meta(batch[2], batch_size=len(batch[0]), strict=True)

    def forward(self, pose_inputs, world_loc_changes=None, world_rot_changes=None, identity_world=False):
        from oracle import pose_head as O
        loc, rot = pose_inputs if isinstance(pose_inputs, tuple) else (pose_inputs, None)
        o = O.pose_head(loc, 'absolute_loc', self._skel_type, None if identity_world else world_loc_changes,
                        None if identity_world else world_rot_changes, transform='none')
        out = {k: o[k].contiguous() for k in ('absolute_pose_loc', 'world_loc', 'world_rot')}
        out.update(relative_pose_loc=None, relative_pose_rot=None, absolute_pose_rot=rot)
        return o['projection_2d'], out


def location_flow(output_type='absolute_loc'):
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    from test_carla_pose import HostDataModule
    torch.manual_seed(12)
    model = LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, movements_output_type=output_type)
    flow = LitPoseLiftingFlow(movements_model=model, loss_modes=['loc_2d_3d'])
    flow.projection = LocationProjection()
    flow.attach_datamodule(HostDataModule())
    return flow


def test_retargeter_leaves_the_predict_step_dict_and_the_rows_of_its_export():
    from pedestrians_video_2_carla_amd.walker_control.carla_pose import CarlaPose, export_clips
    from pedestrians_video_2_carla_amd.walker_control.location_retargeter import LocationRetargeter
    loc, _ = fixture()
    loc = loc[:12].reshape(3, 4, 26, 3)
    meta = {'age': ['adult', 'child', 'nan'], 'gender': ['male', 'neutral', 'female']}
    st = torch.tensor([1, 2, 0])                 # (adult, male); (child, neutral -> female); (nan -> adult, female)
    r = LocationRetargeter()
    sliced = r.retarget(loc, meta)
    assert set(sliced) == {'relative_pose_loc', 'relative_pose_rot', 'absolute_pose_loc', 'absolute_pose_rot', 'world_loc', 'world_rot'}
    ref_loc, _ = ref.get_relative_tensors()
    assert torch.equal(sliced['relative_pose_loc'], ref_loc[st][:, None].expand(3, 4, 26, 3))
    assert float(sliced['world_loc'].abs().sum()) == 0.0 and torch.equal(sliced['world_rot'], torch.eye(3).expand(3, 4, 3, 3))
    direct = ik.fit_carla_rotations(loc, st)
    for k in POSE_KEYS:
        assert torch.equal(sliced[k], direct[k]), k
    assert torch.equal(r.retarget(loc, st.int())['relative_pose_rot'], direct['relative_pose_rot'])
    # the dict of predict_step, its world tensors used
    wl, wr = torch.randn(3, 4, 3), direct['absolute_pose_rot'][:, :, 7]
    predicted = {'absolute_pose_loc': loc, 'world_loc': wl, 'world_rot': wr, 'projection_2d': torch.zeros(3, 4, 26, 2)}
    again = r.retarget((predicted, meta))
    assert torch.equal(again['world_loc'], wl) and torch.equal(again['relative_pose_rot'], direct['relative_pose_rot'])
    bones, root = r.export(predicted, meta)
    want_bones, want_root = export_clips(again)
    assert np.array_equal(bones.numpy(), want_bones) and np.array_equal(root.numpy(), want_root)
    poses, _ = CarlaPose().clips_to_transforms(again)
    assert poses[2][1]['crl_arm__L'].rotation.yaw == pytest.approx(float(bones[2, 1, 5, 4]))
    _, root0 = r.export(loc, meta)
    assert float(root0.abs().sum()) == 0.0                     # no world: the identity world's row
    with pytest.raises(KeyError):
        r.retarget({'relative_pose_rot': direct['relative_pose_rot']}, meta)
    with pytest.raises(RuntimeError):
        r.retarget(loc[..., :25, :], meta)
    with pytest.raises(RuntimeError):
        r.retarget(loc)                                        # which skeleton?


def test_retargeter_refuses_other_output_nodes_and_rotation_models():
    from pedestrians_video_2_carla_amd.data.openpose.skeleton import BODY_25_SKELETON
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    from pedestrians_video_2_carla_amd.walker_control.location_retargeter import LocationRetargeter
    from test_carla_pose import host_batches, host_flow

    class Flow:
        training = False

        def __init__(self, model):
            self.movements_model = model

    other = Flow(LinearAE(input_nodes=CARLA_SKELETON, output_nodes=BODY_25_SKELETON, movements_output_type='absolute_loc'))
    with pytest.raises(RuntimeError, match='CARLA_SKELETON'):
        LocationRetargeter().lift(other, host_batches(1, 2, 3)[0])
    rotations = host_flow(LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON))
    with pytest.raises(RuntimeError, match='absolute locations'):
        LocationRetargeter().lift(rotations, host_batches(1, 2, 3)[0])


@pytest.mark.parametrize('output_type', ['absolute_loc', 'absolute_loc_rot'])
def test_predict_carla_with_ik_plays_a_location_model(output_type):
    from pedestrians_video_2_carla_amd.trainer import Trainer
    from pedestrians_video_2_carla_amd.walker_control.location_retargeter import LocationRetargeter
    from test_carla_pose import host_batches
    flow = location_flow(output_type)
    batches = host_batches(2, 2, 3)
    flow.train()
    if output_type == 'absolute_loc':
        with pytest.warns(UserWarning, match='one-launch path'):
            with pytest.raises(KeyError):
                Trainer().predict_carla(flow, batches)             # the default is unchanged
        assert flow.training
    got = Trainer().predict_carla(flow, batches, ik=True)
    assert flow.training and len(got) == 2
    sl = flow.movements_model.eval_slice
    frames_out = len(range(3)[sl])
    for (bones, root, meta), batch in zip(got, batches):
        assert meta is batch[2] and bones.shape == (2, frames_out, 26, 6) and root.shape == (2, frames_out, 6)
        assert bool(torch.isfinite(bones).all()) and bool(torch.isfinite(root).all())
        sliced, _ = flow.eval().predict_step(batch, 0)
        flow.train()
        assert sliced.get('relative_pose_rot') is None                       # nothing for export_clips to export
        want_bones, want_root = LocationRetargeter().export(sliced, meta)
        assert torch.equal(bones, want_bones) and torch.equal(root, want_root)
        # the rows are those of the fit of the predicted locations, whatever rotations the model has of its own
        st = ref.skeleton_types_from_meta(meta)
        fit = ik.fit_carla_rotations(sliced['absolute_pose_loc'], st, want=('bones',))
        assert torch.equal(bones, fit['bones'])


def test_predict_carla_with_ik_leaves_rotation_models_on_their_own_path():
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    from pedestrians_video_2_carla_amd.trainer import Trainer
    from test_carla_pose import host_batches, host_flow
    torch.manual_seed(2)
    flow = host_flow(LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON))
    batches = host_batches(1, 2, 3)
    plain, with_ik = Trainer().predict_carla(flow, batches), Trainer().predict_carla(flow, batches, ik=True)
    assert torch.equal(plain[0][0], with_ik[0][0]) and torch.equal(plain[0][1], with_ik[0][1])


def test_ik_carla_animation_round_trips_through_load(tmp_path):
    from pedestrians_video_2_carla_amd.data.carla.animation import ik_carla_animation, load_carla_animation
    from pedestrians_video_2_carla_amd.trainer import Trainer
    from test_carla_pose import host_batches
    flow = location_flow()
    batches = host_batches(2, 2, 3)
    got = load_carla_animation(ik_carla_animation(str(tmp_path / 'ik'), flow, batches, fps=25.0))
    rows = Trainer().predict_carla(flow, batches, ik=True)
    assert got['bones'].shape == (4, 3, 26, 6) and got['root'].shape == (4, 3, 6) and got['fps'] == 25.0
    assert np.array_equal(got['bones'], torch.cat([r[0] for r in rows]).numpy())
    assert np.array_equal(got['root'], torch.cat([r[1] for r in rows]).numpy())
    assert got['bone_names'] == [m.name for m in CARLA_SKELETON]
    assert got['age'] == batches[0][2]['age'] + batches[1][2]['age'] and got['gender'] == batches[0][2]['gender'] + batches[1][2]['gender']
    with pytest.raises(ValueError):
        ik_carla_animation(str(tmp_path / 'none'), flow, [])


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_k36_symbol_is_declared_bound_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    header = open(os.path.join(ROOT, 'include', 'p2c.h')).read()
    declared = set(re.findall(r'P2C_API[^;(]*?\b(p2c_\w+)\s*\(', header))
    name = 'p2c_loc_to_carla_fwd'
    assert name in declared and name in _lib.SYMBOLS and getattr(_lib.lib(), name) is not None
    res, args = _lib.SYMBOLS[name]
    assert res is ctypes.c_int and args[-1] is ctypes.c_void_p and name in _lib._PoisonedLib(_lib.lib())._wrap
    decl = re.search(r'P2C_API int p2c_loc_to_carla_fwd\((.*?)\);', header, re.S).group(1)
    params = [' '.join(p.split()) for p in decl.split(',')]
    ctype = {'const float *': ctypes.c_void_p, 'float *': ctypes.c_void_p, 'const int32_t *': ctypes.c_void_p, 'void *': ctypes.c_void_p,
             'int64_t ': ctypes.c_int64, 'int32_t ': ctypes.c_int32}
    assert [ctype[re.match(r'(.*?)(\w+)$', p).group(1)] for p in params] == list(args)
    assert [re.match(r'(.*?)(\w+)$', p).group(2) for p in params] == [
        'loc', 'skel_type', 'frames_per_type', 'ref_rel_loc', 'ref_rel_rot', 'world_loc', 'world_rot', 'relative_pose_rot',
        'absolute_pose_loc', 'absolute_pose_rot', 'bones', 'root', 'N', 'max_blocks', 'stream']
    # the kernel file shares the Procrustes and row arithmetic, allocates no LDS and needs no inline assembly
    source = open(os.path.join(ROOT, 'pedestrians_video_2_carla_amd', 'csrc', 'p2c_ik.hip')).read()
    assert '#include "p2c_procrustes_dev.h"' in source and '#include "p2c_carla_dev.h"' in source
    assert 'p2c_procrustes::solve(' in source and 'p2c_carla::carla_row(' in source
    assert '__shared__' not in source and 'asm' not in source.replace('__launch_bounds__', '') and '__syncthreads' not in source


def test_kernel_tree_tables_match_parents():
    """The per-lane depth and child tables of csrc/p2c_ik.hip, read from the source, against ``PARENTS``."""
    source = open(os.path.join(ROOT, 'pedestrians_video_2_carla_amd', 'csrc', 'p2c_ik.hip')).read()
    numbers = lambda text: [int(x) for x in text.replace('\n', ' ').split(',')]                    # noqa: E731
    depth = numbers(re.search(r'c_depth\[ph::GROUP\] = \{(.*?)\};', source, re.S).group(1))
    rows = [numbers(r) for r in re.findall(r'\{([^{}]*)\}', re.search(r'c_child\[3\]\[ph::GROUP\] = \{(.*?)\};', source, re.S).group(1))]
    want = []
    for parent in PARENTS:
        want.append(0 if parent < 0 else want[parent] + 1)
    assert len(depth) == 32 and depth[:26] == want and all(d >= 8 for d in depth[26:]) and max(want) == 7
    assert int(re.search(r'kLevels = (\d+)', source).group(1)) == 8
    assert len(rows) == 3 and all(len(r) == 32 for r in rows)
    for lane in range(32):
        assert [r[lane] for r in rows if r[lane] >= 0] == (list(ik.CHILDREN[lane]) if lane < 26 else []), lane


def test_k36_refusals_need_no_launch():
    """Every refusal comes back before anything is launched, so they can be asked for without a GPU; the pointers are host
    addresses that are never followed."""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    fwd = _lib.lib().p2c_loc_to_carla_fwd
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def call(loc=p, st=p, fpt=1, rloc=p, rrot=p, wl=None, wr=None, outs=(p, None, None, None, None), N=1, cap=0):
        return fwd(loc, st, fpt, rloc, rrot, wl, wr, *outs, N, cap, None)

    assert call(N=-1) == -2 and call(fpt=0) == -2 and call(cap=-1) == -2
    assert call(N=-1, loc=None) == -2                       # the shape is looked at first
    for missing in ('loc', 'st', 'rloc', 'rrot'):
        assert call(**{missing: None}) == -1, missing
    assert call(outs=(None,) * 5) == -1                     # no output at all
    assert call(wl=p) == -1 and call(wr=p) == -1            # one world input without the other
    assert call(outs=(None, None, None, None, p)) == -1     # a root row of no world
    assert call(N=0) == 0 and call(N=0, wl=p, wr=p, outs=(p,) * 5) == 0      # nothing to do, nothing launched
