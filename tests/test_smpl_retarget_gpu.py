"""GPU: K35 (csrc/p2c_smpl.hip, ``ops.smpl_to_carla``) against the fp64 tensor definition (data/smpl/retarget.py) on the same
fp32 inputs, and against itself.

Bound: |kernel - fp64 definition| <= 4 * e_ref per pose output, e_ref measured from the fixture alone (the reference's fp32
outputs against the fp64 definition, test_smpl_retarget.py). The margin is 4x because the kernel orders the 3x3 products
differently (closed-form Euler matrix, pointer-doubling forward kinematics) and contracts multiply-adds, each of which moves a
result by a few ulp of values <= 1.1. Everything else here is bit for bit: grid regimes, runs, output subsets, per-type calls and
the rows, which must be K30's on K35's own rotations. Measured ratios: DESIGN section 4, K35."""
import functools
import itertools

import numpy as np
import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.data.carla import reference as ref
from pedestrians_video_2_carla_amd.data.smpl import retarget
from test_smpl_retarget import POSE_KEYS, bones_of_original_joint, expected_nan, fixture, truth

pytestmark = pytest.mark.gpu

ALL = ops.SMPL_CARLA_OUTPUTS
TAIL = {'relative_pose_rot': (26, 3, 3), 'absolute_pose_loc': (26, 3), 'absolute_pose_rot': (26, 3, 3), 'bones': (26, 6), 'root': (6,)}


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def problem(N):
    """N frames on the host: the fixture's random frames repeated with a per-repeat offset, types cycling, a world per frame."""
    pose, _, _ = fixture()
    g = torch.Generator().manual_seed(1000 + N)
    reps = -(-N // 64)
    body = (pose[136:].repeat(reps, 1) + 0.37 * torch.arange(reps).repeat_interleave(64)[:, None])[:N].contiguous()
    skel_type = (torch.arange(N) % 4).to(torch.int32)
    from pedestrians_video_2_carla_amd.transforms.rotation_conversions import euler_angles_to_matrix
    world_loc = torch.randn(N, 3, generator=g)
    world_rot = euler_angles_to_matrix((torch.rand(N, 3, generator=g) * 2 - 1) * 1.2, 'XYZ')
    return body, skel_type, world_loc, world_rot


def run_all(N, max_blocks=0):
    body, skel_type, wl, wr = (t.to(dev()) for t in problem(N))
    return ops.smpl_to_carla(body, skel_type, wl, wr, want=ALL, max_blocks=max_blocks)


@functools.lru_cache(maxsize=None)
def baseline(N):
    """The all-outputs call at the kernel's own grid, on the host: what every other regime must reproduce bit for bit."""
    return {k: v.cpu() for k, v in run_all(N).items()}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- parity
def test_fixture_parity_within_four_e_ref():
    pose, skel_type, _ = fixture()
    t64, e_ref = truth()
    got = ops.smpl_to_carla(pose.to(dev()), skel_type.to(dev()))
    assert set(got) == set(POSE_KEYS)
    for k in POSE_KEYS:
        assert got[k].is_cuda and got[k].dtype == torch.float32
        err = float((got[k].double().cpu() - t64[k]).abs().max())
        print(f'{k}: K35 {err:.3e} from fp64, e_ref {e_ref[k]:.3e}, ratio {err / e_ref[k]:.2f} (allowed 4)')
        assert np.isfinite(err) and err <= 4 * e_ref[k], k


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize('N', [1, 2, 3, 31, 32, 33, 127, 128, 129, 1025])
def test_every_grid_regime_and_a_second_run_give_the_same_bits(N):
    """8 frames per workgroup: N = 1025 at max_blocks = 1 makes every lane group stride 128 times (and once more for one)."""
    want = baseline(N)
    body, skel_type, _, _ = problem(N)
    t64 = retarget.convert_smpl_to_carla(body.double(), skel_type)
    _, e_ref = truth()
    for k in POSE_KEYS:
        assert want[k].shape == (N,) + TAIL[k]
        err = float((want[k].double() - t64[k]).abs().max())
        assert np.isfinite(err) and err <= 4 * e_ref[k], (k, err)
    for max_blocks in (0, 1, 2):
        got = run_all(N, max_blocks)
        for k in ALL:
            assert same_bits(got[k], want[k]), (k, max_blocks)


def test_clips_with_one_type_each_equal_per_type_calls():
    body, _, wl, wr = (t[:15].reshape(5, 3, -1).to(dev()) for t in problem(33))
    wr = wr.reshape(5, 3, 3, 3)
    skel_type = torch.tensor([0, 1, 2, 3, 1], dtype=torch.int32, device=dev())
    got = ops.smpl_to_carla(body, skel_type, wl, wr, want=ALL)
    for k in ALL:
        assert got[k].shape == (5, 3) + TAIL[k]
    for b in range(5):
        one = ops.smpl_to_carla(body[b], skel_type[b:b + 1].expand(3), wl[b], wr[b], want=ALL)
        for k in ALL:
            assert same_bits(got[k][b], one[k]), (k, b)
    # int64 types, as a loader's meta may hold them
    again = ops.smpl_to_carla(body, skel_type.long(), wl, wr, want=ALL)
    assert all(same_bits(again[k], got[k]) for k in ALL)
    # types still on the host are moved, not a reason to leave the kernel
    moved = ops.smpl_to_carla(body, skel_type.cpu(), wl, wr, want=ALL)
    assert all(same_bits(moved[k], got[k]) for k in ALL)


# ------------------------------------------------------------------------------------------------------ output selection
def test_every_subset_of_outputs_has_the_bits_of_the_full_call_and_writes_nothing_else():
    """Straight through the C ABI, so that the buffers not asked for exist: they keep their prefill."""
    N = 33
    want = baseline(N)
    body, skel_type, wl, wr = (t.to(dev()) for t in problem(N))
    ref_loc, ref_rot = ref.get_relative_tensors(dev())
    _, ref_abs = ref.get_absolute_tensors(dev())
    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    fill = -7.25
    for r in range(1, len(ALL) + 1):
        for subset in itertools.combinations(ALL, r):
            bufs = {k: torch.full((N,) + TAIL[k], fill, device=dev()) for k in ALL}
            rc = lib.p2c_smpl_to_carla_fwd(body.data_ptr(), skel_type.data_ptr(), 1, ref_loc.data_ptr(), ref_rot.data_ptr(),
                                           ref_abs.data_ptr(), wl.data_ptr(), wr.data_ptr(),
                                           *(bufs[k].data_ptr() if k in subset else None for k in ALL), N, 0, stream)
            assert rc == 0, subset
            for k in ALL:
                if k in subset:
                    assert same_bits(bufs[k], want[k]), (subset, k)
                else:
                    assert bool((bufs[k] == fill).all()), (subset, k)
    # and through ops: what is asked for, nothing else, the same bits; no world -> bones alone
    got = ops.smpl_to_carla(body, skel_type, want=('bones',))
    assert set(got) == {'bones'} and same_bits(got['bones'], want['bones'])


def test_rows_are_k30s_on_k35s_rotations():
    N = 129
    want = baseline(N)
    _, skel_type, wl, wr = (t.to(dev()) for t in problem(N))
    ref_loc, _ = ref.get_relative_tensors(dev())
    bones, root = ops.carla_pose_export(ref_loc[skel_type.long()], want['relative_pose_rot'].to(dev()), wl, wr)
    assert same_bits(bones, want['bones']) and same_bits(root, want['root'])


# ------------------------------------------------------------------------------------------------------------------- NaN
@pytest.mark.parametrize('orig', [0, 6, 9, 16])          # Pelvis, Spine2 (through the spare lane), Spine3, L_Shoulder
def test_one_nan_joint_gives_the_pattern_of_the_definition(orig):
    body, skel_type, _, _ = problem(3)
    body = body.clone()
    body[1, orig * 3:orig * 3 + 3] = float('nan')
    got = ops.smpl_to_carla(body.to(dev()), skel_type.to(dev()))
    host = retarget.convert_smpl_to_carla(body, skel_type)
    masks = expected_nan(bones_of_original_joint(orig))
    clean = baseline(3)
    for k in POSE_KEYS:
        nan = torch.isnan(got[k].cpu())
        assert torch.equal(nan, torch.isnan(host[k])) and torch.equal(nan[1], masks[k]) and not bool(nan[[0, 2]].any()), k
        assert same_bits(got[k][[0, 2]], clean[k][[0, 2]]), k
        assert torch.equal(got[k][1].cpu()[~masks[k]], clean[k][1][~masks[k]]), k


def test_a_whole_nan_frame_leaves_its_neighbours_bits():
    N = 3
    body, skel_type, wl, wr = problem(N)
    body = body.clone()
    body[1] = float('nan')
    got = ops.smpl_to_carla(body.to(dev()), skel_type.to(dev()), wl.to(dev()), wr.to(dev()), want=ALL)
    clean = baseline(N)
    host = retarget.convert_smpl_to_carla(body, skel_type)
    for k in ALL:
        assert same_bits(got[k][[0, 2]], clean[k][[0, 2]]), k
    for k in POSE_KEYS:
        assert torch.equal(torch.isnan(got[k].cpu()), torch.isnan(host[k])), k
    assert same_bits(got['root'], clean['root'])                                  # the world is not the body's business
    assert bool(torch.isnan(got['bones'][1, 1:, 3:]).any()) and same_bits(got['bones'][1, :, :3], clean['bones'][1, :, :3])


# -------------------------------------------------------------------------------------------------------------- dispatch
def test_dispatch_views_joint_layout_and_the_framework_switch(monkeypatch):
    N = 40
    want = baseline(N)
    body, skel_type, _, _ = (t.to(dev()) for t in problem(N))
    as_joints = ops.smpl_to_carla(body.reshape(N, 22, 3), skel_type)
    wide = torch.zeros(N, 80, device=dev())
    wide[:, 7:73] = body
    view = wide[:, 7:73]
    assert not view.is_contiguous()
    from_view = ops.smpl_to_carla(view, skel_type)
    for k in POSE_KEYS:
        assert same_bits(as_joints[k], want[k]) and same_bits(from_view[k], want[k]), k
    t64 = retarget.convert_smpl_to_carla(problem(N)[0].double(), problem(N)[1])
    _, e_ref = truth()
    with monkeypatch.context() as m:
        m.setenv('P2C_SMPL_FRAMEWORK', '1')
        fw = ops.smpl_to_carla(body, skel_type)
    for k in POSE_KEYS:
        assert fw[k].is_cuda and fw[k].dtype == torch.float32
        err = float((fw[k].double().cpu() - t64[k]).abs().max())
        print(f'{k}: tensor definition on the device {err:.3e} from fp64 (allowed {4 * e_ref[k]:.3e})')
        assert np.isfinite(err) and err <= 4 * e_ref[k], k
    d64 = ops.smpl_to_carla(body.double(), skel_type)
    assert d64['absolute_pose_loc'].dtype == torch.float64 and float((d64['absolute_pose_loc'].cpu() - t64['absolute_pose_loc']).abs().max()) <= 1e-12


def test_abi_refusals_come_before_any_launch_and_n_zero_launches_nothing():
    body, skel_type, wl, wr = (t.to(dev()) for t in problem(3))
    ref_loc, ref_rot = ref.get_relative_tensors(dev())
    _, ref_abs = ref.get_absolute_tensors(dev())
    out = torch.zeros(3, 26, 3, 3, device=dev())
    root = torch.zeros(3, 6, device=dev())
    fwd = _lib.lib().p2c_smpl_to_carla_fwd
    p = lambda t: t.data_ptr()                                                  # noqa: E731
    tables = (p(ref_loc), p(ref_rot), p(ref_abs))
    assert fwd(p(body), p(skel_type), 1, *tables, None, None, p(out), None, None, None, None, -1, 0, None) == -2
    assert fwd(p(body), p(skel_type), 0, *tables, None, None, p(out), None, None, None, None, 3, 0, None) == -2
    assert fwd(p(body), p(skel_type), 1, *tables, None, None, p(out), None, None, None, None, 3, -1, None) == -2
    assert fwd(None, p(skel_type), 1, *tables, None, None, p(out), None, None, None, None, 3, 0, None) == -1
    assert fwd(p(body), p(skel_type), 1, *tables, None, None, None, None, None, None, None, 3, 0, None) == -1
    assert fwd(p(body), p(skel_type), 1, *tables, p(wl), None, p(out), None, None, None, p(root), 3, 0, None) == -1
    assert fwd(p(body), p(skel_type), 1, *tables, None, None, p(out), None, None, None, p(root), 3, 0, None) == -1
    assert fwd(p(body), p(skel_type), 1, *tables, p(wl), p(wr), p(out), None, None, None, p(root), 0, 0, None) == 0
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and float(root.abs().sum()) == 0.0
    empty = ops.smpl_to_carla(body[:0], skel_type[:0])
    assert empty['relative_pose_rot'].shape == (0, 26, 3, 3) and empty['relative_pose_rot'].is_cuda


# ---------------------------------------------------------------------------------------------------------- data wrapper
def test_smpl_carla_targets_over_a_device_batch():
    from pedestrians_video_2_carla_amd.data.smpl.targets import SmplCarlaTargets
    B, T = 4, 5
    body, _, _, _ = problem(B * T)
    body = body.reshape(B, T, 66).clone()
    body[2] = float('nan')                                                      # a clip of another source
    skel_type = torch.tensor([1, 0, 3, 2], dtype=torch.int32)
    batch = (torch.zeros(B, T, 26, 2, device=dev()), {'amass_body_pose': body.to(dev())}, {'skel_type': skel_type.to(dev())})
    other = (batch[0], {'projection_2d': batch[0]}, {})
    first, second = list(SmplCarlaTargets([batch, other]))
    assert second is other
    direct = ops.smpl_to_carla(body.to(dev()), skel_type.to(dev()))
    host = retarget.convert_smpl_to_carla(body, skel_type)
    for k in POSE_KEYS:
        t = first[1]['carla_' + k]
        assert t.is_cuda and t.shape == (B, T) + TAIL[k] and same_bits(t, direct[k]), k
        assert torch.equal(torch.isnan(t.cpu()), torch.isnan(host[k])) and bool(torch.isnan(t[2, :, 1:]).any()), k
        assert not bool(torch.isnan(t[[0, 1, 3]]).any()), k
