"""GPU: K36 (csrc/p2c_ik.hip, ``ops.locations_to_carla``) against the fp64 tensor definition
(walker_control/inverse_kinematics.py) on the same fp32 inputs, and against itself.

Bound: |kernel - fp64 definition| <= 4 * e_ref per pose output, e_ref measured on the host from the round-trip inputs alone (the
fp32 definition against the fp64 one, test_ik.py), never from the kernel. The margin is 4x because operation order and
multiply-add contraction differ (K35's rule); K36 runs its fit in fp64, so what it is charged with is the rounding of the fp32
reference tables and of its outputs. Everything else here is bit for bit: grid regimes, runs, output subsets, per-clip calls and
the rows, which must be K30's on K36's own rotations. A wavefront takes chunks of F = 2 p frames and a workgroup of G = 8 p, with
p = min(10, ceil(N / 2048)) pairs chosen from N (``frames_per_wavefront``): up to 2 048 frames F = 2 and G = 8. Measured
ratios: DESIGN section 4, K36."""
import functools
import itertools

import numpy as np
import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.data.carla import reference as ref
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
from pedestrians_video_2_carla_amd.walker_control import inverse_kinematics as ik
from test_ik import POSE_KEYS, fixture, nan_joint_cases, round_trip, truth
from test_smpl_retarget_gpu import TAIL, dev, same_bits      # the two converters have the same outputs

pytestmark = pytest.mark.gpu

ALL = ops.IK_CARLA_OUTPUTS


def frames_per_wavefront(N):
    """The chunk of the kernel's host side: 2 * min(10, ceil(N / 2048)) frames, at least 2."""
    return 2 * min(10, max(1, -(-N // 2048)))


F, G = frames_per_wavefront(1), 4 * frames_per_wavefront(1)
# N at which the kernel takes larger chunks: p = 2 (F = 4, G = 16: 2049 = 512 F + 1, 2051 = 512 F + 3, 2063 / 2064 / 2065 = 129 G - 1,
# 129 G, 129 G + 1) and p = 10 (F = 20, G = 80: 18433 = 921 F + 13 = 230 G + 33, 18480 = 231 G)
CHUNKED = [2049, 2051, 2063, 2064, 2065, 18433, 18480]


@functools.lru_cache(maxsize=None)
def problem(N):
    """N frames on the host: round-trip poses at angle scale 0.6, moved and scaled per frame (the fit must not care), types
    cycling, a world per frame."""
    from pedestrians_video_2_carla_amd.transforms.rotation_conversions import euler_angles_to_matrix
    g = torch.Generator().manual_seed(1000 + N)
    skel_type, _, loc, _ = round_trip(0.6, N, 1000 + N)
    loc = loc * (0.5 + torch.rand(N, 1, 1, generator=g, dtype=torch.float64)) + torch.randn(N, 1, 3, generator=g, dtype=torch.float64)
    world_loc = torch.randn(N, 3, generator=g)
    world_rot = euler_angles_to_matrix((torch.rand(N, 3, generator=g) * 2 - 1) * 1.2, 'XYZ')
    return loc.float().contiguous(), skel_type, world_loc, world_rot


def run_all(N, max_blocks=0):
    loc, skel_type, wl, wr = (t.to(dev()) for t in problem(N))
    return ops.locations_to_carla(loc, skel_type, wl, wr, want=ALL, max_blocks=max_blocks)


@functools.lru_cache(maxsize=None)
def baseline(N):
    """The all-outputs call at the kernel's own grid, on the host: what every other regime must reproduce bit for bit."""
    return {k: v.cpu() for k, v in run_all(N).items()}


def within_bound(got, t64, what):
    _, e_ref = truth()
    for k in POSE_KEYS:
        finite = torch.isfinite(t64[k])
        err = float((got[k].double().cpu() - t64[k])[finite].abs().max())
        print(f'{what} {k}: {err:.3e} from fp64, e_ref {e_ref[k]:.3e}, ratio {err / e_ref[k]:.2f} (allowed 4)')
        assert np.isfinite(err) and err <= 4 * e_ref[k], (what, k, err)


# ---------------------------------------------------------------------------------------------------------------- parity
def test_round_trip_inputs_parity_within_four_e_ref():
    loc, skel_type = fixture()
    t64, _ = truth()
    got = ops.locations_to_carla(loc.to(dev()), skel_type.to(dev()))
    assert set(got) == set(POSE_KEYS)
    for k in POSE_KEYS:
        assert got[k].is_cuda and got[k].dtype == torch.float32 and bool(torch.isfinite(got[k]).all())
    within_bound(got, t64, 'K36')


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize('N', sorted({1, F - 1, F, F + 1, G - 1, G, G + 1}) + [41, 1025] + CHUNKED)
def test_every_grid_regime_and_a_second_run_give_the_same_bits(N):
    """One pair per wavefront: N = 1 (= F - 1), F, F + 1, G - 1, G, G + 1; N = 41 at max_blocks = 1 makes every wavefront stride
    at least five times; N = 1025 is 129 workgroups at the kernel's own grid. Larger chunks: ``CHUNKED``; at max_blocks = 1 the
    four wavefronts stride 128 and 230 times. A frame's bits do not depend on the chunk it was in."""
    want = baseline(N)
    loc, skel_type, _, _ = problem(N)
    t64 = ik.fit_carla_rotations(loc.double(), skel_type)
    for k in POSE_KEYS:
        assert want[k].shape == (N,) + TAIL[k]
    within_bound(want, t64, f'N={N}')
    for max_blocks in (0, 1, 2):
        got = run_all(N, max_blocks)
        for k in ALL:
            assert same_bits(got[k], want[k]), (k, max_blocks)
    if frames_per_wavefront(N) > F:
        first = ops.locations_to_carla(*(t[:G + 1].to(dev()) for t in problem(N)), want=ALL)       # the same frames, a pair at a time
        last = ops.locations_to_carla(*(t[-3:].to(dev()) for t in problem(N)), want=ALL)
        for k in ALL:
            assert same_bits(first[k], want[k][:G + 1]) and same_bits(last[k], want[k][-3:]), k


def test_clips_with_one_type_each_equal_per_clip_calls():
    loc, _, wl, wr = (t[:15].to(dev()) for t in problem(41))
    loc, wl, wr = loc.reshape(5, 3, 26, 3), wl.reshape(5, 3, 3), wr.reshape(5, 3, 3, 3)
    skel_type = torch.tensor([0, 1, 2, 3, 1], dtype=torch.int32, device=dev())
    got = ops.locations_to_carla(loc, skel_type, wl, wr, want=ALL)
    for k in ALL:
        assert got[k].shape == (5, 3) + TAIL[k]
    for b in range(5):
        one = ops.locations_to_carla(loc[b], skel_type[b:b + 1].expand(3), wl[b], wr[b], want=ALL)
        for k in ALL:
            assert same_bits(got[k][b], one[k]), (k, b)
    again = ops.locations_to_carla(loc, skel_type.long(), wl, wr, want=ALL)          # int64 types, as a loader's meta may hold them
    assert all(same_bits(again[k], got[k]) for k in ALL)
    moved = ops.locations_to_carla(loc, skel_type.cpu(), wl, wr, want=ALL)           # types still on the host are moved
    assert all(same_bits(moved[k], got[k]) for k in ALL)


# ------------------------------------------------------------------------------------------------------ output selection
def test_every_subset_of_outputs_has_the_bits_of_the_full_call_and_writes_nothing_else():
    """Straight through the C ABI, so that the buffers not asked for exist: they keep their prefill."""
    N = G + 1
    want = baseline(N)
    loc, skel_type, wl, wr = (t.to(dev()) for t in problem(N))
    ref_loc, ref_rot = ref.get_relative_tensors(dev())
    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    fill = -7.25
    for r in range(1, len(ALL) + 1):
        for subset in itertools.combinations(ALL, r):
            bufs = {k: torch.full((N,) + TAIL[k], fill, device=dev()) for k in ALL}
            rc = lib.p2c_loc_to_carla_fwd(loc.data_ptr(), skel_type.data_ptr(), 1, ref_loc.data_ptr(), ref_rot.data_ptr(),
                                          wl.data_ptr(), wr.data_ptr(),
                                          *(bufs[k].data_ptr() if k in subset else None for k in ALL), N, 0, stream)
            assert rc == 0, subset
            for k in ALL:
                if k in subset:
                    assert same_bits(bufs[k], want[k]), (subset, k)
                else:
                    assert bool((bufs[k] == fill).all()), (subset, k)
    got = ops.locations_to_carla(loc, skel_type, want=('bones',))                    # no world -> bones alone
    assert set(got) == {'bones'} and same_bits(got['bones'], want['bones'])


def test_rows_are_k30s_on_k36s_rotations():
    N = 41
    want = baseline(N)
    _, skel_type, wl, wr = (t.to(dev()) for t in problem(N))
    ref_loc, _ = ref.get_relative_tensors(dev())
    bones, root = ops.carla_pose_export(ref_loc[skel_type.long()], want['relative_pose_rot'].to(dev()), wl, wr)
    assert same_bits(bones, want['bones']) and same_bits(root, want['root'])


# ------------------------------------------------------------------------------------------------------- NaN, zero frames
@pytest.mark.parametrize('joint', nan_joint_cases())
def test_one_nan_joint_gives_the_pattern_of_the_definition(joint):
    loc, skel_type, _, _ = problem(3)
    loc = loc.clone()
    loc[1, joint] = float('nan')
    got = ops.locations_to_carla(loc.to(dev()), skel_type.to(dev()))
    host = ik.fit_carla_rotations(loc.double(), skel_type)
    clean = baseline(3)
    for k in POSE_KEYS:
        nan = torch.isnan(got[k].cpu())
        assert torch.equal(nan, torch.isnan(host[k])) and bool(nan[1].any()) and not bool(nan[[0, 2]].any()), k
        assert same_bits(got[k][[0, 2]], clean[k][[0, 2]]), k
    within_bound(got, host, f'NaN at {CARLA_SKELETON(joint).name}')


def test_a_whole_nan_frame_leaves_its_neighbours_bits():
    N = 3
    loc, skel_type, wl, wr = problem(N)
    loc = loc.clone()
    loc[1] = float('nan')
    got = ops.locations_to_carla(loc.to(dev()), skel_type.to(dev()), wl.to(dev()), wr.to(dev()), want=ALL)
    clean = baseline(N)
    host = ik.fit_carla_rotations(loc.double(), skel_type)
    for k in ALL:
        assert same_bits(got[k][[0, 2]], clean[k][[0, 2]]), k
    for k in POSE_KEYS:
        assert torch.equal(torch.isnan(got[k].cpu()), torch.isnan(host[k])), k
    assert same_bits(got['root'], clean['root'])                                  # the world is not the pose's business
    assert bool(torch.isnan(got['bones'][1, 1:, 3:]).any()) and same_bits(got['bones'][1, :, :3], clean['bones'][1, :, :3])


def test_an_all_zero_frame_between_ordinary_ones_is_the_reference_pose():
    N = 5
    loc, skel_type, wl, wr = problem(N)
    loc = loc.clone()
    loc[2] = 0.0
    loc[3] = -1.25                                                                # coincident joints anywhere
    got = ops.locations_to_carla(loc.to(dev()), skel_type.to(dev()), wl.to(dev()), wr.to(dev()), want=ALL)
    clean = baseline(N)
    ref_loc, ref_rot = ref.get_relative_tensors(dev())
    st = skel_type.long().to(dev())
    rows, _ = ops.carla_pose_export(ref_loc[st], ref_rot[st])
    abs_loc, abs_rot = ref.get_absolute_tensors(dtype=torch.float64)
    _, e_ref = truth()
    for n in (2, 3):
        assert same_bits(got['relative_pose_rot'][n], ref_rot[st[n]]) and same_bits(got['bones'][n], rows[n])
        assert float((got['absolute_pose_loc'][n].double().cpu() - abs_loc[skel_type[n]]).abs().max()) <= 4 * e_ref['absolute_pose_loc']
        assert float((got['absolute_pose_rot'][n].double().cpu() - abs_rot[skel_type[n]]).abs().max()) <= 4 * e_ref['absolute_pose_rot']
    for k in ALL:
        assert same_bits(got[k][[0, 1, 4]], clean[k][[0, 1, 4]]), k


# -------------------------------------------------------------------------------------------------------------- dispatch
def test_dispatch_views_and_the_framework_switch(monkeypatch):
    N = 41
    want = baseline(N)
    loc, skel_type, _, _ = (t.to(dev()) for t in problem(N))
    wide = torch.zeros(N, 26, 5, device=dev())
    wide[..., 1:4] = loc
    view = wide[..., 1:4]
    assert not view.is_contiguous()
    from_view = ops.locations_to_carla(view, skel_type)
    strided = ops.locations_to_carla(loc.repeat_interleave(2, 0)[::2], skel_type)
    for k in POSE_KEYS:
        assert same_bits(from_view[k], want[k]) and same_bits(strided[k], want[k]), k
    t64 = ik.fit_carla_rotations(problem(N)[0].double(), problem(N)[1])
    with monkeypatch.context() as m:
        m.setenv('P2C_IK_FRAMEWORK', '1')
        fw = ops.locations_to_carla(loc, skel_type)
    for k in POSE_KEYS:
        assert fw[k].is_cuda and fw[k].dtype == torch.float32
    within_bound(fw, t64, 'tensor definition on the device')
    d64 = ops.locations_to_carla(loc.double(), skel_type)
    for k in POSE_KEYS:
        assert d64[k].is_cuda and d64[k].dtype == torch.float64 and float((d64[k].cpu() - t64[k]).abs().max()) <= 1e-12, k


def test_abi_refusals_come_before_any_launch_and_n_zero_launches_nothing():
    loc, skel_type, wl, wr = (t.to(dev()) for t in problem(3))
    ref_loc, ref_rot = ref.get_relative_tensors(dev())
    out = torch.zeros(3, 26, 3, 3, device=dev())
    root = torch.zeros(3, 6, device=dev())
    fwd = _lib.lib().p2c_loc_to_carla_fwd
    p = lambda t: t.data_ptr()                                                  # noqa: E731
    tables = (p(ref_loc), p(ref_rot))
    assert fwd(p(loc), p(skel_type), 1, *tables, None, None, p(out), None, None, None, None, -1, 0, None) == -2
    assert fwd(p(loc), p(skel_type), 0, *tables, None, None, p(out), None, None, None, None, 3, 0, None) == -2
    assert fwd(p(loc), p(skel_type), 1, *tables, None, None, p(out), None, None, None, None, 3, -1, None) == -2
    assert fwd(None, p(skel_type), 1, *tables, None, None, p(out), None, None, None, None, 3, 0, None) == -1
    assert fwd(p(loc), p(skel_type), 1, *tables, None, None, None, None, None, None, None, 3, 0, None) == -1
    assert fwd(p(loc), p(skel_type), 1, *tables, p(wl), None, p(out), None, None, None, p(root), 3, 0, None) == -1
    assert fwd(p(loc), p(skel_type), 1, *tables, None, None, p(out), None, None, None, p(root), 3, 0, None) == -1
    assert fwd(p(loc), p(skel_type), 1, *tables, p(wl), p(wr), p(out), None, None, None, p(root), 0, 0, None) == 0
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and float(root.abs().sum()) == 0.0
    empty = ops.locations_to_carla(loc[:0], skel_type[:0])
    assert empty['relative_pose_rot'].shape == (0, 26, 3, 3) and empty['relative_pose_rot'].is_cuda


def test_under_the_two_audit_modes_the_bits_stay(monkeypatch):
    """Every LDS byte NaN before the launch (``P2C_POISON_LDS=1``; the kernel allocates none) and NaN-filled ``torch.empty``
    (``P2C_POISON_EMPTY=1``): an output element that was not written would show as NaN."""
    N = G + 1
    want = baseline(N)
    monkeypatch.setenv('P2C_POISON_LDS', '1')
    monkeypatch.setenv('P2C_POISON_EMPTY', '1')
    monkeypatch.setattr(_lib, '_lib', None)                  # the next lib() wraps every launch with the LDS poisoning
    deterministic, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    monkeypatch.setattr(torch.utils.deterministic, 'fill_uninitialized_memory', True)
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        assert isinstance(_lib.lib(), _lib._PoisonedLib) and bool(torch.isnan(torch.empty(8, device=dev())).all())
        got = run_all(N)
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(deterministic, warn_only=warn_only)
    for k in ALL:
        assert same_bits(got[k], want[k]) and bool(torch.isfinite(got[k]).all()), k


# ------------------------------------------------------------------------------------------------------------ end to end
def test_a_location_model_flow_to_carla_rows_end_to_end(tmp_path):
    """LitPoseLiftingFlow(Baseline3DPose) on the device, B = 2, T = 4: ``Trainer.predict_carla(ik=True)`` gives finite rows of
    the right shape, those of ``LocationRetargeter.export`` on the flow's own ``predict_step`` output, where the default
    loop refuses; ``ik_carla_animation`` stores them."""
    from pedestrians_video_2_carla_amd.data.carla.animation import ik_carla_animation, load_carla_animation
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.baseline_3d_pose import Baseline3DPose
    from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything
    from pedestrians_video_2_carla_amd.walker_control.location_retargeter import LocationRetargeter
    seed_everything(36)
    B, T = 2, 4
    dm = SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B)
    model = Baseline3DPose(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, linear_size=64, num_stage=1)
    flow = LitPoseLiftingFlow(movements_model=model, loss_modes=['loc_2d_3d'], transform='hips_neck_bbox')
    trainer = Trainer(max_steps=1, device=dev()).setup(flow, dm)
    batch = dm.generate_batch(dev())
    flow.train()
    with pytest.warns(UserWarning, match='one-launch path'):
        with pytest.raises(KeyError):
            trainer.predict_carla(flow, [batch])
    (bones, root, meta), = trainer.predict_carla(flow, [batch], ik=True)
    assert flow.training and meta is batch[2]
    assert bones.is_cuda and bones.shape == (B, T, 26, 6) and root.shape == (B, T, 6)
    assert bool(torch.isfinite(bones).all()) and bool(torch.isfinite(root).all())
    flow.eval()
    with torch.no_grad():
        sliced, _ = flow.predict_step(batch, 0)
    flow.train()
    assert sliced.get('relative_pose_rot') is None and sliced['absolute_pose_loc'].shape == (B, T, 26, 3)
    want_bones, want_root = LocationRetargeter().export(sliced, meta)
    assert same_bits(bones, want_bones) and same_bits(root, want_root)
    got = load_carla_animation(ik_carla_animation(str(tmp_path / 'ik'), flow, [batch]))
    assert np.array_equal(got['bones'], bones.cpu().numpy()) and np.array_equal(got['root'], root.cpu().numpy())
