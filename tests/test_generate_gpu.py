"""GPU: K38 (csrc/p2c_generate.hip, ``ops.generate_carla_batch``) against the definition of its draws (data/carla/generator.py, to
the bit), against K11 on its own projection (the tail, to the bit), against the fp64 oracle of the projection layer (the
geometry), against the composed arm (``P2C_GENERATE_FRAMEWORK=1``) and against itself (chunks, output subsets, grids, mappings).

The geometry bound is the pose head's (tests/test_pose_head_gpu.py ``close``, restated here): max|a - b| <= max(1e-4 max|b|, 2 x
the error of the same oracle run in fp32). Shapes: B in {1, 3, 9, 17} (an odd clip in a wavefront, a workgroup's last partial
row), T in {1, 2, 17}, and B = 17 on one workgroup (the grid-stride regime)."""
import functools
import itertools
import math

import pytest
import torch

from oracle import pose_head as O
from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.data.carla import generator

pytestmark = pytest.mark.gpu

RTOL = 1e-4
SEED, J = 38, 26
SHAPES = [(B, T, 0) for B in (1, 3, 9, 17) for T in (1, 2, 17)] + [(17, 17, 1)]          # (B, T, max_blocks)
DEEP = [(B, 17, 0) for B in (1, 3, 9, 17)] + [(17, 17, 1)]
WORLDS = {'off': {}, 'on': dict(max_world_rot_change_in_deg=15.0, max_initial_world_rot_change_in_deg=180.0)}
GEOMETRY = ('pose_changes', 'relative_pose_rot', 'absolute_pose_loc', 'absolute_pose_rot', 'world_rot', 'projection_2d',
            'projection_2d_transformed')
EYE = torch.eye(3)


def dev():
    return torch.device('cuda:0')


def close(a, b, what, rtol=RTOL, fp32_ref=None):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    bound = rtol * scale + 1e-30
    if fp32_ref is not None:
        bound = max(bound, 2.0 * (fp32_ref.detach().double().cpu() - b).abs().max().item())
    print(f'{what}: max err {err:.3e}, scale {scale:.3e}, bound {bound:.3e}')
    assert math.isfinite(err) and err <= bound, f'{what}: max err {err:.3e} vs scale {scale:.3e} (bound {bound:.3e})'
    return err


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


def generate(B, T, max_blocks=0, **kw):
    kw.setdefault('max_change_in_deg', 15.0)
    out = ops.generate_carla_batch(B, T, seed=SEED, device=dev(), max_blocks=max_blocks, **kw)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def definition(B, T, world='off', noise='zero', first_clip=0, stream=0, k=3):
    return generator.draws(SEED, stream, first_clip, B, T, random_changes_each_frame=k, max_change_in_deg=15.0, noise=noise,
                           noise_param=3.0, **WORLDS[world])


@functools.lru_cache(maxsize=None)
def oracle(B, T, world, transform):
    """The fp64 oracle of the projection layer and the same oracle in fp32, on the definition's fp32 angles and yaws."""
    d = definition(B, T, world)
    out = []
    for dtype in (torch.float64, torch.float32):
        changes = O.euler_angles_to_matrix_xyz(d['angles'].to(dtype))
        drot = None
        if world == 'on':
            yaw = torch.zeros(B, T, 3, dtype=dtype)
            yaw[..., 2] = d['world_yaw'].to(dtype)
            drot = O.euler_angles_to_matrix_xyz(yaw)
        o = O.pose_head(changes, 'pose_changes', d['skel_type'], drot=drot, transform=transform)
        o = {k: v for k, v in o.items() if k in GEOMETRY and v is not None}
        for k in ('projection_2d', 'projection_2d_transformed'):
            if k in o:
                o[k] = o[k][..., :2]
        out.append(o)
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------- 1. draws
@pytest.mark.parametrize('B,T,max_blocks', SHAPES)
def test_draws_are_the_definitions(B, T, max_blocks):
    p = 0.3
    for world, k in (('off', 3), ('on', 1)):
        d = definition(B, T, world, 'uniform', k=k)
        got = generate(B, T, max_blocks, random_changes_each_frame=k, noise='uniform', noise_param=3.0, miss_prob=p, **WORLDS[world])
        assert torch.equal(got['skel_type'].cpu(), d['skel_type']) and got['skel_type'].dtype == torch.int32
        changes = got['pose_changes'].cpu()
        assert torch.equal(changes[~d['picked']], EYE.expand_as(changes[~d['picked']]))          # exactly the identity
        moved = d['picked'] & (d['angles'] != 0).any(-1)
        assert int(moved.sum()) == B * T * k and bool((changes[moved] != EYE).flatten(1).any(1).all())
        # the Euler matrices of the definition's angles: an entry is at most three products and a sum (four roundings of values
        # below 1, 2^-24 each) of sines and cosines that are each within 2 ulp (2^-23): 4 + 3 * 2 = 10 units of 2^-24, 16 allowed
        want = O.euler_angles_to_matrix_xyz(d['angles'].double())
        assert float((changes.double() - want).abs().max()) <= 16 * 2.0 ** -24
        # deformation: exactly (0, 0) where the draw says missing, exactly projection + noise elsewhere
        missing = d['miss_u'] < p
        deformed, projection = got['projection_2d_deformed'].cpu(), got['projection_2d'].cpu()
        assert bool((deformed[missing] == 0).all())
        assert same_bits(deformed[~missing], (projection + d['noise'])[~missing])
        # the world: yaw only, exactly the identity without the parameters
        changes_w = got['world_rot_changes'].cpu()
        if world == 'off':
            assert torch.equal(changes_w, EYE.expand_as(changes_w)) and torch.equal(got['world_rot'].cpu(), changes_w)
        else:
            assert bool((changes_w[..., 2, 2] == 1).all()) and bool((changes_w[..., 2, :2] == 0).all())
            # (fp32 sine, cosine and arctangent of angles up to pi, where an ulp is 2.4e-7: 16 ulp)
            assert float((torch.atan2(changes_w[..., 1, 0], changes_w[..., 0, 0]) - d['world_yaw']).abs().max()) <= 4e-6
        assert bool((got['world_loc'] == 0).all()) and bool((got['world_loc_changes'] == 0).all())


@pytest.mark.parametrize('k', [0, 26])
def test_none_and_all_joints(k):
    got = generate(3, 2, random_changes_each_frame=k)
    changes = got['pose_changes'].cpu()
    if k == 0:
        assert torch.equal(changes, EYE.expand_as(changes))
        _, rel = O.relative_tensors(torch.float32)
        assert torch.equal(got['relative_pose_rot'].cpu(), rel[got['skel_type'].cpu().long()][:, None].expand(3, 2, J, 3, 3))
    else:
        d = definition(3, 2, k=26)
        assert bool(d['picked'].all()) and bool((changes != EYE).flatten(3).any(3).all())


# -------------------------------------------------------------------------------------------------------- 2. tail, to the bit
TAILS = [(None, 'zero'), (0.0, 'zero'), (0.3, 'zero'), (1.0, 'zero'), (tuple(j / 25 for j in range(J)), 'zero'), (None, 'uniform'),
         (0.3, 'uniform')]


@pytest.mark.parametrize('transform', ['none', 'hips_neck', 'bbox', 'hips_neck_bbox'])
@pytest.mark.parametrize('miss,noise', TAILS)
def test_tail_equals_k11_on_k38s_own_projection(transform, miss, noise):
    for B, T, max_blocks in SHAPES:
        d = definition(B, T, 'on', noise)
        got = generate(B, T, max_blocks, transform=transform, miss_prob=miss, noise=noise, noise_param=3.0, **WORLDS['on'])
        probs = ops.generate_miss_prob(miss)
        frames, targets = ops.collate(got['projection_2d'], noise=d['noise'].to(dev()) if d['noise'] is not None else None,
                                      miss_u=d['miss_u'].to(dev()) if probs is not None else None, miss_prob=probs,
                                      transform=transform)
        torch.cuda.synchronize()
        assert torch.equal(got['frames'], frames), (B, T)
        assert torch.equal(targets['projection_2d'], got['projection_2d'])
        if 'projection_2d_deformed' in targets:
            assert torch.equal(got['projection_2d_deformed'], targets['projection_2d_deformed']), (B, T)
        else:
            assert torch.equal(got['projection_2d_deformed'], got['projection_2d'])
        if transform == 'none':
            assert not any(k in got for k in ('projection_2d_transformed', 'projection_2d_shift', 'projection_2d_scale'))
            with pytest.raises(RuntimeError):
                generate(B, T, transform='none', want=('projection_2d_shift',))
        else:
            for k in ('projection_2d_transformed', 'projection_2d_shift', 'projection_2d_scale'):
                assert torch.equal(got[k], targets[k]), (k, B, T)
        if miss == 1.0:
            assert bool((got['frames'] == 0).all())


# ------------------------------------------------------------------------------------------------------ 3. geometry, against fp64
@pytest.mark.parametrize('world', ['off', 'on'])
@pytest.mark.parametrize('B,T,max_blocks', DEEP)
def test_geometry_against_the_fp64_oracle(B, T, max_blocks, world):
    for transform in ('hips_neck_bbox', 'bbox', 'hips_neck', 'none'):
        o64, o32 = oracle(B, T, world, transform)
        got = generate(B, T, max_blocks, transform=transform, **WORLDS[world])
        for k in GEOMETRY:
            if k == 'projection_2d_transformed' and transform == 'none':
                continue
            close(got[k], o64[k], f'{k} B={B} world={world} {transform}', fp32_ref=o32[k])
        # no deformation: the model input is the transformed projection itself
        assert torch.equal(got['frames'], got['projection_2d_transformed' if transform != 'none' else 'projection_2d'])
        rel_loc, _ = O.relative_tensors(torch.float32)
        assert torch.equal(got['relative_pose_loc'].cpu(), rel_loc[got['skel_type'].cpu().long()][:, None].expand(B, T, J, 3))


# -------------------------------------------------------------------------------------------------------------- 4. composed arm
@pytest.mark.parametrize('world', ['off', 'on'])
@pytest.mark.parametrize('B,T,max_blocks', SHAPES)
def test_composed_arm_agrees(monkeypatch, B, T, max_blocks, world):
    """Every output of ``P2C_GENERATE_FRAMEWORK=1`` within the geometry rule of K38's; what the draws alone determine (item 1),
    exactly, on both arms."""
    p = 0.3
    kw = dict(transform='hips_neck_bbox', **WORLDS[world])
    k38 = generate(B, T, max_blocks, **kw)
    deformed38 = generate(B, T, max_blocks, noise='uniform', noise_param=3.0, miss_prob=p, **kw)
    monkeypatch.setenv('P2C_GENERATE_FRAMEWORK', '1')
    composed = generate(B, T, **kw)
    deformed = generate(B, T, noise='uniform', noise_param=3.0, miss_prob=p, **kw)
    monkeypatch.delenv('P2C_GENERATE_FRAMEWORK')
    assert tuple(composed) == tuple(k38) == ops.GENERATE_OUTPUTS
    o64, o32 = oracle(B, T, world, 'hips_neck_bbox')
    fp32_error = {k: (o32[k].double() - o64[k]).abs().max().item() for k in GEOMETRY}
    fp32_error.update(frames=fp32_error['projection_2d_transformed'], projection_2d_deformed=fp32_error['projection_2d'])
    for k in ops.GENERATE_OUTPUTS:
        a, b = composed[k].double().cpu(), k38[k].double().cpu()
        err, bound = (a - b).abs().max().item(), max(RTOL * b.abs().max().item(), 2.0 * fp32_error.get(k, 0.0))
        print(f'composed vs K38, B={B} T={T} world {world}: {k}: max difference {err:.3e} (bound {bound:.3e})')
        assert a.shape == b.shape and composed[k].dtype == k38[k].dtype and math.isfinite(err) and err <= bound, (k, err, bound)
    d = definition(B, T, world, 'uniform')
    missing = d['miss_u'] < p
    moved = d['picked'] & (d['angles'] != 0).any(-1)
    for arm, out in (('composed', deformed), ('k38', deformed38)):
        assert torch.equal(out['skel_type'].cpu(), d['skel_type']), arm
        changes = out['pose_changes'].cpu()
        assert torch.equal(changes[~d['picked']], EYE.expand_as(changes[~d['picked']])), arm
        assert int(moved.sum()) == B * T * 3 and bool((changes[moved] != EYE).flatten(1).any(1).all()), arm
        own_deformed, own_projection = out['projection_2d_deformed'].cpu(), out['projection_2d'].cpu()
        assert bool((own_deformed[missing] == 0).all()), arm
        assert same_bits(own_deformed[~missing], (own_projection + d['noise'])[~missing]), arm
    a, b = deformed['projection_2d_deformed'].double().cpu(), deformed38['projection_2d_deformed'].double().cpu()
    assert (a - b).abs().max().item() <= max(RTOL * b.abs().max().item(), 2.0 * fp32_error['projection_2d'])


# ------------------------------------------------------------------------------------------------------ 5. invariances, to the bit
FULL = dict(transform='hips_neck_bbox', noise='uniform', noise_param=3.0, miss_prob=0.3, **WORLDS['on'])


def assert_same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert same_bits(a[k], b[k]), (what, k)


@pytest.mark.parametrize('first', [0, (1 << 40) + 5])
def test_chunks_and_far_clips(first):
    T = 5
    whole = generate(12, T, first_clip=first, **FULL)
    head, tail = generate(5, T, first_clip=first, **FULL), generate(7, T, first_clip=first + 5, **FULL)
    assert_same(whole, {k: torch.cat((head[k], tail[k])) for k in whole}, first)
    d = definition(12, T, 'on', 'uniform', first_clip=first)
    assert torch.equal(whole['skel_type'].cpu(), d['skel_type'])
    changes = whole['pose_changes'].cpu()
    assert torch.equal((changes != EYE).flatten(3).any(3), d['picked'] & (d['angles'] != 0).any(-1))
    if first:
        near = generate(12, T, first_clip=5, **FULL)
        assert not torch.equal(near['pose_changes'], whole['pose_changes'])
    other = generate(12, T, first_clip=first, stream=1, **FULL)
    assert not torch.equal(other['pose_changes'], whole['pose_changes'])


@pytest.mark.parametrize('B,T,max_blocks', SHAPES)
def test_every_output_alone_is_itself_in_the_full_call(B, T, max_blocks):
    full = generate(B, T, **FULL)
    assert tuple(full) == ops.GENERATE_OUTPUTS
    for k in ops.GENERATE_OUTPUTS:
        for mapping in ('sequential', 'frame_parallel'):
            alone = generate(B, T, max_blocks, want=(k,), mapping=mapping, **FULL)
            assert tuple(alone) == (k,) and same_bits(alone[k], full[k]), (k, mapping)


@pytest.mark.parametrize('B,T', [(17, 17), (3, 2), (1, 1), (512, 16), (513, 16)])
def test_grids_and_mappings_give_the_same_bits(B, T):
    """One workgroup striding over everything, the default grid, a group per clip and a group per frame; B T = 8 192 frames is the
    last size at which 'auto' takes the frame-parallel mapping (P2C_GENERATE_FRAME_PARALLEL_MAX_FRAMES), 8 208 the first sequential."""
    assert (B * T > _lib.P2C_GENERATE_FRAME_PARALLEL_MAX_FRAMES) == (B == 513)
    want = generate(B, T, mapping='sequential', **FULL)
    for mapping, max_blocks in itertools.product(('auto', 'sequential', 'frame_parallel'), (0, 1, 3)):
        assert_same(generate(B, T, max_blocks, mapping=mapping, **FULL), want, (mapping, max_blocks))
    assert_same(generate(B, T, **FULL), want, 'twice')


# ------------------------------------------------------------------------------------------------------ 6. audits and the trainer
@pytest.mark.parametrize('B,T,max_blocks', SHAPES)
def test_under_the_two_audit_modes_the_bits_stay(monkeypatch, B, T, max_blocks):
    """NaN-filled ``torch.empty`` (``P2C_POISON_EMPTY=1``) and poisoned LDS (the kernel allocates none): an output element that was
    not written would show as NaN."""
    want = {m: generate(B, T, max_blocks, mapping=m, **FULL) for m in ('sequential', 'frame_parallel')}
    monkeypatch.setenv('P2C_POISON_LDS', '1')
    monkeypatch.setenv('P2C_POISON_EMPTY', '1')
    monkeypatch.setattr(_lib, '_lib', None)
    deterministic, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    monkeypatch.setattr(torch.utils.deterministic, 'fill_uninitialized_memory', True)
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        assert isinstance(_lib.lib(), _lib._PoisonedLib) and bool(torch.isnan(torch.empty(8, device=dev())).all())
        got = {m: generate(B, T, max_blocks, mapping=m, **FULL) for m in want}
    finally:
        torch.use_deterministic_algorithms(deterministic, warn_only=warn_only)
    for m in want:
        for k in ops.GENERATE_OUTPUTS:
            assert same_bits(got[m][k], want[m][k]), (m, k)
            assert k == 'skel_type' or bool(torch.isfinite(got[m][k]).all()), (m, k)


def test_a_train_step_on_a_generated_batch(monkeypatch):
    """LitPoseLiftingFlow + LinearAE, B = 8, T = 16: the step on a ``Carla2D3DDataModule`` batch gives a finite loss, the loss of the
    same step (same initial weights) on the composed arm's batch within 1e-4 relative."""
    from pedestrians_video_2_carla_amd.data.carla.carla_2d3d import Carla2D3DDataModule
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything
    losses = {}
    for arm in ('0', '1'):
        monkeypatch.setenv('P2C_GENERATE_FRAMEWORK', arm)
        seed_everything(38)
        dm = Carla2D3DDataModule(clip_length=16, batch_size=8, missing_joint_probabilities=0.1, seed=SEED)
        flow = LitPoseLiftingFlow(movements_model=LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON),
                                  loss_modes=['loc_2d_3d'], transform='hips_neck_bbox')
        trainer = Trainer(max_steps=1, device=dev()).setup(flow, dm)
        batch = next(iter(dm.train_batches(dev(), 1)))
        frames, targets, meta = batch
        assert frames.shape == (8, 16, J, 2) and frames.is_cuda and meta['skel_type'].dtype == torch.int32
        assert {'pose_changes', 'world_loc_changes', 'world_rot_changes', 'projection_2d_deformed'} <= set(targets)
        assert len(meta['age']) == 8 and (meta['age'], meta['gender']) == generator.age_gender(meta['skel_type'].cpu())
        loss = trainer.train_step(flow, batch, 0)
        torch.cuda.synchronize()
        losses[arm] = float(loss)
        assert math.isfinite(losses[arm])
    print(f"train step loss on a K38 batch {losses['0']:.8f}, on the composed arm's {losses['1']:.8f}")
    close(torch.tensor(losses['0']), torch.tensor(losses['1']), 'loss of the step')


def test_outside_the_fused_tail_the_kernel_makes_the_raw_part_and_k11_the_tail():
    """Gaussian noise and an OpenPose input skeleton: K38 with ``transform='none'`` for the raw part, ``DeviceProjection2DPipeline``
    for the tail. The raw targets are the fused call's, to the bit; the frames are the pipeline's, on the input skeleton."""
    from pedestrians_video_2_carla_amd.data.carla.carla_2d3d import Carla2D3DDataModule
    from pedestrians_video_2_carla_amd.data.openpose.skeleton import BODY_25_SKELETON
    B, T = 9, 5
    common = dict(clip_length=T, batch_size=B, seed=SEED, max_world_rot_change_in_deg=15, max_initial_world_rot_change_in_deg=180)
    fused_dm = Carla2D3DDataModule(**common)
    raw = ('projection_2d', 'pose_changes', 'relative_pose_loc', 'relative_pose_rot', 'absolute_pose_loc', 'absolute_pose_rot',
           'world_loc', 'world_rot', 'world_loc_changes', 'world_rot_changes')
    _, fused_targets, fused_meta = fused_dm.generate_batch(dev(), seed_offset=2)
    for kwargs, joints in ((dict(noise='gaussian', noise_param=2.0), J), (dict(input_nodes=BODY_25_SKELETON), len(BODY_25_SKELETON)),
                           (dict(noise='gaussian', input_nodes=BODY_25_SKELETON, missing_joint_probabilities=[0.2],
                                 augment_rotate=True), len(BODY_25_SKELETON))):
        dm = Carla2D3DDataModule(**common, **kwargs)
        assert not dm.fused(True)
        frames, targets, meta = dm.generate_batch(dev(), seed_offset=2)
        torch.cuda.synchronize()
        assert frames.shape == (B, T, joints, 2) and bool(torch.isfinite(frames).all())
        assert torch.equal(meta['skel_type'], fused_meta['skel_type']) and meta['age'] == fused_meta['age']
        assert set(raw) | {'projection_2d_transformed', 'projection_2d_shift', 'projection_2d_scale'} <= set(targets)
        for k in raw[1:]:
            assert same_bits(targets[k], fused_targets[k]), k
        if joints == J and 'augment_rotate' not in kwargs:
            assert same_bits(targets['projection_2d'], fused_targets['projection_2d'])
            assert same_bits(targets['projection_2d_transformed'], fused_targets['projection_2d_transformed'])
            assert 'projection_2d_deformed' in targets and not torch.equal(targets['projection_2d_deformed'], targets['projection_2d'])
        assert targets['projection_2d'].shape == (B, T, joints, 2) and targets['projection_2d_scale'].shape == (B, T)
