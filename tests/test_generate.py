"""No GPU: the counter-based draws of the Carla2D3D generator (data/carla/generator.py -- the definition K38 equals to the bit),
their statistics, the data module's interface on the definition alone, the launcher's flags and the C ABI of K38.

Every statistical bound is five standard deviations of the exact law of the statistic under independent uniform words, written
next to the assertion; none is a tuned number. The seeds are fixed, so a run either passes always or never."""
import argparse
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.data.carla import generator
from pedestrians_video_2_carla_amd.data.carla.carla_2d3d import Carla2D3DDataModule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J = 26
KEYS = ('skel_type', 'picked', 'angles', 'world_yaw', 'miss_u', 'noise')
FULL = dict(max_world_rot_change_in_deg=15, max_initial_world_rot_change_in_deg=180, noise='uniform', noise_param=2.5)


def same(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in KEYS)


def cat(a, b):
    return {k: None if a[k] is None else torch.cat((a[k], b[k])) for k in KEYS}


# -------------------------------------------------------------------------------------------------------- the draw definition
def test_mix32_is_the_lowbias32_finaliser_of_the_kernels():
    source = open(os.path.join(ROOT, 'pedestrians_video_2_carla_amd', 'csrc', 'p2c_rec_dev.h')).read()
    assert '0x7feb352du' in source and '0x846ca68bu' in source
    x = np.array([0, 1, 0xFFFFFFFF, 0x12345678], dtype=np.uint32)
    assert [generator.mix32(int(v)) for v in x] == generator.mix32(x).tolist()
    assert generator.mix32(0) == 0
    assert len(set(generator.mix32(np.arange(1 << 16, dtype=np.uint32)).tolist())) == 1 << 16     # a bijection does not collide


def test_same_arguments_same_tensors_and_shapes():
    a = generator.draws(7, 0, 0, 5, 4, **FULL)
    b = generator.draws(7, 0, 0, 5, 4, **FULL)
    assert same(a, b)
    assert a['skel_type'].shape == (5,) and a['skel_type'].dtype == torch.int32
    assert a['picked'].shape == (5, 4, J) and a['picked'].dtype == torch.bool
    assert a['angles'].shape == (5, 4, J, 3) and a['angles'].dtype == torch.float32
    assert a['world_yaw'].shape == (5, 4) and a['miss_u'].shape == (5, 4, J) and a['noise'].shape == (5, 4, J, 2)
    assert generator.draws(7, 0, 0, 5, 4)['noise'] is None
    assert bool((a['miss_u'] >= 0).all()) and bool((a['miss_u'] < 1).all())
    assert bool((a['noise'] >= -1.25).all()) and bool((a['noise'] <= 1.25).all())


@pytest.mark.parametrize('first', [0, (1 << 40) + 5])
def test_chunk_invariance(first):
    whole = generator.draws(11, 3, first, 12, 3, **FULL)
    parts = cat(generator.draws(11, 3, first, 5, 3, **FULL), generator.draws(11, 3, first + 5, 7, 3, **FULL))
    assert same(whole, parts)


def test_the_upper_half_of_the_clip_index_is_used():
    low, high = generator.draws(11, 3, 5, 7, 3, **FULL), generator.draws(11, 3, (1 << 40) + 5, 7, 3, **FULL)
    assert not torch.equal(low['angles'], high['angles']) and not torch.equal(low['miss_u'], high['miss_u'])
    for b in range(7):
        assert not torch.equal(low['miss_u'][b], high['miss_u'][b]), b


def test_stream_and_seed_give_other_clips():
    base = generator.draws(11, 3, 0, 6, 3, **FULL)
    for other in (generator.draws(11, 4, 0, 6, 3, **FULL), generator.draws(12, 3, 0, 6, 3, **FULL),
                  generator.draws(11 + (1 << 32), 3, 0, 6, 3, **FULL)):      # the seed's upper half counts too
        for k in ('angles', 'miss_u', 'noise', 'world_yaw'):
            assert not torch.equal(base[k], other[k]), k
    assert generator.launch_keys(11, 3) != generator.launch_keys(11, 4) and generator.launch_keys(11, 3) != generator.launch_keys(12, 3)
    # the stream and both seed halves reach BOTH keys
    k = generator.launch_keys(11, 3)
    for other in (generator.launch_keys(11, 4), generator.launch_keys(12, 3), generator.launch_keys(11 + (1 << 32), 3)):
        assert k[0] != other[0] and k[1] != other[1]


@pytest.mark.parametrize('k', [0, 1, 3, 26])
def test_exactly_k_joints_per_frame_and_exact_zeros_elsewhere(k):
    max_deg = 15.0
    d = generator.draws(5, 0, 0, 64, 8, random_changes_each_frame=k, max_change_in_deg=max_deg)
    assert bool((d['picked'].sum(-1) == k).all())
    angles = d['angles']
    assert bool((angles[~d['picked']] == 0).all())
    assert float(angles.abs().max()) <= np.float32(math.radians(max_deg))
    if k:
        assert bool((angles[d['picked']] != 0).any(-1).all())        # a picked joint with three zero angles: 2^-72


def test_world_yaw_follows_the_two_parameters():
    off = generator.draws(5, 0, 0, 16, 6)
    assert bool((off['world_yaw'] == 0).all())
    initial = generator.draws(5, 0, 0, 16, 6, max_initial_world_rot_change_in_deg=180)
    assert bool((initial['world_yaw'][:, 0] != 0).all()) and bool((initial['world_yaw'][:, 1:] == 0).all())
    assert float(initial['world_yaw'].abs().max()) <= np.float32(math.pi)
    later = generator.draws(5, 0, 0, 16, 6, max_world_rot_change_in_deg=15)
    assert bool((later['world_yaw'][:, 0] == 0).all()) and bool((later['world_yaw'][:, 1:] != 0).all())
    assert float(later['world_yaw'].abs().max()) <= np.float32(math.radians(15))


def test_refusals():
    with pytest.raises(ValueError):
        generator.draws(1, 0, 0, 2, 2, random_changes_each_frame=27)
    with pytest.raises(ValueError):
        generator.draws(1, 0, 0, 2, 0)
    with pytest.raises(ValueError):
        generator.draws(1, 0, 0, 2, 2, noise='gaussian')
    with pytest.raises(ValueError):
        generator.draws(1, 0, -1, 2, 2)


# ------------------------------------------------------------------------------------------------- statistics of the definition
B_STAT, T_STAT = 512, 8
N_FRAMES = B_STAT * T_STAT


@pytest.fixture(scope='module')
def stat_draws():
    return {k: generator.draws(2024, 0, 0, B_STAT, T_STAT, random_changes_each_frame=k, max_change_in_deg=5.0) for k in (1, 3, 13)}


@pytest.mark.parametrize('k', [1, 3, 13])
def test_every_joint_is_picked_k_in_26_of_the_time(stat_draws, k):
    """A joint's pick count over n frames is Binomial(n, k / 26): mean n k / 26, sigma sqrt(n (k / 26)(1 - k / 26))."""
    counts = stat_draws[k]['picked'].reshape(-1, J).sum(0).double()
    p = k / J
    bound = 5 * math.sqrt(N_FRAMES * p * (1 - p))
    assert float((counts - N_FRAMES * p).abs().max()) <= bound, (counts, bound)


def test_the_angles_of_picked_joints_are_centred(stat_draws):
    """U(-m, m) has sigma m / sqrt(3): the mean of n of them lies within 5 (m / sqrt(3)) / sqrt(n) of 0; per axis and overall."""
    d = stat_draws[3]
    m = math.radians(5.0)
    picked = d['angles'][d['picked']].double()                     # (n, 3)
    n = picked.shape[0]
    assert n == N_FRAMES * 3
    for axis in range(3):
        assert abs(float(picked[:, axis].mean())) <= 5 * (m / math.sqrt(3)) / math.sqrt(n), axis
    assert abs(float(picked.mean())) <= 5 * (m / math.sqrt(3)) / math.sqrt(3 * n)
    # and they fill the range: the variance of n uniforms has relative sigma sqrt(4 / (5 n)) (kurtosis 9 / 5)
    var = float((picked ** 2).mean())
    assert abs(var / (m * m / 3) - 1) <= 5 * math.sqrt(4 / (5 * 3 * n))


def _lag1(x, dim):
    """The sample correlation of neighbours along ``dim``: for independent values it is N(0, 1 / n) to first order."""
    x = x.double()
    a, b = x.narrow(dim, 0, x.shape[dim] - 1).reshape(-1), x.narrow(dim, 1, x.shape[dim] - 1).reshape(-1)
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt(float((a * a).sum()) * float((b * b).sum()))), a.numel()


@pytest.mark.parametrize('dim,name', [(0, 'clips'), (1, 'frames'), (2, 'joints')])
def test_no_lag_one_correlation_between_neighbours(stat_draws, dim, name):
    u = stat_draws[3]['miss_u']
    r, n = _lag1(u, dim)
    assert abs(r) <= 5 / math.sqrt(n), (name, r, n)


def test_no_correlation_between_the_channels_of_a_joint():
    d = generator.draws(2024, 0, 0, B_STAT, T_STAT, random_changes_each_frame=26, max_change_in_deg=5.0, noise='uniform')
    cols = [d['angles'][..., 0], d['angles'][..., 1], d['angles'][..., 2], d['miss_u'], d['noise'][..., 0], d['noise'][..., 1]]
    n = cols[0].numel()
    for i in range(len(cols)):
        for j in range(i + 1, len(cols)):
            a, b = cols[i].double().reshape(-1), cols[j].double().reshape(-1)
            a, b = a - a.mean(), b - b.mean()
            r = float((a * b).sum() / math.sqrt(float((a * a).sum()) * float((b * b).sum())))
            assert abs(r) <= 5 / math.sqrt(n), (i, j, r)


def test_the_four_skeletons_are_equally_likely_and_age_and_gender_independent():
    """Counts over B clips are Binomial(B, 1 / 4): B / 4 +- 5 sqrt(B 3 / 16); age and gender each Binomial(B, 1 / 2)."""
    B = 4096
    st = generator.skeleton_types(2024, 0, 0, B)
    assert torch.equal(torch.from_numpy(st), generator.draws(2024, 0, 0, B, 1)['skel_type'])
    counts = np.bincount(st, minlength=4)
    assert counts.sum() == B and np.abs(counts - B / 4).max() <= 5 * math.sqrt(B * 3 / 16), counts
    assert abs(int((st >> 1).sum()) - B / 2) <= 5 * math.sqrt(B / 4) and abs(int((st & 1).sum()) - B / 2) <= 5 * math.sqrt(B / 4)
    age, gender = generator.age_gender(st[:8])
    from pedestrians_video_2_carla_amd.data.carla.reference import CARLA_REFERENCE_SKELETON_TYPES
    assert list(zip(age, gender)) == [CARLA_REFERENCE_SKELETON_TYPES[i] for i in st[:8]]
    assert CARLA_REFERENCE_SKELETON_TYPES[2] == ('child', 'female') and CARLA_REFERENCE_SKELETON_TYPES[1] == ('adult', 'male')


def test_miss_frequency_at_one_in_ten(stat_draws):
    """u < p happens Binomial(n, p) times."""
    u = stat_draws[3]['miss_u']
    n, p = u.numel(), 0.1
    assert abs(int((u < p).sum()) - n * p) <= 5 * math.sqrt(n * p * (1 - p))
    assert abs(float(u.double().mean()) - 0.5) <= 5 * math.sqrt(1 / 12 / n)


# ---------------------------------------------------------------------------------------------------- data module and launcher
class FakeGenerate:
    """Stands in for ``ops.generate_carla_batch``: the definition's skeleton types and zeros of the right shapes, on the host; records
    which clips were asked for."""

    def __init__(self):
        self.calls = []

    def __call__(self, B, T, *, seed, stream=0, first_clip=0, want=None, device=None, transform='hips_neck_bbox', **kwargs):
        self.calls.append(dict(B=B, T=T, seed=seed, stream=stream, first_clip=first_clip, want=tuple(want), transform=transform,
                               **kwargs))
        out = {o: torch.zeros((B, T) + ops._GENERATE_TAIL[o]) for o in want if o != 'skel_type'}
        out['skel_type'] = torch.from_numpy(generator.skeleton_types(seed, stream, first_clip, B))
        return out


@pytest.fixture
def fake(monkeypatch):
    f = FakeGenerate()
    monkeypatch.setattr(ops, 'generate_carla_batch', f)
    return f


SYNTHETIC_KEYS = {'projection_2d', 'absolute_pose_loc', 'absolute_pose_rot', 'relative_pose_loc', 'relative_pose_rot', 'world_loc',
                  'world_rot', 'projection_2d_transformed', 'projection_2d_shift', 'projection_2d_scale'}


def test_data_module_batches_keys_shapes_and_meta(fake):
    dm = Carla2D3DDataModule(clip_length=6, batch_size=5, val_set_size=12, test_set_size=3, seed=99)
    assert Carla2D3DDataModule.uses_infinite_train_set() is True
    frames, targets, meta = dm.generate_batch('cpu')
    assert frames.shape == (5, 6, J, 2)
    assert set(targets) == SYNTHETIC_KEYS | {'pose_changes', 'world_loc_changes', 'world_rot_changes'}
    assert targets['pose_changes'].shape == (5, 6, J, 3, 3) and targets['world_rot_changes'].shape == (5, 6, 3, 3)
    assert targets['world_loc_changes'].shape == (5, 6, 3) and targets['projection_2d_scale'].shape == (5, 6)
    st = generator.draws(99, 0, 0, 5, 6)['skel_type']
    assert torch.equal(meta['skel_type'], st) and meta['skel_type'].dtype == torch.int32
    assert (meta['age'], meta['gender']) == generator.age_gender(st)
    assert fake.calls[0]['miss_prob'] is None and fake.calls[0]['noise'] == 'zero'
    # deforming adds the deformed target; transform none drops the three normaliser targets
    dm2 = Carla2D3DDataModule(clip_length=6, batch_size=5, missing_joint_probabilities=[0.2], noise='uniform', transform='none')
    _, targets2, _ = dm2.generate_batch('cpu')
    assert set(targets2) == (SYNTHETIC_KEYS - {'projection_2d_transformed', 'projection_2d_shift', 'projection_2d_scale'}) | {
        'pose_changes', 'world_loc_changes', 'world_rot_changes', 'projection_2d_deformed'}
    assert fake.calls[-1]['miss_prob'] == (0.2,) * J and fake.calls[-1]['noise'] == 'uniform' and fake.calls[-1]['transform'] == 'none'


def test_training_step_i_of_rank_r_is_a_fixed_range_of_clips(fake):
    dm = Carla2D3DDataModule(clip_length=4, batch_size=5, seed=99)
    run = list(dm.train_batches('cpu', 4, rank=2))
    assert [(c['stream'], c['first_clip'], c['B']) for c in fake.calls] == [(2, 0, 5), (2, 5, 5), (2, 10, 5), (2, 15, 5)]
    resumed = list(dm.train_batches('cpu', 2, rank=2, first_step=2))
    assert [(c['stream'], c['first_clip']) for c in fake.calls[4:]] == [(2, 10), (2, 15)]
    for (_, _, m0), (_, _, m1) in zip(run[2:], resumed):
        assert torch.equal(m0['skel_type'], m1['skel_type']) and m0['age'] == m1['age']
    # and on the definition: the draws of step 3 are those of clips 15..19, whatever came before
    assert same(dm.draws('train', 3, rank=2), generator.draws(99, 2, 15, 5, 4))
    assert not torch.equal(dm.draws('train', 3, rank=2)['angles'], dm.draws('train', 3, rank=1)['angles'])


def test_validation_and_test_are_fixed_sets_with_a_short_last_batch(fake):
    dm = Carla2D3DDataModule(clip_length=4, batch_size=5, val_set_size=12, test_set_size=3, seed=99)
    val = dm.val_batches('cpu')
    assert [b[0].shape[0] for b in val] == [5, 5, 2]
    assert [(c['stream'], c['first_clip'], c['B']) for c in fake.calls] == [(generator.VAL_STREAM, 0, 5), (generator.VAL_STREAM, 5, 5),
                                                                            (generator.VAL_STREAM, 10, 2)]
    assert dm.val_batches('cpu') is val and len(fake.calls) == 3            # generated once and kept
    test = dm.test_batches('cpu')
    assert [b[0].shape[0] for b in test] == [3] and fake.calls[-1]['stream'] == generator.TEST_STREAM
    assert generator.VAL_STREAM != generator.TEST_STREAM and min(generator.VAL_STREAM, generator.TEST_STREAM) > 1 << 30
    assert Carla2D3DDataModule(val_set_size=0, batch_size=5).val_batches('cpu') == []


def test_what_is_outside_the_fused_tail_goes_through_the_pipeline(fake):
    from pedestrians_video_2_carla_amd.data.openpose.skeleton import BODY_25_SKELETON
    assert Carla2D3DDataModule().fused(True) and Carla2D3DDataModule(noise='uniform').fused(True)
    assert not Carla2D3DDataModule(noise='gaussian').fused(True)
    assert not Carla2D3DDataModule(augment_rotate=True).fused(True) and Carla2D3DDataModule(augment_rotate=True).fused(False)
    assert not Carla2D3DDataModule(input_nodes=BODY_25_SKELETON).fused(True)
    with pytest.raises(RuntimeError, match='same number of dimensions'):
        Carla2D3DDataModule(needs_confidence=True).generate_batch('cpu')
    with pytest.raises(ValueError):
        Carla2D3DDataModule(missing_joint_probabilities=[0.1, 0.2])
    with pytest.raises(ValueError):
        Carla2D3DDataModule(random_changes_each_frame=27)


def test_launcher_knows_the_module_and_its_flags():
    from pedestrians_video_2_carla_amd import modeling
    assert modeling.data_modules()['Carla2D3D'] is Carla2D3DDataModule
    assert modeling.add_program_args(argparse.ArgumentParser()).parse_args([]).data_module_name == 'SyntheticCarlaRecorded'
    parser, dm_cls, _, _ = modeling.build_parser(['--data_module_name', 'Carla2D3D'])
    assert dm_cls is Carla2D3DDataModule
    args = parser.parse_args(['--data_module_name', 'Carla2D3D'])
    assert (args.random_changes_each_frame, args.max_change_in_deg, args.max_world_rot_change_in_deg,
            args.max_initial_world_rot_change_in_deg, args.val_set_size, args.test_set_size) == (3, 5, 0, 0, 8192, 8192)
    args = parser.parse_args(['--data_module_name', 'Carla2D3D', '--max_change_in_deg', '15', '--max_world_rot_change_in_deg', '15',
                              '--max_initial_world_rot_change_in_deg', '180', '--random_changes_each_frame', '7',
                              '--val_set_size', '64', '--test_set_size', '32'])
    assert (args.random_changes_each_frame, args.max_change_in_deg, args.max_world_rot_change_in_deg,
            args.max_initial_world_rot_change_in_deg, args.val_set_size, args.test_set_size) == (7, 15, 15, 180, 64, 32)
    for bad in (['--max_change_in_deg', '16'], ['--max_change_in_deg', '-1'], ['--max_world_rot_change_in_deg', '16'],
                ['--max_initial_world_rot_change_in_deg', '181']):
        with pytest.raises(SystemExit):
            parser.parse_args(['--data_module_name', 'Carla2D3D'] + bad)
    # the default module has no such flags
    default_parser, _, _, _ = modeling.build_parser([])
    with pytest.raises(SystemExit):
        default_parser.parse_args(['--max_change_in_deg', '5'])
    dm = Carla2D3DDataModule(**vars(args))
    assert Carla2D3DDataModule(seed=0).seed == 0 and Carla2D3DDataModule(seed=None).seed == 22742      # 0 is a seed like any other
    assert dm.max_initial_world_rot_change_in_deg == 180 and dm.val_set_size == 64 and dm.seed == args.seed


# ---------------------------------------------------------------------------------------------------------------------- C ABI
NAME = 'p2c_carla_generate_fwd'


def test_k38_symbol_is_declared_bound_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    header = open(os.path.join(ROOT, 'include', 'p2c.h')).read()
    declared = set(re.findall(r'P2C_API[^;(]*?\b(p2c_\w+)\s*\(', header))
    assert NAME in declared and NAME in _lib.SYMBOLS and getattr(_lib.lib(), NAME) is not None
    res, args = _lib.SYMBOLS[NAME]
    assert res is ctypes.c_int and args[-1] is ctypes.c_void_p and NAME in _lib._PoisonedLib(_lib.lib())._wrap
    decl = re.search(r'P2C_API int ' + NAME + r'\((.*?)\);', header, re.S).group(1)
    params = [' '.join(p.split()) for p in decl.split(',')]
    host_floats = ctypes.POINTER(ctypes.c_float)
    ctype = {'const float *': ctypes.c_void_p, 'float *': ctypes.c_void_p, 'int32_t *': ctypes.c_void_p, 'void *': ctypes.c_void_p,
             'int64_t ': ctypes.c_int64, 'int32_t ': ctypes.c_int32, 'float ': ctypes.c_float}
    names = [re.match(r'(.*?)(\w+)$', p).group(2) for p in params]
    want = [host_floats if n in ('miss_prob', 'camera') else ctype[re.match(r'(.*?)(\w+)$', p).group(1)] for n, p in zip(names, params)]
    assert want == list(args)
    assert names[:5] == ['seed', 'draw_stream', 'first_clip', 'B', 'T'] and names[-3:] == ['mapping', 'max_blocks', 'stream']
    assert names[names.index('frames'):names.index('mapping')] == list(ops.GENERATE_OUTPUTS)
    assert int(re.search(r'#define P2C_GENERATE_MAX_T (\d+)', header).group(1)) == _lib.P2C_GENERATE_MAX_T == generator.MAX_CLIP_LENGTH
    assert int(re.search(r'#define P2C_GENERATE_FRAME_PARALLEL_MAX_FRAMES (\d+)', header).group(1)) == \
        _lib.P2C_GENERATE_FRAME_PARALLEL_MAX_FRAMES


def test_k38_refusals_need_no_launch():
    """Every refusal comes back before anything is launched: the pointers are host addresses that are never followed."""
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    fwd = getattr(_lib.lib(), NAME)
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    cam = (ctypes.c_float * 5)(400, 400, 300, 3.1, 1.2)

    def call(B=1, T=2, first=0, k=3, transform=3, noise=0, camera=cam, loc=p, rot=p, outs=None, mapping=0, cap=0):
        outs = outs if outs is not None else (p,) + (None,) * 15
        return fwd(1, 0, first, B, T, k, 0.1, 0.0, 0.0, transform, noise, 1.0, None, 1e-5, camera, loc, rot, *outs, mapping, cap, None)

    assert call(B=-1) == -2 and call(T=0) == -2 and call(T=_lib.P2C_GENERATE_MAX_T + 1) == -2 and call(first=-1) == -2
    assert call(k=-1) == -2 and call(k=27) == -2 and call(cap=-1) == -2 and call(B=(1 << 40), T=2) == -2
    assert call(transform=4) == -3 and call(noise=2) == -3 and call(mapping=3) == -3
    transformed_only = (None, None, None, p) + (None,) * 12
    assert call(transform=0, outs=transformed_only) == -3 and call(transform=1, outs=transformed_only, B=0) == 0
    assert call(camera=None) == -1 and call(loc=None) == -1 and call(rot=None) == -1 and call(outs=(None,) * 16) == -1
    assert call(B=0) == 0


def test_ops_refuses_before_the_device_is_needed():
    with pytest.raises(_lib.P2CError, match='no CPU implementation'):
        ops.generate_carla_batch(2, 2, seed=1, device='cpu')
    assert ops.generate_miss_prob(None) is None and ops.generate_miss_prob(()) is None
    assert ops.generate_miss_prob(0.25) == (0.25,) * J and ops.generate_miss_prob([0.5]) == (0.5,) * J
    with pytest.raises(ValueError):
        ops.generate_miss_prob([0.1] * 25)
