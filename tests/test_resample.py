"""K37 on the host: the definition of the CARLA row resampler (walker_control/resample.py) in fp64, the streaming resampler on the
tensor path, the file tool and the writers' ``out_fps``, and the C ABI's declaration. No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.walker_control import resample as rs
from pedestrians_video_2_carla_amd.walker_control.resample import CarlaResampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (1, 3, 1, 7, 2, 9)
REFUSED = (ValueError, RuntimeError)


def rows64(N, T, J, seed=0, root=True):
    """Random rows in fp64: locations of unit scale, yaw and roll over +-180 degrees, pitch over +-89."""
    g = torch.Generator().manual_seed(seed)

    def make(*lead):
        loc = torch.randn(*lead, 3, generator=g, dtype=torch.float64)
        u = torch.rand(*lead, 3, generator=g, dtype=torch.float64) * 2 - 1
        return torch.cat((loc, u * torch.tensor([89.0, 180.0, 180.0], dtype=torch.float64)), -1)
    return make(N, T, J), (make(N, T) if root else None)


def resample(bones, root, src, dst, **kw):
    return ops.resample_carla_rows(bones, root, src_fps=src, dst_fps=dst, **kw)


def matrices(rows):
    return ops.carla_pose_import(rows.unsqueeze(-2) if rows.ndim == 1 else rows)[1]


def geodesic(Ra, Rb):
    """The rotation angle of Ra^T Rb, from the skew part and the trace (well conditioned at small angles)."""
    M = Ra.transpose(-1, -2) @ Rb
    skew = torch.stack((M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]), -1)
    return torch.atan2(skew.norm(dim=-1) / 2, (M.diagonal(dim1=-2, dim2=-1).sum(-1) - 1) / 2)


# ---------------------------------------------------------------------------------------------------------- rates that copy
def test_equal_rates_and_integer_decimation_copy_bits():
    bones, root = rows64(2, 13, 5)
    for src, dst, step in ((30, 30, 1), (30, 10, 3), (120, 30, 4)):
        b, r = resample(bones, root, src, dst)
        assert torch.equal(b, bones[:, ::step]) and torch.equal(r, root[:, ::step]), (src, dst)
        assert b.dtype == torch.float64 and not b.requires_grad


@pytest.mark.parametrize('src,dst', [(30, 25), (25, 30)])
def test_hold_is_a_gather_at_the_floor(src, dst):
    bones, root = rows64(2, 23, 4, seed=1)
    b, r = resample(bones, root, src, dst, mode='hold')
    ratio = src / dst
    idx = [math.floor(k * ratio) for k in range(b.shape[1])]
    assert b.shape[1] == rs.output_count(22, ratio) and max(idx) <= 22
    assert torch.equal(b, bones[:, idx]) and torch.equal(r, root[:, idx])


@pytest.mark.parametrize('T', [1, 2, 23, 1000])
@pytest.mark.parametrize('src,dst', [(30, 25), (25, 30), (30, 120), (30, 10), (29.97, 20), (120, 30)])
def test_output_count_is_the_brute_force_count(T, src, dst):
    ratio = rs.rate_ratio(src, dst)
    brute = 0
    while float(brute) * ratio <= T - 1:
        brute += 1
    assert rs.output_count(T - 1, ratio) == brute
    i0, frac = rs.sample_positions(0, brute, ratio)
    assert int(i0[-1]) <= T - 1 and (int(i0[-1]) < T - 1 or float(frac[-1]) == 0.0)
    assert rs.output_count(-1, ratio) == 0


# ------------------------------------------------------------------------------------------------------------- the geometry
@pytest.mark.parametrize('column,a,b', [(4, 170.0, -170.0), (3, 80.0, 89.0), (5, -30.0, 45.0)])
def test_a_fixed_axis_is_linear_in_the_angle_the_short_way_round(column, a, b):
    rows = torch.zeros(1, 2, 1, 6, dtype=torch.float64)
    rows[0, 0, 0, column], rows[0, 1, 0, column] = a, b
    rows[0, :, 0, :3] = torch.tensor([[1.0, -2.0, 3.0], [2.0, 0.0, -1.0]], dtype=torch.float64)
    out, _ = resample(rows, None, 1.0, 4.0)                      # ratio 0.25: positions 0, .25, .5, .75, 1
    assert out.shape == (1, 5, 1, 6)
    span = (b - a + 180.0) % 360.0 - 180.0
    for k in range(5):
        want = a + span * k / 4
        err = abs((float(out[0, k, 0, column]) - want + 180.0) % 360.0 - 180.0)
        assert err <= 1e-9, (column, k, float(out[0, k, 0, column]), want)
        others = [c for c in (3, 4, 5) if c != column]
        assert float(out[0, k, 0, others].abs().max()) <= 1e-9
        assert torch.allclose(out[0, k, 0, :3], rows[0, 0, 0, :3] + (k / 4) * (rows[0, 1, 0, :3] - rows[0, 0, 0, :3]), rtol=0, atol=1e-15)
    assert torch.equal(out[0, 0], rows[0, 0]) and torch.equal(out[0, 4], rows[0, 1])


@pytest.mark.parametrize('through_the_pole', [False, True])
def test_constant_angular_speed_stays_constant(through_the_pole):
    """A rotation about a fixed axis at 2 degrees a source frame, upsampled 10 -> 30; the second case turns about the y axis
    through pitch = 90 degrees, where Euler interpolation fails. The speed: above 0.52 degrees (d < 0.99999: the slerp arm,
    the lerp arm is not uniform), and small enough for the definition's float32 ``frac`` -- 1/3 and 2/3 are 1e-8 and 2e-8 off,
    which moves a step by up to 2e-8 of the source step: 7e-10 rad at 2 degrees."""
    from pedestrians_video_2_carla_amd.transforms.rotation_conversions import euler_angles_to_matrix
    T = 16
    step = math.radians(2.0)
    if through_the_pole:
        axis = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    else:
        axis = torch.randn(3, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
        axis = axis / axis.norm()
    K = torch.zeros(3, 3, dtype=torch.float64)
    K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -axis[2], axis[1], axis[2], -axis[0], -axis[1], axis[0]
    R0 = euler_angles_to_matrix(torch.tensor([0.3, -0.2, 0.5] if not through_the_pole else [0.0, math.radians(76.0), 0.0],
                                             dtype=torch.float64), 'XYZ')
    rots = torch.stack([(torch.eye(3, dtype=torch.float64) + math.sin(t * step) * K + (1 - math.cos(t * step)) * (K @ K)) @ R0
                        for t in range(T)])
    rows, _ = ops.carla_pose_export(torch.zeros(T, 1, 3, dtype=torch.float64), rots.unsqueeze(1))
    if through_the_pole:
        assert float(rows[..., 3].abs().max()) > 80.0 and float(rows[..., 4].abs().max()) > 170.0      # over the pole: yaw flips
    out, _ = resample(rows.unsqueeze(0), None, 10, 30)
    assert out.shape[1] == 3 * (T - 1) + 1
    R = matrices(out[0])[:, 0]
    angles = geodesic(R[:-1], R[1:])
    assert float((angles - step / 3).abs().max()) <= 1e-9, float((angles - step / 3).abs().max())


# --------------------------------------------------------------------------------------------------------- cut invariance
@pytest.mark.parametrize('src,dst', [(30, 25), (25, 30), (29.97, 20), (30, 120), (30, 10), (30, 30)])
def test_pushed_chunks_give_the_uncut_video(src, dst):
    T = sum(CHUNKS)
    assert T == 23
    bones, root = rows64(2, T, 3, seed=2)
    whole_b, whole_r = resample(bones, root, src, dst)
    ratio = rs.rate_ratio(src, dst)
    stream = CarlaResampler(src, dst)
    pieces, positions, t = [], [], 0
    for n in CHUNKS:
        first = stream.outputs
        b, r = stream.push(bones[:, t:t + n], root[:, t:t + n])
        assert b.shape[0] == 2 and b.shape[2:] == (3, 6) and r.shape == b.shape[:2] + (6,)
        positions.append(rs.sample_positions(first, b.shape[1], ratio))
        pieces.append((b, r))
        t += n
    got_b, got_r = torch.cat([p[0] for p in pieces], 1), torch.cat([p[1] for p in pieces], 1)
    assert got_b.shape == whole_b.shape and got_r.shape == whole_r.shape and stream.frames == T
    i0, frac = rs.sample_positions(0, whole_b.shape[1], ratio)
    assert torch.equal(torch.cat([p[0] for p in positions]), i0) and torch.equal(torch.cat([p[1] for p in positions]), frac)
    exact = frac == 0
    assert torch.equal(got_b[:, exact], bones[:, i0[exact]]) and torch.equal(got_r[:, exact], root[:, i0[exact]])
    if bool(exact.all()):
        assert torch.equal(got_b, whole_b) and torch.equal(got_r, whole_r)
    # compared as rotations: near +-180 degrees the same rotation has two rows
    err = max(float((matrices(got_b) - matrices(whole_b)).abs().max()), float((matrices(got_r) - matrices(whole_r)).abs().max()),
              float((got_b[..., :3] - whole_b[..., :3]).abs().max()), float((got_r[..., :3] - whole_r[..., :3]).abs().max()))
    print(f'{src} -> {dst}: cut against uncut, largest difference {err:.3e}')
    assert err <= 1e-12
    rows_err = max(float((got_b - whole_b).abs().max()), float((got_r - whole_r).abs().max()))
    print(f'{src} -> {dst}: rows, largest difference {rows_err:.3e} degree')
    assert rows_err <= 1e-12                                              # and the rows themselves


def test_a_push_can_yield_nothing_and_reset_starts_over():
    bones, root = rows64(1, 6, 2, seed=3)
    stream = CarlaResampler(30, 10)                                       # outputs at frames 0, 3
    shapes = [stream.push(bones[:, t:t + 1], root[:, t:t + 1])[0].shape for t in range(6)]
    assert [s[1] for s in shapes] == [1, 0, 0, 1, 0, 0] and shapes[1] == (1, 0, 2, 6)
    stream.reset()
    b, _ = stream.push(bones, None)
    assert torch.equal(b, bones[:, ::3])
    with pytest.raises(REFUSED):
        stream.push(bones, root)                                          # a root after none
    with pytest.raises(REFUSED):
        stream.push(torch.cat((bones, bones)), None)                      # another N
    with pytest.raises(REFUSED):
        stream.push(bones[:, :, :1], None)                                # another J
    stream.reset()
    assert stream.push(torch.cat((bones, bones)), None)[0].shape == (2, 2, 2, 6)


def test_outputs_that_need_a_frame_not_given_raise():
    bones, _ = rows64(1, 4, 1, seed=6)
    with pytest.raises(REFUSED):
        resample(bones, None, 30, 60, count=8)                            # output 7 sits at 3.5
    assert resample(bones, None, 30, 60, count=7)[0].shape[1] == 7
    with pytest.raises(REFUSED):
        resample(bones, None, 30, 60, first_frame=2, first_output=2)      # output 2 sits at frame 1
    with pytest.raises(REFUSED):
        resample(bones, None, 30, 60, first_frame=2, first_output=3)      # 1.5: frame 1 would be the carry
    got = resample(bones, None, 30, 60, first_frame=2, first_output=3, carry=(bones[:, 0], None), count=2)[0]
    want = resample(torch.cat((bones[:, :1], bones), 1), None, 30, 60, first_frame=1, first_output=3, count=2)[0]
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------------------- NaN
@pytest.mark.parametrize('mode', ['slerp', 'hold'])
def test_a_nan_clip_stays_nan_and_touches_nothing_else(mode):
    bones, root = rows64(3, 9, 4, seed=7)
    bones[1], root[1] = float('nan'), float('nan')
    b, r = resample(bones, root, 30, 25, mode=mode)
    assert bool(torch.isnan(b[1]).all()) and bool(torch.isnan(r[1]).all())
    for n in (0, 2):
        alone_b, alone_r = resample(bones[n:n + 1], root[n:n + 1], 30, 25, mode=mode)
        assert torch.equal(b[n:n + 1], alone_b) and torch.equal(r[n:n + 1], alone_r)
        assert not bool(torch.isnan(b[n]).any())
    # one NaN angle in one source row: the outputs between its neighbours, in that bone only
    bones, _ = rows64(1, 5, 3, seed=8, root=False)
    bones[0, 2, 1, 4] = float('nan')
    clean, _ = rows64(1, 5, 3, seed=8, root=False)
    b, _ = resample(bones, None, 1, 2)                                    # outputs at 0, .5, 1, ..., 4
    bad = torch.isnan(b).any(-1)[0]                                       # (K, J)
    assert bad[:, 1].tolist() == [False, False, False, True, True, True, False, False, False] and not bool(bad[:, (0, 2)].any())
    assert torch.equal(b[0][~bad], resample(clean, None, 1, 2)[0][0][~bad])


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    bones, root = rows64(2, 4, 3)
    for src, dst in ((30, 0), (-30, 20), (30, -20), (30, float('nan')), (float('inf'), 30), (1, 2000), (2000, 1)):
        with pytest.raises(REFUSED):
            resample(bones, root, src, dst)
        with pytest.raises(REFUSED):
            CarlaResampler(src, dst)
    assert resample(bones, root, 1024, 1)[0].shape[1] == 1 and resample(bones[:, :2], None, 1, 1024)[0].shape[1] == 1025
    with pytest.raises(REFUSED):
        resample(bones, root, 30, 20, mode='cubic')
    with pytest.raises(REFUSED):
        CarlaResampler(30, 20, mode='cubic')
    with pytest.raises(REFUSED):
        resample(bones[..., :5], None, 30, 20)
    with pytest.raises(REFUSED):
        resample(bones[0], None, 30, 20)                                  # (T,J,6): no video dimension
    with pytest.raises(REFUSED):
        resample(bones, root[:1], 30, 20)
    with pytest.raises(REFUSED):
        resample(bones, root[:, :3], 30, 20)
    with pytest.raises(REFUSED):
        resample(bones, root.float(), 30, 20)
    with pytest.raises(REFUSED):
        resample(bones, root, 30, 20, first_frame=1, carry=(bones[:1, 0], root[:1, 0]))
    with pytest.raises(REFUSED):
        resample(bones, root, 30, 20, first_frame=1, carry=(bones[:, 0], None))
    stream = CarlaResampler(30, 20)
    stream.push(bones, root)
    with pytest.raises(REFUSED):
        stream.push(bones[:1], root[:1])


def test_other_dtypes_and_views_take_the_definition():
    bones, root = rows64(2, 7, 3, seed=9)
    b32, r32 = resample(bones.float(), root.float(), 30, 20)
    b64, r64 = resample(bones.float().double(), root.float().double(), 30, 20)
    assert b32.dtype == torch.float32 and r32.dtype == torch.float32
    assert float((matrices(b32.double()) - matrices(b64)).abs().max()) < 1e-5
    wide = torch.zeros(2, 7, 3, 8, dtype=torch.float64)
    wide[..., 1:7] = bones
    assert torch.equal(resample(wide[..., 1:7], None, 30, 20)[0], resample(bones, None, 30, 20)[0])
    grad = bones.clone().requires_grad_()
    assert not resample(grad, None, 30, 20)[0].requires_grad


# ----------------------------------------------------------------------------------------------------------------- files
def animation_batches():
    from test_carla_pose import host_batches
    return host_batches(2, 2, 13)


def linear_flow():
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.movements.linear import Linear
    from test_carla_pose import host_flow
    torch.manual_seed(3)
    return host_flow(Linear(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON))


def test_resample_carla_animation_rewrites_a_file(tmp_path):
    from pedestrians_video_2_carla_amd.data.carla.animation import (load_carla_animation, resample_carla_animation,
                                                                    save_carla_animation)
    from pedestrians_video_2_carla_amd.trainer import Trainer
    flow, batches = linear_flow(), animation_batches()
    outputs = Trainer().predict(flow, batches)
    src = load_carla_animation(save_carla_animation(str(tmp_path / 'walk'), outputs, fps=30.0))
    T = src['bones'].shape[1]
    whole = load_carla_animation(resample_carla_animation(str(tmp_path / 'walk.npz'), str(tmp_path / 'walk20'), 20.0))
    K = rs.output_count(T - 1, 30.0 / 20.0)
    assert whole['bones'].shape == (4, K, 26, 6) and whole['root'].shape == (4, K, 6) and whole['fps'] == 20.0
    assert whole['bones'].dtype == np.float32
    assert all(whole[k] == src[k] for k in ('age', 'gender', 'bone_names'))
    want_b, want_r = resample(torch.from_numpy(src['bones']), torch.from_numpy(src['root']), 30.0, 20.0)
    assert np.array_equal(whole['bones'], want_b.numpy()) and np.array_equal(whole['root'], want_r.numpy())
    assert np.array_equal(whole['bones'][:, ::2], src['bones'][:, ::3])                 # every second output is a source frame
    cut = load_carla_animation(resample_carla_animation(str(tmp_path / 'walk.npz'), str(tmp_path / 'walk20c'), 20.0, chunk=5))
    assert cut['bones'].shape == whole['bones'].shape and cut['fps'] == 20.0 and cut['age'] == src['age']
    i0, frac = rs.sample_positions(0, K, 1.5)
    exact = (frac == 0).numpy()
    assert np.array_equal(cut['bones'][:, exact], src['bones'][:, i0.numpy()[exact]])
    assert np.array_equal(cut['root'][:, exact], src['root'][:, i0.numpy()[exact]])
    for k in ('bones', 'root'):
        diff = np.abs(cut[k].astype(np.float64) - whole[k].astype(np.float64))
        diff[..., 3:] = np.minimum(diff[..., 3:], 360.0 - diff[..., 3:])                # the same angle on both sides of the seam
        scale = np.maximum(np.abs(whole[k][..., :3]).max(), 1.0)
        assert diff[..., 3:].max() <= 1e-5 and diff[..., :3].max() <= 1e-6 * scale, (k, diff.max())
    hold = load_carla_animation(resample_carla_animation(str(tmp_path / 'walk.npz'), str(tmp_path / 'walkh'), 20.0, mode='hold'))
    assert np.array_equal(hold['bones'], src['bones'][:, [math.floor(k * 1.5) for k in range(K)]])


def test_writers_with_out_fps(tmp_path):
    from pedestrians_video_2_carla_amd.data.carla import animation
    from pedestrians_video_2_carla_amd.trainer import Trainer
    flow, batches = linear_flow(), animation_batches()
    outputs = Trainer().predict(flow, batches)
    plain = animation.save_carla_animation(str(tmp_path / 'a'), outputs, fps=30.0)
    explicit = animation.save_carla_animation(str(tmp_path / 'b'), outputs, fps=30.0, out_fps=None)
    assert open(plain, 'rb').read() == open(explicit, 'rb').read()                      # None: the bytes of the call without it
    lifted = animation.lift_carla_animation(str(tmp_path / 'c'), flow, batches, fps=30.0)
    lifted_none = animation.lift_carla_animation(str(tmp_path / 'd'), flow, batches, fps=30.0, out_fps=None)
    assert open(lifted, 'rb').read() == open(lifted_none, 'rb').read()
    src = animation.load_carla_animation(plain)
    want_b, want_r = resample(torch.from_numpy(src['bones']), torch.from_numpy(src['root']), 30.0, 20.0)
    for path in (animation.save_carla_animation(str(tmp_path / 'e'), outputs, fps=30.0, out_fps=20.0),
                 animation.lift_carla_animation(str(tmp_path / 'f'), flow, batches, fps=30.0, out_fps=20.0)):
        got = animation.load_carla_animation(path)
        assert got['fps'] == 20.0 and got['age'] == src['age'] and got['gender'] == src['gender']
        assert np.array_equal(got['bones'], want_b.numpy()) and np.array_equal(got['root'], want_r.numpy())
    rows = Trainer().predict_carla(flow, batches)
    fast = Trainer().predict_carla(flow, batches, src_fps=30, out_fps=20)
    again = Trainer().predict_carla(flow, batches, src_fps=None, out_fps=None)
    for (b, r, meta), (fb, fr, fmeta), (ab, ar, _) in zip(rows, fast, again):
        assert torch.equal(ab, b) and torch.equal(ar, r) and fmeta is meta
        wb, wr = CarlaResampler(30, 20).resample(b, r)
        assert torch.equal(fb, wb) and torch.equal(fr, wr) and fb.shape[1] == rs.output_count(b.shape[1] - 1, 1.5)
    with pytest.raises(ValueError):
        Trainer().predict_carla(flow, batches, out_fps=20)


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_k37_symbol_is_declared_bound_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    header = open(os.path.join(ROOT, 'include', 'p2c.h')).read()
    declared = set(re.findall(r'P2C_API[^;(]*?\b(p2c_\w+)\s*\(', header))
    name = 'p2c_carla_resample_fwd'
    assert name in declared and name in _lib.SYMBOLS and getattr(_lib.lib(), name) is not None
    res, args = _lib.SYMBOLS[name]
    assert res is ctypes.c_int and args[-1] is ctypes.c_void_p and name in _lib._PoisonedLib(_lib.lib())._wrap
    decl = re.search(r'P2C_API int p2c_carla_resample_fwd\((.*?)\);', header, re.S).group(1)
    params = [' '.join(p.split()) for p in decl.split(',')]
    ctype = {'const float *': ctypes.c_void_p, 'float *': ctypes.c_void_p, 'void *': ctypes.c_void_p, 'int64_t ': ctypes.c_int64,
             'int32_t ': ctypes.c_int32, 'double ': ctypes.c_double}
    assert [ctype[re.match(r'(.*?)(\w+)$', p).group(1)] for p in params] == list(args)
    assert [re.match(r'(.*?)(\w+)$', p).group(2) for p in params] == [
        'bones', 'root', 'carry_bones', 'carry_root', 'out_bones', 'out_root', 'N', 'T', 'J', 'K', 'first_output', 'first_frame',
        'ratio', 'mode', 'max_blocks', 'stream']
    assert (rs.MODES['slerp'], rs.MODES['hold']) == tuple(
        int(re.search(rf'P2C_RESAMPLE_{m} = (\d+)', header).group(1)) for m in ('SLERP', 'HOLD'))
    # the kernel file shares the row arithmetic, allocates no LDS, has no atomics and needs no inline assembly
    source = open(os.path.join(ROOT, 'pedestrians_video_2_carla_amd', 'csrc', 'p2c_resample.hip')).read()
    assert '#include "p2c_carla_dev.h"' in source and 'carla_row(' in source and 'p2c_host::grid_for(' in source
    assert '__shared__' not in source and 'asm' not in source.replace('__launch_bounds__', '') and '__syncthreads' not in source
    assert 'atomic' not in source and 'fminf' not in source and 'fmaxf' not in source
