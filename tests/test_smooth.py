"""K39 on the host: the definition of the CARLA row smoother (walker_control/smooth.py) in fp64 and fp32, the streaming smoother on
the tensor path, the file tool and the writers' ``smooth``, and the C ABI's declarations. No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.walker_control import smooth as sm
from pedestrians_video_2_carla_amd.walker_control.smooth import CarlaSmoother
from test_carla_pose_gpu import MATRIX_FLOOR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (1, 3, 1, 7, 2, 9, 17)
REFUSED = (ValueError, RuntimeError)
GAUSS = dict(mode='gaussian', sigma=2.0, radius=6)
EURO = dict(mode='one_euro', fps=30.0, min_cutoff=1.0, beta_loc=0.5, beta_rot=0.5)
F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------------ inputs
def rodrigues(axis, angle):
    """Unit ``axis`` (...,3) and ``angle`` (...) in radians -> rotation matrices (...,3,3)."""
    x, y, z = axis.unbind(-1)
    o = torch.zeros_like(x)
    K = torch.stack((o, -z, y, z, o, -x, -y, x, o), -1).reshape(axis.shape[:-1] + (3, 3))
    eye = torch.eye(3, dtype=axis.dtype).expand_as(K)
    s, c = torch.sin(angle)[..., None, None], torch.cos(angle)[..., None, None]
    return eye + s * K + (1 - c) * (K @ K)


def unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def random_rotations(g, *lead):
    """Over the whole sphere: pitch reaches +-90 degrees and yaw crosses the seam."""
    return rodrigues(unit(torch.randn(*lead, 3, generator=g, dtype=F64)), (torch.rand(*lead, generator=g, dtype=F64) * 2 - 1) * math.pi)


def rows_of(loc, rot):
    """Locations (...,3) as stored in a row and rotations (...,3,3) -> rows (...,6), through the fp64 ``carla_pose_export``."""
    stored = loc * torch.tensor([1.0, 1.0, -1.0], dtype=loc.dtype)
    return ops.carla_pose_export(stored.unsqueeze(-2), rot.unsqueeze(-3))[0].squeeze(-2)


def matrices(rows):
    return ops.carla_pose_import(rows.unsqueeze(-2))[1].squeeze(-3)


def geodesic(Ra, Rb):
    """The rotation angle of Ra^T Rb in radians, from the skew part and the trace (well conditioned at small angles)."""
    M = Ra.transpose(-1, -2) @ Rb
    skew = torch.stack((M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]), -1)
    return torch.atan2(skew.norm(dim=-1) / 2, (M.diagonal(dim1=-2, dim2=-1).sum(-1) - 1) / 2)


def smooth_paths(N, T, J, seed=0):
    """fp64 rows ``(bones (N,T,J,6), root (N,T,6))`` of smooth quaternion paths: a random base orientation, increments of at
    most 5 degrees a frame about random axes, 1 degree (s.d.) of jitter on top; unit-scale locations drifting with small noise."""
    g = torch.Generator().manual_seed(7000 + 1000 * N + 10 * T + J + seed)

    def make(*lead):                                       # lead = (N, ...) without the time dimension
        rot = [random_rotations(g, *lead)]
        loc = [torch.randn(*lead, 3, generator=g, dtype=F64)]
        for _ in range(T - 1):
            step = rodrigues(unit(torch.randn(*lead, 3, generator=g, dtype=F64)),
                             torch.rand(*lead, generator=g, dtype=F64) * math.radians(5.0))
            rot.append(rot[-1] @ step)
            loc.append(loc[-1] + 0.02 * torch.randn(*lead, 3, generator=g, dtype=F64))
        rot, loc = torch.stack(rot, 1), torch.stack(loc, 1)
        jitter = rodrigues(unit(torch.randn(*rot.shape[:-2], 3, generator=g, dtype=F64)),
                           torch.randn(*rot.shape[:-2], generator=g, dtype=F64) * math.radians(1.0))
        return rows_of(loc + 0.005 * torch.randn(loc.shape, generator=g, dtype=F64), rot @ jitter)
    return make(N, J), make(N)


def smooth(bones, root=None, **kw):
    return ops.smooth_carla_rows(bones, root, **kw)[:2]


def table_of(sigma, R):
    return [float(np.float32(math.exp(-d * d / (2.0 * sigma * sigma)))) for d in range(R + 1)]


# ------------------------------------------------------------------------------------------------------------------ copies
@pytest.mark.parametrize('dtype', [torch.float32, F64])
def test_copies_and_constant_videos(dtype):
    bones, root = (t.to(dtype) for t in smooth_paths(2, 9, 5))
    for kw in (dict(sigma=0.0), dict(sigma=0.0, radius=4), dict(sigma=2.0, radius=0)):
        b, r = smooth(bones, root, mode='gaussian', **kw)
        assert torch.equal(b, bones) and torch.equal(r, root) and b.data_ptr() != bones.data_ptr(), kw
        assert b.dtype == dtype and not b.requires_grad
    b, r, state = ops.smooth_carla_rows(bones, root, **EURO)
    assert torch.equal(b[:, 0], bones[:, 0]) and torch.equal(r[:, 0], root[:, 0]) and b.shape == bones.shape
    assert state[0].shape == (2, 5, 12) and state[1].shape == (2, 12) and state[0].dtype == dtype
    assert sm.gauss_table(2.0, 6).tolist() == table_of(2.0, 6) and sm.gauss_table(2.0, 6).dtype == torch.float32
    # a constant video comes back constant
    still_b, still_r = bones[:, :1].expand(-1, 20, -1, -1).contiguous(), root[:, :1].expand(-1, 20, -1).contiguous()
    scale = float(still_b[..., :3].abs().max())
    eps = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    for kw in (GAUSS, EURO):
        b, r = smooth(still_b, still_r, **kw)
        rot_err = max(float((matrices(b.double()) - matrices(still_b.double())).abs().max()),
                      float((matrices(r.double()) - matrices(still_r.double())).abs().max()))
        loc_err = max(float((b[..., :3] - still_b[..., :3]).abs().max()), float((r[..., :3] - still_r[..., :3]).abs().max()))
        print(f'{kw["mode"]} {dtype}: a constant video moves by {rot_err:.3e} (matrix entries), {loc_err:.3e} (locations)')
        # locations: 2R + 1 products, as many additions of the sum of the weights and a division, each rounded once
        assert rot_err < MATRIX_FLOOR and loc_err <= (4 * 6 + 4) * eps * scale, kw['mode']


# ------------------------------------------------------------------------------------------- the window on uniform motion
def test_the_gaussian_window_is_unbiased_on_uniform_motion():
    g = torch.Generator().manual_seed(11)
    N, T, J, R = 2, 30, 4, 6
    base, axis = random_rotations(g, N, 1, J), unit(torch.randn(N, 1, J, 3, generator=g, dtype=F64))
    t = torch.arange(T, dtype=F64).reshape(1, T, 1)
    rot = base @ rodrigues(axis.expand(N, T, J, 3), (math.radians(3.0) * t).expand(N, T, J))
    loc = torch.randn(N, 1, J, 3, generator=g, dtype=F64) + t.unsqueeze(-1) * torch.randn(N, 1, J, 3, generator=g, dtype=F64) * 0.1
    bones = rows_of(loc, rot)
    root = rows_of(loc[:, :, 0], rot[:, :, 0])
    b, r = smooth(bones, root, **GAUSS)
    inner = slice(R, T - R)
    err = max(float((matrices(b) - matrices(bones))[:, inner].abs().max()), float((matrices(r) - matrices(root))[:, inner].abs().max()),
              float((b - bones)[:, inner, :, :3].abs().max()), float((r - root)[:, inner, :3].abs().max()))
    print(f'uniform motion, interior frames: smoothed against the input {err:.3e}')
    assert err <= 1e-9
    edge = float(geodesic(matrices(b), matrices(bones))[:, :R].max())
    assert edge > 1e-3                                           # the truncated windows at the ends are one-sided: they do move


# ------------------------------------------------------------------------------------------------------------ seam and pole
@pytest.mark.parametrize('pitch,roll', [(0.0, 0.0), (88.0, 10.0)])
@pytest.mark.parametrize('dtype', [torch.float32, F64])
def test_the_seam_and_the_pole(pitch, roll, dtype):
    yaw = torch.arange(160.0, 202.0, 2.0, dtype=F64)
    yaw = torch.where(yaw > 180.0, yaw - 360.0, yaw)             # 160 .. 180, -178 .. -160
    T, R = len(yaw), 3
    assert T == 21 and float(yaw[-1]) == -160.0
    rows = torch.zeros(1, T, 1, 6, dtype=F64)
    rows[..., 3], rows[..., 4], rows[..., 5] = pitch, yaw.reshape(1, T, 1), roll
    rows = rows.to(dtype)
    inner = slice(R, T - R)
    for kw in (dict(mode='gaussian', sigma=1.5, radius=R), dict(mode='one_euro', fps=30.0, min_cutoff=10.0)):
        out, _ = smooth(rows, None, **kw)
        off = torch.rad2deg(geodesic(matrices(out.double()), matrices(rows.double())))[0, inner]
        print(f'pitch {pitch} {dtype} {kw["mode"]}: at most {float(off.max()):.3e} degree from the input')
        assert float(off.max()) <= 2.0
    # the average of the Euler angles themselves leaves the path at the seam
    w = torch.tensor(table_of(1.5, R), dtype=F64)
    w = torch.cat((w.flip(0)[:-1], w))
    naive = torch.stack([(rows[0, t - R:t + R + 1, 0].double() * w[:, None]).sum(0) / w.sum() for t in range(R, T - R)])
    off = torch.rad2deg(geodesic(matrices(naive), matrices(rows.double()[0, inner, 0])))
    assert float(off.max()) > 2.0


# --------------------------------------------------------------------------------------------------------- noise reduction
def test_gaussian_noise_reduction_is_what_the_table_says():
    g = torch.Generator().manual_seed(5)
    N, T, J, R, sigma = 4, 64, 26, 6, 2.0
    pose, place = random_rotations(g, N, 1, J), torch.randn(N, 1, J, 3, generator=g, dtype=F64)
    jitter = torch.randn(N, T, J, 3, generator=g, dtype=F64) * math.radians(1.0)          # a rotation vector, 1 degree s.d. an axis
    rot = pose @ rodrigues(unit(jitter), jitter.norm(dim=-1))
    loc = place + 0.01 * torch.randn(N, T, J, 3, generator=g, dtype=F64)
    bones = rows_of(loc, rot)
    out, _ = smooth(bones, None, mode='gaussian', sigma=sigma, radius=R)

    def rotation_vectors(rows):                                  # of pose^T R: the skew part, sin(angle) ~ angle at a degree
        M = pose.transpose(-1, -2) @ matrices(rows)
        return torch.stack((M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]), -1) / 2

    def rms(v):
        return float(v[:, R:T - R].pow(2).mean().sqrt())
    w = torch.tensor(table_of(sigma, R), dtype=F64)
    w = torch.cat((w.flip(0)[:-1], w))
    want = float(w.pow(2).sum().sqrt() / w.sum())
    assert abs(want - 0.38) < 0.01
    got_rot = rms(rotation_vectors(out)) / rms(rotation_vectors(bones))
    got_loc = rms(out[..., :3] - place) / rms(bones[..., :3] - place)
    print(f'noise after / before: rotations {got_rot:.4f}, locations {got_loc:.4f}, sqrt(sum w^2) / sum w = {want:.4f}')
    assert 0.75 * want <= got_rot <= 1.25 * want and 0.75 * want <= got_loc <= 1.25 * want


# ---------------------------------------------------------------------------------------------------------------- one euro
def test_one_euro_locations_are_the_plain_recursion_without_beta():
    bones, root = smooth_paths(2, 25, 3, seed=1)
    fps, fc = 30.0, 1.5
    b, r = smooth(bones, root, mode='one_euro', fps=fps, min_cutoff=fc)
    alpha = 1.0 / (1.0 + fps / (2.0 * math.pi * fc))
    for got, src in ((b, bones), (r, root)):
        x = src[:, 0, ..., :3].clone()
        want = [x]
        for t in range(1, src.shape[1]):
            x = x + alpha * (src[:, t, ..., :3] - x)
            want.append(x)
        err = float((got[..., :3] - torch.stack(want, 1)).abs().max())
        print(f'one_euro without beta against the recursion: {err:.3e}')
        assert err <= 1e-12


def test_one_euro_with_beta_lags_less_behind_a_step():
    T, step = 12, 5
    rows = torch.zeros(1, T, 1, 6, dtype=F64)
    rows[0, step:, 0, 4] = 30.0
    target = matrices(rows[:, -1])
    slow, _ = smooth(rows, None, mode='one_euro', fps=30.0, beta_rot=0.0)
    fast, _ = smooth(rows, None, mode='one_euro', fps=30.0, beta_rot=0.5)
    off_slow = float(torch.rad2deg(geodesic(matrices(slow[:, step + 2]), target)))
    off_fast = float(torch.rad2deg(geodesic(matrices(fast[:, step + 2]), target)))
    print(f'two frames after a 30 degree step: {off_slow:.3f} degree behind without beta_rot, {off_fast:.3f} with')
    assert 0.0 < off_fast < off_slow < 30.0
    assert torch.equal(slow[:, :step], rows[:, :step]) and torch.equal(fast[:, :step], rows[:, :step])   # nothing moves before it


# --------------------------------------------------------------------------------------------------------------- streaming
@pytest.mark.parametrize('dtype', [torch.float32, F64])
@pytest.mark.parametrize('with_root', [True, False])
@pytest.mark.parametrize('kw', [dict(mode='gaussian', sigma=1.0, radius=3), EURO], ids=['gaussian', 'one_euro'])
def test_pushed_chunks_give_the_bits_of_the_uncut_video(kw, with_root, dtype):
    T = sum(CHUNKS)
    assert T == 40
    bones, root = (t.to(dtype) for t in smooth_paths(2, T, 5, seed=2))
    root = root if with_root else None
    stream = CarlaSmoother(**kw)
    whole_b, whole_r = stream.smooth(bones, root)
    assert whole_b.shape == bones.shape and whole_b.dtype == dtype
    pieces, t = [], 0
    for n in CHUNKS:
        pieces.append(stream.push(bones[:, t:t + n], root[:, t:t + n] if with_root else None))
        t += n
    counts = [p[0].shape[1] for p in pieces]
    assert counts == ([0, 1, 1, 7, 2, 9, 17] if kw['mode'] == 'gaussian' else list(CHUNKS))
    assert pieces[0][0].shape == (2, counts[0], 5, 6) and pieces[0][0].dtype == dtype
    assert stream.frames == T and stream.outputs == sum(counts)
    last = stream.flush()
    assert last[0].shape == (2, T - sum(counts), 5, 6) and stream.frames == 0
    pieces.append(last)
    assert torch.equal(torch.cat([p[0] for p in pieces], 1), whole_b)
    if with_root:
        assert all(p[1].shape == p[0].shape[:2] + (6,) for p in pieces)
        assert torch.equal(torch.cat([p[1] for p in pieces], 1), whole_r)
    else:
        assert whole_r is None and all(p[1] is None for p in pieces)


@pytest.mark.parametrize('kw', [dict(mode='gaussian', sigma=1.0, radius=3), EURO], ids=['gaussian', 'one_euro'])
def test_a_layout_change_raises_until_reset(kw):
    bones, root = smooth_paths(2, 8, 3, seed=3)
    stream = CarlaSmoother(**kw)
    with pytest.raises(REFUSED):
        stream.flush()                                                    # nothing was pushed
    stream.push(bones[:, :4], root[:, :4])
    for b, r in ((bones[:1, 4:], root[:1, 4:]), (bones[:, 4:, :2], root[:, 4:]), (bones[:, 4:], None)):
        with pytest.raises(REFUSED):
            stream.push(b, r)
    with pytest.raises(REFUSED):
        stream.push(bones[:, :0], root[:, :0])                            # a chunk holds a frame
    stream.push(bones[:, 4:], root[:, 4:])                                # the videos go on
    stream.reset()
    b, _ = stream.push(bones[:1, :7, :2], None)
    b = torch.cat((b, stream.flush()[0]), 1)
    assert torch.equal(b, stream.smooth(bones[:1, :7, :2])[0])


# --------------------------------------------------------------------------------------------------------------------- NaN
@pytest.mark.parametrize('kw', [dict(mode='gaussian', sigma=1.0, radius=2), EURO], ids=['gaussian', 'one_euro'])
def test_nan_goes_where_the_arithmetic_takes_it_and_nowhere_else(kw):
    bones, root = smooth_paths(3, 12, 4, seed=4)
    clean_b, clean_r = smooth(bones, root, **kw)
    poisoned_b, poisoned_r = bones.clone(), root.clone()
    poisoned_b[1], poisoned_r[1] = float('nan'), float('nan')
    b, r = smooth(poisoned_b, poisoned_r, **kw)
    assert bool(torch.isnan(b[1]).all()) and bool(torch.isnan(r[1]).all())
    for n in (0, 2):
        alone_b, alone_r = smooth(bones[n:n + 1], root[n:n + 1], **kw)
        assert torch.equal(b[n:n + 1], alone_b) and torch.equal(r[n:n + 1], alone_r)
        assert not bool(torch.isnan(b[n]).any()) and not bool(torch.isnan(r[n]).any())
    # one NaN row: that bone within R frames (gaussian), that chain from there on (one_euro)
    one = bones.clone()
    one[0, 5, 1] = float('nan')
    b, r = smooth(one, root, **kw)
    bad = torch.isnan(b).any(-1)
    want = torch.zeros_like(bad)
    if kw['mode'] == 'gaussian':
        want[0, 3:8, 1] = True
    else:
        want[0, 5:, 1] = True
    assert torch.equal(bad, want) and torch.equal(b[~bad], clean_b[~bad]) and torch.equal(r, clean_r)


# ----------------------------------------------------------------------------------------------------------------- writers
def test_writers_and_the_file_tool(tmp_path):
    from pedestrians_video_2_carla_amd.data.carla import animation
    from pedestrians_video_2_carla_amd.trainer import Trainer
    from pedestrians_video_2_carla_amd.walker_control.resample import CarlaResampler
    from test_resample import animation_batches, linear_flow
    flow, batches = linear_flow(), animation_batches()
    outputs = Trainer().predict(flow, batches)
    plain = animation.save_carla_animation(str(tmp_path / 'a'), outputs, fps=30.0)
    explicit = animation.save_carla_animation(str(tmp_path / 'b'), outputs, fps=30.0, smooth=None)
    assert open(plain, 'rb').read() == open(explicit, 'rb').read()         # None: the bytes of the call without it
    lifted = animation.lift_carla_animation(str(tmp_path / 'c'), flow, batches, fps=30.0)
    lifted_none = animation.lift_carla_animation(str(tmp_path / 'd'), flow, batches, fps=30.0, smooth=None)
    assert open(lifted, 'rb').read() == open(lifted_none, 'rb').read()
    src = animation.load_carla_animation(plain)
    src_b, src_r = torch.from_numpy(src['bones']), torch.from_numpy(src['root'])
    T = src_b.shape[1]
    assert T == 13
    for kw in (dict(mode='gaussian', sigma=1.0), dict(mode='one_euro', beta_rot=0.2)):
        full = dict(kw, fps=src['fps']) if kw['mode'] == 'one_euro' else kw
        want_b, want_r = CarlaSmoother(**full).smooth(src_b, src_r)
        assert not torch.equal(want_b, src_b)
        # the file tool: whole and in chunks
        whole = animation.load_carla_animation(animation.smooth_carla_animation(plain, str(tmp_path / 'w'), **kw))
        cut = animation.load_carla_animation(animation.smooth_carla_animation(plain, str(tmp_path / 'x'), chunk=7, **kw))
        for got in (whole, cut):
            assert np.array_equal(got['bones'], want_b.numpy()) and np.array_equal(got['root'], want_r.numpy())
            assert got['fps'] == 30.0 and all(got[k] == src[k] for k in ('age', 'gender', 'bone_names'))
            assert got['bones'].dtype == np.float32
        # the writers: a dict or a smoother, per batch where the rows are
        for smoother in (kw, CarlaSmoother(**full)):
            for path in (animation.save_carla_animation(str(tmp_path / 'e'), outputs, fps=30.0, smooth=smoother),
                         animation.lift_carla_animation(str(tmp_path / 'f'), flow, batches, fps=30.0, smooth=smoother)):
                got = animation.load_carla_animation(path)
                assert got['fps'] == 30.0 and np.array_equal(got['bones'], want_b.numpy()) and np.array_equal(got['root'], want_r.numpy())
        # smoothing comes before the resampling, at the source rate
        rate_b, rate_r = CarlaResampler(30.0, 20.0).resample(want_b, want_r)
        other_b, _ = CarlaSmoother(**(dict(full, fps=20.0) if kw['mode'] == 'one_euro' else full)).smooth(
            *CarlaResampler(30.0, 20.0).resample(src_b, src_r))
        assert not torch.equal(other_b, rate_b)
        for path in (animation.save_carla_animation(str(tmp_path / 'g'), outputs, fps=30.0, out_fps=20.0, smooth=kw),
                     animation.lift_carla_animation(str(tmp_path / 'h'), flow, batches, fps=30.0, out_fps=20.0, smooth=kw)):
            got = animation.load_carla_animation(path)
            assert got['fps'] == 20.0 and np.array_equal(got['bones'], rate_b.numpy()) and np.array_equal(got['root'], rate_r.numpy())
        rows = Trainer().predict_carla(flow, batches)
        smoothed = Trainer().predict_carla(flow, batches, smooth=full)
        both = Trainer().predict_carla(flow, batches, src_fps=30, out_fps=20, smooth=kw)
        for (b, r, meta), (sb, sr, smeta), (fb, fr, _) in zip(rows, smoothed, both):
            wb, wr = CarlaSmoother(**full).smooth(b, r)
            assert torch.equal(sb, wb) and torch.equal(sr, wr) and smeta is meta
            xb, xr = CarlaResampler(30, 20).resample(wb, wr)
            assert torch.equal(fb, xb) and torch.equal(fr, xr)
    with pytest.raises(REFUSED):
        animation.smooth_carla_animation(plain, str(tmp_path / 'y'), chunk=0, sigma=1.0)
    with pytest.raises(REFUSED):
        animation.save_carla_animation(str(tmp_path / 'z'), outputs, smooth=dict(sigma=1.0))          # no mode


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    bones, root = smooth_paths(2, 6, 3, seed=5)
    for kw in (dict(mode='median', sigma=1.0), dict(mode='gaussian'), dict(mode='gaussian', sigma=-1.0),
               dict(mode='gaussian', sigma=float('nan')), dict(mode='gaussian', sigma=1.0, radius=33),
               dict(mode='gaussian', sigma=1.0, radius=-1), dict(mode='gaussian', sigma=11.0),  # ceil(3 sigma) = 33
               dict(mode='gaussian', sigma=1.0, radius=2.5), dict(mode='one_euro'), dict(mode='one_euro', fps=0.0),
               dict(mode='one_euro', fps=-30.0), dict(mode='one_euro', fps=float('inf')), dict(mode='one_euro', fps=float('nan')),
               dict(mode='one_euro', fps=30.0, min_cutoff=0.0), dict(mode='one_euro', fps=30.0, d_cutoff=-1.0),
               dict(mode='one_euro', fps=30.0, beta_loc=-0.1), dict(mode='one_euro', fps=30.0, beta_rot=float('nan'))):
        with pytest.raises(REFUSED):
            smooth(bones, root, **kw)
        with pytest.raises(REFUSED):
            CarlaSmoother(**kw)
    with pytest.raises(REFUSED):
        CarlaSmoother('gaussian', sigma=1.0, fps=30.0)                    # not an argument of this mode
    assert smooth(bones, root, mode='gaussian', sigma=10.0, radius=32)[0].shape == bones.shape
    g = dict(mode='gaussian', sigma=1.0, radius=2)
    # a span that is not covered: the end is not known and the last windows reach past the frames; frames before the first given
    assert ops.smooth_carla_rows(bones, root, last_frame=-1, **g)[0].shape[1] == 4
    for kw in (dict(last_frame=-1, count=5), dict(first_frame=3, first_output=4), dict(first_frame=0, first_output=5, count=2),
               dict(last_frame=4, count=6), dict(last_frame=9), dict(first_output=-1), dict(first_frame=-1), dict(count=-1),
               dict(last_frame=-2)):
        with pytest.raises(REFUSED):
            ops.smooth_carla_rows(bones, root, **g, **kw)
    assert ops.smooth_carla_rows(bones, root, first_frame=3, first_output=5, last_frame=-1, **g)[0].shape[1] == 2
    for b, r in ((bones[..., :5], None), (bones[0], None), (bones, root[:1]), (bones, root[:, :3]), (bones, root.float())):
        with pytest.raises(REFUSED):
            smooth(b, r, **g)
    for state in ((torch.zeros(2, 3, 11, dtype=F64), torch.zeros(2, 12, dtype=F64)), (torch.zeros(2, 3, 12, dtype=F64), None),
                  (torch.zeros(2, 3, 12), torch.zeros(2, 12))):
        with pytest.raises(REFUSED):
            ops.smooth_carla_rows(bones, root, state=state, **EURO)


def test_other_dtypes_and_views_take_the_definition():
    bones, root = smooth_paths(2, 9, 3, seed=6)
    for kw in (GAUSS, EURO):
        b32, r32 = smooth(bones.float(), root.float(), **kw)
        b64, r64 = smooth(bones.float().double(), root.float().double(), **kw)
        assert b32.dtype == torch.float32 and r32.dtype == torch.float32
        assert float((matrices(b32.double()) - matrices(b64)).abs().max()) < 1e-5
        wide = torch.zeros(2, 9, 3, 8, dtype=F64)
        wide[..., 1:7] = bones
        assert torch.equal(smooth(wide[..., 1:7], None, **kw)[0], smooth(bones, None, **kw)[0])
        assert not smooth(bones.clone().requires_grad_(), None, **kw)[0].requires_grad
    # the given state is left as it was
    _, _, state = ops.smooth_carla_rows(bones[:, :4], root[:, :4], **EURO)
    kept = [s.clone() for s in state]
    _, _, after = ops.smooth_carla_rows(bones[:, 4:], root[:, 4:], state=state, **EURO)
    assert torch.equal(state[0], kept[0]) and torch.equal(state[1], kept[1]) and not torch.equal(after[0], kept[0])


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_k39_symbols_are_declared_bound_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    header = open(os.path.join(ROOT, 'include', 'p2c.h')).read()
    declared = set(re.findall(r'P2C_API[^;(]*?\b(p2c_\w+)\s*\(', header))
    ctype = {'const float *': ctypes.c_void_p, 'float *': ctypes.c_void_p, 'void *': ctypes.c_void_p, 'int64_t ': ctypes.c_int64,
             'int32_t ': ctypes.c_int32, 'double ': ctypes.c_double}
    names = {'p2c_carla_smooth_gauss_fwd': ['bones', 'root', 'out_bones', 'out_root', 'weights', 'N', 'S', 'J', 'K', 'first_frame',
                                            'first_output', 'last_frame', 'R', 'max_blocks', 'stream'],
             'p2c_carla_smooth_euro_fwd': ['bones', 'root', 'state_bones', 'state_root', 'out_bones', 'out_root', 'N', 'T', 'J',
                                           'has_state', 'fps', 'min_cutoff', 'beta_loc', 'beta_rot', 'd_cutoff', 'max_blocks',
                                           'stream']}
    for name, want in names.items():
        assert name in declared and name in _lib.SYMBOLS and getattr(_lib.lib(), name) is not None
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p and name in _lib._PoisonedLib(_lib.lib())._wrap
        decl = re.search(rf'P2C_API int {name}\((.*?)\);', header, re.S).group(1)
        params = [' '.join(p.split()) for p in decl.split(',')]
        assert [ctype[re.match(r'(.*?)(\w+)$', p).group(1)] for p in params] == list(args)
        assert [re.match(r'(.*?)(\w+)$', p).group(2) for p in params] == want
    assert int(re.search(r'#define P2C_SMOOTH_MAX_RADIUS (\d+)', header).group(1)) == sm.MAX_RADIUS == _lib.P2C_SMOOTH_MAX_RADIUS == 32
    # the kernel file shares the row arithmetic with K37 (moved, not copied), has no atomics and needs no inline assembly
    csrc = os.path.join(ROOT, 'pedestrians_video_2_carla_amd', 'csrc')
    source = open(os.path.join(csrc, 'p2c_smooth.hip')).read()
    assert '#include "p2c_carla_dev.h"' in source and 'carla_row(' in source and 'p2c_host::grid_for(' in source
    assert 'sincosf(' not in source and 'sincosf(' not in open(os.path.join(csrc, 'p2c_resample.hip')).read()
    assert open(os.path.join(csrc, 'p2c_carla_dev.h')).read().count('void row_quat(') == 1
    assert 'asm' not in source.replace('__launch_bounds__', '') and 'atomic' not in source.replace('no atomics', '')
    assert 'fminf' not in source and 'fmaxf' not in source
