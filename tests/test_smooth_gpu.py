"""K39 (csrc/p2c_smooth.hip) on the device: against the fp64 definition in matrix space, the outputs that must be copies, bit
stability across grids, tiles, requests, views and cuts of the video, NaN clips, the dispatch and the C ABI's refusals, and
``Trainer.predict_carla`` with a smoother.

The allowance is the project's rule (tests/test_carla_pose_gpu.py, tests/test_resample_gpu.py): what the fp32 tensor restatement
of the definition, run on the device (``P2C_SMOOTH_FRAMEWORK=1``), is from fp64 on the same fp32 inputs is measured, and the
kernel gets four times that, with the floors ``MATRIX_FLOOR`` (matrix entries) and ``1e-6 max|loc|`` (locations). Rows are
compared as the matrices ``carla_pose_import`` makes of them in fp64.

Inputs are smooth quaternion paths (``test_smooth.smooth_paths``): a base orientation anywhere on the sphere, at most 5 degrees
a frame plus a degree of jitter. Which sign a neighbour's quaternion gets is decided by a dot product; where that is near 0 the
decision is ill posed and no fp32 code can agree with fp64. On these paths a neighbour R <= 6 frames away is at most about
R * 7 degrees from its centre, a dot product of at least cos(R * 3.5 degrees) >= 0.93 in magnitude; every case asserts >= 0.5 on
its fp64 reference.
"""
import functools
import math

import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.walker_control import smooth as sm
from pedestrians_video_2_carla_amd.walker_control.resample import _row_quat
from pedestrians_video_2_carla_amd.walker_control.smooth import CarlaSmoother
from test_carla_pose_gpu import MATRIX_FLOOR
from test_smooth import smooth_paths

pytestmark = pytest.mark.gpu

# (N, T, J, max_blocks): a window longer than the video; truncated on both sides at once (R = 3); several tiles, the root the
# 27th row; one row a frame; a partial last tile; two workgroups striding over the tiles
SHAPES = [(1, 1, 26, 0), (2, 5, 26, 0), (3, 40, 26, 0), (1, 40, 1, 0), (2, 33, 5, 0), (2, 40, 26, 2)]
CONFIGS = {'gauss-1-3': dict(mode='gaussian', sigma=1.0, radius=3), 'gauss-2-6': dict(mode='gaussian', sigma=2.0, radius=6),
           'euro-0': dict(mode='one_euro', fps=30.0, beta_loc=0.0, beta_rot=0.0),
           'euro-0.5': dict(mode='one_euro', fps=30.0, beta_loc=0.5, beta_rot=0.5)}
LOC_FLOOR = 1e-6
WELL_POSED = 0.5


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def problem(N, T, J, seed=0):
    """fp32 rows on the host, rounded from the fp64 paths."""
    bones, root = smooth_paths(N, T, J, seed)
    return bones.float(), root.float()


def sign_margin(src, out, kw):
    """The smallest magnitude among the dot products that decide a sign, on fp64 rows ``src`` (N,T,...,6) and their result."""
    q = _row_quat(src)
    T = src.shape[1]
    if kw['mode'] == 'gaussian':
        dots = [(q[:, d:] * q[:, :T - d]).sum(-1).abs().min() for d in range(1, min(kw['radius'], T - 1) + 1)]
    else:
        dots = [(_row_quat(out)[:, :-1] * q[:, 1:]).sum(-1).abs().min()] if T > 1 else []
    return min([float(d) for d in dots], default=1.0)


@functools.lru_cache(maxsize=None)
def reference(N, T, J, config):
    """The fp64 definition on the host, on the fp32 inputs of ``problem``: rows, their matrices and the condition of the case."""
    kw = CONFIGS[config]
    bones, root = (t.double() for t in problem(N, T, J))
    b, r, _ = ops.smooth_carla_rows(bones, root, **kw)
    margin = min(sign_margin(bones, b, kw), sign_margin(root, r, kw))
    return b, r, ops.carla_pose_import(b)[1], ops.carla_pose_import(r.unsqueeze(-2))[1], margin


def errors(rows, want_rows, want_rot):
    """(largest matrix entry difference, largest location difference) of device rows against the fp64 reference."""
    rows = rows.double().cpu()
    assert rows.shape == want_rows.shape
    rot = ops.carla_pose_import(rows if rows.ndim == 4 else rows.unsqueeze(-2))[1]
    return float((rot - want_rot).abs().max()), float((rows[..., :3] - want_rows[..., :3]).abs().max())


def kernel(bones, root, **kw):
    out = ops.smooth_carla_rows(bones, root, **kw)
    torch.cuda.synchronize()
    return out


def no_library():
    raise AssertionError('the library was asked for: a launch where none belongs')


def framework(monkeypatch, bones, root, **kw):
    with monkeypatch.context() as m:
        m.setenv('P2C_SMOOTH_FRAMEWORK', '1')
        m.setattr(_lib, 'lib', no_library)
        return kernel(bones, root, **kw)


@pytest.mark.parametrize('config', list(CONFIGS))
@pytest.mark.parametrize('N,T,J,max_blocks', SHAPES)
def test_against_fp64_and_bit_stability(N, T, J, max_blocks, config, monkeypatch):
    kw = CONFIGS[config]
    bones, root = (t.to(dev()) for t in problem(N, T, J))
    want_b, want_r, want_b_rot, want_r_rot, margin = reference(N, T, J, config)
    print(f'({N},{T},{J}) {config}: the sign decisions have a dot product of at least {margin:.3f}')
    assert margin >= WELL_POSED
    got_b, got_r, got_state = kernel(bones, root, max_blocks=max_blocks, **kw)
    assert got_b.shape == (N, T, J, 6) and got_r.shape == (N, T, 6) and got_b.dtype == torch.float32 and got_b.is_cuda
    fw_b, fw_r, fw_state = framework(monkeypatch, bones, root, **kw)
    scale = max(float(bones[..., :3].abs().max()), float(root[..., :3].abs().max()))
    for what, got, fw, want, want_rot in (('bones', got_b, fw_b, want_b, want_b_rot), ('root', got_r, fw_r, want_r, want_r_rot)):
        fw_rot_err, fw_loc_err = errors(fw, want, want_rot)
        rot_err, loc_err = errors(got, want, want_rot)
        rot_tol, loc_tol = max(4 * fw_rot_err, MATRIX_FLOOR), max(4 * fw_loc_err, LOC_FLOOR * scale)
        print(f'({N},{T},{J}) cap {max_blocks} {config} {what}: tensor restatement {fw_rot_err:.3e} / {fw_loc_err:.3e}, '
              f'K39 {rot_err:.3e} / {loc_err:.3e} from fp64 (matrix entries / locations; allowed {rot_tol:.3e} / {loc_tol:.3e})')
        assert math.isfinite(rot_err) and rot_err <= rot_tol, what
        assert math.isfinite(loc_err) and loc_err <= loc_tol, what
    if kw['mode'] == 'one_euro':
        # frame 0 is a copy; the state is (x^, v^, q^, w^, 0) of the last frame, q^ the quaternion of the last output row
        assert torch.equal(got_b[:, 0], bones[:, 0]) and torch.equal(got_r[:, 0], root[:, 0])
        assert got_state[0].shape == (N, J, 12) and got_state[1].shape == (N, 12) and bool(torch.isfinite(got_state[0]).all())
        assert torch.equal(got_state[0][..., :3], got_b[:, -1, :, :3]) and float(got_state[0][..., 11].abs().max()) == 0.0
        for s, f in zip(got_state, fw_state):
            assert float((s - f).abs().max()) <= 1e-2 * max(1.0, float(f.abs().max()))
        if T > 1:
            q_state, q_row = got_state[0][..., 6:10].double().cpu(), _row_quat(got_b[:, -1].double().cpu())
            assert float(((q_state * q_row).sum(-1).abs() - 1).abs().max()) <= 1e-5
    else:
        assert got_state is None
        zero_b, zero_r, _ = kernel(bones, root, mode='gaussian', sigma=1.0, radius=0, max_blocks=max_blocks)
        assert torch.equal(zero_b, bones) and torch.equal(zero_r, root) and zero_b.data_ptr() != bones.data_ptr()
    # bit stability: a repeat, the full grid, without the root rows, from a strided view
    again_b, again_r, _ = kernel(bones, root, max_blocks=max_blocks, **kw)
    assert torch.equal(again_b, got_b) and torch.equal(again_r, got_r)
    if max_blocks:
        full_b, full_r, _ = kernel(bones, root, **kw)
        assert torch.equal(full_b, got_b) and torch.equal(full_r, got_r)
    else:
        two_b, two_r, _ = kernel(bones, root, max_blocks=2, **kw)
        assert torch.equal(two_b, got_b) and torch.equal(two_r, got_r)
    alone_b, none, _ = kernel(bones, None, max_blocks=max_blocks, **kw)
    assert none is None and torch.equal(alone_b, got_b)
    wide_b, wide_r = torch.zeros(N, T, J, 8, device=dev()), torch.zeros(N, 2 * T, 6, device=dev())
    wide_b[..., 1:7], wide_r[:, ::2] = bones, root
    view_b, view_r, _ = kernel(wide_b[..., 1:7], wide_r[:, ::2], max_blocks=max_blocks, **kw)
    assert torch.equal(view_b, got_b) and torch.equal(view_r, got_r)


@pytest.mark.parametrize('R', [3, 32])
def test_a_window_of_outputs_has_the_bits_of_the_whole(R):
    """Outputs asked for in pieces, from the frames their windows need and no others: other tiles, the same rows. R = 32 is the
    largest LDS image (22 output frames to a tile)."""
    N, T, J = 2, 40, 26
    bones, root = (t.to(dev()) for t in problem(N, T, J))
    kw = dict(mode='gaussian', sigma=R / 3.0, radius=R)
    whole_b, whole_r, _ = kernel(bones, root, **kw)
    assert bool(torch.isfinite(whole_b).all())
    for first, count in ((0, 7), (7, 23), (30, 10), (17, 1)):
        lo, hi = max(first - R, 0), min(first + count - 1 + R, T - 1)
        b, r, _ = kernel(bones[:, lo:hi + 1], root[:, lo:hi + 1], first_frame=lo, first_output=first, count=count, last_frame=T - 1, **kw)
        assert torch.equal(b, whole_b[:, first:first + count]) and torch.equal(r, whole_r[:, first:first + count]), (first, count)
    with pytest.raises((ValueError, RuntimeError)):
        kernel(bones[:, 1:], root[:, 1:], first_frame=1, first_output=0, count=4, last_frame=T - 1, **kw)


@pytest.mark.parametrize('config', ['gauss-2-6', 'euro-0.5'])
def test_more_rows_than_a_chunk(config):
    """J = 30 with the root is 31 rows a frame: the gaussian kernel takes them in two chunks of its LDS image (27 + 4, the root in
    the second). A row's bits are those it has in a call of its own bones."""
    kw = CONFIGS[config]
    N, T, J = 2, 40, 30
    bones, root = (t.to(dev()) for t in problem(N, T, J))
    got_b, got_r, _ = kernel(bones, root, **kw)
    head_b, head_r, _ = kernel(bones[:, :, :26], root, **kw)
    tail_b, none, _ = kernel(bones[:, :, 26:], None, max_blocks=2, **kw)
    assert none is None and bool(torch.isfinite(got_b).all())
    assert torch.equal(got_b[:, :, :26], head_b) and torch.equal(got_b[:, :, 26:], tail_b) and torch.equal(got_r, head_r)


@pytest.mark.parametrize('config', ['gauss-1-3', 'euro-0.5'])
def test_pushed_chunks_carry_the_bits_of_the_uncut_video(config, monkeypatch):
    chunks = (1, 3, 1, 7, 2, 9, 17)
    N, T, J = 2, sum(chunks), 26
    assert T == 40
    bones, root = (t.to(dev()) for t in problem(N, T, J))
    for with_root in (True, False):
        stream = CarlaSmoother(**CONFIGS[config])
        whole_b, whole_r = stream.smooth(bones, root if with_root else None)
        pieces, t = [], 0
        for i, n in enumerate(chunks):
            with monkeypatch.context() as m:
                if i == 0 and config.startswith('gauss'):
                    m.setattr(_lib, 'lib', no_library)                    # a push that completes no output: no launch
                pieces.append(stream.push(bones[:, t:t + n], root[:, t:t + n] if with_root else None))
            t += n
        assert pieces[0][0].shape == (N, 0 if config.startswith('gauss') else 1, J, 6) and pieces[0][0].is_cuda
        assert stream.frames == T
        pieces.append(stream.flush())
        torch.cuda.synchronize()
        got_b = torch.cat([p[0] for p in pieces], 1)
        assert got_b.shape == whole_b.shape and got_b.dtype == torch.float32 and torch.equal(got_b, whole_b)
        if with_root:
            assert torch.equal(torch.cat([p[1] for p in pieces], 1), whole_r)
        with pytest.raises((ValueError, RuntimeError)):
            stream.push(bones[:, :2], root[:, :2] if with_root else None)
            stream.push(bones[:1, 2:3], root[:1, 2:3] if with_root else None)


@pytest.mark.parametrize('config', ['gauss-1-3', 'euro-0.5'])
def test_a_nan_clip_stays_nan_and_touches_nothing_else(config):
    kw = CONFIGS[config]
    N, T, J = 3, 40, 26
    bones, root = (t.to(dev()).clone() for t in problem(N, T, J))
    clean_b, clean_r, _ = kernel(bones, root, **kw)
    bones[1], root[1] = float('nan'), float('nan')
    b, r, _ = kernel(bones, root, **kw)
    assert bool(torch.isnan(b[1]).all()) and bool(torch.isnan(r[1]).all())
    for n in (0, 2):
        alone_b, alone_r, _ = kernel(bones[n:n + 1], root[n:n + 1], **kw)
        assert torch.equal(b[n:n + 1], alone_b) and torch.equal(r[n:n + 1], alone_r)
        assert not bool(torch.isnan(b[n]).any()) and not bool(torch.isnan(r[n]).any())
    # one NaN row, next to a tile's edge: that bone within R frames, that chain from there on
    one_b, one_r = (t.to(dev()).clone() for t in problem(N, T, J))
    one_b[0, 31, 7] = float('nan')
    b, r, _ = kernel(one_b, one_r, **kw)
    bad = torch.isnan(b).any(-1)
    want = torch.zeros_like(bad)
    if kw['mode'] == 'gaussian':
        want[0, 31 - kw['radius']:31 + kw['radius'] + 1, 7] = True
    else:
        want[0, 31:, 7] = True
    assert torch.equal(bad, want) and torch.equal(b[~bad], clean_b[~bad]) and torch.equal(r, clean_r)


@pytest.mark.parametrize('config', ['gauss-2-6', 'euro-0.5'])
def test_dispatch(config, monkeypatch):
    kw = CONFIGS[config]
    N, T, J = 2, 5, 26
    bones, root = (t.to(dev()) for t in problem(N, T, J))
    want_b, want_r, want_b_rot, want_r_rot, _ = reference(N, T, J, config)
    fw_b, fw_r, _ = framework(monkeypatch, bones, root, **kw)             # the library is not asked for
    assert fw_b.dtype == torch.float32 and fw_b.is_cuda
    fw_err, fw_loc = errors(fw_b, want_b, want_b_rot)
    tol = max(4 * fw_err, MATRIX_FLOOR)
    with monkeypatch.context() as m:
        m.setattr(_lib, 'lib', no_library)
        d_b, d_r, _ = kernel(bones.double(), root.double(), **kw)
        h_b, h_r, _ = ops.smooth_carla_rows(bones.cpu(), root.cpu(), **kw)
        with torch.autocast('cuda', dtype=torch.bfloat16):
            ac_b, _, _ = kernel(bones, root, **kw)
    assert d_b.dtype == torch.float64 and d_b.is_cuda and d_r.dtype == torch.float64
    assert h_b.dtype == torch.float32 and not h_b.is_cuda and not h_r.is_cuda
    err64, loc64 = errors(d_b, want_b, want_b_rot)
    err_r64, _ = errors(d_r, want_r, want_r_rot)
    print(f'{config}: fp64 on the device {err64:.3e} / {loc64:.3e}, fp32 tensor restatement {fw_err:.3e} / {fw_loc:.3e} (allowed {tol:.3e})')
    assert err64 <= tol and err_r64 <= tol and fw_err <= tol
    assert errors(ac_b, want_b, want_b_rot)[0] <= tol and errors(h_b, want_b, want_b_rot)[0] <= tol
    got_b, _, _ = kernel(bones, root, **kw)
    assert errors(got_b, want_b, want_b_rot)[0] <= tol


def test_gauss_abi_refusals_come_before_any_launch():
    lib = _lib.lib()
    N, S, J, K, R = 2, 6, 3, 6, 2
    bones, root = torch.zeros(N, S, J, 6, device=dev()), torch.zeros(N, S, 6, device=dev())
    out_b, out_r = torch.zeros(N, K, J, 6, device=dev()), torch.zeros(N, K, 6, device=dev())
    weights = sm.gauss_table(1.0, R).to(dev())
    base = dict(bones=bones.data_ptr(), root=root.data_ptr(), out_bones=out_b.data_ptr(), out_root=out_r.data_ptr(),
                weights=weights.data_ptr(), N=N, S=S, J=J, K=K, first_frame=0, first_output=0, last_frame=S - 1, R=R, max_blocks=0)

    def call(**changes):
        a = {**base, **changes}
        return lib.p2c_carla_smooth_gauss_fwd(*a.values(), None)

    for changes in (dict(N=-1), dict(S=-1), dict(K=-1), dict(first_output=-1), dict(first_frame=-1), dict(last_frame=-2),
                    dict(max_blocks=-1), dict(J=0), dict(R=-1), dict(R=33), dict(N=2 ** 30, K=2 ** 10), dict(N=2 ** 30, S=2 ** 10),
                    dict(S=0), dict(first_frame=2 ** 40), dict(first_output=2 ** 40)):
        assert call(**changes) == -2, changes
    assert call(N=-1, bones=None) == -2 and call(R=33, weights=None) == -2        # shapes are looked at first
    for changes in (dict(bones=None), dict(out_bones=None), dict(out_root=None), dict(root=None), dict(weights=None)):
        assert call(**changes) == -1, changes
    assert call(N=0) == 0 and call(K=0) == 0 and call(K=0, S=0) == 0
    torch.cuda.synchronize()
    assert float(out_b.abs().sum()) == 0.0 and float(out_r.abs().sum()) == 0.0   # nothing ran
    bones.fill_(1.0), root.fill_(2.0)
    bones[..., 3:], root[..., 3:] = 0.0, 0.0
    assert call() == 0 and call(root=None, out_root=None) == 0 and call(R=0, weights=None) == 0 and call(last_frame=-1) == 0
    torch.cuda.synchronize()
    assert float((out_b[..., :3] - 1.0).abs().max()) <= 1e-6 and float((out_r[..., :3] - 2.0).abs().max()) <= 1e-6
    assert float(out_b[..., 3:].abs().max()) <= 1e-4
    # a window is clamped into the given frames, never followed outside: outputs 2..7 of frames 0..5, the last two have no centre
    bones[:, 5, :, 0] = 7.0
    assert call(first_output=2, last_frame=-1) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out_b[:, :4]).all()) and bool(torch.isnan(out_b[:, 4:]).all())
    assert float(out_b[0, 0, 0, 0]) == 1.0 and 1.0 < float(out_b[0, 1, 0, 0]) < float(out_b[0, 3, 0, 0]) < 7.0


def test_euro_abi_refusals_come_before_any_launch():
    lib = _lib.lib()
    N, T, J = 2, 4, 3
    bones, root = torch.zeros(N, T, J, 6, device=dev()), torch.zeros(N, T, 6, device=dev())
    sb, sr = torch.zeros(N, J, 12, device=dev()), torch.zeros(N, 12, device=dev())
    out_b, out_r = torch.zeros(N, T, J, 6, device=dev()), torch.zeros(N, T, 6, device=dev())
    base = dict(bones=bones.data_ptr(), root=root.data_ptr(), state_bones=sb.data_ptr(), state_root=sr.data_ptr(),
                out_bones=out_b.data_ptr(), out_root=out_r.data_ptr(), N=N, T=T, J=J, has_state=0, fps=30.0, min_cutoff=1.0,
                beta_loc=0.0, beta_rot=0.0, d_cutoff=1.0, max_blocks=0)

    def call(**changes):
        a = {**base, **changes}
        return lib.p2c_carla_smooth_euro_fwd(*a.values(), None)

    nan, inf = float('nan'), float('inf')
    for changes in (dict(N=-1), dict(T=-1), dict(J=0), dict(max_blocks=-1), dict(has_state=2), dict(has_state=-1),
                    dict(N=2 ** 30, T=2 ** 10), dict(fps=0.0), dict(fps=-1.0), dict(fps=nan), dict(fps=inf), dict(fps=1e-60),
                    dict(fps=1e60), dict(min_cutoff=0.0), dict(min_cutoff=nan), dict(d_cutoff=0.0), dict(d_cutoff=inf),
                    dict(beta_loc=-1.0), dict(beta_rot=-1.0), dict(beta_loc=nan), dict(beta_rot=inf)):
        assert call(**changes) == -2, changes
    assert call(fps=0.0, bones=None) == -2                                        # shapes are looked at first
    for changes in (dict(bones=None), dict(out_bones=None), dict(out_root=None), dict(root=None),
                    dict(has_state=1, state_bones=None), dict(has_state=1, state_root=None)):
        assert call(**changes) == -1, changes
    assert call(N=0) == 0 and call(T=0) == 0
    torch.cuda.synchronize()
    assert float(out_b.abs().sum()) == 0.0 and float(out_r.abs().sum()) == 0.0 and float(sb.abs().sum()) == 0.0   # nothing ran
    bones[..., :3], root[..., :3] = 1.0, 2.0
    assert call() == 0 and call(state_bones=None, state_root=None) == 0 and call(root=None, out_root=None, state_root=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out_b, bones) and torch.equal(out_r, root)                 # a constant video, the identity rotation
    assert float(sb[..., :3].min()) == 1.0 and float(sr[..., :3].min()) == 2.0 and abs(float(sb[..., 6].min()) - 1.0) <= 1e-6
    bones[..., 0] = 3.0
    assert call(has_state=1) == 0                                                 # the state goes on: x^ moves from 1 towards 3
    torch.cuda.synchronize()
    first, last = float(out_b[0, 0, 0, 0]), float(out_b[0, -1, 0, 0])
    assert 1.0 < first < last < 3.0 and float(sb[0, 0, 0]) == last


def test_predict_carla_with_a_smoother():
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything
    from pedestrians_video_2_carla_amd.walker_control.resample import CarlaResampler
    seed_everything(11)
    B, T = 2, 8
    dm = SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B)
    flow = LitPoseLiftingFlow(movements_model=LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON),
                              loss_modes=['loc_2d_3d'], transform='hips_neck_bbox')
    trainer = Trainer(max_steps=1, device=dev()).setup(flow, dm)
    batches = [dm.generate_batch(dev()), dm.generate_batch(dev())]
    plain = trainer.predict_carla(flow, batches)
    same = trainer.predict_carla(flow, batches, smooth=None)
    for kw in (dict(mode='gaussian', sigma=1.0), dict(mode='one_euro', fps=30.0, beta_rot=0.2)):
        smoother = CarlaSmoother(**kw)
        smoothed = trainer.predict_carla(flow, batches, smooth=smoother)
        both = trainer.predict_carla(flow, batches, src_fps=30, out_fps=20, smooth={k: v for k, v in kw.items() if k != 'fps'})
        torch.cuda.synchronize()
        for (b, r, meta), (nb, nr, _), (sb, sr, smeta), (fb, fr, _) in zip(plain, same, smoothed, both):
            assert torch.equal(nb, b) and torch.equal(nr, r)
            wb, wr = smoother.smooth(b, r)
            assert sb.is_cuda and sb.shape == (B, T, 26, 6) and smeta is meta and not torch.equal(sb, b)
            assert torch.equal(sb, wb) and torch.equal(sr, wr)
            xb, xr = CarlaResampler(30, 20).resample(wb, wr)
            assert torch.equal(fb, xb) and torch.equal(fr, xr)
